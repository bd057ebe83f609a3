// Policy actor: live weights.  The context keeps the flat fp32 parameter vector on the device (PolicyNet::live, after
// either load entry); pnpx_policy_load_device derives the packed layout the forward reads from it with four launches on
// the caller's stream and refreshes an already loaded actor in place -- no allocation, no device-wide synchronisation, the
// activation arena is kept.  The per-convolution weight scales are launch arguments of the half-split instances, so a
// refresh ends with one small read-back and a synchronisation of that stream (not capturable).
//
// What is derived (policy.hip::policy_load is the host statement of the same arithmetic):
//   pol_fold_kernel      per output channel: scale = g / sqrt(v + eps), shift = b - m * scale in the host's fp32 roundings
//                        (correctly rounded sqrt -- taken in double and rounded once more -- and divide; the host object
//                        code has no fused multiply-add, so the shift is two roundings: contraction is off), and
//                        max |folded weight| = fl(max |w| * |scale|)
//   pol_scale_kernel     per convolution: the power-of-two half-split scale 2^(14 - exponent(max |w|)) into the read-back block
//   pol_pack_hs_kernel   the 12 stride-1 convolutions (9 taps), the stem and the 4 stage-entry conv1 as 2x2-window sparse-tap
//                        launches over the space-to-depth input (0x01B), the 4 shortcuts (0x010): hi / lo f16 fragments
//   live_copy_kernel     the shifts as biases, the head matrices (live_params.hip, shared with the critic)
//
// ONE blob layout (make_layout): per convolution its half-split packing and its bias, then the head matrices, every entry
// 256-float aligned.  It depends on the network's shape alone, so the blob policy_load packs on the host and the one a
// device load allocates are the same bytes at the same offsets, and either is refreshed in place.
#include <cmath>

#include "common.h"
#include "conv_hs.h"
#include "pack_desc.h"
#include "policy_grad.h"
#include "resnet18_hs.h"

namespace pnpx {
namespace {

constexpr float BN_EPS = 1e-5f;
constexpr int NCV = TRUNK_LAYERS;   // BatchNorm-ed convolutions in parameter order = the trunk's layer numbering (resnet18_hs.h)
constexpr int MAXCOPY = 27, NRB = 32;   // 21 biases + up to 6 head tensors; floats of the read-back block
constexpr int RB_NORM = NCV;            // behind the 21 scales, written by policy_adam_step alone: gradient norm, clip coefficient

struct PolFoldDesc {
  unsigned src_w, src_bn;    // floats into the parameter vector: weights; BatchNorm weight, bias, running_mean, running_var
  unsigned chan0;            // first output channel in the per-channel arrays
  int cout, fan;
};
struct PolPackTable {
  PolFoldDesc fold[NCV];
  PackDesc pack[NCV];
  CopyDesc copy[MAXCOPY];
  unsigned nchan;
  int ncopy;
};
struct PolicyLayout {        // the table + the blob offsets (floats) the host needs
  PolPackTable T;
  size_t hs_bias[NCV];
  size_t smw, smb, dw, db, d2w, d2b, total;
  PackDims dims;             // the launch dimensions of T (stored with the workspace the table is uploaded to)
};

// Offsets of HostBlob as policy_load fills it (256-float alignment before every entry), sources in pnpx_policy_load's order.
bool make_layout(int num_inputs, int n_det, int spi_head, PolicyLayout& L) {
  L = PolicyLayout();
  const int cin_pad = (num_inputs + 7) / 8 * 8;
  BlobCursor cur;
  unsigned chan = 0;
  int ncopy = 0;
  bool ok = true;
  auto copy = [&](unsigned from, size_t to, size_t n, unsigned space) {
    if (ncopy < MAXCOPY) L.T.copy[ncopy] = CopyDesc{from, (unsigned)to, (unsigned)n, space};
    ++ncopy;
    if (n > L.dims.max_copy) L.dims.max_copy = (unsigned)n;
  };
  auto take_conv = [&](int ci, int cout, int cin, int ks) {
    PolFoldDesc& F = L.T.fold[ci];
    F.src_w = cur.take((size_t)cout * cin * ks);
    F.src_bn = cur.take((size_t)4 * cout);
    F.chan0 = chan;
    F.cout = cout;
    F.fan = cin * ks;
    chan += cout;
  };
  // half-split packing of convolution ci + its bias
  auto put_hs = [&](int ci, int kind, int cin, int Cp, int K, int mask) {
    const PolFoldDesc& F = L.T.fold[ci];
    PackDesc& P = L.T.pack[ci];
    P.src_v = F.src_w;
    P.chan0 = F.chan0;
    P.conv = ci;
    P.rows = F.cout;
    P.K = K;
    P.mt = 64;
    pack_desc_window(P, mask);
    P.kind = kind;
    P.cin = cin;
    P.Cp = Cp;
    P.items = (unsigned)((size_t)P.rows * (P.K / 8) * P.nt);
    P.dst = (unsigned)cur.put((size_t)P.rows * P.K * P.nt);
    ok = ok && P.rows % 64 == 0 && P.K % 16 == 0;
    if (P.items > L.dims.max_items) L.dims.max_items = P.items;
    L.hs_bias[ci] = cur.put(F.cout);
    copy(F.chan0, L.hs_bias[ci], F.cout, 1);
  };
  take_conv(0, 64, num_inputs, 9);
  put_hs(0, 1, num_inputs, cin_pad, 4 * cin_pad, 0x01B);
  int in_planes = 64;
  for (int s = 0; s < 4; ++s) {
    const int p = stage_planes(s), c0 = 1 + 5 * s;
    take_conv(c0 + 0, p, in_planes, 9);
    take_conv(c0 + 1, p, p, 9);
    take_conv(c0 + 2, p, in_planes, 1);
    take_conv(c0 + 3, p, p, 9);
    take_conv(c0 + 4, p, p, 9);
    put_hs(c0 + 0, 1, in_planes, in_planes, 4 * in_planes, 0x01B);
    put_hs(c0 + 2, 2, in_planes, 0, in_planes, 0x010);
    put_hs(c0 + 1, 0, p, 0, p, 0x1FF);
    put_hs(c0 + 3, 0, p, 0, p, 0x1FF);
    put_hs(c0 + 4, 0, p, 0, p, 0x1FF);
    in_planes = p;
  }
  auto head = [&](size_t n) {
    const size_t to = cur.put(n);
    copy(cur.take(n), to, n, 0);
    return to;
  };
  L.smw = head(2 * 512);
  L.smb = head(2);
  if (spi_head) {
    L.dw = head((size_t)64 * 512);
    L.db = head(64);
    L.d2w = head((size_t)n_det * 64);
    L.d2b = head(n_det);
  } else {
    L.dw = head((size_t)n_det * 512);
    L.db = head(n_det);
  }
  L.total = cur.dst + 8192;   // DMA over-read slack
  L.T.nchan = L.dims.nchan = chan;
  L.T.ncopy = L.dims.ncopy = ncopy;
  return ok && ncopy <= MAXCOPY && cur.src == policy_num_params(num_inputs, n_det, spi_head) && L.total < ((size_t)1 << 32);
}

int layout_of(const char* who, int num_inputs, int n_det, int spi_head, PolicyLayout& L) {
  if (make_layout(num_inputs, n_det, spi_head, L)) return PNPX_OK;
  set_error("%s: internal layout error for (%d inputs, %d outputs, spi %d)", who, num_inputs, n_det, spi_head);
  return PNPX_ERR_SHAPE;
}

// device workspace: the table, then scale[nchan], shift[nchan], chmax[nchan], the read-back block
struct PolPackWs {
  PolPackTable* T;
  float *sc, *sh, *chmax, *rb;
};
inline size_t ws_table_bytes() { return (sizeof(PolPackTable) + 255) & ~(size_t)255; }
inline PolPackWs pack_ws(const PackWorkspace& W) {
  const unsigned nchan = W.dims.nchan;
  char* p = static_cast<char*>(W.ws.p);
  PolPackWs w;
  w.T = reinterpret_cast<PolPackTable*>(p);
  w.sc = reinterpret_cast<float*>(p + ws_table_bytes());
  w.sh = w.sc + nchan;
  w.chmax = w.sh + nchan;
  w.rb = w.chmax + nchan;
  return w;
}

// policy.hip::bn_fold of one output channel + the largest folded weight of that channel.  One 64-lane workgroup per channel
// walks the channel's fan: a maximum does not depend on the order.  fl(|w| * |scale|) is monotonic in |w|, so the largest
// folded weight is the fold of the largest |w|.  A NaN weight makes the channel's maximum NaN (the refresh is then refused).
// raw != 0: no fold -- scale exactly 1, shift exactly 0, the maximum of the weights themselves (the train-mode packing, policy_bn.hip).
__global__ __launch_bounds__(64) void pol_fold_kernel(const PolPackTable* __restrict__ T, const float* __restrict__ P,
                                                      float* __restrict__ sc, float* __restrict__ sh, float* __restrict__ chmax, int raw) {
#pragma clang fp contract(off)
  __shared__ float part[64];
  __shared__ int nan_seen;
  const unsigned ch = blockIdx.x;
  const int tid = threadIdx.x;
  int li = 0;
  while (li + 1 < NCV && T->fold[li + 1].chan0 <= ch) ++li;
  const PolFoldDesc F = T->fold[li];
  const unsigned co = ch - F.chan0;
  const float* w = P + F.src_w + (size_t)co * F.fan;
  if (tid == 0) nan_seen = 0;
  __syncthreads();
  float vmax = 0.f;
  bool bad = false;
  for (int i = tid; i < F.fan; i += 64) {
    const float x = w[i];
    bad |= (x != x);
    vmax = fmaxf(vmax, fabsf(x));
  }
  part[tid] = vmax;
  if (bad) nan_seen = 1;
  __syncthreads();
  for (int st = 32; st > 0; st >>= 1) {
    if (tid < st) part[tid] = fmaxf(part[tid], part[tid + st]);
    __syncthreads();
  }
  if (tid != 0) return;
  if (raw) {
    sc[ch] = 1.f;
    sh[ch] = 0.f;
    chmax[ch] = nan_seen ? NAN : part[0];
    return;
  }
  const float* bn = P + F.src_bn + co;
  const float g = bn[0], b = bn[F.cout], m = bn[2 * (size_t)F.cout], v = bn[3 * (size_t)F.cout];
  // the fp32 square root as the host's sqrtss rounds it: the correctly rounded double root, rounded once more (exact for 53 >= 2 * 24 + 2
  // bits); the fp32 device intrinsic compiles to the 1-ulp hardware instruction
  const float root = (float)__dsqrt_rn((double)(v + BN_EPS));
  const float scale = __fdiv_rn(g, root);
  const float prod = m * scale;
  sc[ch] = scale;
  sh[ch] = b - prod;
  chmax[ch] = nan_seen ? NAN : fabsf(part[0] * scale);
}

// block li: the scale 2^(14 - exponent(max |w|)) of convolution li (pack_conv_weights_hs_taps); NaN unless the maximum is finite
__global__ __launch_bounds__(256) void pol_scale_kernel(const PolPackTable* __restrict__ T, const float* __restrict__ chmax,
                                                        float* __restrict__ rb) {
  __shared__ float part[256];
  __shared__ int bad_seen;
  const int li = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) bad_seen = 0;
  __syncthreads();
  float m = 0.f;
  bool bad = false;
  for (int c = tid; c < T->fold[li].cout; c += 256) {
    const float x = chmax[T->fold[li].chan0 + c];
    bad |= !(fabsf(x) <= 3.402823466e38f);
    m = fmaxf(m, x);
  }
  part[tid] = m;
  if (bad) bad_seen = 1;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) part[tid] = fmaxf(part[tid], part[tid + st]);
    __syncthreads();
  }
  if (tid != 0) return;
  m = part[0];
  int e = 0;
  if (m > 0.f) {
    (void)frexpf(m, &e);
    e = 14 - e;
  }
  rb[li] = bad_seen ? NAN : ldexpf(1.0f, e);
}

// One thread per (cout tile, K chunk, tap, K half, row) of a half-split packing (pack_desc.h)
__global__ __launch_bounds__(256) void pol_pack_hs_kernel(const PolPackTable* __restrict__ T, const float* __restrict__ P,
                                                          const float* __restrict__ sc, const float* __restrict__ rb,
                                                          float* __restrict__ blob) {
  const PackDesc& D = T->pack[blockIdx.y];
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.items) return;
  hs_pack_item(D, i, rb[D.conv], blob, [&](int row, int k, int tap) {
    const long long off = eff_src_offset(D, row, k, tap);
    return off < 0 ? 0.f : P[D.src_v + off] * sc[D.chan0 + row];
  });
}

// The adjoint packings of the fold-free table (parameter gradients, policy_bn.hip::policy_param_grad): layer li's input-gradient launch
// reads the same raw weights with rows / K transposed and the taps mirrored (PackDesc::adj; windows 0x1FF / 0x1B0 / 0x010), in the same
// power-of-two weight scale.  Layers 1..20: the stem's adjoint is never run.  A blob and a table of their own, so that eval-only and
// forward-only users allocate none of it.
struct PolAdjTable {
  PackDesc pack[NCV];   // [0] unused (no items)
};
struct PolAdjLayout {
  PolAdjTable T;
  size_t zero = 0, total = 0;   // zero: 1024 zeros, the bias operand of the adjoint launches
  unsigned max_items = 0;
};
bool make_adj_layout(const PolicyLayout& L, PolAdjLayout& A) {
  A = PolAdjLayout();
  BlobCursor cur;
  bool ok = true;
  for (int li = 1; li < NCV; ++li) {
    const PackDesc& F = L.T.pack[li];
    PackDesc& P = A.T.pack[li];
    P = F;
    P.rows = F.K;
    P.K = F.rows;
    P.mt = 64;
    pack_desc_window(P, trunk_taps(li, true));
    P.adj = 1;
    P.items = (unsigned)((size_t)P.rows * (P.K / 8) * P.nt);
    P.dst = (unsigned)cur.put((size_t)P.rows * P.K * P.nt);
    ok = ok && P.rows % 64 == 0 && P.K % 16 == 0;
    if (P.items > A.max_items) A.max_items = P.items;
  }
  A.zero = cur.put(1024);
  A.total = cur.dst + 8192;   // DMA over-read slack
  return ok && A.total < ((size_t)1 << 32);
}
// One thread per (cout tile, K chunk, tap, K half, row) of adjoint packing blockIdx.y + 1; rb: the raw packing's weight scales
__global__ __launch_bounds__(256) void pol_pack_adj_kernel(const PolAdjTable* __restrict__ T, const float* __restrict__ P,
                                                           const float* __restrict__ rb, float* __restrict__ blob) {
  const PackDesc& D = T->pack[blockIdx.y + 1];
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.items) return;
  hs_pack_item(D, i, rb[D.conv], blob, [&](int row, int k, int tap) {
    const long long off = eff_src_offset(D, k, row, 8 - tap);
    return off < 0 ? 0.f : P[D.src_v + off];
  });
}

// the packing workspace with its table
int alloc_pack_ws(PackWorkspace& W, const PolicyLayout& L) {
  return W.alloc(&L.T, sizeof(PolPackTable), (size_t)3 * L.dims.nchan * sizeof(float), NRB, L.dims, "policy packing workspace");
}
// a fresh blob (zero padding and over-read slack) and its packing workspace
int alloc_device_layout(PolicyPack& N, PackWorkspace& W, const PolicyLayout& L) {
  PNPX_TRY(alloc_dev(N.weights, L.total * sizeof(float), "policy weight"));
  PNPX_TRY(alloc_pack_ws(W, L));
  PNPX_HIP(hipMemset(N.weights.p, 0, N.weights.bytes));
  PNPX_HIP(hipDeviceSynchronize());
  return PNPX_OK;
}

// launch descriptors over the blob (the scales follow from the read-back)
void bind_blob(PolicyPack& N, const PolicyLayout& L, int spi_head) {
  float* base = static_cast<float*>(N.weights.p);
  for (int ci = 0; ci < NCV; ++ci) {
    const PackDesc& P = L.T.pack[ci];
    ConvLayerHsDev& D = N.hs[ci];
    D.cin = D.cin_pad = P.K;
    D.cout = P.rows;
    D.mt = P.mt;
    D.w = reinterpret_cast<char*>(base + P.dst);
    N.hs_bias[ci] = base + L.hs_bias[ci];
  }
  N.fc_sm_w = base + L.smw;
  N.fc_sm_b = base + L.smb;
  N.fc_det_w = base + L.dw;
  N.fc_det_b = base + L.db;
  N.fc_det2_w = spi_head ? base + L.d2w : nullptr;
  N.fc_det2_b = spi_head ? base + L.d2b : nullptr;
}

// master -> weight blob on stream s, then the one read-back: the 21 half-split scales.  raw: the fold-free packing (PolicyNet::raw)
int repack(pnpx_ctx* ctx, hipStream_t s, bool raw = false) {
  PolicyNet& N = ctx->policy;
  PolicyPack& K = raw ? N.raw : static_cast<PolicyPack&>(N);
  const PackWorkspace& W = raw ? N.raw_ws : N.pack_ws;
  const PackDims& d = W.dims;
  float* const rb_host = W.readback;
  const PolPackWs w = pack_ws(W);
  const float* P = N.live.p();
  float* blob = static_cast<float*>(K.weights.p);
  hipLaunchKernelGGL(pol_fold_kernel, dim3(d.nchan), dim3(64), 0, s, w.T, P, w.sc, w.sh, w.chmax, raw ? 1 : 0);
  PNPX_LAUNCH_CHECK();
  hipLaunchKernelGGL(pol_scale_kernel, dim3(NCV), dim3(256), 0, s, w.T, w.chmax, w.rb);
  PNPX_LAUNCH_CHECK();
  hipLaunchKernelGGL(pol_pack_hs_kernel, dim3((d.max_items + 255) / 256, NCV), dim3(256), 0, s, w.T, P, w.sc, w.rb, blob);
  PNPX_LAUNCH_CHECK();
  PNPX_TRY(launch_live_copy(w.T->copy, dim3((d.max_copy + 255) / 256, d.ncopy), P, w.sh, blob, s));
  PNPX_HIP(hipMemcpyAsync(rb_host, w.rb, (raw ? NCV : RB_NORM + 1) * sizeof(float), hipMemcpyDeviceToHost, s));   // + the optimiser's norm
  PNPX_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < NCV; ++i)
    if (!std::isfinite(rb_host[i])) {
      set_error("policy refresh: the weight scale of convolution %d is not finite (NaN weight, or a BatchNorm scale that is not finite: "
                "running_var NaN or below -eps)", i);
      PNPX_HIP(hipDeviceSynchronize());
      policy_free(ctx);
      return PNPX_ERR_ARG;
    }
  for (int ci = 0; ci < NCV; ++ci) K.hs[ci].inv_scale = 1.0f / (rb_host[ci] * HS_ASCALE);
  if (raw) {
    N.raw_valid = true;
  } else {
    N.loaded = true;
    N.eval_stale = false;
  }
  return PNPX_OK;
}

}  // namespace

int policy_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n, int num_inputs, int n_det, int spi_head, hipStream_t s) {
  spi_head = spi_head ? 1 : 0;
  const bool shape_ok = num_inputs >= 1 && num_inputs <= 64 && n_det >= 1 && n_det <= 64;
  if (!params_dev || !shape_ok || n != policy_num_params(num_inputs, n_det, spi_head)) {
    set_error("pnpx_policy_load_device: expected %zu parameters for (%d inputs, %d outputs, spi %d), got %zu",
              shape_ok ? policy_num_params(num_inputs, n_det, spi_head) : (size_t)0, num_inputs, n_det, spi_head, n);
    return PNPX_ERR_ARG;
  }
  PolicyNet& N = ctx->policy;
  const bool same_net = N.loaded && N.num_inputs == num_inputs && N.n_det == n_det && N.spi_head == spi_head;
  if (!same_net) {   // first load / another network: allocate (a refresh allocates nothing)
    PolicyLayout L;
    PNPX_TRY(layout_of("pnpx_policy_load_device", num_inputs, n_det, spi_head, L));
    PNPX_HIP(hipDeviceSynchronize());
    policy_free(ctx);
    N.num_inputs = num_inputs;
    N.cin_pad = (num_inputs + 7) / 8 * 8;
    N.n_det = n_det;
    N.spi_head = spi_head;
    int st = alloc_device_layout(N, N.pack_ws, L);
    if (st == PNPX_OK) st = N.live.alloc(n, "policy parameter");
    if (st == PNPX_OK) st = policy_upload_frozen(ctx);
    if (st != PNPX_OK) {
      policy_free(ctx);
      return st;
    }
    bind_blob(N, L, N.spi_head);
  }
  N.raw_valid = false;   // new weights: the train-mode packing follows on the next train forward
  N.adj_valid = false;   // ... and its adjoints on the next gradient call
  policy_kept_drop(N, "the weights were loaded again (pnpx_policy_load_device) after the kept forward");
  PNPX_TRY(N.live.set_device(params_dev, s));
  return repack(ctx, s);
}

// ------------------------------------------------------------------------------------------- optimiser
// The running statistics are buffers of the reference module, not parameters: clip_grad_norm_ and Adam (trainer.py:201-204) never see
// them.  In the live vector they follow each BatchNorm's weight and bias: one frozen range of 2 cout floats per BatchNorm layer.
int policy_frozen_ranges(int num_inputs, int n_det, int spi_head, FrozenRange* out, int* n_out) {
  PolicyLayout L;
  PNPX_TRY(layout_of("policy frozen ranges", num_inputs, n_det, spi_head ? 1 : 0, L));
  FrozenRange r[2 * NCV];
  for (int ci = 0; ci < NCV; ++ci) {
    const PolFoldDesc& F = L.T.fold[ci];
    r[2 * ci] = FrozenRange{(size_t)F.src_bn + 2 * (size_t)F.cout, (size_t)F.cout};       // running_mean
    r[2 * ci + 1] = FrozenRange{(size_t)F.src_bn + 3 * (size_t)F.cout, (size_t)F.cout};   // running_var
  }
  if (live_merge_frozen(r, 2 * NCV, policy_num_params(num_inputs, n_det, spi_head ? 1 : 0), out, n_out) != PNPX_OK) {
    set_error("policy frozen ranges: internal layout error for (%d inputs, %d outputs, spi %d)", num_inputs, n_det, spi_head);
    return PNPX_ERR_SHAPE;
  }
  return PNPX_OK;
}

int policy_upload_frozen(pnpx_ctx* ctx) {
  PolicyNet& N = ctx->policy;
  FrozenRange r[LIVE_OPTIM_MAX_FROZEN];
  int n = 0;
  PNPX_TRY(policy_frozen_ranges(N.num_inputs, N.n_det, N.spi_head, r, &n));
  return N.optim.set_frozen(r, n, N.live.n, "policy frozen-range table");
}

namespace {

int check_vector(const PolicyNet& N, const char* who, bool ptrs, size_t n, const char* what) {
  if (!N.loaded) {
    set_error("%s called before an actor was loaded", who);
    return PNPX_ERR_NO_WEIGHTS;
  }
  const size_t want = policy_num_params(N.num_inputs, N.n_det, N.spi_head);
  if (!ptrs || n != want) {
    set_error("%s: the loaded actor (%d inputs, %d outputs, spi %d) has %zu parameters, got %s%zu", who, N.num_inputs, N.n_det, N.spi_head,
              want, what, n);
    return PNPX_ERR_ARG;
  }
  return PNPX_OK;
}

}  // namespace

// clip_grad_norm_(max_norm) + Adam.step() (trainer/mddpg/trainer.py:201-204) on the live vector, the running statistics frozen, then
// what pnpx_policy_load_device does on the vector itself: the eval packing is re-derived now (its read-back brings the norm), the
// fold-free packing, its adjoints and a kept forward are stale.  The update reads the coefficient on the device and does nothing when
// the norm is not finite; the host learns the norm from the refresh's read-back and only then advances the step counter.
int policy_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n, float lr, float beta1, float beta2, float eps, float max_norm,
                     float* grad_norm_dev, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  PNPX_TRY(check_vector(N, "pnpx_policy_adam_step", grad_dev != nullptr, n, "a gradient of "));
  if (!(lr >= 0.f) || !std::isfinite(lr) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) ||
      !std::isfinite(eps) || !(max_norm > 0.f)) {
    set_error("pnpx_policy_adam_step: need lr >= 0 and finite, betas in [0, 1), eps > 0 and finite, max_norm > 0 (got lr %g, betas %g %g, "
              "eps %g, max_norm %g)", (double)lr, (double)beta1, (double)beta2, (double)eps, (double)max_norm);
    return PNPX_ERR_ARG;
  }
  float* slot = pack_ws(N.pack_ws).rb + RB_NORM;
  PNPX_TRY(N.optim.launch_step(N.live, grad_dev, lr, beta1, beta2, eps, max_norm, slot, grad_norm_dev, "policy optimiser state", s));
  PNPX_TRY(repack(ctx, s));   // (a weight stepped to a non-finite value: the actor is gone, as after any such refresh)
  const float norm = N.pack_ws.readback[RB_NORM];
  if (!std::isfinite(norm)) {   // nothing was written: every packing and a kept forward are still those of the weights
    set_error("pnpx_policy_adam_step: the gradient norm is not finite (%g); parameters and optimiser state are unchanged", (double)norm);
    return PNPX_ERR_ARG;
  }
  N.raw_valid = false;
  N.adj_valid = false;
  policy_kept_drop(N, "the weights were stepped (pnpx_policy_adam_step) after the kept forward");
  N.optim.commit();
  return PNPX_OK;
}

int policy_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n, long long* step_host, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  PNPX_TRY(check_vector(N, "pnpx_policy_optim_state", exp_avg_dst && exp_avg_sq_dst, n, "room for "));
  return N.optim.copy_state(n, exp_avg_dst, exp_avg_sq_dst, step_host, s);
}

// back to "before the first step": the next step allocates zero-filled moments and counts as step 1
int policy_optim_reset(pnpx_ctx* ctx) { return ctx->policy.optim.reset(); }

int policy_pack_raw(pnpx_ctx* ctx, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  if (!N.raw.weights.p) {
    PolicyLayout L;
    PNPX_TRY(layout_of("policy train forward", N.num_inputs, N.n_det, N.spi_head, L));
    PNPX_TRY(alloc_device_layout(N.raw, N.raw_ws, L));
    bind_blob(N.raw, L, N.spi_head);
  }
  return repack(ctx, s, true);
}

int policy_pack_adj(pnpx_ctx* ctx, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  if (!N.raw_valid) PNPX_TRY(policy_pack_raw(ctx, s));
  PolicyLayout L;
  PNPX_TRY(layout_of("policy parameter gradient", N.num_inputs, N.n_det, N.spi_head, L));
  PolAdjLayout A;
  if (!make_adj_layout(L, A)) {
    set_error("policy parameter gradient: internal adjoint layout error for %d inputs", N.num_inputs);
    return PNPX_ERR_SHAPE;
  }
  if (!N.raw_adj.p) {
    PNPX_TRY(alloc_dev(N.raw_adj, A.total * sizeof(float), "policy adjoint weight"));
    if (!N.raw_adj_table.p) PNPX_TRY(alloc_dev(N.raw_adj_table, sizeof(PolAdjTable), "policy adjoint table"));
    PNPX_HIP(hipMemset(N.raw_adj.p, 0, N.raw_adj.bytes));
    PNPX_HIP(hipMemcpy(N.raw_adj_table.p, &A.T, sizeof(PolAdjTable), hipMemcpyHostToDevice));
    PNPX_HIP(hipDeviceSynchronize());
  }
  float* blob = static_cast<float*>(N.raw_adj.p);
  for (int li = 1; li < NCV; ++li) {
    const PackDesc& P = A.T.pack[li];
    ConvLayerHsDev& D = N.raw_bwd[li];
    D.cin = D.cin_pad = P.K;
    D.cout = P.rows;
    D.mt = P.mt;
    D.w = reinterpret_cast<char*>(blob + P.dst);
    D.inv_scale = N.raw.hs[li].inv_scale;
  }
  N.raw_adj_zero = blob + A.zero;
  hipLaunchKernelGGL(pol_pack_adj_kernel, dim3((A.max_items + 255) / 256, NCV - 1), dim3(256), 0, s,
                     static_cast<const PolAdjTable*>(N.raw_adj_table.p), N.live.p(), pack_ws(N.raw_ws).rb, blob);
  PNPX_LAUNCH_CHECK();
  N.adj_valid = true;
  return PNPX_OK;
}

int policy_pack_descs(const PolicyNet& N, PackDesc* out21) {
  PolicyLayout L;
  PNPX_TRY(layout_of("policy parameter gradient", N.num_inputs, N.n_det, N.spi_head, L));
  for (int li = 0; li < NCV; ++li) out21[li] = L.T.pack[li];
  return PNPX_OK;
}

int policy_refresh_eval(pnpx_ctx* ctx, hipStream_t s) { return repack(ctx, s); }

// policy_load's last step.  Every later refresh writes into the blob the host packed (the 21 packings pk, the head matrices at heads[]
// in bind_blob's order, `total` floats), so the layout table has to describe exactly those offsets.
int policy_adopt_host_blob(pnpx_ctx* ctx, const Packed* pk, const size_t* heads, size_t total) {
  PolicyNet& N = ctx->policy;
  PolicyLayout L;
  PNPX_TRY(layout_of("pnpx_policy_load", N.num_inputs, N.n_det, N.spi_head, L));
  const size_t want[6] = {L.smw, L.smb, L.dw, L.db, L.d2w, L.d2b};
  bool same = L.total == total;
  for (int i = 0; same && i < (N.spi_head ? 6 : 4); ++i) same = heads[i] == want[i];
  for (int ci = 0; same && ci < NCV; ++ci) {
    const PackDesc& P = L.T.pack[ci];
    same = P.dst == pk[ci].w && L.hs_bias[ci] == pk[ci].b && P.mt == pk[ci].mt && P.K == pk[ci].cin && P.rows == pk[ci].cout;
  }
  if (!same) {
    set_error("pnpx_policy_load: the device packing table disagrees with the host layout (%d inputs, %d outputs, spi %d)", N.num_inputs,
              N.n_det, N.spi_head);
    return PNPX_ERR_SHAPE;
  }
  bind_blob(N, L, N.spi_head);
  for (int ci = 0; ci < NCV; ++ci) N.hs[ci].inv_scale = 1.0f / (pk[ci].scale * HS_ASCALE);
  return alloc_pack_ws(N.pack_ws, L);
}

int policy_params(pnpx_ctx* ctx, float* dst_dev, size_t n, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  if (!N.loaded) {
    set_error("pnpx_policy_params called before an actor was loaded");
    return PNPX_ERR_NO_WEIGHTS;
  }
  const size_t want = policy_num_params(N.num_inputs, N.n_det, N.spi_head);
  if (!dst_dev || n != want) {
    set_error("pnpx_policy_params: the loaded actor (%d inputs, %d outputs, spi %d) has %zu parameters, got room for %zu",
              N.num_inputs, N.n_det, N.spi_head, want, n);
    return PNPX_ERR_ARG;
  }
  return N.live.copy_out(dst_dev, s);
}

}  // namespace pnpx
