// Probe of the training kernels of the actor and the critic, for tests (tests/test_gpu_net_train.py): ONE call of the launcher(s) of
// policy_grad.h / critic_grad.h -- the very functions the network walks call -- on tensors the caller laid out, and a wait for it.  The
// scratch a walk keeps in its workspace (K-split slab, partial sums, head rows, the range bits) is allocated here and filled with NaN
// before the launch, so a piece or a tile that a finishing kernel reads but no thread wrote shows in the result.
// pnpx_net_train_probe_plan answers the launchers' own host-only piece counts.  Nothing in the library calls either; they add no option.
#include <cmath>

#include "common.h"
#include "conv_hs.h"
#include "critic_grad.h"
#include "policy_grad.h"

using namespace pnpx;

namespace {

int bad(int code, const char* what) {
  set_error("pnpx_net_train_probe: %s", what);
  return code;
}

constexpr long long MAX_PIXELS = 1LL << 24;     // B h w of one call: tests stay far below
constexpr long long MAX_RECORDS = 1LL << 28;    // records of one tensor

bool pow2_or_zero(float v) {
  if (v == 0.f) return true;
  int e;
  return v > 0.f && std::isfinite(v) && std::frexp(v, &e) == 0.5f;
}

int wgrad_fan(const pnpx_net_train_probe_desc& d) { return d.kind == 2 ? d.cin : d.cin * 9; }
int head_n1(const pnpx_net_train_probe_desc& d) { return d.spi ? 64 : d.n_det; }

// sizes: what the op cannot run, and fields the op has no place for.  *plan = what pnpx_net_train_probe_plan returns.
int validate_sizes(const pnpx_net_train_probe_desc& d, int* plan) {
  *plan = 1;
  const int op = d.op;
  if (op < PNPX_NT_BN_STATS || op > PNPX_NT_GRAD_SEED) return bad(PNPX_ERR_ARG, "unknown op");
  const bool wg = op == PNPX_NT_WGRAD_PLAIN || op == PNPX_NT_WGRAD_WN;
  const bool bn = op == PNPX_NT_BN_STATS || op == PNPX_NT_BN_APPLY || op == PNPX_NT_BN_BWD;
  const bool has_G = bn || op == PNPX_NT_CLIP_MASK || op == PNPX_NT_ALPHA_DOT;
  const bool has_hw = op != PNPX_NT_ALPHA_FINISH;
  if (!wg && (d.cout || d.K || d.cin || d.Cp || d.kind || d.Gg || d.Xg)) return bad(PNPX_ERR_ARG, "cout / K / cin / Cp / kind / Gg / Xg belong to the weight gradients only");
  if (!has_G && d.G) return bad(PNPX_ERR_ARG, "the op has no group count");
  if (!has_hw && (d.h || d.w)) return bad(PNPX_ERR_ARG, "the op has no image size");
  if (op != PNPX_NT_ALPHA_DOT && (d.resG || d.mG)) return bad(PNPX_ERR_ARG, "resG / mG belong to ALPHA_DOT only");
  if (op != PNPX_NT_HEAD_GRAD && (d.n_det || d.spi)) return bad(PNPX_ERR_ARG, "n_det / spi belong to HEAD_GRAD only");
  if (op != PNPX_NT_BN_STATS && (d.update || d.momentum != 0.f)) return bad(PNPX_ERR_ARG, "momentum / update belong to BN_STATS only");
  if (op != PNPX_NT_CLIP_MASK && op != PNPX_NT_FC_GRAD && d.thr != 0.f) return bad(PNPX_ERR_ARG, "thr belongs to CLIP_MASK and FC_GRAD only");
  if (op != PNPX_NT_BN_BWD && op != PNPX_NT_GRAD_SEED && d.boost != 0.f) return bad(PNPX_ERR_ARG, "boost belongs to BN_BWD and GRAD_SEED only");
  if (!wg && op != PNPX_NT_ALPHA_FINISH && d.inv_w != 0.f) return bad(PNPX_ERR_ARG, "inv_w belongs to the weight gradients and ALPHA_FINISH only");
  if (op != PNPX_NT_WGRAD_WN && d.inv_b != 0.f) return bad(PNPX_ERR_ARG, "inv_b belongs to WGRAD_WN only");
  if (d.B <= 0 || (has_hw && (d.h <= 0 || d.w <= 0)) || (has_G && d.G <= 0)) return bad(PNPX_ERR_SHAPE, "non-positive size");
  const long long npix = has_hw ? (long long)d.B * d.h * d.w : d.B;
  if (npix > MAX_PIXELS) return bad(PNPX_ERR_SHAPE, "more pixels than the probe takes");
  const int groups = has_G ? d.G : wg ? (d.Gg > d.Xg ? d.Gg : d.Xg) : 64;
  if (has_hw && (long long)d.B * groups * (d.h + 2) * (d.w + 2) > MAX_RECORDS) return bad(PNPX_ERR_SHAPE, "a tensor larger than the probe takes");
  switch (op) {
    case PNPX_NT_BN_STATS:
      if (!(d.momentum >= 0.f && d.momentum <= 1.f)) return bad(PNPX_ERR_SHAPE, "momentum outside [0, 1]");
      if (d.update != 0 && d.update != 1) return bad(PNPX_ERR_SHAPE, "update is 0 or 1");
      if (d.update && npix < 2) return bad(PNPX_ERR_SHAPE, "the running variance needs more than one value per channel");
      *plan = (int)bn_fwd_pieces(npix);
      break;
    case PNPX_NT_BN_APPLY:
      *plan = (int)(((size_t)npix * d.G + 255) / 256);
      break;
    case PNPX_NT_BN_BWD:
      if (!pow2_or_zero(d.boost)) return bad(PNPX_ERR_SHAPE, "boost is a power of two");
      *plan = (int)bn_bwd_pieces(npix);
      break;
    case PNPX_NT_WGRAD_PLAIN:
    case PNPX_NT_WGRAD_WN:
      if (d.cout <= 0 || d.K <= 0 || d.cin <= 0 || d.cout % 32 || d.K % 32) return bad(PNPX_ERR_SHAPE, "cout and K are positive multiples of 32, cin positive");
      if (d.kind < 0 || d.kind > 2) return bad(PNPX_ERR_SHAPE, "kind is 0, 1 or 2");
      if (d.kind == 1 ? (d.Cp <= 0 || d.K != 4 * d.Cp || d.cin > d.Cp) : (d.Cp != 0 || d.cin > d.K))
        return bad(PNPX_ERR_SHAPE, "kind 1: K = 4 Cp and cin <= Cp; kinds 0 and 2: Cp = 0 and cin <= K");
      if (d.Gg < d.cout / 8 || d.Xg < d.K / 8) return bad(PNPX_ERR_SHAPE, "Gg below cout / 8 or Xg below K / 8");
      if (!(d.inv_w != 0.f) || (op == PNPX_NT_WGRAD_WN && !(d.inv_b != 0.f))) return bad(PNPX_ERR_SHAPE, "inv_w / inv_b is zero");
      *plan = critic_wgrad_pieces(d.cout, d.K, d.B, d.h, d.w) + 256 * critic_wgrad_chunks_per_piece(d.cout, d.K, d.B, d.h, d.w);
      break;
    case PNPX_NT_ALPHA_DOT:
      if (d.resG < 0 || d.mG < d.resG || (d.resG == 0) != (d.mG == 0)) return bad(PNPX_ERR_SHAPE, "0 < resG <= mG with a residual, both 0 without");
      break;
    case PNPX_NT_HEAD_GRAD:
      if (d.n_det < 1 || d.n_det > 64 || (d.spi != 0 && d.spi != 1)) return bad(PNPX_ERR_SHAPE, "1 <= n_det <= 64, spi 0 or 1");
      *plan = 2 + head_n1(d) + (d.spi ? d.n_det : 0);
      break;
    case PNPX_NT_GRAD_SEED:
      if (!(d.boost > 0.f) || !pow2_or_zero(d.boost)) return bad(PNPX_ERR_SHAPE, "boost is a positive power of two");
      break;
    default:
      break;
  }
  return PNPX_OK;
}

// operands: each op's own, all of them, and no other
int validate_operands(const pnpx_net_train_probe_desc& d) {
  enum : unsigned {
    Z0 = 1u << 0, Z1 = 1u << 1, GT = 1u << 2, ACT = 1u << 3, RES = 1u << 4, X = 1u << 5, M = 1u << 6, ST0 = 1u << 7, ST1 = 1u << 8, GV = 1u << 9,
    SLOT = 1u << 10, FIN = 1u << 11, FIN2 = 1u << 12, PAR = 1u << 13, DIN = 1u << 14, DIN2 = 1u << 15, ASRC = 1u << 16, OUT = 1u << 17,
    OUT2 = 1u << 18, DY = 1u << 19, GRAD = 1u << 20, COEF = 1u << 21, FOUT = 1u << 22, FOUT2 = 1u << 23, DOUT = 1u << 24, FLAG = 1u << 25
  };
  const void* p[26] = {d.z0,  d.z1,   d.g,    d.act,  d.res,       d.x,   d.m,    d.st0,    d.st1,  d.gv,   d.slot, d.fin,   d.fin2,
                       d.params, d.din, d.din2, d.alpha_src, d.out, d.out2, d.dy_out, d.grad, d.coef, d.fout, d.fout2, d.dout, d.flag};
  unsigned need = 0, may = 0, have = 0;
  for (int i = 0; i < 26; ++i)
    if (p[i]) have |= 1u << i;
  auto together = [&](unsigned bits) { return (have & bits) == 0 || (have & bits) == bits; };
  switch (d.op) {
    case PNPX_NT_BN_STATS: need = Z0 | PAR | FOUT; break;
    case PNPX_NT_BN_APPLY:
      need = Z0 | ST0;
      may = Z1 | ST1 | RES | OUT | OUT2;
      if (!together(Z1 | ST1)) return bad(PNPX_ERR_ARG, "the second summand is z1 and st1, both or neither");
      if (!(have & (OUT | OUT2))) return bad(PNPX_ERR_ARG, "neither out nor out2");
      if ((have & OUT2) && (d.h % 2 || d.w % 2)) return bad(PNPX_ERR_SHAPE, "the space-to-depth copy needs even sizes");
      break;
    case PNPX_NT_BN_BWD:
      need = GT | ACT | Z0 | ST0 | PAR | GRAD | COEF | OUT;
      may = Z1 | ST1 | OUT2 | DY | SLOT | FLAG;
      if (!together(Z1 | ST1 | OUT2)) return bad(PNPX_ERR_ARG, "the second layer is z1, st1 and out2, all or none");
      break;
    case PNPX_NT_WGRAD_PLAIN: need = GT | X | GV | GRAD; break;
    case PNPX_NT_WGRAD_WN: need = GT | X | GV | PAR | GRAD; break;
    case PNPX_NT_CLIP_MASK: need = ACT | OUT; break;
    case PNPX_NT_ALPHA_DOT:
      need = GT | X | DOUT;
      may = RES | M;
      if (!together(RES | M) || ((have & RES) != 0) != (d.resG > 0)) return bad(PNPX_ERR_ARG, "the residual is res, m, resG and mG, all or none");
      break;
    case PNPX_NT_FC_GRAD: need = ACT | GV | FIN | FOUT | DOUT; break;
    case PNPX_NT_ALPHA_FINISH:
      need = ASRC | DIN | DIN2 | GV | GRAD;
      if (d.alpha_src)
        for (int i = 0; i < 21; ++i)
          if (d.alpha_src[i] < -1 || d.alpha_src[i] > 20) return bad(PNPX_ERR_ARG, "alpha_src[i] is -1 or an index below 21");
      break;
    case PNPX_NT_HEAD_GRAD: need = ACT | PAR | FIN | FIN2 | FOUT | GRAD; break;
    default: need = FIN | FOUT | OUT | FOUT2; break;   // GRAD_SEED
  }
  for (int i = 0; i < 26; ++i) {
    const unsigned bit = 1u << i;
    if ((need & bit) && !p[i]) return bad(PNPX_ERR_ARG, "an operand of the op is null");
    if (!((need | may) & bit) && p[i]) return bad(PNPX_ERR_ARG, "an operand the op has no place for");
  }
  return PNPX_OK;
}

// device scratch for the length of one call, filled with NaN (every byte 0xFF) on the call's stream
struct Scratch {
  void* p = nullptr;
  ~Scratch() {
    if (p) (void)hipFree(p);
  }
  int get(size_t bytes, hipStream_t s) {
    PNPX_HIP(hipMalloc(&p, bytes));
    PNPX_HIP(hipMemsetAsync(p, 0xFF, bytes, s));
    return PNPX_OK;
  }
};

// the FORWARD packing descriptor of a convolution from the plain numbers; src_v: where its raw weights start in params / grad
PackDesc wgrad_desc(const pnpx_net_train_probe_desc& d, unsigned src_v) {
  PackDesc D = PackDesc();
  D.src_v = src_v;
  D.rows = d.cout;
  D.K = d.K;
  D.mt = d.cout % 64 == 0 ? 64 : 32;
  D.kind = d.kind;
  D.cin = d.cin;
  D.Cp = d.Cp;
  pack_desc_window(D, pack_kind_window(d.kind));
  D.items = (unsigned)((size_t)D.rows * (D.K / 8) * D.nt);
  return D;
}

int run_wgrad(const pnpx_net_train_probe_desc& d, hipStream_t s, Scratch& slab) {
  const bool wn = d.op == PNPX_NT_WGRAD_WN;
  const PackDesc D = wgrad_desc(d, wn ? 2u * (unsigned)d.cout : 0u);
  const int pieces = critic_wgrad_pieces(d.cout, d.K, d.B, d.h, d.w), fan = wgrad_fan(d);
  PNPX_TRY(slab.get((size_t)pieces * critic_wgrad_piece_floats(d.cout, d.K, D.nt) * sizeof(float), s));
  WgradJob W;
  W.G = static_cast<const HsRec*>(d.g);
  W.X = static_cast<const HsRec*>(d.x);
  W.gv = d.gv;
  W.Gg = d.Gg;
  W.Xg = d.Xg;
  W.cout = d.cout;
  W.K = d.K;
  W.nt = D.nt;
  for (int t = 0; t < D.nt; ++t) W.tap[t] = D.tap[t];
  W.B = d.B;
  W.h = d.h;
  W.w = d.w;
  PNPX_TRY(launch_critic_wgrad(W, static_cast<float*>(slab.p), s));
  if (!wn) return launch_pol_wgrad_finish(D, fan, pieces, d.inv_w, static_cast<const float*>(slab.p), d.grad, s);
  WnGradJob J;
  J.D = D;
  J.src_b = 0;
  J.src_g = (unsigned)d.cout;
  J.fan = fan;
  J.pieces = pieces;
  J.inv_w = d.inv_w;
  J.inv_b = d.inv_b;
  return launch_critic_wn_grad(J, static_cast<const float*>(slab.p), d.params, d.grad, s);
}

int run_bn_bwd(const pnpx_net_train_probe_desc& d, hipStream_t s, Scratch& part, Scratch& slot) {
  const int cout = d.G * 8;
  const long long npix = (long long)d.B * d.h * d.w;
  PNPX_TRY(part.get(bn_bwd_pieces(npix) * (size_t)cout * 3 * sizeof(double), s));
  const float2* sl = reinterpret_cast<const float2*>(d.slot);
  if (!sl) {
    const float one[2] = {1.f, 1.f};
    PNPX_TRY(slot.get(sizeof(one), s));
    PNPX_HIP(hipMemcpyAsync(slot.p, one, sizeof(one), hipMemcpyHostToDevice, s));
    PNPX_HIP(hipStreamSynchronize(s));      // `one` leaves scope
    sl = static_cast<const float2*>(slot.p);
  }
  BnBwdJob J;
  J.g = static_cast<const HsRec*>(d.g);
  J.act = static_cast<const HsRec*>(d.act);
  J.l0.z = static_cast<const HsRec*>(d.z0);
  J.l0.mean = d.st0;
  J.l0.var = d.st0 + cout;
  J.l0.bn = 0;
  J.l0.coef = d.coef;
  J.l0.dz = static_cast<HsRec*>(d.out);
  if (d.z1) {
    J.l1.z = static_cast<const HsRec*>(d.z1);
    J.l1.mean = d.st1;
    J.l1.var = d.st1 + cout;
    J.l1.bn = (size_t)4 * cout;
    J.l1.coef = d.coef + 3 * (size_t)cout;
    J.l1.dz = static_cast<HsRec*>(d.out2);
  }
  J.dy_out = static_cast<HsRec*>(d.dy_out);
  J.G = d.G;
  J.B = d.B;
  J.h = d.h;
  J.w = d.w;
  J.part = static_cast<double*>(part.p);
  J.params = d.params;
  J.grad = d.grad;
  J.slot = sl;
  J.inv_boost = d.boost == 0.f ? 1.f : 1.0f / d.boost;
  J.range_flag = d.flag;
  return launch_bn_bwd(J, s);
}

int run_head_grad(const pnpx_net_train_probe_desc& d, hipStream_t s, Scratch& rows) {
  PNPX_TRY(rows.get((size_t)d.B * POL_HEAD_STRIDE * sizeof(float), s));
  const int n1 = head_n1(d);
  PolHeadGradJob J;
  J.feat = static_cast<const HsRec*>(d.act);
  J.h = d.h;
  J.w = d.w;
  J.B = d.B;
  J.n_det = d.n_det;
  J.spi = d.spi;
  J.sm_w = d.params;
  J.sm_b = J.sm_w + 2 * 512;
  J.d_w = J.sm_b + 2;
  J.d_b = J.d_w + (size_t)n1 * 512;
  if (d.spi) {
    J.d2_w = J.d_b + n1;
    J.d2_b = J.d2_w + (size_t)d.n_det * 64;
  }
  J.gp = d.fin;
  J.gd = d.fin2;
  J.gf = d.fout;
  J.rows = static_cast<float*>(rows.p);
  J.grad = d.grad;
  J.head_src = 0;
  return launch_pol_head_grad(J, s);
}

}  // namespace

extern "C" int pnpx_net_train_probe_plan(const pnpx_net_train_probe_desc* desc) {
  if (!desc) return 0;
  int plan = 0;
  if (validate_sizes(*desc, &plan) != PNPX_OK) return 0;
  return plan;
}

extern "C" int pnpx_net_train_probe(pnpx_ctx* ctx, const pnpx_net_train_probe_desc* desc, void* stream) {
  if (!ctx || !desc) {
    set_error("pnpx_net_train_probe: null context or descriptor");
    return PNPX_ERR_ARG;
  }
  const pnpx_net_train_probe_desc& d = *desc;
  int plan = 0;
  PNPX_TRY(validate_sizes(d, &plan));
  PNPX_TRY(validate_operands(d));
  std::lock_guard<std::mutex> lk(ctx->mu);
  PNPX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto rec = [](const void* p) { return static_cast<const HsRec*>(p); };
  auto wrec = [](void* p) { return static_cast<HsRec*>(p); };
  Scratch sa, sb;
  const int cout = d.G * 8;
  int rc = PNPX_OK;
  switch (d.op) {
    case PNPX_NT_BN_STATS: {
      rc = sa.get(bn_fwd_pieces((long long)d.B * d.h * d.w) * (size_t)cout * 2 * sizeof(double), s);
      if (rc != PNPX_OK) break;
      BnStatsJob J;
      J.z = rec(d.z0);
      J.G = d.G;
      J.B = d.B;
      J.h = d.h;
      J.w = d.w;
      J.part = static_cast<double*>(sa.p);
      J.params = d.params;
      J.bn = 0;
      J.mean = d.fout;
      J.var = d.fout + cout;
      J.scale = d.fout + 2 * (size_t)cout;
      J.shift = d.fout + 3 * (size_t)cout;
      J.momentum = d.momentum;
      J.update = d.update;
      rc = launch_bn_stats(J, s);
      break;
    }
    case PNPX_NT_BN_APPLY: {
      BnApplyJob J;
      J.a = BnSrc{rec(d.z0), d.st0, d.st0 + cout, d.st0 + 2 * (size_t)cout};
      if (d.z1) J.b = BnSrc{rec(d.z1), d.st1, d.st1 + cout, d.st1 + 2 * (size_t)cout};
      J.res = rec(d.res);
      J.out = wrec(d.out);
      J.s2d_hs = wrec(d.out2);
      J.G = d.G;
      J.B = d.B;
      J.h = d.h;
      J.w = d.w;
      rc = launch_bn_apply(J, s);
      break;
    }
    case PNPX_NT_BN_BWD:
      rc = run_bn_bwd(d, s, sa, sb);
      break;
    case PNPX_NT_WGRAD_PLAIN:
    case PNPX_NT_WGRAD_WN:
      rc = run_wgrad(d, s, sa);
      break;
    case PNPX_NT_CLIP_MASK:
      rc = launch_critic_clip_mask(rec(d.act), wrec(d.out), d.thr, d.B, d.G, d.h, d.w, s);
      break;
    case PNPX_NT_ALPHA_DOT:
      rc = launch_critic_alpha_dot(rec(d.g), rec(d.x), d.G, rec(d.res), d.resG, rec(d.m), d.mG, d.B, d.h, d.w, d.dout, s);
      break;
    case PNPX_NT_FC_GRAD:
      rc = launch_critic_fc_grad(rec(d.act), d.gv, d.fin, d.thr, d.B, d.h, d.w, d.fout, d.dout, s);
      break;
    case PNPX_NT_ALPHA_FINISH: {
      AlphaFinishJob J;
      for (int i = 0; i < 21; ++i) J.alpha_src[i] = d.alpha_src[i];
      J.head_src = 21;
      J.fcb_src = 22;
      J.B = d.B;
      J.inv = d.inv_w;
      rc = launch_critic_alpha_finish(J, d.din, d.din2, d.gv, d.grad, s);
      break;
    }
    case PNPX_NT_HEAD_GRAD:
      rc = run_head_grad(d, s, sa);
      break;
    default: {
      rc = sa.get(sizeof(unsigned), s);      // the bits of max |g_f|: the launcher zeroes them itself
      if (rc != PNPX_OK) break;
      rc = launch_pol_grad_seed(d.fin, static_cast<unsigned*>(sa.p), reinterpret_cast<float2*>(d.fout), wrec(d.out), d.fout2, d.boost, d.B, d.h,
                                d.w, s);
      break;
    }
  }
  const hipError_t e = hipStreamSynchronize(s);      // (before the scratch is freed)
  if (rc == PNPX_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(net train probe)", __FILE__, __LINE__);
  return rc;
}
