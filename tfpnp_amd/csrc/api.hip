// C-ABI entry points of libpnpx.so: context, weights, denoiser, generic transforms.  (Solver loops live next to
// their kernels in csmri.hip / tasks.hip.)
#include <climits>
#include <cstring>

#include "common.h"
#include "conv3x3.h"
#include "conv_hs.h"
#include "solver_loop.h"   // LOCK_CTX

namespace pnpx {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  set_error("HIP error %d (%s) at %s:%d in %s", (int)e, hipGetErrorString(e), file, line, what);
  return PNPX_ERR_HIP;
}

int ctx_scratch(pnpx_ctx* ctx, size_t bytes, void** out) {
  if (ctx->scratch.bytes < bytes) {
    PNPX_HIP(hipDeviceSynchronize());
    if (ctx->scratch.p) PNPX_HIP(hipFree(ctx->scratch.p));
    ctx->scratch = DeviceBuf();
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      set_error("scratch allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
      return PNPX_ERR_ALLOC;
    }
    ctx->scratch.p = p;
    ctx->scratch.bytes = bytes;
  }
  *out = ctx->scratch.p;
  return PNPX_OK;
}

int alloc_dev(DeviceBuf& b, size_t bytes, const char* what) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    set_error("%s allocation of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
    return PNPX_ERR_ALLOC;
  }
  b.p = p;
  b.bytes = bytes;
  return PNPX_OK;
}

// UNet(2,1) layer table in state_dict order (tfpnp/pnp/denoiser/models/unet.py:37-46).
struct LayerSpec {
  int cin, cout;
};
static void unet_layers(LayerSpec out[27]) {
  const int blocks[9][2] = {{2, 32},    {32, 64},   {64, 128}, {128, 256}, {256, 512},
                            {768, 256}, {384, 128}, {192, 64}, {96, 32}};
  for (int b = 0; b < 9; ++b)
    for (int j = 0; j < 3; ++j) out[3 * b + j] = LayerSpec{j == 0 ? blocks[b][0] : blocks[b][1], blocks[b][1]};
}

// A DRUNet context answers a tripped guard in steps (r5): the bias-free ReLU network is positively homogeneous, so the
// first two trips move its passes 16x further inside the range each (DruNet::shift 4, then 8: exact up to f16 subnormals, 4e-6 at
// 2^-8); a third trip latches the context to conv_mode 0 like a UNet context (drunet_f32.hip: exact fp32, forward and -- since r5 --
// VJP).  Larger shifts are not used: at 2^-12 the lo halves sit in the f16 subnormals (1e-4 class errors, silently).
// One trip = one step: the device is drained before the flag is cleared, so that kernels of the offending call still in flight
// cannot set it again behind the host's back, and range_guard_enter steps only once per acknowledged trip.
constexpr int DRUNET_MAX_SHIFT = 8;
static int drunet_rescale(pnpx_ctx* ctx) {
  PNPX_HIP(hipDeviceSynchronize());
  if (ctx->drunet.shift < DRUNET_MAX_SHIFT) ctx->drunet.shift += 4;
  else ctx->conv_mode = CONV_F32;
  *ctx->range_flag_host = 0;
  return PNPX_OK;
}

void range_guard_enter(pnpx_ctx* ctx) {
  if (!ctx->opt_range_guard || !ctx->range_flag_host) return;
  if (*static_cast<volatile unsigned*>(ctx->range_flag_host) == 0 || ctx->range_tripped) return;
  ctx->range_tripped = true;          // an EARLIER call overflowed: its output was invalid (pnpx_ctx_status reports it)
  // later calls: 16x further inside the range / exact.  ADVICE r5: if the rescale step itself fails (its device synchronisation
  // returned an error) neither the shift nor the flag clear happened and, the trip being latched, no later call would step either:
  // fall back to the exact family right away so that nothing invalid is produced from here on (the HIP error resurfaces at the
  // call's own first launch).
  if (ctx->drunet.loaded && ctx->conv_mode == CONV_HS) {
    if (drunet_rescale(ctx) != PNPX_OK) ctx->conv_mode = CONV_F32;
  } else ctx->conv_mode = CONV_F32;     // every later call is exact
}

int range_guard_strict(pnpx_ctx* ctx, hipStream_t s, bool* rerun) {
  *rerun = false;
  PNPX_HIP(hipStreamSynchronize(s));
  if (*static_cast<volatile unsigned*>(ctx->range_flag_host) == 0) return PNPX_OK;
  if (ctx->conv_mode != CONV_HS || ctx->range_tripped) {
    // nothing left to fall back to (the flag was set although the exact family ran, or an unacknowledged trip is pending): strict
    // mode's contract is that nothing invalid leaves the call as a success
    set_error("half-split range guard: the call's result is invalid and no fallback is left (conv_mode %d)", ctx->conv_mode);
    return PNPX_ERR_RANGE;
  }
  if (ctx->drunet.loaded) PNPX_TRY(drunet_rescale(ctx));   // this call is repeated 16x further inside the range (or in exact fp32) before it returns
  else {
    ctx->conv_mode = CONV_F32;        // this call is repeated in exact fp32 before it returns: nothing invalid escapes
    *ctx->range_flag_host = 0;
  }
  *rerun = true;
  return PNPX_OK;
}

}  // namespace pnpx

using namespace pnpx;

extern "C" {

const char* pnpx_version(void) { return "pnpx 0.1 (gfx950)"; }
const char* pnpx_last_error(void) { return g_err.c_str(); }

int pnpx_ctx_create(int device, pnpx_ctx** out) {
  if (!out) {
    set_error("pnpx_ctx_create: null out");
    return PNPX_ERR_ARG;
  }
  int n = 0;
  PNPX_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) {
    set_error("pnpx_ctx_create: device %d out of range (%d visible)", device, n);
    return PNPX_ERR_ARG;
  }
  PNPX_HIP(hipSetDevice(device));
  pnpx_ctx* c = new pnpx_ctx();
  c->device = device;
  // range-guard word: pinned, host-mapped, written by the device only in the (rare) overflow branch
  void* h = nullptr;
  hipError_t e = hipHostMalloc(&h, 64, hipHostMallocMapped);
  if (e != hipSuccess) {
    delete c;
    return hip_fail(e, "hipHostMalloc(range flag)", __FILE__, __LINE__);
  }
  c->range_flag_host = static_cast<unsigned*>(h);
  *c->range_flag_host = 0;
  void* d = nullptr;
  e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(h);
    delete c;
    return hip_fail(e, "hipHostGetDevicePointer(range flag)", __FILE__, __LINE__);
  }
  c->range_flag_dev = static_cast<unsigned*>(d);
  *out = c;
  return PNPX_OK;
}

int pnpx_ctx_destroy(pnpx_ctx* ctx) {
  if (!ctx) return PNPX_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  if (ctx->weights.p) (void)hipFree(ctx->weights.p);
  for (pnpx::UNetArena* a : {&ctx->arena, &ctx->arena_grad})
    if (a->buf.p) (void)hipFree(a->buf.p);
  policy_free(ctx);
  pnpx::critic_free(ctx);
  pnpx::drunet_free(ctx);
  pnpx::train_cache_free(ctx);
  if (ctx->scratch.p) (void)hipFree(ctx->scratch.p);
  for (auto& t : ctx->twiddle)
    if (t.second) (void)hipFree(t.second);
  for (auto e : ctx->events) (void)hipEventDestroy(e);
  if (ctx->range_flag_host) (void)hipHostFree(ctx->range_flag_host);
  for (hipStream_t st : ctx->side_streams) (void)hipStreamDestroy(st);
  for (hipEvent_t ev : ctx->ev_pool) (void)hipEventDestroy(ev);
  delete ctx;
  return PNPX_OK;
}

size_t pnpx_policy_num_params(int num_inputs, int n_det, int spi_head) {
  return policy_num_params(num_inputs, n_det, spi_head);
}

int pnpx_policy_load(pnpx_ctx* ctx, const float* params_host, size_t n_params, int num_inputs, int n_det,
                     int spi_head) {
  LOCK_CTX(ctx);
  return policy_load(ctx, params_host, n_params, num_inputs, n_det, spi_head);
}

int pnpx_policy_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n_params, int num_inputs, int n_det, int spi_head,
                            void* stream) {
  LOCK_CTX(ctx);
  return policy_load_device(ctx, params_dev, n_params, num_inputs, n_det, spi_head, static_cast<hipStream_t>(stream));
}

int pnpx_policy_params(pnpx_ctx* ctx, float* dst_dev, size_t n_params, void* stream) {
  LOCK_CTX(ctx);
  return policy_params(ctx, dst_dev, n_params, static_cast<hipStream_t>(stream));
}

int pnpx_policy_forward(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W,
                        void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !probs || !det) {
    set_error("pnpx_policy_forward: null pointer");
    return PNPX_ERR_ARG;
  }
  return policy_forward(ctx, ob, probs, det, B, H, W, static_cast<hipStream_t>(stream));
}

int pnpx_policy_forward_train(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                              int update_running, void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !probs || !det) {
    set_error("pnpx_policy_forward_train: null pointer");
    return PNPX_ERR_ARG;
  }
  return policy_forward_train(ctx, ob, probs, det, B, H, W, momentum, update_running, static_cast<hipStream_t>(stream));
}

int pnpx_policy_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_probs, const float* grad_det, float* grad_params,
                           size_t n_params, int B, int H, int W, void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !grad_probs || !grad_det || !grad_params) {
    set_error("pnpx_policy_param_grad: null pointer");
    return PNPX_ERR_ARG;
  }
  return policy_param_grad(ctx, ob, grad_probs, grad_det, grad_params, n_params, B, H, W, static_cast<hipStream_t>(stream));
}

int pnpx_policy_forward_train_keep(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                                   int update_running, void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !probs || !det) {
    set_error("pnpx_policy_forward_train_keep: null pointer");
    return PNPX_ERR_ARG;
  }
  return policy_forward_train_keep(ctx, ob, probs, det, B, H, W, momentum, update_running, static_cast<hipStream_t>(stream));
}

int pnpx_policy_param_grad_kept(pnpx_ctx* ctx, const float* grad_probs, const float* grad_det, float* grad_params, size_t n_params,
                                void* stream) {
  LOCK_CTX(ctx);
  if (!grad_probs || !grad_det || !grad_params) {
    set_error("pnpx_policy_param_grad_kept: null pointer");
    return PNPX_ERR_ARG;
  }
  return policy_param_grad_kept(ctx, grad_probs, grad_det, grad_params, n_params, static_cast<hipStream_t>(stream));
}

int pnpx_policy_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n_params, float lr, float beta1, float beta2, float eps,
                          float max_norm, float* grad_norm_dev, void* stream) {
  LOCK_CTX(ctx);
  return policy_adam_step(ctx, grad_dev, n_params, lr, beta1, beta2, eps, max_norm, grad_norm_dev, static_cast<hipStream_t>(stream));
}

int pnpx_policy_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n_params, long long* step_host,
                            void* stream) {
  LOCK_CTX(ctx);
  return policy_optim_state(ctx, exp_avg_dst, exp_avg_sq_dst, n_params, step_host, static_cast<hipStream_t>(stream));
}

int pnpx_policy_optim_reset(pnpx_ctx* ctx) {
  LOCK_CTX(ctx);
  return policy_optim_reset(ctx);
}

int pnpx_policy_frozen_ranges(int num_inputs, int n_det, int spi_head, size_t* first, size_t* count, int capacity) {
  if (num_inputs < 1 || num_inputs > 64 || n_det < 1 || n_det > 64) return -1;
  FrozenRange r[LIVE_OPTIM_MAX_FROZEN];
  int n = 0;
  if (policy_frozen_ranges(num_inputs, n_det, spi_head, r, &n) != PNPX_OK) return -1;
  for (int i = 0; i < n && i < capacity && first && count; ++i) {
    first[i] = r[i].first;
    count[i] = r[i].count;
  }
  return n;
}

size_t pnpx_policy_num_bn_channels(void) { return POLICY_BN_CHANNELS; }

int pnpx_policy_bn_stats(pnpx_ctx* ctx, float* mean_dev, float* var_dev, size_t n, void* stream) {
  LOCK_CTX(ctx);
  return policy_bn_stats(ctx, mean_dev, var_dev, n, static_cast<hipStream_t>(stream));
}

size_t pnpx_critic_num_params(int num_inputs) {
  return (num_inputs >= 1 && num_inputs <= 64) ? critic_num_params(num_inputs) : 0;
}

int pnpx_critic_load(pnpx_ctx* ctx, const float* params_host, size_t n_params, int num_inputs) {
  LOCK_CTX(ctx);
  return critic_load(ctx, params_host, n_params, num_inputs);
}

int pnpx_critic_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n_params, int num_inputs, void* stream) {
  LOCK_CTX(ctx);
  return critic_load_device(ctx, params_dev, n_params, num_inputs, static_cast<hipStream_t>(stream));
}

int pnpx_critic_soft_update(pnpx_ctx* ctx, const float* src_params_dev, size_t n_params, float one_minus_tau, float tau,
                            void* stream) {
  LOCK_CTX(ctx);
  return critic_soft_update(ctx, src_params_dev, n_params, one_minus_tau, tau, static_cast<hipStream_t>(stream));
}

int pnpx_critic_params(pnpx_ctx* ctx, float* dst_dev, size_t n_params, void* stream) {
  LOCK_CTX(ctx);
  return critic_params(ctx, dst_dev, n_params, static_cast<hipStream_t>(stream));
}

int pnpx_critic_forward(pnpx_ctx* ctx, const float* ob, float* value, int B, int H, int W, void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !value) {
    set_error("pnpx_critic_forward: null pointer");
    return PNPX_ERR_ARG;
  }
  return critic_forward(ctx, ob, value, B, H, W, static_cast<hipStream_t>(stream));
}

int pnpx_critic_backward(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_ob, int B, int H, int W,
                         void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !grad_value || !grad_ob) {
    set_error("pnpx_critic_backward: null pointer");
    return PNPX_ERR_ARG;
  }
  return critic_backward(ctx, ob, grad_value, grad_ob, B, H, W, static_cast<hipStream_t>(stream));
}

int pnpx_critic_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_params, size_t n_params, int B, int H,
                           int W, void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !grad_value || !grad_params) {
    set_error("pnpx_critic_param_grad: null pointer");
    return PNPX_ERR_ARG;
  }
  return critic_param_grad(ctx, ob, grad_value, grad_params, n_params, B, H, W, static_cast<hipStream_t>(stream));
}

int pnpx_critic_value_loss_grad(pnpx_ctx* ctx, const float* ob, const float* q_target, float* value, float* loss, float* grad_params,
                                size_t n_params, int B, int H, int W, void* stream) {
  LOCK_CTX(ctx);
  if (!ob || !q_target || !value || !loss || !grad_params) {
    set_error("pnpx_critic_value_loss_grad: null pointer");
    return PNPX_ERR_ARG;
  }
  return critic_value_loss_grad(ctx, ob, q_target, value, loss, grad_params, n_params, B, H, W, static_cast<hipStream_t>(stream));
}

int pnpx_critic_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n_params, float lr, float beta1, float beta2, float eps,
                          float max_norm, float* grad_norm_dev, void* stream) {
  LOCK_CTX(ctx);
  return critic_adam_step(ctx, grad_dev, n_params, lr, beta1, beta2, eps, max_norm, grad_norm_dev, static_cast<hipStream_t>(stream));
}

int pnpx_critic_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n_params, long long* step_host,
                            void* stream) {
  LOCK_CTX(ctx);
  return critic_optim_state(ctx, exp_avg_dst, exp_avg_sq_dst, n_params, step_host, static_cast<hipStream_t>(stream));
}

int pnpx_critic_optim_reset(pnpx_ctx* ctx) {
  LOCK_CTX(ctx);
  return critic_optim_reset(ctx);
}

int pnpx_mddpg_policy_loss(pnpx_ctx* ctx, const float* p_stop, const int64_t* idx_stop, const float* v_cur, const float* v_next_target,
                           const float* v_next, const float* reward, float discount, float loop_penalty, float lambda_e, int B,
                           float* q_target, float* log_prob, float* entropy, float* scalars, float* grad_p_stop, float* grad_v_next,
                           float* grad_reward, void* stream) {
  LOCK_CTX(ctx);
  return mddpg_policy_loss(p_stop, reinterpret_cast<const long long*>(idx_stop), v_cur, v_next_target, v_next, reward, discount,
                           loop_penalty, lambda_e, B, q_target, log_prob, entropy, scalars, grad_p_stop, grad_v_next, grad_reward,
                           static_cast<hipStream_t>(stream));
}

int pnpx_ctx_reserve(pnpx_ctx* ctx, int B, int H, int W) {
  LOCK_CTX(ctx);
  if (B <= 0 || H < 16 || W < 16) {
    set_error("pnpx_ctx_reserve: need B > 0 and H, W >= 16");
    return PNPX_ERR_SHAPE;
  }
  return ctx_reserve_unet(ctx, B, H, W);
}

// The plain integer options: a field of the context and its accepted range, read by pnpx_ctx_set_option and pnpx_ctx_get_option alike
// (include/pnpx.h describes each).  Options with a side effect or another rule are explicit cases of the two functions.
namespace {
struct PlainOption {
  const char* name;
  int pnpx_ctx::*field;
  int lo, hi;
};
const PlainOption PLAIN_OPTIONS[] = {
    {"conv_mode", &pnpx_ctx::conv_mode, CONV_F32, CONV_HS},
    {"subbatch", &pnpx_ctx::opt_subbatch, 0, INT_MAX},
    {"fuse_pool", &pnpx_ctx::opt_fuse_pool, 0, 1},
    {"fuse_outc", &pnpx_ctx::opt_fuse_outc, 0, 1},
    {"fuse_first", &pnpx_ctx::opt_fuse_first, 0, 1},
    {"fold_first", &pnpx_ctx::opt_fold_first, 0, 1},
    {"fft_tile", &pnpx_ctx::opt_fft_tile, 0, 8192},
    {"fft_fast", &pnpx_ctx::opt_fft_fast, 0, 1},
    {"fft_affine", &pnpx_ctx::opt_fft_affine, 0, 1},
    {"chains", &pnpx_ctx::opt_chains, 0, 8},
    {"wreg", &pnpx_ctx::opt_wreg, 0, 2},
    {"fuse_up", &pnpx_ctx::opt_fuse_up, 0, 2},
    {"fp32_winograd", &pnpx_ctx::opt_fp32_winograd, 0, 1},
    {"fp32_chains", &pnpx_ctx::opt_fp32_chains, 0, 8},
    {"fp32_fuse_up", &pnpx_ctx::opt_fp32_fuse_up, 0, 1},
    {"fp32_ksplit", &pnpx_ctx::opt_fp32_ksplit, 0, 2},
    {"fp32_ksplit_rule", &pnpx_ctx::opt_ksplit_rule, 1, 255},      // tuning: 1 the default rule, else pieces per tile class (conv3x3_wino8_ksplit)
    {"fp32_wino8_layers", &pnpx_ctx::opt_fp32_wino8, 0, (1 << 27) - 1},      // bit li: layer li on the 8-wave Winograd kernel
    {"fp32_winof4_layers", &pnpx_ctx::opt_fp32_winof4, 0, (1 << 27) - 1},    // bit li: layer li on the F(4x4,3x3) kernel (forward passes)
    {"fp32_winof4_entries", &pnpx_ctx::opt_fp32_winof4_entries, 0, (1 << 27) - 1},      // bits 15, 18, 21: that decoder entry on it
    {"fp32_winof4_fuse_up", &pnpx_ctx::opt_fp32_winof4_fuse_up, 0, (1 << 27) - 1},      // bits 15, 18, 21: ... up-sampling its second source itself
};
constexpr int WINOF4_C32_BITS = (1 << 1) | (1 << 2) | (1 << 25);      // the layers the 32-cout F(4x4,3x3) weights are packed for
const PlainOption* plain_option(const char* key) {
  for (const PlainOption& o : PLAIN_OPTIONS)
    if (key && !std::strcmp(key, o.name)) return &o;
  return nullptr;
}
}  // namespace

int pnpx_ctx_set_option(pnpx_ctx* ctx, const char* key, int value) {
  LOCK_CTX(ctx);
  auto is = [&](const char* k) { return key && !std::strcmp(key, k); };
  if (const PlainOption* o = plain_option(key)) {
    if (value >= o->lo && value <= o->hi) {
      ctx->*(o->field) = value;
      return PNPX_OK;
    }
  }
  if (is("fp32_winof4_c32") && value >= 0 && (value & ~WINOF4_C32_BITS) == 0) {   // bits 1, 2, 25: that layer on the 32-cout F(4x4,3x3) instance
    ctx->opt_fp32_winof4_c32 = value;
    return PNPX_OK;
  }
  if (is("drunet_shift") && value >= 0 && value <= 8 && (value & 3) == 0) {   // DRUNet passes run on inputs scaled by 2^-value
    ctx->drunet.shift = value;                                                 // (raised by 4 whenever the range guard trips)
    return PNPX_OK;
  }
  if (is("policy_s2_hs") && (value == 0 || value == 1)) return PNPX_OK;   // accepted, without effect (include/pnpx.h)
  if (is("range_guard") && value >= 0 && value <= 2) {   // also re-arms a tripped guard
    PNPX_HIP(hipDeviceSynchronize());
    ctx->opt_range_guard = value;
    ctx->range_tripped = false;
    *ctx->range_flag_host = 0;
    return PNPX_OK;
  }
  if (is("train_cache_gb") && value >= -1) {   // -1 = automatic budget; shrinking to 0 also releases what is held
    ctx->opt_train_cache_gb = value;
    ctx->train_alloc_failed = false;
    ctx->train_budget_bytes = 0;
    if (value == 0) pnpx::train_cache_free(ctx);
    return PNPX_OK;
  }
  if (is("train_cache_release")) {   // give the ring's memory back now (budget unchanged; it re-grows on the next
    pnpx::train_cache_free(ctx);     // forward under autograd).  Outstanding tickets fall back to re-computation.
    ctx->train_alloc_failed = false;
    ctx->train_budget_bytes = 0;
    return PNPX_OK;
  }
  set_error("pnpx_ctx_set_option: unknown option '%s' or bad value %d", key ? key : "(null)", value);
  return PNPX_ERR_ARG;
}

int pnpx_ctx_get_option(pnpx_ctx* ctx, const char* key, int* value) {
  LOCK_CTX(ctx);
  auto is = [&](const char* k) { return key && !std::strcmp(key, k); };
  if (!value) {
    set_error("pnpx_ctx_get_option: null value pointer");
    return PNPX_ERR_ARG;
  }
  if (const PlainOption* o = plain_option(key)) *value = ctx->*(o->field);
  else if (is("fp32_winof4_c32")) *value = ctx->opt_fp32_winof4_c32;
  else if (is("drunet_shift")) *value = ctx->drunet.shift;
  else if (is("policy_s2_hs")) *value = 1;
  else if (is("range_guard")) *value = ctx->opt_range_guard;
  else if (is("train_cache_gb")) *value = ctx->opt_train_cache_gb;
  else {
    set_error("pnpx_ctx_get_option: unknown option '%s'", key ? key : "(null)");
    return PNPX_ERR_ARG;
  }
  return PNPX_OK;
}

int pnpx_ctx_status(pnpx_ctx* ctx) {
  LOCK_CTX(ctx);
  range_guard_enter(ctx);
  if (ctx->range_tripped) {
    if (ctx->drunet.loaded)
      set_error("half-split range guard tripped: an activation of an earlier DRUNet call left the f16 hi/lo range (|v| >= 4095 "
                "or NaN); that call's output is invalid.  The context now runs %s (the bias-free network is positively "
                "homogeneous: inputs scaled by 2^-%d, the tail multiplies back; a trip at 2^-8 selects exact fp32); acknowledge "
                "with pnpx_ctx_set_option(ctx, \"range_guard\", 1)", ctx->conv_mode == CONV_HS ? "re-scaled passes" : "conv_mode 0",
                ctx->drunet.shift);
    else
    set_error("half-split range guard tripped: an activation of an earlier call left the f16 hi/lo range (|v| >= 4095 or "
              "NaN); that call's output is invalid.  The context now runs conv_mode 0 (exact fp32 MFMA); re-arm with "
              "pnpx_ctx_set_option(ctx, \"range_guard\", 1)");
    return PNPX_ERR_RANGE;
  }
  return PNPX_OK;
}

size_t pnpx_ctx_bytes(const pnpx_ctx* ctx) {
  if (!ctx) return 0;
  size_t n = ctx->weights.bytes + ctx->arena.buf.bytes + ctx->arena_grad.buf.bytes + ctx->scratch.bytes +
             ctx->drunet.weights.bytes + ctx->drunet.arena.buf.bytes + ctx->drunet.arena_grad.buf.bytes + ctx->drunet.f32.weights.bytes +
             ctx->drunet.f32_arena.buf.bytes + ctx->drunet.f32_bwd.weights.bytes + ctx->drunet.f32_arena_grad.buf.bytes +
             ctx->policy.weights.bytes + ctx->policy.arena.bytes + ctx->policy.live.master.bytes + ctx->policy.pack_ws.ws.bytes + ctx->policy.raw.weights.bytes + ctx->policy.raw_ws.ws.bytes +
             ctx->policy.train_ws.bytes + ctx->policy.bn_buf.bytes + ctx->policy.optim.state.bytes + ctx->critic.weights.bytes + ctx->critic.arena.bytes +
             ctx->critic.live.master.bytes + ctx->critic.pack_ws.ws.bytes + ctx->critic.optim.state.bytes;
  for (const auto& sl : ctx->train_ring) n += sl.arena.buf.bytes + sl.pre.bytes;
  return n;
}

size_t pnpx_unet_num_params(void) {
  LayerSpec L[27];
  unet_layers(L);
  size_t n = 0;
  for (int i = 0; i < 27; ++i) n += (size_t)L[i].cin * L[i].cout * 9 + L[i].cout;
  return n + 32 + 1;
}

size_t pnpx_drunet_num_params(int nb) { return (nb >= 1 && nb <= 8) ? pnpx::drunet_num_params(nb) : 0; }

int pnpx_drunet_load(pnpx_ctx* ctx, const float* params_host, size_t n_params, int nb) {
  LOCK_CTX(ctx);
  return pnpx::drunet_load(ctx, params_host, n_params, nb);
}

int pnpx_unet_load(pnpx_ctx* ctx, const float* params_host, size_t n_params) {
  LOCK_CTX(ctx);
  pnpx::drunet_free(ctx);   // a context holds ONE denoiser
  if (!params_host || n_params != pnpx_unet_num_params()) {
    set_error("pnpx_unet_load: expected %zu parameters, got %zu", pnpx_unet_num_params(), n_params);
    return PNPX_ERR_ARG;
  }
  LayerSpec L[27];
  unet_layers(L);
  // device blob: packed conv weights (each 256-float aligned) + biases + outc, + slack for DMA over-read
  std::vector<float> host;
  size_t woff[27], boff[27];
  auto align = [&]() { host.resize((host.size() + 255) & ~(size_t)255, 0.f); };
  const float* src = params_host;
  for (int i = 0; i < 27; ++i) {
    const int mt = conv_pack_mt(L[i].cout), cc = conv_pack_cc(L[i].cin);
    align();
    woff[i] = host.size();
    host.resize(host.size() + (size_t)L[i].cin * L[i].cout * 9);
    pack_conv_weights(src, L[i].cout, L[i].cin, mt, cc, host.data() + woff[i]);
    src += (size_t)L[i].cin * L[i].cout * 9;
    align();
    boff[i] = host.size();
    host.insert(host.end(), src, src + L[i].cout);
    src += L[i].cout;
    ctx->conv[i].cin = L[i].cin;
    ctx->conv[i].cout = L[i].cout;
    ctx->conv[i].mt = mt;
    ctx->conv[i].cc = cc;
  }
  // Winograd F(2x2,3x3) transformed weights for the fp32 family (conv3x3_wino.hip), layers conv3x3_wino_packs() accepts
  size_t uoff[27];
  {
    const float* wsrc = params_host;
    for (int i = 0; i < 27; ++i) {
      uoff[i] = 0;
      if (conv3x3_wino_packs(L[i].cout, L[i].cin)) {
        align();
        uoff[i] = host.size();
        host.resize(host.size() + conv3x3_wino_floats(L[i].cout, L[i].cin));
        pack_conv_weights_wino(wsrc, L[i].cout, L[i].cin, host.data() + uoff[i]);
      }
      wsrc += (size_t)L[i].cin * L[i].cout * 9 + L[i].cout;
    }
  }
  // half-split (f16 hi/lo) packing of the same convolutions for conv_hs.hip
  size_t hoff[27];
  float hscale[27];
  for (int i = 0; i < 27; ++i) {
    const int mt = conv_hs_mt(L[i].cout);
    const int cin_pad = (L[i].cin + 15) / 16 * 16;
    align();
    hoff[i] = host.size();
    const size_t n16 = (size_t)L[i].cout * cin_pad * 9 * 2;       // f16 elements (hi + lo)
    host.resize(host.size() + (n16 + 1) / 2, 0.f);
    const float* wsrc = params_host;
    for (int k = 0; k < i; ++k) wsrc += (size_t)L[k].cin * L[k].cout * 9 + L[k].cout;
    hscale[i] = pack_conv_weights_hs(wsrc, L[i].cout, L[i].cin, mt, reinterpret_cast<uint16_t*>(host.data() + hoff[i]));
    ctx->conv_hs[i].cin = L[i].cin;
    ctx->conv_hs[i].cout = L[i].cout;
    ctx->conv_hs[i].cin_pad = cin_pad;
    ctx->conv_hs[i].mt = mt;
    ctx->conv_hs[i].inv_scale = 1.0f / (hscale[i] * HS_ASCALE);
  }
  // adjoint (input-gradient) convolutions for the backward pass: transposed, tap-flipped, fp32 kernel family
  size_t toff[27];
  for (int i = 0; i < 27; ++i) {
    const int cout_pad = (L[i].cin + 31) / 32 * 32;            // adjoint output channels = forward input channels
    const int mt = (cout_pad % 64 == 0) ? 64 : 32;
    align();
    toff[i] = host.size();
    host.resize(host.size() + (size_t)cout_pad * L[i].cout * 9);
    const float* wsrc = params_host;
    for (int k = 0; k < i; ++k) wsrc += (size_t)L[k].cin * L[k].cout * 9 + L[k].cout;
    pack_conv_weights_transposed(wsrc, L[i].cout, L[i].cin, cout_pad, mt, 8, host.data() + toff[i]);
    ctx->conv_bwd[i].cin = L[i].cout;
    ctx->conv_bwd[i].cout = cout_pad;
    ctx->conv_bwd[i].mt = mt;
    ctx->conv_bwd[i].cc = 8;
  }
  // ... and the same adjoint convolutions for the half-split kernel family (backward pass of conv_mode 1)
  // Winograd F(4x4,3x3) weights (conv3x3_winof4.hip) for the layers that can be eligible: the plain single-source 64-cout-tile layers of
  // levels 1-3 (2.25 x the F(2x2) bytes, so not for the 16 x 16 level, whose layers the kernel is not used on) and the decoder entries
  // of the same levels (15, 18, 21: packed over both sources' channels; 28 MB for layer 15)
  size_t u4off[27];
  {
    const float* wsrc = params_host;
    for (int i = 0; i < 27; ++i) {
      u4off[i] = 0;
      const bool plain = (i >= 3 && i <= 11) || i == 16 || i == 17 || i == 19 || i == 20 || i == 22 || i == 23;
      const bool entry = i == 15 || i == 18 || i == 21;
      if ((plain || entry) && conv3x3_winof4_packs(L[i].cout, L[i].cin)) {
        align();
        u4off[i] = host.size();
        host.resize(host.size() + conv3x3_winof4_floats(L[i].cout, L[i].cin));
        pack_conv_weights_winof4(wsrc, L[i].cout, L[i].cin, host.data() + u4off[i]);
      }
      wsrc += (size_t)L[i].cin * L[i].cout * 9 + L[i].cout;
    }
  }
  // ... and in the 32-cout instance's layout for the full-resolution 32 -> 32 layers (1, 2, 25: 36 * 32 * 32 floats each)
  size_t u4c32off[27];
  {
    const float* wsrc = params_host;
    for (int i = 0; i < 27; ++i) {
      u4c32off[i] = 0;
      if (((WINOF4_C32_BITS >> i) & 1) && conv3x3_winof4_c32_packs(L[i].cout, L[i].cin)) {
        align();
        u4c32off[i] = host.size();
        host.resize(host.size() + conv3x3_winof4_floats(L[i].cout, L[i].cin));
        pack_conv_weights_winof4_c32(wsrc, L[i].cout, L[i].cin, host.data() + u4c32off[i]);
      }
      wsrc += (size_t)L[i].cin * L[i].cout * 9 + L[i].cout;
    }
  }
  size_t thoff[27], tuoff[27];      // tuoff: the same adjoint layers as Winograd weights of the fp32 family (conv3x3_wino8.hip, r5)
  float thscale[27];
  {
    std::vector<float> wt;
    for (int i = 0; i < 27; ++i) {
      const int cin_t = L[i].cout;                                 // adjoint input channels (multiple of 32)
      const int cout_t = (L[i].cin + 31) / 32 * 32;                // adjoint output channels, zero-padded
      const int mt = (cout_t % 64 == 0) ? 64 : 32;
      const float* wsrc = params_host;
      for (int k = 0; k < i; ++k) wsrc += (size_t)L[k].cin * L[k].cout * 9 + L[k].cout;
      transpose_flip_conv_weights(wsrc, L[i].cout, L[i].cin, cout_t, wt);
      align();
      thoff[i] = host.size();
      const size_t n16 = (size_t)cout_t * cin_t * 9 * 2;
      host.resize(host.size() + (n16 + 1) / 2, 0.f);
      thscale[i] = pack_conv_weights_hs(wt.data(), cout_t, cin_t, mt, reinterpret_cast<uint16_t*>(host.data() + thoff[i]));
      tuoff[i] = 0;
      if (conv3x3_wino_packs(cout_t, cin_t)) {
        align();
        tuoff[i] = host.size();
        host.resize(host.size() + conv3x3_wino_floats(cout_t, cin_t));
        pack_conv_weights_wino(wt.data(), cout_t, cin_t, host.data() + tuoff[i]);
      }
      ctx->conv_hs_bwd[i].cin = cin_t;
      ctx->conv_hs_bwd[i].cout = cout_t;
      ctx->conv_hs_bwd[i].cin_pad = cin_t;
      ctx->conv_hs_bwd[i].mt = mt;
      ctx->conv_hs_bwd[i].inv_scale = 1.0f / (thscale[i] * HS_ASCALE);
    }
  }
  align();
  const size_t oc0 = host.size();          // first convolution, native [32][2][3][3] layout
  host.insert(host.end(), params_host, params_host + 32 * 2 * 9);
  align();
  const size_t ozero = host.size();
  host.resize(host.size() + 768, 0.f);
  align();
  const size_t ow = host.size();
  host.insert(host.end(), src, src + 32);
  src += 32;
  align();
  const size_t ob = host.size();
  host.push_back(*src);
  host.resize(host.size() + 1024, 0.f);  // slack: the last weight block's 16-byte DMA may over-read
  PNPX_HIP(hipDeviceSynchronize());
  if (ctx->weights.p) PNPX_HIP(hipFree(ctx->weights.p));
  ctx->weights = DeviceBuf();
  ctx->has_weights = false;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, host.size() * sizeof(float));
  if (e != hipSuccess) {
    set_error("weight allocation of %zu bytes failed: %s", host.size() * sizeof(float), hipGetErrorString(e));
    return PNPX_ERR_ALLOC;
  }
  PNPX_HIP(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  float* d = static_cast<float*>(p);
  for (int i = 0; i < 27; ++i) {
    ctx->conv[i].w = d + woff[i];
    ctx->conv[i].b = d + boff[i];
    ctx->conv_wino_u[i] = uoff[i] ? d + uoff[i] : nullptr;
    ctx->conv_wino_u_bwd[i] = tuoff[i] ? d + tuoff[i] : nullptr;
    ctx->conv_winof4_u[i] = u4off[i] ? d + u4off[i] : nullptr;
    ctx->conv_winof4_c32_u[i] = u4c32off[i] ? d + u4c32off[i] : nullptr;
    ctx->conv_hs[i].w = reinterpret_cast<char*>(d + hoff[i]);
    ctx->conv_bwd[i].w = d + toff[i];
    ctx->conv_bwd[i].b = nullptr;
    ctx->conv_hs_bwd[i].w = reinterpret_cast<char*>(d + thoff[i]);
  }
  ctx->conv0_w = d + oc0;
  ctx->zero_bias = d + ozero;
  ctx->outc_w = d + ow;
  ctx->outc_b = d + ob;
  ctx->weights.p = p;
  ctx->weights.bytes = host.size() * sizeof(float);
  ctx->has_weights = true;
  pnpx::train_cache_free(ctx);   // activations parked by training forwards belong to the previous weights
  return PNPX_OK;
}

int pnpx_unet_denoise(pnpx_ctx* ctx, const float* x, const float* sigma, float* out, float* out_preclamp, int B,
                      int H, int W, void* stream) {
  LOCK_CTX(ctx);
  return pnpx::guarded(ctx, static_cast<hipStream_t>(stream), [&]() -> int {
  if (!x || !sigma || !out) {
    set_error("pnpx_unet_denoise: null pointer");
    return PNPX_ERR_ARG;
  }
  return unet_denoise(ctx, x, sigma, 1, out, out_preclamp, B, H, W, static_cast<hipStream_t>(stream), nullptr);
  });
}

int pnpx_unet_denoise_backward(pnpx_ctx* ctx, const float* x, const float* sigma, const float* grad_out, float* grad_x,
                               float* grad_sigma, int B, int H, int W, void* stream) {
  LOCK_CTX(ctx);
  return pnpx::guarded(ctx, static_cast<hipStream_t>(stream), [&]() -> int {
  if (!x || !sigma || !grad_out || !grad_x || !grad_sigma) {
    set_error("pnpx_unet_denoise_backward: null pointer");
    return PNPX_ERR_ARG;
  }
  return unet_denoise_backward(ctx, x, sigma, 1, grad_out, grad_x, grad_sigma, B, H, W, static_cast<hipStream_t>(stream));
  });
}

int pnpx_unet_denoise_train(pnpx_ctx* ctx, const float* x, const float* sigma, float* out, int B, int H, int W,
                            unsigned long long* ticket, void* stream) {
  LOCK_CTX(ctx);
  return pnpx::guarded(ctx, static_cast<hipStream_t>(stream), [&]() -> int {
    if (!x || !sigma || !out || !ticket) {
      set_error("pnpx_unet_denoise_train: null pointer");
      return PNPX_ERR_ARG;
    }
    return unet_denoise_train(ctx, x, sigma, 1, out, B, H, W, static_cast<hipStream_t>(stream), ticket);
  });
}

int pnpx_unet_denoise_backward_ticket(pnpx_ctx* ctx, const float* x, const float* sigma, const float* grad_out,
                                      float* grad_x, float* grad_sigma, int B, int H, int W, unsigned long long ticket,
                                      void* stream) {
  LOCK_CTX(ctx);
  return pnpx::guarded(ctx, static_cast<hipStream_t>(stream), [&]() -> int {
    if (!x || !sigma || !grad_out || !grad_x || !grad_sigma) {
      set_error("pnpx_unet_denoise_backward_ticket: null pointer");
      return PNPX_ERR_ARG;
    }
    return unet_denoise_backward_ticket(ctx, x, sigma, 1, grad_out, grad_x, grad_sigma, B, H, W,
                                        static_cast<hipStream_t>(stream), ticket);
  });
}

int pnpx_unet_profile(pnpx_ctx* ctx, const float* x, const float* sigma, float* out, int B, int H, int W,
                      void* stream, int cap, float* ms_out, double* flops_out, const char** names_out, int* n_out) {
  LOCK_CTX(ctx);
  if (!x || !sigma || !out || !ms_out || !flops_out || !names_out || !n_out || cap <= 0) {
    set_error("pnpx_unet_profile: null pointer");
    return PNPX_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  // make sure the arena exists before timing (growth synchronises)
  PNPX_TRY(unet_denoise(ctx, x, sigma, 1, out, nullptr, B, H, W, s, nullptr));
  while (ctx->events.size() < 1024) {
    hipEvent_t e;
    PNPX_HIP(hipEventCreate(&e));
    ctx->events.push_back(e);
  }
  ProfileSink sink;
  sink.events = &ctx->events;
  PNPX_TRY(unet_denoise(ctx, x, sigma, 1, out, nullptr, B, H, W, s, &sink));
  PNPX_HIP(hipStreamSynchronize(s));
  int n = sink.n < cap ? sink.n : cap;
  for (int i = 0; i < n; ++i) {
    float ms = 0.f;
    PNPX_HIP(hipEventElapsedTime(&ms, ctx->events[i], ctx->events[i + 1]));
    ms_out[i] = ms;
    flops_out[i] = sink.flops[i];
    names_out[i] = sink.names[i];
  }
  *n_out = n;
  return PNPX_OK;
}

int pnpx_fft2(pnpx_ctx* ctx, const float* in, float* out, int n_img, int H, int W, int inverse, int centered,
              void* stream) {
  LOCK_CTX(ctx);
  if (!in || !out) {
    set_error("pnpx_fft2: null pointer");
    return PNPX_ERR_ARG;
  }
  return fft2(ctx, in, out, n_img, H, W, inverse != 0, centered != 0, static_cast<hipStream_t>(stream));
}

}  // extern "C"
