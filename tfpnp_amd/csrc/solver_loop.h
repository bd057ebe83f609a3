// Host-side pieces that every fused solver loop (csmri.hip, tasks.hip) and every C-ABI entry shares.  Nothing here launches a
// kernel of its own or chooses one: a loop stays a straight-line sequence of launches and calls these where its copy of the same
// lines used to stand.
#pragma once
#include "common.h"

#define LOCK_CTX(ctx)                         \
  if (!(ctx)) {                               \
    pnpx::set_error("null context");          \
    return PNPX_ERR_ARG;                      \
  }                                           \
  std::lock_guard<std::mutex> _lk((ctx)->mu); \
  PNPX_HIP(hipSetDevice((ctx)->device))
#define REQUIRE(cond, msg)     \
  if (!(cond)) {               \
    pnpx::set_error(msg);      \
    return PNPX_ERR_ARG;       \
  }

namespace pnpx {

// ------------------------------------------------------------------ entries
// Body of an extern "C" entry that runs the denoiser: context lock, device, stream cast, range-guard re-run wrapper (common.h
// guarded).  `body(stream)` returns the status.  The backward entries keep their whole loop in `body`.
template <class F>
int solver_entry(pnpx_ctx* ctx, void* stream, F&& body) {
  LOCK_CTX(ctx);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return guarded(ctx, s, [&]() -> int { return body(s); });
}
// The same for a *_train entry; `name` is the prefix of its own message ("csmri_admm_train", "pnpx_pr_iadmm_train", ...).
// `saved_ok`: saved is there or not needed.  The two files differ on a negative T with a null saved -- csmri.hip passes
// `saved || T <= 0` (the call goes on to the loop's own argument check), tasks.hip `saved || T == 0` (rejected here) -- and
// each entry keeps its rule, so every bad call keeps its message.
template <class F>
int solver_train_entry(pnpx_ctx* ctx, const char* name, bool saved_ok, const unsigned long long* ticket, void* stream,
                       F&& body) {
  LOCK_CTX(ctx);
  if (!saved_ok || !ticket) {
    set_error("%s: saved / ticket is null", name);
    return PNPX_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  return guarded(ctx, s, [&]() -> int { return body(s); });
}

// ------------------------------------------------------------------ forward prologue
// Sizes of a state tensor [B, nvar, H, W(, 2)]: pixels per plane, item stride and pixels per batch (in elements of the state:
// float2 for the complex CS-MRI / PR states, float for SPI / CT).
struct StateDims {
  int HW;
  size_t is, n;
};
inline StateDims state_dims(int B, int H, int W, int nvar) {
  return StateDims{H * W, (size_t)nvar * H * W, (size_t)B * H * W};
}
// The state passed through unchanged: the whole result of a T == 0 call, the starting point of the loops that update in place.
inline int copy_state(void* dst, const void* src, size_t bytes, hipStream_t s) {
  PNPX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  return PNPX_OK;
}

// ------------------------------------------------------------------ prox step
// What the denoiser calls of one forward share.  `ticket_out` is non-null only when the call parks its activations.
struct Prox {
  pnpx_ctx* ctx;
  const float* sigma_d;
  int param_stride, B, H, W;
  hipStream_t s;
  unsigned long long* ticket_out;
};
// Zeroes the caller's ticket and decides whether the call parks: saved && ticket_out.  The static *_forward functions are reached
// from their two entries only, with saved and ticket both null (inference) or ticket non-null and saved non-null whenever T > 0
// (solver_train_entry), so on every call that reaches the loop this is the same as `saved` alone; a null ticket_out is never written.
inline Prox prox_begin(pnpx_ctx* ctx, const float* sigma_d, int param_stride, int B, int H, int W, const float* saved,
                       unsigned long long* ticket_out, hipStream_t s) {
  if (ticket_out) *ticket_out = 0;
  return Prox{ctx, sigma_d, param_stride, B, H, W, s, saved ? ticket_out : nullptr};
}
// Iteration i: out = D(d, sigma_d[:, i]).  `save_d` (optional) first receives a copy of d, the denoiser input the VJP needs; a
// loop that builds d in `saved` itself passes none.  A parking call hands out consecutive tickets under the context lock: the
// first one goes to the caller, iteration i holds ticket + i (0: the first iteration was not parked).
inline int prox_step(const Prox& p, int i, const float* d, float* out, float* save_d = nullptr) {
  if (save_d)
    PNPX_HIP(hipMemcpyAsync(save_d, d, sizeof(float) * p.B * p.H * p.W, hipMemcpyDeviceToDevice, p.s));
  if (p.ticket_out) {
    unsigned long long tk = 0;
    PNPX_TRY(unet_denoise_train(p.ctx, d, p.sigma_d + i, p.param_stride, out, p.B, p.H, p.W, p.s, &tk));
    if (i == 0) *p.ticket_out = tk;
    return PNPX_OK;
  }
  return unet_denoise(p.ctx, d, p.sigma_d + i, p.param_stride, out, nullptr, p.B, p.H, p.W, p.s, nullptr);
}
// Iteration i of a backward loop: (grad_d, grad_sigma_d[i]) = D^T(grad_out) at the saved input saved_d[i], from the activations
// parked under ticket + i if the ring still holds them, else by re-computation (ticket 0).
inline int prox_vjp(pnpx_ctx* ctx, int i, const float* saved_d, const float* sigma_d, int param_stride, const float* grad_out,
                    float* grad_d, float* grad_sigma_d, int B, int H, int W, hipStream_t s, unsigned long long ticket) {
  return unet_denoise_backward_ticket(ctx, saved_d + (size_t)i * B * H * W, sigma_d + i, param_stride, grad_out, grad_d,
                                      grad_sigma_d + (size_t)i * B, B, H, W, s, ticket ? ticket + i : 0);
}

}  // namespace pnpx
