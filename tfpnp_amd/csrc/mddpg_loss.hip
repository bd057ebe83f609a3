// The MDDPG policy loss and its backward in one launch -- tfpnp/trainer/mddpg/trainer.py::_update, lines 174 and 179-197, and what
// policy_loss.backward() (:202) leaves in the loss's direct inputs.  The networks around it (actor, critic, target critic, the
// environment's one-step model) are other entries of this library; this file is the O(B) arithmetic between them, which the
// reference spreads over about 25 elementwise torch launches and an autograd graph.
//
// Per row i (eps = FLT_EPSILON, the clamp_min of ResNetActorBase.head and of torch's Categorical):
//   r    = reward - loop_penalty                                  (:174)
//   g    = discount * (1 - idx_stop)                              (:184, :191)
//   logp = log(max(p_stop[idx_stop], eps));  ent = -(xlogy(p0, p0) + xlogy(p1, p1))
//   Qt   = g * v_next_target + r                                  (:183-185)
//   adv  = Qt - v_cur                                             (:186, detached)
//   term = logp * adv + (g * v_next + r) + lambda_e * ent         (:187-197)
//   policy_loss = -(1 / B) * sum(term)
//
// The value arithmetic of a row (r, g, Qt, adv, the DDPG term, the a2c gradient) is fp32, operation by operation in the order torch
// evaluates the reference's expressions and their autograd formulas, with no contraction: q_target has the bytes of
// `discount * (1 - stop) * V + reward` written in torch.  The two logarithms of a row are taken in double and everything made of
// them (logp, ent, the entropy gradient) is rounded to fp32 once.  The reason is accuracy: an fp32 p * logf(p) carries logf's
// last-place error into both summands of the entropy, which are of one size, and at B = 256 such an entropy sat at 1.3 of the
// tests' bar (tests/mddpg_cases.py) where the host's fp32 evaluation happened to be exact; with double logarithms every output stays
// below 0.5 of it (profiles/mddpg_loss.md).  Double logarithms are slow on the device; their cost here -- two per row, each thread
// of one workgroup owning B / 256 rows -- has not been measured apart from the update that contains them
// (tools/time_mddpg_update.py).
// The two sums (term, ent) are taken in double: thread t of the ONE workgroup owns rows t, t + 256, t + 512, ... and adds them in that
// order, the 256 partials are added by a fixed tree in LDS -- no atomics, the result depends neither on the alignment of any
// pointer (all accesses are 4 or 8 bytes wide at their natural alignment; idx_stop is an int64 array) nor on anything but B.  This
// is the convention of live_optim.hip's norm, and the tree is live_optim's as well: eight barrier steps over 4 KB of LDS.  Reducing
// each wave by shuffles first and leaving four partials in LDS would save six of the eight barriers; a double travels as two 32-bit
// shuffles, it is a second reduction scheme in the library to keep bit-stable, and it shortens a tail of well under a microsecond in
// a launch that runs once per update next to network passes of milliseconds -- so the plain tree stays.  One workgroup is right for
// what this is: B is a replay batch (tens of rows), and a second launch for the final sum would cost more than the whole loop.
//
// Gradients of policy_loss (invB = 1 / B; the advantage is detached, so only the DDPG term carries v_next and reward):
//   grad_v_next  = -(invB * g)                   exactly zero where idx_stop is 1
//   grad_reward  = -invB
//   grad_p_stop  = lambda_e * invB * (log p_j + 1) at both entries                                       (entropy)
//                + (-invB * adv) / max(p, eps) at the taken entry where p >= eps, nothing where p < eps   (clamp_min's backward)
// At p_j == 0 exactly the forward is finite (xlogy(0, 0) = 0; logp = log(eps)); torch's gradient there is NaN (xlogy's 0 / 0).
// The kernel writes what the line above gives: -inf for lambda_e > 0, NaN for lambda_e == 0 (0 * inf), +inf for lambda_e < 0.
#include <cfloat>
#include <cmath>

#include "common.h"

namespace pnpx {
namespace {

constexpr int LOSS_THREADS = 256;
constexpr double LOG_EPS = -23.0 * 0.6931471805599453;   // log(FLT_EPSILON) = log(2^-23)
static_assert(FLT_EPSILON == 1.1920928955078125e-7f, "FLT_EPSILON is 2^-23");

__global__ __launch_bounds__(LOSS_THREADS) void mddpg_policy_loss_kernel(
    const float* __restrict__ p_stop, const long long* __restrict__ idx_stop, const float* __restrict__ v_cur,
    const float* __restrict__ v_next_target, const float* __restrict__ v_next, const float* __restrict__ reward, float discount,
    float loop_penalty, float lambda_e, int B, float* __restrict__ q_target, float* __restrict__ log_prob, float* __restrict__ entropy,
    float* __restrict__ scalars, float* __restrict__ grad_p_stop, float* __restrict__ grad_v_next, float* __restrict__ grad_reward) {
#pragma clang fp contract(off)
  __shared__ double part_term[LOSS_THREADS];
  __shared__ double part_ent[LOSS_THREADS];
  const float invB = 1.0f / (float)B;
  const float G = lambda_e * invB;
  double acc_term = 0.0, acc_ent = 0.0;
  for (size_t i = threadIdx.x; i < (size_t)B; i += LOSS_THREADS) {
    const float p0 = p_stop[2 * i], p1 = p_stop[2 * i + 1];
    const bool stop = idx_stop[i] != 0;
    const float r = reward[i] - loop_penalty;
    const float g = discount * (stop ? 0.0f : 1.0f);
    const float p = stop ? p1 : p0;
    const float pc = p < FLT_EPSILON ? FLT_EPSILON : p;   // a NaN stays a NaN, as clamp_min leaves it
    const double l0 = log((double)p0), l1 = log((double)p1);
    const double logp_d = p < FLT_EPSILON ? LOG_EPS : (stop ? l1 : l0);
    const double ent_d = -((p0 == 0.0f ? 0.0 : (double)p0 * l0) + (p1 == 0.0f ? 0.0 : (double)p1 * l1));
    const float qt = g * v_next_target[i] + r;
    const float adv = qt - v_cur[i];
    const float ddpg = g * v_next[i] + r;
    q_target[i] = qt;
    log_prob[i] = (float)logp_d;
    entropy[i] = (float)ent_d;
    acc_term += logp_d * (double)adv + (double)ddpg + (double)lambda_e * ent_d;
    acc_ent += ent_d;
    // backward
    const float e0 = (float)((double)G * (l0 + 1.0)), e1 = (float)((double)G * (l1 + 1.0));
    const float a2c = p < FLT_EPSILON ? 0.0f : (-invB * adv) / pc;
    grad_p_stop[2 * i] = stop ? e0 : e0 + a2c;
    grad_p_stop[2 * i + 1] = stop ? e1 + a2c : e1;
    grad_v_next[i] = 0.0f - invB * g;
    grad_reward[i] = -invB;
  }
  part_term[threadIdx.x] = acc_term;
  part_ent[threadIdx.x] = acc_ent;
  __syncthreads();
  for (int st = LOSS_THREADS / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      part_term[threadIdx.x] += part_term[threadIdx.x + st];
      part_ent[threadIdx.x] += part_ent[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    scalars[0] = (float)(-(part_term[0] / (double)B));
    scalars[1] = (float)(part_ent[0] / (double)B);
  }
}

}  // namespace

int mddpg_policy_loss(const float* p_stop, const long long* idx_stop, const float* v_cur, const float* v_next_target, const float* v_next,
                      const float* reward, float discount, float loop_penalty, float lambda_e, int B, float* q_target, float* log_prob,
                      float* entropy, float* scalars, float* grad_p_stop, float* grad_v_next, float* grad_reward, hipStream_t s) {
  if (B <= 0) {
    set_error("pnpx_mddpg_policy_loss: B must be positive, got %d", B);
    return PNPX_ERR_ARG;
  }
  if (!p_stop || !idx_stop || !v_cur || !v_next_target || !v_next || !reward || !q_target || !log_prob || !entropy || !scalars ||
      !grad_p_stop || !grad_v_next || !grad_reward) {
    set_error("pnpx_mddpg_policy_loss: null pointer");
    return PNPX_ERR_ARG;
  }
  if (!std::isfinite(discount) || !std::isfinite(loop_penalty) || !std::isfinite(lambda_e)) {
    set_error("pnpx_mddpg_policy_loss: discount, loop_penalty and lambda_e must be finite");
    return PNPX_ERR_ARG;
  }
  hipLaunchKernelGGL(mddpg_policy_loss_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, p_stop, idx_stop, v_cur, v_next_target, v_next, reward,
                     discount, loop_penalty, lambda_e, B, q_target, log_prob, entropy, scalars, grad_p_stop, grad_v_next, grad_reward);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

}  // namespace pnpx
