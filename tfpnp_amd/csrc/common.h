// Internal declarations shared by the translation units of libpnpx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pnpx.h"

namespace pnpx {

// ---------------------------------------------------------------------------------------------------
// Error plumbing: nothing throws across the C ABI.
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define PNPX_HIP(expr)                                                       \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) return ::pnpx::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)
#define PNPX_TRY(expr)          \
  do {                          \
    int _s = (expr);            \
    if (_s != PNPX_OK) return _s; \
  } while (0)
#define PNPX_LAUNCH_CHECK() PNPX_HIP(hipGetLastError())

// ---------------------------------------------------------------------------------------------------
// Padded planar activation layout used INSIDE the denoiser (never visible at the C ABI):
//   tensor [B][C][Hp][Wp] fp32, interior pixel (y,x) at row y+1, column x+PADL.  All border cells are
//   zero for the lifetime of the workspace (memset once, producers write interiors only), so 3x3
//   convolutions read their zero padding straight from memory and need no bounds checks.
constexpr int PADL = 4;
__host__ __device__ inline int padded_w(int W) { return W + 2 * PADL; }
__host__ __device__ inline int padded_h(int H) { return H + 2; }

struct ActDesc {      // one activation tensor in the arena
  size_t off = 0;     // float offset into the arena
  int C = 0, H = 0, W = 0;
  size_t per_image() const { return (size_t)C * padded_h(H) * padded_w(W); }
};

// ---------------------------------------------------------------------------------------------------
struct ConvLayer {          // one 3x3 conv of the UNet, weights repacked for the MFMA kernel
  int cin = 0, cout = 0;
  int mt = 0, cc = 0;       // cout tile and cin chunk the packing was made for
  float* w = nullptr;       // device: [cout/mt][cin/cc][9][cc][mt]
  float* b = nullptr;       // device: [cout]
};

struct DeviceBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
// hipMalloc into an empty DeviceBuf; on failure the error reads "<what> allocation of N bytes failed"
int alloc_dev(DeviceBuf& b, size_t bytes, const char* what);

}  // namespace pnpx
#include "live_params.h"   // LiveParams, PackWorkspace: the actor's and the critic's live weights
namespace pnpx {

struct UNetArena {
  DeviceBuf buf;
  int capB = 0, capH = 0, capW = 0, mode = -1;
};

struct ConvLayerHsDev {     // the same conv packed for the half-split f16 kernel (conv_hs.hip)
  int cin = 0, cout = 0, cin_pad = 0, mt = 0;
  char* w = nullptr;        // device: [cout/mt][cin_pad/16][9][hi,lo][2][mt][8] f16
  float inv_scale = 1.f;    // 1 / (weight scale * activation scale)
};

enum ConvMode { CONV_F32 = 0, CONV_HS = 1 };

// ---------------------------------------------------------------------------------------------------
// Policy actor (ResNet-18 encoder + heads) -- policy.hip.  BatchNorm is folded into weights / bias when the eval packing is derived;
// every convolution runs on the half-split launches of the trunk the critic shares (resnet18_hs.h).
// the packed weights one forward reads: launch descriptors over one device blob
struct PolicyPack {
  // the 21 convolutions of the trunk packed for the half-split launches, in the layer numbering of resnet18_hs.h: the stem and the
  // stage-entry conv1 as 2x2-window sparse-tap convolutions over the HS8 space-to-depth input (tap mask 0x01B), the 1x1 shortcuts
  // (0x010, first Cin channels), the stride-1 convolutions (f16x3 MFMA kernel, conv_hs.hip)
  ConvLayerHsDev hs[21];
  const float* hs_bias[21] = {};
  const float* fc_sm_w = nullptr;   // [2][512], [2]
  const float* fc_sm_b = nullptr;
  const float* fc_det_w = nullptr;  // [n_det][512] ([64][512] with the SPI head)
  const float* fc_det_b = nullptr;
  const float* fc_det2_w = nullptr; // SPI head only: [n_det][64]
  const float* fc_det2_b = nullptr;
  DeviceBuf weights;
};
struct PolicyNet : PolicyPack {   // the base: the eval-mode packing (BatchNorm folded from the running statistics)
  bool loaded = false;
  int num_inputs = 0, cin_pad = 0, n_det = 0, spi_head = 0;
  DeviceBuf arena;           // activations for capB observations of capH x capW, zero borders
  int capB = 0, capH = 0, capW = 0;
  // live weights (policy_pack.hip): the flat fp32 parameter vector in pnpx_policy_load's order, kept after either load entry
  LiveParams live;
  PackWorkspace pack_ws;     // layer table, per-channel BatchNorm scales / shifts / weight maxima; read back: the 21 half-split weight scales
  // train-mode forward (policy_bn.hip): the same convolutions packed WITHOUT the fold (scale 1, shift 0), derived from `live` by the
  // first train forward after a load; moving the running statistics does not stale it, but it stales the eval packing above, which the
  // next eval forward re-derives once (eval_stale)
  PolicyPack raw;
  PackWorkspace raw_ws;
  bool raw_valid = false, eval_stale = false;
  DeviceBuf train_ws;        // raw convolution outputs + activations of the train forward, zero borders
  int tcapB = 0, tcapH = 0, tcapW = 0;
  DeviceBuf bn_buf;          // per BatchNorm channel: batch mean, biased batch variance, scale, shift; then the reduction partials
  bool bn_have_stats = false;
  // parameter gradients (pnpx_policy_param_grad; policy_bn.hip, policy_grad.hip): the adjoint packings of `raw` (transposed, tap-mirrored;
  // layers 1..20 -- the stem's adjoint is never run), derived by the first gradient call after a load; a workspace of its own that keeps
  // every raw convolution output, every activation and the gradient tensors (zero borders); the K-split slabs and the head scratch.
  // Forward-only users allocate none of it.
  ConvLayerHsDev raw_bwd[21];
  DeviceBuf raw_adj, raw_adj_table;
  const float* raw_adj_zero = nullptr;   // [1024] zeros inside raw_adj: the bias operand of the adjoint launches
  bool adj_valid = false;
  DeviceBuf grad_ws;
  int gcapB = 0, gcapH = 0, gcapW = 0;
  DeviceBuf grad_slab;
  // kept forward (pnpx_policy_forward_train_keep): every raw output and activation of ONE train forward sits in grad_ws, its batch
  // statistics in bn_buf, and pnpx_policy_param_grad_kept may run on them.  Valid for the observation shape and the workspace capacity
  // (the plan's offsets) it was run with; kept_lost says what ended it (policy_kept_drop: a change of the trainable weights, a train
  // forward or a re-computing gradient call, which overwrite bn_buf / grad_ws).  Moving the running statistics does not end it.
  bool kept_valid = false;
  int keptB = 0, keptH = 0, keptW = 0, kept_capB = 0, kept_capH = 0, kept_capW = 0;
  const char* kept_lost = "no pnpx_policy_forward_train_keep has run on this actor";
  // optimiser state (pnpx_policy_adam_step; live_params.h): kept by a refresh of the same actor, dropped with the actor; the frozen
  // ranges are the running statistics
  LiveOptim optim;
};
inline void policy_kept_drop(PolicyNet& N, const char* why) {
  if (N.kept_valid) N.kept_lost = why;
  N.kept_valid = false;
}

// Value network (critic.hip): ResNet_wobn(num_inputs, 18, 1).  The raw parameters live on the device (`live`); the packed
// weights the launches read are derived from them, on the host by critic_load and on the device by every later refresh
// (critic_load_device, critic_soft_update).  Layer index: the trunk's (resnet18_hs.h).
struct CriticNet {
  bool loaded = false;
  int num_inputs = 0, cin_pad = 0;
  ConvLayerHsDev fwd[21], bwd[21];   // forward packings and their adjoints (transposed, tap-mirrored)
  const float* bias[21] = {};
  float alpha[21] = {};              // TReLU threshold behind the layer (shortcuts: unused)
  const float* fc_w = nullptr;       // [512]
  const float* fc_b = nullptr;       // [1]
  const float* zero = nullptr;       // [1024] zeros: bias operand of the adjoint launches
  float fc_wmax = 0.f;               // max |fc_w|: the backward pass scales its gradients to O(1)
  DeviceBuf weights, arena;          // arena: every forward activation + the gradient tensors, zero borders
  int capB = 0, capH = 0, capW = 0;
  // live weights: the flat fp32 parameter vector (pnpx_critic_load's order) and what the device-side packing needs
  LiveParams live;                   // [critic_num_params(num_inputs)] floats
  PackWorkspace pack_ws;             // layer table, per-channel fold scales and maxima; read back: 21 weight scales, 21 thresholds, max |fc_w|
  // parameter gradients (pnpx_critic_param_grad): clip indicator, W * indicator, K-split slabs + reduction blocks; each grows to
  // the largest size seen
  DeviceBuf grad_m, grad_wm, grad_slab;
  // optimiser state (pnpx_critic_adam_step; live_params.h): kept by a refresh, dropped with the critic; no frozen ranges
  LiveOptim optim;
};

// number of independent launch chains for a B-image denoiser forward (unet.hip; option "chains", 0 = automatic)
int launch_chains(const pnpx_ctx* ctx, int B, int H, int W);
// a launch-chain fan-out failed half way: drain the side streams before the error is returned, so that nothing queued on them
// is still writing the shared arena / output buffers when the caller (or the next call) re-uses them
void join_side_streams_after_failure(pnpx_ctx* ctx);
// DRUNet denoiser (drunet.hip): packed weights per MFMA launch in state_dict order + its own activation arenas
struct DruArena {   // one arena and the layout it holds (drunet_net.h: dru_arena_reserve)
  DeviceBuf buf;
  int capB = 0, capH = 0, capW = 0;
  bool keeps = false;   // the layout has room for every ResBlock's middle activation (forward arenas, for the VJP)
};
struct DruF32Pack {   // fp32 packings of every layer (drunet_f32.hip), made on first use
  bool ready = false;
  std::vector<ConvLayer> layers;       // direct fp32 MFMA kernel
  std::vector<const float*> wino;      // Winograd weights of the 3x3 ResBlock layers (else null)
  DeviceBuf weights;
};
struct DruNet {
  bool loaded = false;
  int nb = 0;
  std::vector<ConvLayerHsDev> layers;
  std::vector<int> taps;           // per layer: 3x3 tap mask its weights are packed with (0x010 for the 1x1 layers)
  const float* head_w = nullptr;   // [64][2][3][3] native (VALU head convolution)
  const float* zero = nullptr;     // [1024] zeros: the bias operand of the bias-free network
  const float* e0 = nullptr;       // [5][32]: row k = (2^(4k), 0, ...): channel selector of the fused tail epilogue that also undoes a
                                   // 2^-(4k) down-scaling of the pass (shift, below); followed by zeros
  // Range handling.  The network is bias-free with ReLU activations only, i.e. positively homogeneous: f(a * in) = a * f(in) for
  // a > 0, and a power-of-two `a` commutes exactly with every step (the hi/lo split included, subnormals aside).  When the
  // half-split range guard trips (an activation left |v| < 4095) the pass is repeated / later passes run on inputs scaled by
  // 2^-shift (in the head convolution's store) with the tail multiplying back.  0, 4 or 8; a trip at 8 latches the context to
  // conv_mode 0 (drunet_f32.hip) like a UNet context.
  int shift = 0;
  // adjoint (input-gradient) layers, index-parallel to `layers` (transposed, tap-flipped; the head's adjoint is a 64 -> 32
  // launch whose channels 0 / 1 are the image / noise-map gradients; the tail's adjoint runs on the vector ALU)
  std::vector<ConvLayerHsDev> layers_bwd;
  const float* tail_bwd_w = nullptr;   // [64][2][3][3]: conv_first_hs_kernel weights of the tail's adjoint (1 -> 64 channels)
  DeviceBuf weights;
  DruArena arena, arena_grad;          // half-split family: activations (+ keep planes), gradients
  // conv_mode 0 (drunet_f32.hip): fp32 packings of the same layers, made on first use from the host copy of the parameters
  std::vector<float> params_host;
  DruF32Pack f32, f32_bwd;             // forward layers; their adjoints (made on the first fp32 VJP)
  DruArena f32_arena, f32_arena_grad;
};

}  // namespace pnpx

struct pnpx_ctx {
  int device = 0;
  std::mutex mu;
  // --- denoiser
  bool has_weights = false;
  pnpx::ConvLayer conv[27];
  pnpx::ConvLayerHsDev conv_hs[27];
  int conv_mode = pnpx::CONV_F32;  // which conv kernel family the denoiser runs (pnpx_ctx_set_option).  r6: the DEFAULT is the fp32 family (the
                                   // reference's own arithmetic, inside 1e-4 of the fp32 oracle on every drift seed); CONV_HS is the opt-in fast mode
  // --- options (pnpx_ctx_set_option; no environment variables are read on any launch path)
  int opt_subbatch = 24;           // images per level-0 sub-batch of the half-split forward (0 = whole batch)
  int opt_fuse_pool = 1;           // fused 2x2 max-pool epilogue
  int opt_fuse_outc = 1;           // fused 1x1 out-conv + residual + clamp epilogue
  int opt_fuse_first = 1;          // VALU first convolution straight from the fp32 image (no padded-input tensor)
  int opt_fuse_up = 1;             // bilinear x2 of the full-resolution decoder entry inside the conv kernel (producer waves): r5 default --
                                   // bit-identical to the separate kernel (tools/ab_fuse_up.py), forward 5.82 -> 5.76 ms at 48 x 256^2
  int opt_fold_first = 0;          // opt-in: first convolution folded into the loader of the second one (conv_hs WREG == 2;
                                   // bit-identical, 400 MB less HBM traffic per forward, time-neutral: 5.835 vs 5.841 ms)
  int opt_fft_tile = 0;            // complex points per FFT workgroup tile (0 = FFT_TILE_POINTS)
  int opt_fft_fast = 1;            // N = 256 lines on the register-radix-16 FFT kernels (fft_lds.h fft256_*)
  int opt_fft_affine = 1;          // XCD-affine block -> image mapping of the FFT passes (fft_lds.h)
  int lds_block_limit = 0;         // the device's per-block LDS limit in bytes (queried by the first FFT plan; 0 = not yet)
  int opt_chains = 0;              // denoiser forward as n independent launch chains over slices of the batch (0 = auto)
  std::vector<hipStream_t> side_streams;
  // fork / join events of the launch chains: a ROTATING pool.  An event must not be re-recorded while a hipStreamWaitEvent on
  // its previous record may still sit un-submitted in another stream's host-side queue: with one fork event and one join event
  // per side stream re-recorded every call, two host threads driving two contexts on one GPU lost joins (a slice's output read
  // before it was written: one item of a batch wrong, 15 of 25 stress runs; r4, tools/attic/stress_threads.py).
  std::vector<hipEvent_t> ev_pool;
  size_t ev_next = 0;
  int opt_wreg = 2;                // weights-in-registers instances for the 32 -> 32 channel layers (0 off, 1 / 2 = shape)
  int opt_range_guard = 1;         // 0 off, 1 sticky flag + latch to conv_mode 0, 2 strict (sync + transparent re-run)
  int opt_train_cache_gb = -1;     // training path: keep the activations of up to this many GiB of denoiser forwards for
                                   // the backward pass instead of re-computing them (0 = always re-compute; -1 = auto:
                                   // a quarter of the device memory free when the ring is first laid out, <= 96 GiB)
  size_t train_budget_bytes = 0;   // the automatic budget once measured (reset by set_option / train_cache_release)
  // --- half-split range guard: host-mapped word the conv_hs epilogues set when a stored value leaves the f16 range
  unsigned* range_flag_host = nullptr;   // pinned host allocation
  unsigned* range_flag_dev = nullptr;    // its device address
  bool range_tripped = false;            // latched by the host once the flag was seen set (cleared by set_option)
  float* conv_wino_u[27] = {};     // Winograd-transformed fp32 weights of the layers conv3x3_wino.hip can run (else null)
  float* conv_wino_u_bwd[27] = {}; // ... of the adjoint (transposed, tap-flipped) convolutions of the fp32 backward pass (r5)
  int opt_fp32_winograd = 1;       // conv_mode 0: run those layers as F(2x2,3x3) (fp32 arithmetic, 2.25x fewer MFMAs; 0 = the direct kernel everywhere)
  int opt_fp32_wino8 = (1 << 27) - 1;   // bit li: layer li runs on the 8-wave Winograd kernel (conv3x3_wino8.hip) where its geometry allows; a DRUNet
                                   // context: any bit = its ResBlock layers do
  float* conv_winof4_u[27] = {};   // Winograd F(4x4,3x3) weights of the layers conv3x3_winof4.hip can run in the UNet (levels 1-3: plain 64-cout layers and the decoder entries; else null)
  // bit li: layer li runs on the F(4x4,3x3) kernel in forward passes, where its geometry allows, its fp32_wino8_layers bit is set and
  // the K-split does not claim it.  Default: the plain 64-cout-tile layers of levels 1-3 (3-11, 16, 17, 19, 20, 22, 23), every one of
  // which measured faster than on the F(2x2) kernel at 48 x 256^2 (profiles/winof4.md; drift table profiles/winof4_probe.md)
  int opt_fp32_winof4 = (0x1ff << 3) | (3 << 16) | (3 << 19) | (3 << 22);
  // bits 15, 18, 21: that decoder entry (768 -> 256, 384 -> 128, 192 -> 64) runs on the F(4x4,3x3) kernel's two-source instance, behind
  // the separate up-sampling kernel, where the fused F(2x2) instance would run it in one piece (profiles/winof4_entries.md)
  int opt_fp32_winof4_entries = (1 << 15) | (1 << 18) | (1 << 21);
  // bits 15, 18, 21: where fp32_winof4_entries puts that entry on the F(4x4,3x3) kernel, the instance that up-samples the low-resolution
  // second source itself runs it and the up-sampling launch is skipped; same bits in the result.  Default: entry 21 alone, the one whose
  // up-sampling launch costs more than the interpolation in the kernel does (profiles/winof4_fuse_up.md)
  int opt_fp32_winof4_fuse_up = 1 << 21;
  float* conv_winof4_c32_u[27] = {};   // F(4x4,3x3) weights in the 32-cout instance's layout: the full-resolution 32 -> 32 layers 1, 2, 25 (else null)
  // bits 1, 2, 25: that layer runs on the F(4x4,3x3) kernel's 32-cout instance in forward passes where its geometry allows (H % 16 == 0,
  // W % 64 == 0) and its fp32_wino8_layers bit is set.  All three layers measured faster on it by the same 0.055-0.06 ms at 48 x 256^2;
  // the default holds layers 1 and 25, the largest set that keeps two noise-level distances of the existing suite under their bars
  // (episode drift of seed 36 against the fp32 oracle, 1e-4: layers 1 + 2 reach 1.02e-4; training against inference forward of the HQS
  // solver at 3 x 48 x 64, 1e-6: all three reach 1.016e-6; profiles/winof4_c32.md, drift table profiles/winof4_c32_probe.md)
  int opt_fp32_winof4_c32 = (1 << 1) | (1 << 25);
  int opt_fp32_chains = 2;         // conv_mode 0: n >= 2 = the forward as n launch chains over slices of the batch (default 2: this family is not
                                   // power-capped, a second chain fills the other's tails and partial rounds: 8.76 -> 8.44 ms at 48 x 256^2, -7 % at
                                   // B = 24; 3 and 4 chains measured slower); 1 = only the bottom level forks two chains; 0 = one chain
  int opt_fp32_ksplit = 1;         // conv_mode 0, r6: the deep levels' layers split their channel chunks over 2 / 4 work items (conv3x3_wino8.hip KSPLIT):
                                   // 1 = in calls whose unsplit tiles cannot fill the chip, 2 = always (bit-identical across all batch sizes), 0 = never
  int opt_ksplit_rule = 1;         // tuning: pieces per tile class (conv3x3_wino8_ksplit; 1 = the default rule)
  int opt_fp32_fuse_up = 1;        // conv_mode 0: the decoder entries up-sample their second source inside the 8-wave Winograd kernel (no up-sampled tensor)
  pnpx::ConvLayer conv_bwd[27];    // adjoint (input-gradient) convolutions, fp32 kernel family
  pnpx::ConvLayerHsDev conv_hs_bwd[27];  // ... and packed for the half-split kernel family
  float* zero_bias = nullptr;      // [768] zeros (bias operand of the adjoint convolutions)
  float* conv0_w = nullptr;  // [32][2][9] fp32: the first convolution in its native layout (VALU kernel, unet.hip)
  float* outc_w = nullptr;   // [32]
  float* outc_b = nullptr;   // [1]
  pnpx::DeviceBuf weights;   // single allocation holding all of the above
  // --- UNet activation arenas (capacity capB images of capH x capW, zero borders valid for one layout `mode`):
  //     arena = forward pass in the ctx's conv_mode (also the re-computation inside the backward pass);
  //     arena_grad = gradients of every activation (fp32 planar)
  pnpx::UNetArena arena, arena_grad;
  // training path: a ring of activation arenas.  Every denoiser forward run for autograd (pnpx_unet_denoise_train, the
  // iterations of pnpx_csmri_admm_train) takes the next slot, keeps every activation + the pre-clamp output there and
  // hands out a ticket; a VJP that presents a ticket still held by its slot skips the re-computation of the forward.
  struct TrainSlot {
    pnpx::UNetArena arena;
    pnpx::DeviceBuf pre;
    unsigned long long ticket = 0;
    int B = 0;
  };
  std::vector<TrainSlot> train_ring;
  unsigned long long train_counter = 0;
  int train_H = 0, train_W = 0, train_mode = -1;   // geometry the ring is laid out for
  bool train_alloc_failed = false;                 // stop retrying after an out-of-memory until the option is set again
  // --- policy actor
  pnpx::PolicyNet policy;
  // --- value network (critic)
  pnpx::CriticNet critic;
  // --- DRUNet denoiser (when loaded it IS the context's denoiser: every prox call of every solver runs it)
  pnpx::DruNet drunet;
  // --- solver scratch (complex fields etc.), grown on demand
  pnpx::DeviceBuf scratch;
  // --- FFT twiddle tables e^{-2 pi i m / N}, one per transform length: device float2[N]
  std::map<int, float2*> twiddle;
  // --- events for pnpx_unet_profile
  std::vector<hipEvent_t> events;
};

namespace pnpx {

int chain_event(pnpx_ctx* ctx, hipEvent_t* ev);        // next event of the rotating pool (unet.hip)
int chain_streams(pnpx_ctx* ctx, int chains);          // make sure chains - 1 side streams exist
// Run `chains` contiguous slices of a B-item batch as independent launch chains: slice 0 on the caller's stream `s`, the others
// on the context's side streams, forked from / joined back into `s` by events.  run_slice(lo, hi, stream) -> status.
template <class F>
int fan_out_chains(pnpx_ctx* ctx, int chains, int B, hipStream_t s, F&& run_slice) {
  PNPX_TRY(chain_streams(ctx, chains));
  hipEvent_t fork = nullptr, joins[16] = {};
  PNPX_TRY(chain_event(ctx, &fork));
  PNPX_HIP(hipEventRecord(fork, s));
  // from here on work may sit on the side streams: EVERY error exit drains them first (nothing queued there may outlive the
  // failing call and write the shared arena / output buffers while the caller re-uses them)
  auto fail = [&](int rc) {
    join_side_streams_after_failure(ctx);
    return rc;
  };
  auto hip = [&](hipError_t e, const char* what) { return e == hipSuccess ? PNPX_OK : hip_fail(e, what, __FILE__, __LINE__); };
  for (int c = chains - 1; c >= 0; --c) {       // the caller's stream takes slice 0 last: its host-side issue overlaps
    const int lo = (int)((long long)B * c / chains), hi = (int)((long long)B * (c + 1) / chains);
    hipStream_t st = c ? ctx->side_streams[c - 1] : s;
    int rc = c ? hip(hipStreamWaitEvent(st, fork, 0), "hipStreamWaitEvent(fork)") : PNPX_OK;
    if (rc == PNPX_OK) rc = run_slice(lo, hi, st);
    if (rc == PNPX_OK && c) rc = chain_event(ctx, &joins[c]);
    if (rc == PNPX_OK && c) rc = hip(hipEventRecord(joins[c], st), "hipEventRecord(join)");
    if (rc != PNPX_OK) return fail(rc);
  }
  for (int c = 1; c < chains; ++c) {
    const int rc = hip(hipStreamWaitEvent(s, joins[c], 0), "hipStreamWaitEvent(join)");
    if (rc != PNPX_OK) return fail(rc);
  }
  return PNPX_OK;
}

int ctx_reserve_unet(pnpx_ctx* ctx, int B, int H, int W);   // main arena, ctx->conv_mode
int reserve_arena(pnpx_ctx* ctx, UNetArena& ar, int mode, int B, int H, int W, size_t extra_bytes);
int ctx_scratch(pnpx_ctx* ctx, size_t bytes, void** out);
int ctx_twiddle(pnpx_ctx* ctx, int N, const float2** out);
// Half-split range guard (api.hip).  range_guard_enter: called at the top of every entry that runs the denoiser; if the
// flag of an earlier call is set, latches the context to conv_mode 0.  range_guard_strict: option value 2 -- synchronise
// `s`, and if the flag was set by THIS call return true after switching to conv_mode 0 so the caller re-runs the call.
void range_guard_enter(pnpx_ctx* ctx);
int range_guard_strict(pnpx_ctx* ctx, hipStream_t s, bool* rerun);
// Wraps the body of a C-ABI entry that runs the denoiser (entries are functional: inputs are never modified, so a body
// can simply be executed again).
template <class F>
int guarded(pnpx_ctx* ctx, hipStream_t s, F&& body) {
  range_guard_enter(ctx);
  int st = body();
  // strict mode: the UNet repeats the call once in exact fp32; a DRUNet context repeats it on inputs scaled down by another
  // factor 16 per attempt (api.hip::range_guard_strict) until the guard stays quiet
  // (a DRUNet context: 2^-4, 2^-8, then exact fp32 -- api.hip::drunet_rescale)
  for (int attempt = 0; attempt < 4 && st == PNPX_OK && ctx->opt_range_guard == 2 && ctx->conv_mode == CONV_HS; ++attempt) {
    bool rerun = false;
    PNPX_TRY(range_guard_strict(ctx, s, &rerun));
    if (!rerun) break;
    st = body();
  }
  return st;
}

struct ProfileSink {      // optional per-launch event recording for pnpx_unet_profile
  std::vector<hipEvent_t>* events = nullptr;
  std::vector<const char*> names;
  std::vector<double> flops;
  int n = 0;
};

// Denoiser forward on padded input already resident in the arena is internal; these are the pieces the
// solver loops call.  x/sigma/out are unpadded [B,1,H,W] / [B] tensors (C-ABI layout).
int unet_denoise(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, float* out, float* out_pre,
                 int B, int H, int W, hipStream_t s, ProfileSink* prof, UNetArena* arena = nullptr, int mode = -1,
                 bool keep_all = false);   // keep_all: store every activation (no fused network tail) -- backward pass
// VJP of the denoiser wrt x and sigma (unet_bwd.hip): recomputes the forward pass in fp32 and back-propagates.
// cached != NULL: the activations (a keep_all forward of exactly this input in `cached`) and its pre-clamp output are
// reused instead of re-computed.
int unet_denoise_backward(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, const float* grad_out,
                          float* grad_x, float* grad_sigma, int B, int H, int W, hipStream_t s,
                          UNetArena* cached = nullptr, const float* cached_pre = nullptr);
size_t unet_arena_bytes(int mode, int B, int H, int W);
void train_cache_free(pnpx_ctx* ctx);
// Denoiser forward for autograd: like unet_denoise, additionally parks the activations in the training ring; *ticket = 0
// when the ring is disabled / out of budget (the VJP then re-computes).
int unet_denoise_train(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, float* out, int B, int H,
                       int W, hipStream_t s, unsigned long long* ticket);
// VJP that looks the ticket up in the ring first (ticket 0 / overwritten slot: re-computation)
int unet_denoise_backward_ticket(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride,
                                 const float* grad_out, float* grad_x, float* grad_sigma, int B, int H, int W,
                                 hipStream_t s, unsigned long long ticket);

// DRUNet denoiser (drunet.hip)
size_t drunet_num_params(int nb);
int drunet_load(pnpx_ctx* ctx, const float* params, size_t n, int nb);
int drunet_denoise(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, float* out, float* out_pre, int B,
                   int H, int W, hipStream_t s, bool keep_mids = false);
// VJP wrt x and sigma: forward re-computed keeping every ResBlock's ReLU output, then the adjoint chain on the same kernels
int drunet_denoise_backward(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, const float* grad_out,
                            float* grad_x, float* grad_sigma, int B, int H, int W, hipStream_t s);
void drunet_free(pnpx_ctx* ctx);
// the fp32 family's pieces (drunet_f32.hip), reached through the two functions above in conv_mode 0: the forward, and the adjoint chain after it
int drunet_denoise_f32(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, float* out, float* out_pre, int B, int H,
                       int W, hipStream_t s, bool keep_mids = false);
int drunet_denoise_backward_f32(pnpx_ctx* ctx, const float* grad_out, const float* pre, float* g_pre, float* part, float* grad_x,
                                float* grad_sigma, int B, int H, int W, hipStream_t s);
void drunet_f32_free(pnpx_ctx* ctx);

// Policy actor (policy.hip)
size_t policy_num_params(int num_inputs, int n_det, int spi_head);
int policy_load(pnpx_ctx* ctx, const float* params, size_t n, int num_inputs, int n_det, int spi_head);
int policy_forward(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, hipStream_t s);
void policy_free(pnpx_ctx* ctx);
// live weights (policy_pack.hip)
int policy_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n, int num_inputs, int n_det, int spi_head, hipStream_t s);
int policy_params(pnpx_ctx* ctx, float* dst_dev, size_t n, hipStream_t s);
int policy_pack_raw(pnpx_ctx* ctx, hipStream_t s);       // live vector -> PolicyNet::raw (allocates on first use)
int policy_refresh_eval(pnpx_ctx* ctx, hipStream_t s);   // live vector -> the eval packing, after the running statistics moved
struct Packed;                                           // one host packing (resnet18_hs.h)
int policy_adopt_host_blob(pnpx_ctx* ctx, const Packed* pk21, const size_t* heads6, size_t total);   // policy_load's last step
// pieces of the eval forward the train forward shares (policy.hip; the half-split ones: resnet18_hs.h)
int policy_launch_heads(const PolicyPack& P, int n_det, int spi_head, const char* feat_hs, int h, int w, int B, float* probs, float* det,
                         hipStream_t s);
// train-mode forward (policy_bn.hip)
constexpr size_t POLICY_BN_CHANNELS = 4864;
int policy_forward_train(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum, int update_running,
                         hipStream_t s);
int policy_bn_stats(pnpx_ctx* ctx, float* mean_dev, float* var_dev, size_t n, hipStream_t s);
// parameter gradients through the train-mode forward (driver: policy_bn.hip; kernels: policy_grad.hip; adjoint packings: policy_pack.hip)
int policy_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_probs, const float* grad_det, float* grad_params, size_t n, int B,
                      int H, int W, hipStream_t s);
int policy_pack_adj(pnpx_ctx* ctx, hipStream_t s);       // live vector -> PolicyNet::raw_bwd (allocates on first use)
// the same forward kept for the backward pass, and the backward pass on what it kept (policy_bn.hip)
int policy_forward_train_keep(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                              int update_running, hipStream_t s);
int policy_param_grad_kept(pnpx_ctx* ctx, const float* grad_probs, const float* grad_det, float* grad_params, size_t n, hipStream_t s);
// clip_grad_norm_ + Adam on the live vector (running statistics frozen), then the refresh (policy_pack.hip; kernels: live_optim.hip)
int policy_frozen_ranges(int num_inputs, int n_det, int spi_head, FrozenRange* out, int* n_out);   // merged; out: LIVE_OPTIM_MAX_FROZEN
int policy_upload_frozen(pnpx_ctx* ctx);                 // ... of the loaded actor -> PolicyNet::optim, at a load that allocates
int policy_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n, float lr, float beta1, float beta2, float eps, float max_norm,
                     float* grad_norm_dev, hipStream_t s);
int policy_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n, long long* step_host, hipStream_t s);
int policy_optim_reset(pnpx_ctx* ctx);

// Value network (critic.hip)
size_t critic_num_params(int num_inputs);
int critic_load(pnpx_ctx* ctx, const float* params, size_t n, int num_inputs);
int critic_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n, int num_inputs, hipStream_t s);
int critic_soft_update(pnpx_ctx* ctx, const float* src_dev, size_t n, float one_minus_tau, float tau, hipStream_t s);
int critic_params(pnpx_ctx* ctx, float* dst_dev, size_t n, hipStream_t s);
int critic_forward(pnpx_ctx* ctx, const float* ob, float* value, int B, int H, int W, hipStream_t s);
int critic_backward(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_ob, int B, int H, int W, hipStream_t s);
int critic_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_params, size_t n, int B, int H, int W,
                      hipStream_t s);
// value_loss = mean((V - q_target)^2) and its backward on one forward (critic.hip)
int critic_value_loss_grad(pnpx_ctx* ctx, const float* ob, const float* q_target, float* value, float* loss, float* grad_params, size_t n,
                           int B, int H, int W, hipStream_t s);
// clip_grad_norm_ + Adam on the live vector, then the refresh (critic.hip; kernels: live_optim.hip)
int critic_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n, float lr, float beta1, float beta2, float eps, float max_norm,
                     float* grad_norm_dev, hipStream_t s);
int critic_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n, long long* step_host, hipStream_t s);
int critic_optim_reset(pnpx_ctx* ctx);
void critic_free(pnpx_ctx* ctx);

// MDDPG policy loss and its gradients, one launch (mddpg_loss.hip); checks its own arguments, keeps no state
int mddpg_policy_loss(const float* p_stop, const long long* idx_stop, const float* v_cur, const float* v_next_target, const float* v_next,
                      const float* reward, float discount, float loop_penalty, float lambda_e, int B, float* q_target, float* log_prob,
                      float* entropy, float* scalars, float* grad_p_stop, float* grad_v_next, float* grad_reward, hipStream_t s);

// FFT building blocks (fft.hip)
int fft2(pnpx_ctx* ctx, const float* in, float* out, int n_img, int H, int W, bool inverse, bool centered,
         hipStream_t s);

}  // namespace pnpx
