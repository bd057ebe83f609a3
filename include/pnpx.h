/* pnpx.h -- C ABI of the MI355X-native PnP proximal-solver inner loop (libpnpx.so).
 *
 * Plain C: pointers, sizes, ints.  No torch / HIP types in any signature (a HIP stream is passed as
 * void*, a null stream is the device's default stream).  Every function returns 0 on success and a
 * non-zero pnpx_status otherwise; nothing throws across this boundary.  pnpx_last_error() returns a
 * thread-local description of the last failure.
 *
 * Each entry point replaces one piece of the reference (Vandermode/TFPnP, /root/reference); the
 * file:line it stands in for is cited on the declaration.  Tensor layouts at this boundary are the
 * reference's own: contiguous fp32, NCHW, complex numbers as a trailing dimension of 2 (re, im),
 * masks as one byte per pixel (torch.bool storage).  All pointers are DEVICE pointers unless a
 * parameter name ends in _host.
 *
 * Threading: a pnpx_ctx belongs to one device; calls on the same ctx are serialised by an internal
 * mutex; different ctxs (one per GPU / per thread, as torch.nn.DataParallel would drive the reference,
 * tfpnp/policy/sync_batchnorm/replicate.py:50-75) are independent.  Work is enqueued on the caller's
 * stream; no call synchronises the device except ctx creation, weight upload and workspace growth.
 */
#ifndef PNPX_H
#define PNPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pnpx_ctx pnpx_ctx; /* opaque: device id, packed UNet weights, workspaces, FFT tables */

enum pnpx_status {
  PNPX_OK = 0,
  PNPX_ERR_ARG = 1,         /* null pointer / non-positive size                                  */
  PNPX_ERR_SHAPE = 2,       /* unsupported geometry (e.g. FFT length > 2048, image side < 16)    */
  PNPX_ERR_NO_WEIGHTS = 3,  /* denoiser used before pnpx_unet_load                               */
  PNPX_ERR_ALLOC = 4,       /* device allocation failed                                          */
  PNPX_ERR_HIP = 5,         /* a HIP runtime call failed; see pnpx_last_error()                  */
  PNPX_ERR_RANGE = 6        /* half-split range guard tripped (pnpx_ctx_status)                  */
};

const char* pnpx_version(void);
const char* pnpx_last_error(void);

/* ---- context ------------------------------------------------------------------------------------- */
int pnpx_ctx_create(int device, pnpx_ctx** out);
int pnpx_ctx_destroy(pnpx_ctx* ctx);
/* Pre-size the internal workspaces for batches up to B of H x W images (optional; otherwise they
 * grow on first use, which synchronises the device once). */
int pnpx_ctx_reserve(pnpx_ctx* ctx, int B, int H, int W);
/* Options (the library reads no environment variables).
 *  "conv_mode": 0 (default since r6) = fp32 MFMA convolutions, the reference's own arithmetic (csrc/conv3x3_wino8.hip /
 *      conv3x3_wino.hip for the layers "fp32_winograd" covers, csrc/conv3x3.hip otherwise): inside 1e-4 of the fp32 oracle over a
 *      whole 30-iteration episode on every seed tested, also on expansive weights (profiles/r5_drift_seeds.md).
 *      1 = the FAST mode: half-split f16 MFMA convolutions (every value an f16 hi + lo pair = 22-bit significand, 3 MFMAs per
 *      product, csrc/conv_hs.hip): 1e-6-class per call and ~1.55x the episode rate, but narrower than fp32 -- on the chaotic
 *      expansive-weight episode 2 of 12 seeds end at 1.0e-4 / 1.24e-4 from the fp32 oracle (default-scale weights: 1e-6 both
 *      modes), and |v| < 4095 behind "range_guard".
 *  "fp32_winograd" (default 1): in conv_mode 0, layers with cout % 64 == 0 (sources % 16, H and W % 16) or cout % 32 == 0
 *      (sources % 8, H % 16, W % 32) run as Winograd F(2x2,3x3) in fp32 (1.3-1.8x per layer; 7e-7 from the fp64 oracle where
 *      the direct kernel is 1.1e-6 -- same accuracy class, different summation order).  0 = the direct kernel on every layer.
 *  "fp32_wino8_layers" (default: all 27 bits set): bit i = layer i of the UNet (state_dict order) runs on the 8-wave Winograd kernel
 *      (csrc/conv3x3_wino8.hip: the 16 positions of a block split over the two waves of a SIMD; forward and adjoint convolutions) where
 *      its geometry allows; 0 = the round-4 4-wave kernel (csrc/conv3x3_wino.hip) everywhere.  A DRUNet context: any bit.
 *  "fp32_winof4_layers" (27-bit layer mask like fp32_wino8_layers): bit i = layer i runs as Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32
 *      (csrc/conv3x3_winof4.hip: 0.5625 x the MFMAs of F(2x2)) in forward passes (inference and training alike), when its fp32_wino8_layers bit is set too,
 *      "fp32_winograd" is 1, the K-split does not claim the layer in this call and its geometry allows: a plain single-source layer with
 *      cout % 64 == 0, >= 16 input channels in multiples of 8, H % 16 == 0, W % 32 == 0 (UNet levels 1-3).  The backward pass,
 *      the DRUNet, the 16 x 16 level and the 32-cout layers always keep the F(2x2) kernel; the decoder entries do not listen to this
 *      mask (they have "fp32_winof4_entries").  0 = F(2x2) on every plain layer (bit-identical to the library before the option existed).
 *  "fp32_winof4_entries" (layer mask numbered like fp32_winof4_layers, 0 .. 2^27 - 1; only bits 15, 18 and 21 mean anything; default: see
 *      profiles/winof4_entries.md): bit i = decoder entry i (768 -> 256 at H/8, 384 -> 128 at H/4, 192 -> 64 at H/2) runs on the
 *      two-source instance of the F(4x4,3x3) kernel in forward passes, in the calls in which the 8-wave kernel would run it in one piece
 *      (its fp32_wino8_layers bit set, "fp32_winograd" 1, the K-split does not claim it) and where its geometry allows (cout % 64 == 0,
 *      H % 16 == 0, W % 32 == 0, both sources whole 8-channel chunks, at least one chunk of the first).  Unless
 *      "fp32_winof4_fuse_up" says otherwise the separate up-sampling kernel runs first, whatever "fp32_fuse_up" says.
 *      "fp32_winof4_layers" never moves an entry.  0 = the entries keep the F(2x2) kernel (bit-identical to the library before the option
 *      existed).
 *  "fp32_winof4_fuse_up" (layer mask numbered like fp32_winof4_entries, 0 .. 2^27 - 1; only bits 15, 18 and 21 mean anything; default:
 *      see profiles/winof4_fuse_up.md): bit i = where "fp32_winof4_entries" puts decoder entry i on the F(4x4,3x3) kernel, that kernel's
 *      third instance runs it: it takes the LOW-resolution second source, interpolates the bilinear x2 (align_corners) into its halo buffer
 *      itself and the up-sampling kernel is not launched.  It needs two 8-channel chunks of the first source (C0 >= 16); an entry without
 *      them, and every call in which the K-split claims the entry, stay as they are.  The result is bit-identical to the two-launch form
 *      (same floats for positions and weights, same rounding sequence), so 0 = the up-sampling kernel + the two-source instance, same bits.
 *  "fp32_winof4_c32" (layer mask numbered like fp32_winof4_layers; only bits 1, 2 and 25 are accepted; default: see
 *      profiles/winof4_c32.md): bit i = the full-resolution 32 -> 32 layer i (layer 2 with its fused max-pool) runs on the 32-cout instance
 *      of the F(4x4,3x3) kernel (a workgroup owns 32 couts x a region of 16 x 64 px) in forward passes, inference and training alike, when
 *      its fp32_wino8_layers bit is set, "fp32_winograd" is 1 and its geometry allows: a single source, cout % 32 == 0 and cout % 64 != 0,
 *      >= 16 input channels in multiples of 8, H % 16 == 0, W % 64 == 0.  The decoder entry 24, the last layer 26 (out-conv epilogue) and
 *      the backward pass keep the F(2x2) kernel.  0 = F(2x2) on these layers (bit-identical to the library before the option existed).
 *  "fp32_chains" (default 2): in conv_mode 0 the denoiser forward runs as n independent launch chains over contiguous slices of the batch
 *      (caller's stream + side streams, joined before the entry returns; bit-identical per image): 2 measured best (-3.6 % at 48 x 256^2,
 *      -7 % at B = 24); 1 = only the bottom level's three launches fork two chains; 0 = one chain.  The VJP's adjoint chain forks exactly
 *      two chains for every n >= 2.
 *  "fp32_fuse_up" (default 1): in conv_mode 0 the decoder-entry convolutions interpolate the bilinear x2 up-sampling of their second
 *      source inside the 8-wave kernel (tfpnp/pnp/denoiser/models/unet.py:92-121; no up-sampled tensor); 0 = the separate kernel
 *      (results agree to 5e-7).
 *  "fp32_ksplit" (default 1, r6): in conv_mode 0 the layers of the two deepest levels (<= 16 tiles of 64 couts x 16 x 16 px per image)
 *      can split their input-channel chunks over 4 / 2 workgroups of the 8-wave kernel; the pieces' partial sums go to a scratch slab and
 *      a second small launch adds them in piece order (deterministic), then bias + activation.
 *      1 = in calls whose unsplit tiles cannot fill the chip (tiles per image x batch < 256: below 32 images of 256 x 256 at the
 *      16 x 16 level, below 16 at 32 x 32; the 32 x 32 decoder entry then runs unfused so that it splits too): -20 % per forward at B = 6,
 *      -9 % at 12, nothing changes from 32 images up.  A given image
 *      gets the same bits in every call of the same class; across the class boundary results differ in the summation order
 *      (5e-7).  2 = split at every batch size: bit-identical per image across ALL batch sizes, +5 % at 48 x 256^2.  0 = never.
 *      "fp32_ksplit_rule" (tuning): pieces per tile class.
 *  "range_guard": the half-split kernels carry activations as f16 hi+lo pairs of 16*v, i.e. |v| < 4095.  Their
 *      epilogues set a sticky flag when a stored value leaves that range or is NaN.
 *      1 (default): the flag is looked at (no synchronisation) at the top of the next call; once seen, the context
 *         switches to conv_mode 0 for good and pnpx_ctx_status() returns PNPX_ERR_RANGE (the call that tripped it
 *         returned invalid numbers).  Setting the option again re-arms the guard.
 *      2 (strict): every denoiser / solver entry synchronises its stream before returning and, if the flag was set,
 *         repeats itself in conv_mode 0 -- the caller always receives valid output, at the price of a sync per call.
 *      0: off.
 *  "train_cache_gb" (default -1): device-memory budget of the training path's activation cache (see
 *      pnpx_csmri_admm_train); -1 = a quarter of the device memory free when the ring is first laid out, at most 96 GiB
 *      (the ring is raw device memory outside any framework allocator); 0 releases it and makes every backward
 *      re-compute.  "train_cache_release" (any value): give the ring's memory back now, budget unchanged.
 *  "wreg" (default 2): weights-in-registers instances of the 32 -> 32 channel convolutions (0 = generic kernel, 1 = four
 *      waves x four pixel blocks, 2 = eight waves x two pixel blocks); bit-identical results.
 *  "chains" (default 0 = automatic): run a denoiser forward (and the half-split VJP's adjoint chain) as n independent launch chains over
 *      slices of the batch on side streams; the convolution launch table picks its tile shapes for the chains running side by side.
 *      Automatic (r5): two chains from 5 images of 256 x 256 up (-4 % at B = 6, -13 % at 9-11, -6 % at 48; profiles/r5_chains_table_hs.txt).
 *      Bit-identical per image for every n.
 *  "fft_affine" (default 1), "fft_tile" (default 0 = 1024 points): XCD-affine image mapping and tile size of the FFT passes.
 *  "fft_fast" (default 1): N = 256 lines on the register-radix-16 kernels (0 = the generic Stockham passes; same results to rounding).
 *  "fuse_first" (default 1): the half-split family's first convolution reads the fp32 image and the noise level directly (no padded
 *      two-channel input tensor); 0 = separate input preparation + the generic kernel (bit-identical).
 *  "policy_s2_hs": accepted (0 or 1, reads back as 1) and without effect -- the fp32 entry kernel that 0 used to select for the policy
 *      actor's stem and stride-2 stage entries is gone, so a caller that sets it keeps running and gets the only path's results.
 *  "fold_first" (default 0): 1 = the network's first convolution is evaluated inside the tile loader of the second one
 *      (its output tensor is neither written nor read; bit-identical, time-neutral).
 *  "fuse_up" (default 1 since r5): 1 = the full-resolution decoder entry (96 -> 32 channels) up-samples its low-resolution source
 *      inside the convolution kernel (four producer waves per workgroup interpolate each K-chunk's halo into LDS), so the
 *      largest up-sampled tensor never exists in HBM.  Same arithmetic (bit-identical on the r5 build at every size tried,
 *      tools/ab_fuse_up.py; the test bound is 1e-6), forward 5.82 -> 5.76 ms at 48 x 256^2.  (conv_mode 0 has its own switch,
 *      "fp32_fuse_up", default 1: all four decoder entries interpolate inside the 8-wave Winograd kernel.)
 *      2 = opt-in: the 64-cout decoder entries too (8-row-tile instance; bit-identical, measured 3 % SLOWER than their separate
 *      up-sampling launches: profiles/r5_hs_fuse_up.md).
 *  "subbatch" (images per level-0 sub-batch, 0 = whole batch), "fuse_pool", "fuse_outc" (0/1): diagnostics. */
int pnpx_ctx_set_option(pnpx_ctx* ctx, const char* key, int value);
int pnpx_ctx_get_option(pnpx_ctx* ctx, const char* key, int* value);
/* PNPX_OK, or PNPX_ERR_RANGE once the range guard has tripped.  Does not synchronise: call it after a point where
 * the stream is known to have drained (e.g. after reading a result back). */
int pnpx_ctx_status(pnpx_ctx* ctx);
/* Bytes of device memory currently held by the context (weights + workspaces). */
size_t pnpx_ctx_bytes(const pnpx_ctx* ctx);

/* ---- denoiser prox: UNetDenoiser2D (tfpnp/pnp/denoiser/base.py:7-32, models/unet.py:34-66) ------- */
/* Number of fp32 parameters of UNet(2,1) (11 773 857) = length of the blob below. */
size_t pnpx_unet_num_params(void);
/* params_host: the reference state_dict's 56 tensors concatenated in state_dict order
 * (inc.conv.conv-0.conv2d.weight, ...bias, ..., outc.conv.weight, outc.conv.bias), each in its native
 * [Cout,Cin,kh,kw] layout -- i.e. what torch.load('unet-nm.pt') holds (denoiser/base.py:15-16).
 * Repacked on the host into the MFMA tile layout and uploaded. */
int pnpx_unet_load(pnpx_ctx* ctx, const float* params_host, size_t n_params);
/* out = clamp(UNet(cat[x, sigma*1]), 0, 1)   (denoiser/base.py:23-32).
 * x, out: [B,1,H,W]; sigma: [B]; out_preclamp (nullable): UNet output before the clamp.
 * Any H, W >= 16; odd level sizes follow the reference's floor-pool / zero-pad rule (models/unet.py:82-85,109-113). */
int pnpx_unet_denoise(pnpx_ctx* ctx, const float* x, const float* sigma, float* out, float* out_preclamp,
                      int B, int H, int W, void* stream);
/* ---- DRUNet denoiser (BASELINE config #5).  The reference ships only the KAIR building blocks
 * (tfpnp/pnp/denoiser/models/basicblock.py: conv :61-101, ResBlock :211-227, upsample_convtranspose :413-419,
 * downsample_strideconv :437-446); the topology is KAIR's UNetRes: bias-free, channels 64-128-256-512, nb ResBlocks per
 * scale each way, strided / transposed 2x2 convolutions, additive skips, input = cat[x, sigma*1], 1 output channel.
 * params_host: the state_dict's tensors concatenated in state_dict order (m_head.weight, m_down1.0.res.0.weight, ...,
 * m_tail.weight; key list: tfpnp_amd/synth.py::drunet_param_specs), native PyTorch layouts.
 * A context holds ONE denoiser: after pnpx_drunet_load every denoiser prox -- pnpx_unet_denoise and the denoiser call
 * inside every solver entry below -- runs the DRUNet (out = clamp(net(cat[x, sigma*1]), 0, 1), H and W multiples of 8);
 * pnpx_unet_load switches back.  The *_backward / *_train entries work too: a DRUNet context has no activation ring
 * (tickets are 0), its VJP re-computes the forward keeping every ResBlock's ReLU output and back-propagates on the same
 * kernel family.  conv_mode 0 runs the DRUNet in fp32 arithmetic throughout (csrc/drunet_f32.hip; forward and, since r5,
 * the *_backward / *_train entries).  Range guard: the bias-free ReLU network is positively homogeneous, so the first two trips
 * make later passes (range_guard 1) or the very call (range_guard 2, repeated) run on inputs scaled by 2^-4, then 2^-8, with the
 * tail multiplying back (option "drunet_shift" reads / sets the exponent: 0, 4 or 8; acknowledging a trip keeps it); a trip at
 * 2^-8 latches the context to conv_mode 0 like a UNet context. */
size_t pnpx_drunet_num_params(int nb);
int pnpx_drunet_load(pnpx_ctx* ctx, const float* params_host, size_t n_params, int nb);
/* Vector-Jacobian product of pnpx_unet_denoise wrt x and sigma (weights are frozen): given grad_out [B,1,H,W] returns
 * grad_x [B,1,H,W] and grad_sigma [B].  This is what autograd computes through UNetDenoiser2D.forward when the
 * reference differentiates the solver for policy training (tfpnp/env/base.py:193-206, trainer/mddpg/trainer.py:171-192).
 * The forward pass is re-computed internally in exact fp32 (gradient checkpointing); nothing is kept between calls. */
int pnpx_unet_denoise_backward(pnpx_ctx* ctx, const float* x, const float* sigma, const float* grad_out,
                               float* grad_x, float* grad_sigma, int B, int H, int W, void* stream);
/* The same pair for autograd graphs that hold many denoiser calls (the reference differentiates T solver iterations,
 * PnPEnv.forward -> solver.forward, tfpnp/env/base.py:193-206): pnpx_unet_denoise_train = pnpx_unet_denoise that also
 * parks every activation of this forward in the context's training ring and names it with *ticket (host memory; 0 when
 * the ring is off or out of budget); pnpx_unet_denoise_backward_ticket skips the re-computation when the ring still
 * holds that ticket and re-computes otherwise (ticket 0, slot re-used by a later forward, other weights) -- identical
 * result either way.  Ring length = "train_cache_gb" budget / arena size (5 GiB at 48 x 256^2), at most 64 slots. */
int pnpx_unet_denoise_train(pnpx_ctx* ctx, const float* x, const float* sigma, float* out, int B, int H, int W,
                            unsigned long long* ticket, void* stream);
int pnpx_unet_denoise_backward_ticket(pnpx_ctx* ctx, const float* x, const float* sigma, const float* grad_out,
                                      float* grad_x, float* grad_sigma, int B, int H, int W, unsigned long long ticket,
                                      void* stream);
/* Per-layer timing of one denoise call with HIP events on `stream` (synchronises).  ms_out[i] for the
 * i-th kernel launch of the forward pass, flops_out[i] its algorithmic FLOPs (0 for non-conv launches),
 * names_out[i] a static string.  Returns the number of entries written (<= cap) in *n_out. */
int pnpx_unet_profile(pnpx_ctx* ctx, const float* x, const float* sigma, float* out, int B, int H, int W,
                      void* stream, int cap, float* ms_out, double* flops_out, const char** names_out,
                      int* n_out);

/* ---- policy actor (tfpnp/policy/network.py) ------------------------------------------------------- */
/* ResNetActorBase (network.py:129-147) in eval mode: ResNet-18 encoder (network.py:87-125; BasicBlock :33-58;
 * SynchronizedBatchNorm2d on running statistics, sync_batchnorm/batchnorm.py:63-68) -> adaptive_avg_pool2d(1) ->
 * fc_softmax (Linear(512,2)+Softmax) and fc_deterministic (Linear(512,n_det)+Sigmoid; spi_head=1: the
 * Linear(512,64)-ReLU-Linear(64,n_det)-Sigmoid head of ResNetActor_SPI, network.py:262-268).
 * `params_host`: fp32 values of the module's state_dict in this order (integer num_batches_tracked entries skipped):
 *   actor_encoder.conv1.weight, actor_encoder.bn1.{weight,bias,running_mean,running_var},
 *   for L in layer1..layer4:  L.0.{conv1.weight, bn1.*, conv2.weight, bn2.*, shortcut.0.weight, shortcut.1.*},
 *                             L.1.{conv1.weight, bn1.*, conv2.weight, bn2.*},
 *   fc_softmax.0.{weight,bias}, fc_deterministic.0.{weight,bias} [, fc_deterministic.2.{weight,bias}]
 * where bn.* = weight, bias, running_mean, running_var.  num_inputs = channels of the policy observation
 * (env.get_policy_ob, e.g. tasks/csmri/env.py:14-23 -> 9), n_det = action_bundle * num_actions. */
size_t pnpx_policy_num_params(int num_inputs, int n_det, int spi_head);
int pnpx_policy_load(pnpx_ctx* ctx, const float* params_host, size_t n_params, int num_inputs, int n_det,
                     int spi_head);
/* ob [B,num_inputs,H,W] (device, contiguous; H, W multiples of 32) -> probs [B,2] (softmax over {continue, stop}),
 * det [B,n_det] (sigmoid outputs, before the action-range mapping of network.py:163-175). */
int pnpx_policy_forward(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W,
                        void* stream);
/* The weights are LIVE, as the critic's are: the context keeps the flat parameter vector on the device after either load entry.
 * pnpx_policy_load_device is pnpx_policy_load from a vector in DEVICE memory (same order, same length): the BatchNorm fold
 * (scale = weight / sqrt(running_var + 1e-5), shift = bias - running_mean * scale, in the host's fp32 roundings), the per-convolution
 * half-split scales and the packed layout the forward reads are derived by a handful of kernels on `stream`.  The outputs of pnpx_policy_forward equal those after pnpx_policy_load of the same values bit for bit.
 * The first call on a context, or one with another (num_inputs, n_det, spi_head), allocates; every later call refreshes in place:
 * no allocation, no device-wide synchronisation, the activation workspace is kept -- on a context that pnpx_policy_load loaded too
 * (the host packs the blob at the offsets the device packing writes to).  Each call ends with one small stream-ordered read-back of the 21 weight scales and a synchronisation of
 * `stream` (the launches take them by value).  A scale that is not finite -- running_var NaN or below -1e-5, a BatchNorm weight
 * that is not finite, a NaN convolution weight -- returns PNPX_ERR_ARG and leaves the context without an actor; a wrong n_params
 * returns PNPX_ERR_ARG and changes nothing.  Not capturable into a graph.
 * Stream rule: issue it on the stream the actor's other calls use.  A forward that ran as several launch chains (option "chains")
 * has joined its side streams back into its caller's stream by events before it returned, so a refresh on that stream is ordered
 * behind every launch of an earlier forward and ahead of a later one; no other stream is ordered against it.
 * params_dev may be dropped once the call returns. */
int pnpx_policy_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n_params, int num_inputs, int n_det, int spi_head,
                            void* stream);
/* Copies the live parameter vector (n_params floats, pnpx_policy_load's order) to dst_dev, ordered on `stream`.
 * PNPX_ERR_NO_WEIGHTS before a load. */
int pnpx_policy_params(pnpx_ctx* ctx, float* dst_dev, size_t n_params, void* stream);
/* The same network in TRAIN mode, as MDDPGTrainer._update runs the actor (trainer.py:128,171): each of the 20 BatchNorm layers
 * normalises with the statistics of the batch -- per channel over B * h * w raw convolution outputs z: mean, biased variance var_b,
 * y = (z - mean) / sqrt(var_b + 1e-5) * weight + bias -- which is F.batch_norm(training=True, momentum, eps = 1e-5); in block 0 of a
 * stage both summands of relu(bn2(conv2) + shortcut_bn(shortcut_conv)) use their own statistics.  Pool and heads are unchanged.
 * update_running != 0 moves the running statistics IN THE LIVE PARAMETER VECTOR (what pnpx_policy_params reads):
 *   running_mean <- (1 - momentum) * running_mean + momentum * mean,
 *   running_var  <- (1 - momentum) * running_var  + momentum * var_b * n / (n - 1);
 * the eval-mode packing is then re-derived once, by the next pnpx_policy_forward (not after every train forward).  With
 * update_running == 0 the parameter vector stays bit-identical.  num_batches_tracked is not kept: momentum is a number.
 * The convolutions run on a second, fold-free packing of the live vector, derived by the first call after a load (one stream
 * synchronisation, as pnpx_policy_load_device) together with a workspace that grows with B; eval-only users pay for neither.
 * Batch statistics couple the images: the call is ONE launch chain whatever option "chains" says, and its result is deterministic
 * (fixed-order reductions in double, no atomics).  Not capturable into a graph.
 * H, W multiples of 32 (else PNPX_ERR_SHAPE); PNPX_ERR_ARG when the last stage has B * (H/32) * (W/32) < 2 values per channel
 * (torch raises there) or momentum is outside [0, 1]; PNPX_ERR_NO_WEIGHTS before a load.  This call keeps nothing for a backward
 * pass (pnpx_policy_param_grad re-computes; pnpx_policy_forward_train_keep is the forward that keeps); the optimiser step is
 * pnpx_policy_adam_step.  Out of scope: statistics synchronised across devices. */
int pnpx_policy_forward_train(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                              int update_running, void* stream);
/* BatchNorm channels of the actor over its 20 layers in state_dict order (stem bn1, then per stage L.0.bn1, L.0.bn2,
 * L.0.shortcut.1, L.1.bn1, L.1.bn2): 4864. */
size_t pnpx_policy_num_bn_channels(void);
/* Batch mean and biased batch variance of the last pnpx_policy_forward_train, concatenated in that order, copied to mean_dev /
 * var_dev (n = pnpx_policy_num_bn_channels() floats each), ordered on `stream`.  PNPX_ERR_NO_WEIGHTS before any train forward. */
int pnpx_policy_bn_stats(pnpx_ctx* ctx, float* mean_dev, float* var_dev, size_t n, void* stream);
/* d sum(grad_probs * probs + grad_det * det) / d params, probs / det being what pnpx_policy_forward_train returns for `ob`
 * (batch-statistics BatchNorm): the actor's half of policy_loss.backward() (trainer.py:171-212), the counterpart of
 * pnpx_critic_param_grad.  grad_params has the layout of pnpx_policy_params (n_params floats); every element is written, the
 * running_mean / running_var slots as zeros.  All pointers are device pointers.  Changes no weights and no running statistics; the
 * batch statistics pnpx_policy_bn_stats reads afterwards are those of a train forward on `ob`.
 * The call re-computes the forward (nothing is kept from pnpx_policy_forward_train), then runs BatchNorm backward, the weight-gradient
 * GEMM and the adjoint convolution per layer.  Deterministic: fixed-order reductions in double, no floating-point atomics; the same bytes
 * on every call, whatever ran before.  Gradients travel scaled by a power of two chosen on the device from the upstream gradients:
 * the result is exactly homogeneous in powers of two of (grad_probs, grad_det), all-zero upstream gradients give an all-zero vector,
 * and there is no host read-back -- a call that grows no buffer allocates nothing and does not synchronise the device.  The first
 * call after a load derives the adjoint packings (and, if no train forward ran yet, the fold-free packing: one stream synchronisation).
 * Argument checks as pnpx_policy_forward_train; PNPX_ERR_ARG for a null pointer or n_params != pnpx_policy_num_params(...).
 * A forward kept by pnpx_policy_forward_train_keep is overwritten.  Out of scope: the observation's gradient, graph capture. */
int pnpx_policy_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_probs /* [B][2] */, const float* grad_det /* [B][n_det] */,
                           float* grad_params, size_t n_params, int B, int H, int W, void* stream);
/* The actor's update without the second forward (trainer.py:171, 201-204): a train-mode forward that is run once and keeps what the
 * backward pass reads, that backward pass, and the optimiser step on the live vector.
 *
 * pnpx_policy_forward_train_keep is pnpx_policy_forward_train -- the same launches, the same arguments and checks, and bit for bit
 * the same probs, det, batch statistics (pnpx_policy_bn_stats) and, with update_running, moved running statistics -- run in the
 * gradient workspace, where every raw convolution output and every activation stays.  The context records that this forward is
 * kept, for which B, H, W and for which capacity of the workspace.
 * pnpx_policy_param_grad_kept is then pnpx_policy_param_grad without its re-computation: heads, gradient range, and per layer
 * BatchNorm backward, weight-gradient GEMM and adjoint, on the kept tensors; grad_probs [B][2], grad_det [B][n_det] for the kept B.
 * grad_params receives the bytes pnpx_policy_param_grad(ob, ...) writes for the observation of the kept forward.  The backward pass
 * writes gradient tensors only, so it may be called any number of times on one kept forward (once per upstream gradient, say), each
 * time with the result of the re-computing call.
 * The kept forward ends with: any change of the trainable weights (pnpx_policy_load, pnpx_policy_load_device, pnpx_policy_adam_step
 * with a finite norm); pnpx_policy_forward_train, which overwrites the batch statistics the backward pass reads;
 * pnpx_policy_param_grad, which overwrites the workspace; a re-allocation of the workspace.  A later
 * pnpx_policy_forward_train_keep replaces it.  Moving the running statistics (either train forward's update_running, which the kept
 * forward itself may have asked for) does not end it: the backward pass reads neither them nor anything folded from them; nor do
 * pnpx_policy_forward and pnpx_policy_params.  Without a kept forward pnpx_policy_param_grad_kept returns PNPX_ERR_ARG, with a
 * message that says what ended it, and writes nothing.  PNPX_ERR_ARG also for a null pointer or a wrong n_params;
 * PNPX_ERR_NO_WEIGHTS before a load. */
int pnpx_policy_forward_train_keep(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                                   int update_running, void* stream);
int pnpx_policy_param_grad_kept(pnpx_ctx* ctx, const float* grad_probs /* [B][2] */, const float* grad_det /* [B][n_det] */,
                                float* grad_params, size_t n_params, void* stream);
/* clip_grad_norm_(actor.parameters(), max_norm) followed by Adam.step() (trainer.py:201-204; no weight decay, no amsgrad) in place on
 * the actor's live parameter vector: argument for argument pnpx_critic_adam_step (below), the same kernels, the same arithmetic,
 * the same rules for alignment, determinism, the moments' lifetime and the error codes, with two differences.
 * FROZEN RANGES: the running_mean / running_var slots of the vector are buffers of the reference module, not parameters, and neither
 * clip_grad_norm_ nor the optimiser sees them.  Whatever grad_dev holds there (pnpx_policy_param_grad writes zeros; garbage, an
 * infinity or a NaN are as good) adds nothing to the norm; the running statistics are not written, and the moments at those slots
 * stay zero.  pnpx_policy_frozen_ranges lists the ranges.
 * THE REFRESH is the actor's: what pnpx_policy_load_device does on the vector itself -- the eval-mode packing is re-derived at once
 * (its read-back carries the norm), the fold-free packing and its adjoints by the next train forward / gradient call, and a kept
 * forward ends.  The next forward of any kind reads the stepped weights.  A gradient whose norm is not finite returns PNPX_ERR_ARG:
 * parameters, moments, packed weights, the step counter and a kept forward are what they were.  The moments and the counter are
 * kept by pnpx_policy_load_device of the same (num_inputs, n_det, spi_head) and dropped by pnpx_policy_load, by a load of another
 * actor and with the context.
 * Out of scope: policy_loss itself (environment, critic, advantage: it stays with the caller), the trainer loop, weight decay /
 * amsgrad / other optimisers, loading the moments from a checkpoint, graph capture, statistics synchronised across devices. */
int pnpx_policy_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n_params, float lr, float beta1, float beta2, float eps,
                          float max_norm, float* grad_norm_dev, void* stream);
/* As pnpx_critic_optim_state / pnpx_critic_optim_reset, for the actor. */
int pnpx_policy_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n_params, long long* step_host,
                            void* stream);
int pnpx_policy_optim_reset(pnpx_ctx* ctx);
/* The frozen ranges of an actor's vector, sorted, adjacent ones merged (running_mean and running_var of a BatchNorm layer are one
 * range): elements [first[i], first[i] + count[i]).  Returns their number (21), writing at most `capacity` of them (first / count may
 * be NULL with capacity 0); -1 for a shape pnpx_policy_num_params refuses.  Needs no context and no device. */
int pnpx_policy_frozen_ranges(int num_inputs, int n_det, int spi_head, size_t* first, size_t* count, int capacity);

/* ---- value network / critic (tfpnp/trainer/mddpg/critic.py) --------------------------------------- */
/* ResNet_wobn(num_inputs, 18, 1) (critic.py:95-131; the trainer never builds another one, trainer/mddpg/critic.py:95 via
 * tasks/<task>/main.py): 3x3 stride-2 stem, four stages of two BasicBlocks (critic.py:37-60) each entered with stride 2 and a 1x1
 * stride-2 shortcut, adaptive_avg_pool2d(1), Linear(512, 1).  Convolutions are weight-normalised with bias
 * (weight = weight_g * weight_v / ||weight_v||, norm per output channel; critic.py:7-8); activations are TReLU
 * (relu(x - alpha) + alpha, one scalar alpha each; critic.py:11-19).  Gradients: with respect to the observation
 * (pnpx_critic_backward) and with respect to the parameters (pnpx_critic_param_grad, pnpx_critic_value_loss_grad); the optimiser step is
 * pnpx_critic_adam_step.  The weights are LIVE: the context keeps the raw parameter vector on the device, and
 * pnpx_critic_load_device / pnpx_critic_soft_update (below) replace or move it and re-derive the packed weights on the device.
 * pnpx_critic_load folds weight-norm and packs on the host (once per checkpoint).  One critic per context.
 * params_host: the fp32 content of state_dict() in registration order (82 tensors),
 *   conv1.{bias, weight_g, weight_v},
 *   for L in layer1..layer4:  L.0.{conv1.*, conv2.*, shortcut.0.*, relu_1.alpha, relu_2.alpha},
 *                             L.1.{conv1.*, conv2.*, relu_1.alpha, relu_2.alpha},
 *   fc.{weight, bias}, relu_1.alpha
 * where conv.* = bias, weight_g [cout,1,1,1], weight_v [cout,cin,k,k].  num_inputs = channels of the evaluation observation
 * (env.get_eval_ob, tfpnp/env/base.py; 1..64).  pnpx_critic_num_params returns 0 for a num_inputs outside that range. */
size_t pnpx_critic_num_params(int num_inputs);
int pnpx_critic_load(pnpx_ctx* ctx, const float* params_host, size_t n_params, int num_inputs);
/* The same load from a parameter vector in DEVICE memory (same order, same length): weight-norm fold, per-convolution scale and
 * both packings run as a handful of kernels on `stream` and produce the weight bytes pnpx_critic_load produces.  The first
 * load (or one with another num_inputs) allocates; every later call with the same num_inputs refreshes in place: no allocation,
 * no device-wide synchronisation, the activation workspace is kept.  Each call ends with one small stream-ordered read-back and
 * a synchronisation of `stream` (the launches take the weight scales and TReLU thresholds by value); a threshold that is not
 * finite returns PNPX_ERR_ARG and leaves the context without a critic, as pnpx_critic_load does.  Not capturable into a graph.
 * Must be issued on the stream the critic's other calls use: that stream alone orders the refresh behind earlier evaluations
 * and ahead of later ones.  params_dev may be dropped once the call returns. */
int pnpx_critic_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n_params, int num_inputs, void* stream);
/* utils/misc.py:81-85 soft_update with this critic as the target: params[i] = params[i] * one_minus_tau + src[i] * tau, the two
 * products and the sum each rounded to fp32 (what `target * (1.0 - tau) + source * tau` computes on fp32 tensors; pass
 * (float)(1.0 - tau) and (float)tau, computed in double), followed by the device-side refresh of pnpx_critic_load_device with
 * its stream rules and its read-back.  src_params_dev: n_params floats on the device in pnpx_critic_load's order.  Works on a
 * critic loaded by either entry; PNPX_ERR_NO_WEIGHTS before a load. */
int pnpx_critic_soft_update(pnpx_ctx* ctx, const float* src_params_dev, size_t n_params, float one_minus_tau, float tau,
                            void* stream);
/* Copies the live parameter vector (n_params floats, pnpx_critic_load's order) to dst_dev, ordered on `stream`.
 * PNPX_ERR_NO_WEIGHTS before a load. */
int pnpx_critic_params(pnpx_ctx* ctx, float* dst_dev, size_t n_params, void* stream);
/* ob [B,num_inputs,H,W] (device, contiguous; H, W positive multiples of 32) -> value [B] (critic.py:121-131).
 * PNPX_ERR_NO_WEIGHTS before a load.  A row's value does not depend on the batch it arrives in. */
int pnpx_critic_forward(pnpx_ctx* ctx, const float* ob, float* value, int B, int H, int W, void* stream);
/* Vector-Jacobian product of pnpx_critic_forward with respect to ob: grad_ob [B,num_inputs,H,W] = grad_value[b] * dV_b / d ob_b
 * (what autograd returns for V_next in trainer/mddpg/trainer.py:180-192).  The forward is re-computed internally; nothing is
 * kept between calls.  Exactly linear in grad_value (a zero entry gives a zero row). */
int pnpx_critic_backward(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_ob, int B, int H, int W,
                         void* stream);

/* Gradient of the critic's output with respect to its own parameters -- value_loss.backward() (trainer/mddpg/trainer.py:198,207):
 * grad_params[i] = d(sum_b grad_value[b] * V_b) / d(params[i]), n_params = pnpx_critic_num_params(num_inputs) floats on the device in
 * pnpx_critic_load's order (the 82 tensors, weight_g and weight_v separately, the 17 thresholds, fc).  Overwrites grad_params; does
 * not accumulate.  ob, grad_value, the shape rules and the error codes are those of pnpx_critic_backward; an n_params that does
 * not match the loaded critic returns PNPX_ERR_ARG.  The forward is re-computed internally and nothing is kept between calls.
 * Deterministic (two calls return the same bytes: the pixel axis is split into pieces that are added in a fixed order, no
 * atomics) and exactly linear in grad_value.  Its workspace belongs to the context and grows to the largest size seen; a call
 * that does not grow it allocates nothing and does not synchronise the device.  The native optimiser is pnpx_critic_adam_step;
 * any other one steps a flat parameter of its own and hands it to pnpx_critic_load_device. */
int pnpx_critic_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_params, size_t n_params, int B,
                           int H, int W, void* stream);
/* value_loss = nn.MSELoss()(Q_target, V_cur) and value_loss.backward() (trainer/mddpg/trainer.py:198,207) from ONE forward:
 * value [B] receives the bytes pnpx_critic_forward returns for ob, loss [1] = (sum_b (value[b] - q_target[b])^2) / B (fp32
 * squares added in index order), and grad_params what pnpx_critic_param_grad returns for
 * grad_value[b] = (2.0f * (value[b] - q_target[b])) * (float)(1.0 / B) -- the fp32 steps of torch's `2.0 * (V - Q) / B` on a
 * device tensor, which divides by a Python number as a product with the rounded reciprocal; that vector lives in the
 * context's workspace.  q_target [B] (device) is the detached target of trainer.py:181-186: it is not differentiated.
 * Shape rules, workspace growth, determinism and error codes are those of pnpx_critic_param_grad. */
int pnpx_critic_value_loss_grad(pnpx_ctx* ctx, const float* ob, const float* q_target, float* value, float* loss, float* grad_params,
                                size_t n_params, int B, int H, int W, void* stream);
/* clip_grad_norm_(critic.parameters(), max_norm) followed by Adam.step() (trainer.py:208-209; no weight decay, no amsgrad),
 * applied in place to the context's live parameter vector, then the device-side refresh pnpx_critic_load_device ends with.
 * grad_dev: n_params floats on the device in pnpx_critic_load's order (any 4-byte alignment; the result does not depend on it).
 * Element by element in fp32, torch's single-tensor Adam:
 *   g = grad * c,  m += (g - m) * (1 - beta1),  v = v * beta2 + (1 - beta2) * g * g,  p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)
 * with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) computed on the host in double from the context's step
 * counter t, and c = min(1, max_norm / (||grad||_2 + 1e-6)) over the whole vector (what clip_grad_norm_ computes from the 82
 * per-tensor norms); max_norm = INFINITY: no clipping.  The norm is summed in double in a fixed order (no atomics: two calls
 * give the same bytes) and never visits the host between the norm and the update.  grad_norm_dev (may be NULL) receives the norm
 * before clipping.  The moments exp_avg / exp_avg_sq (2 x n_params floats, zero-filled) and t live in the context: allocated by
 * the first step (the only one that synchronises the device), kept by every refresh with the same num_inputs
 * (pnpx_critic_load_device, pnpx_critic_soft_update) as overwriting param.data keeps a torch optimiser's state, dropped by a
 * load with another num_inputs, by pnpx_critic_load and with the context.
 * PNPX_ERR_NO_WEIGHTS before a load.  PNPX_ERR_ARG with nothing changed: a wrong n_params, lr negative or not finite, a beta
 * outside [0, 1), eps <= 0, max_norm <= 0.  A gradient whose norm is not finite also returns PNPX_ERR_ARG: parameters, moments,
 * packed weights and t are what they were and the critic stays usable.  Stream rules and "not capturable into a graph" are
 * those of pnpx_critic_load_device (one small read-back, which carries the norm). */
int pnpx_critic_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n_params, float lr, float beta1, float beta2, float eps,
                          float max_norm, float* grad_norm_dev, void* stream);
/* Copies exp_avg and exp_avg_sq (n_params floats each, device) out, ordered on `stream`, and writes t to *step_host (may be
 * NULL).  Before the first step: zeros and 0. */
int pnpx_critic_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n_params, long long* step_host,
                            void* stream);
/* Forgets the moments and t (the state before the first step).  Synchronises the device. */
int pnpx_critic_optim_reset(pnpx_ctx* ctx);

/* ---- MDDPG policy loss (tfpnp/trainer/mddpg/trainer.py:174, :179-197) and its backward (:202), ONE launch ------------------
 * Inputs on the device: p_stop [B][2] (the actor's softmax output), idx_stop [B] int64 (0 = continue; anything else counts as 1 =
 * stop), v_cur = critic(eval_ob), v_next_target = critic_target(eval_ob2), v_next = critic(eval_ob2), reward (as PnPEnv.forward
 * returns it: loop_penalty is subtracted here), [B] floats each.  Per row, eps = FLT_EPSILON:
 *   r = reward - loop_penalty;  g = discount * (1 - idx_stop);  logp = log(max(p_stop[idx_stop], eps));
 *   ent = -(xlogy(p0, p0) + xlogy(p1, p1));  Qt = g * v_next_target + r;  adv = Qt - v_cur (a constant of the backward pass);
 *   policy_loss = -(1 / B) * sum(logp * adv + (g * v_next + r) + lambda_e * ent)
 * Outputs: q_target, log_prob, entropy [B]; scalars [2] = {policy_loss, mean(entropy)}; the gradients of policy_loss:
 *   grad_v_next [B] = -g / B (exactly zero where idx_stop is 1), grad_reward [B] = -1 / B,
 *   grad_p_stop [B][2] = lambda_e * (log p_j + 1) / B at both entries, plus -adv / (B * p) at the taken entry where p >= eps
 *   (clamp_min's backward: nothing where p < eps).
 * Rows are fp32 in torch's order of operations without contraction (q_target has the bytes of the torch expression); the two sums
 * are taken in double in a fixed order by one workgroup, without atomics: two calls give the same bytes, whatever the alignment
 * of the pointers.  At p_j == 0 exactly the forward outputs are finite (xlogy(0, 0) = 0) and torch's gradient is NaN; this call
 * writes the formula's value there: -inf for lambda_e > 0, NaN for lambda_e == 0, +inf for lambda_e < 0.
 * PNPX_ERR_ARG with nothing written: B <= 0, a null pointer, a scalar that is not finite.  Keeps no state: ctx only names the
 * device.  Capturable into a graph. */
int pnpx_mddpg_policy_loss(pnpx_ctx* ctx, const float* p_stop, const int64_t* idx_stop, const float* v_cur, const float* v_next_target,
                           const float* v_next, const float* reward, float discount, float loop_penalty, float lambda_e, int B,
                           float* q_target, float* log_prob, float* entropy, float* scalars, float* grad_p_stop, float* grad_v_next,
                           float* grad_reward, void* stream);

/* ---- transforms (tfpnp/utils/transforms.py) ------------------------------------------------------ */
/* fft2 / ifft2 (transforms.py:68-103): centered (ifftshift -> FFT -> fftshift), orthonormal, over the
 * last two image dims of [n_img, H, W, 2].  centered=0 gives the plain torch.fft(x, 2, normalized=True)
 * used by cdp_forward/backward (transforms.py:300,318).  H, W in [1, 2048], any factorisation. */
int pnpx_fft2(pnpx_ctx* ctx, const float* in, float* out, int n_img, int H, int W, int inverse,
              int centered, void* stream);
/* cdp_forward (transforms.py:282-301): x [B,1,H,W,2], mask [B,S,H,W,2] -> out [B,S,H,W,2]. */
int pnpx_cdp_forward(pnpx_ctx* ctx, const float* x, const float* mask, float* out, int B, int S, int H,
                     int W, void* stream);
/* cdp_backward (transforms.py:304-320): y [B,S,H,W,2], mask [B,S,H,W,2] -> out [B,1,H,W,2] (mean over S). */
int pnpx_cdp_backward(pnpx_ctx* ctx, const float* y, const float* mask, float* out, int B, int S, int H,
                      int W, void* stream);
/* spi_inverse (transforms.py:404-439): ztilde, K1 [B,1,H,W]; K, mu [B] -> out [B,1,H,W]. */
int pnpx_spi_inverse(pnpx_ctx* ctx, const float* ztilde, const float* K1, const float* K, const float* mu,
                     float* out, int B, int H, int W, void* stream);
/* torch_psnr (tfpnp/env/base.py:237-242): output, gt [B,1,H,W] -> psnr [B]. */
int pnpx_psnr(pnpx_ctx* ctx, const float* output, const float* gt, float* psnr, int B, int n_per_item,
              void* stream);

/* ---- episode orchestration: the caller contract of PnPEnv.step (tfpnp/env/base.py:157-191) -------- */
/* Live-row gather `x[self.idx_left, ...]` (base.py:162-166) of n_tensors state tensors in ONE launch:
 * dst_t[r] = src_t[idx[r]] for r < n_rows, rows of row_bytes[t] bytes.  src_host / dst_host / row_bytes_host are HOST
 * arrays (of device pointers / sizes); idx is a device int64 array. */
int pnpx_rows_gather(pnpx_ctx* ctx, int n_tensors, const void* const* src_host, void* const* dst_host,
                     const size_t* row_bytes_host, const int64_t* idx, int n_rows, void* stream);
/* Write-back `state[...][self.idx_left, ...] = value` (base.py:171-172): dst_t[idx[r]] = src_t[r]. */
int pnpx_rows_scatter(pnpx_ctx* ctx, int n_tensors, const void* const* src_host, void* const* dst_host,
                      const size_t* row_bytes_host, const int64_t* idx, int n_rows, void* stream);
/* Replay-memory store: what `for i in range(B): buffer.store(ob[i])` (trainer/mddpg/trainer.py:232-234 over
 * tfpnp/utils/rpm.py:10-19) leaves behind, for every tensor of the observation at once:
 * dst_t[(first_slot + r) % capacity] = src_t[r] for r < n_rows; ONE launch per 12 tensors (and per 65535 rows).  The slot is
 * computed on the device in 64-bit integers -- no index array is built or uploaded -- and a store may wrap around the end of
 * the ring in the middle of a batch.  dst_t holds `capacity` rows of row_bytes[t] bytes.
 * Needs 0 <= first_slot < capacity and 0 <= n_rows <= capacity (two rows must never race for one slot): else PNPX_ERR_ARG
 * and nothing is written.  first_slot and capacity are launch ARGUMENTS, so a captured graph replays the slot it was
 * captured with: with a moving head this call is not graph-capturable.  Sampling needs no entry of its own: it is
 * pnpx_rows_gather with a device list of slots. */
int pnpx_ring_store(pnpx_ctx* ctx, int n_tensors, const void* const* src_host, void* const* dst_host,
                    const size_t* row_bytes_host, int64_t first_slot, int64_t capacity, int n_rows, void* stream);
/* `self.idx_left = self.idx_left[idx_stop == 0]; all_done = len(self.idx_left) == 0` (base.py:180-182) as a
 * device-side stream compaction: idx_out[0..n_live) = the idx_left[i] with idx_stop[i] == 0 (int64, in order).
 * *n_live_host receives the count: this call SYNCHRONISES `stream` -- it is the one host read of an env step
 * (`all_done` is a Python bool in the reference's contract). */
int pnpx_live_compact(pnpx_ctx* ctx, const int64_t* idx_left, const int64_t* idx_stop, int n, int64_t* idx_out,
                      int* n_live_host, void* stream);
/* Policy observation (get_policy_ob: tasks/csmri/env.py:14-23, tasks/pr/env.py:14-21, tasks/ct/env.py:13-20,
 * tasks/spi/env.py:12-19): channel-concatenation of n_entries (<= 12) state tensors, each viewed as
 *   kind 0: fp32 [B,c,H,W] as is;  1: complex2real of [B,c,H,W,2] (transforms.py:16-17);
 *   kind 2: complex2channel of [B,c,H,W,2] (re, im of channel j -> channels 2j, 2j+1; transforms.py:20-26);
 *   kind 3: uint8 / bool [B,c,H,W] cast to float
 * into out [n_rows, sum(channels), H, W].  Row r reads source row idx[r] (idx == NULL: row r). */
int pnpx_policy_ob_pack(pnpx_ctx* ctx, int n_entries, const void* const* src_host, const int* kind_host,
                        const int* channels_host, const int64_t* idx, int n_rows, int H, int W, float* out,
                        void* stream);

/* Adjoint of pnpx_policy_ob_pack for dense rows (what autograd computes through get_policy_ob / get_eval_ob when the observation
 * feeds the critic, tfpnp/env/base.py:193-206 + trainer/mddpg/trainer.py:180-192): grad_out [n_rows, sum(channels), H, W] ->
 * per entry t the tensor dst_host[t] with the shape of the entry's source,
 *   kind 0: the same channels;  kind 1: real part = gradient, imaginary part = 0;  kind 2: re / im interleaved back;
 *   kind 3 (bool / uint8 sources have no gradient): nothing is written, dst_host[t] may be NULL.
 * kind_host / channels_host as given to the pack.  One launch. */
int pnpx_policy_ob_unpack(pnpx_ctx* ctx, int n_entries, void* const* dst_host, const int* kind_host,
                          const int* channels_host, int n_rows, int H, int W, const float* grad_out, void* stream);

/* ---- solver loops: T inner iterations per call ---------------------------------------------------- */
/* Hyper-parameter arrays are [B, param_stride] row-major (the policy's [B, action_pack] tensors,
 * tfpnp/policy/network.py:164-175); iteration i reads column i.  vars_in is never modified; vars_out
 * may not alias it. */

/* ADMMSolver_CSMRI.forward (tasks/csmri/solver.py:29-57).
 * vars [B,3,H,W,2] = cat(x,z,u); y0 [B,1,H,W,2]; mask [B,1,H,W] bytes. */
int pnpx_csmri_admm(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                    const uint8_t* mask, const float* sigma_d, const float* mu, int param_stride, int B,
                    int H, int W, int T, void* stream);
/* Training path of the same call: what autograd records and replays when the reference differentiates
 * ADMMSolver_CSMRI.forward for policy training (PnPEnv.forward, tfpnp/env/base.py:193-206, called from
 * trainer/mddpg/trainer.py:171-192).
 * pnpx_csmri_admm_train = pnpx_csmri_admm (bit-identical vars_out) that also fills `saved`, 3*T*B*H*W floats: the
 *   denoiser input of every iteration [T][B][H*W] followed by the k-space image before the blend [T][B][H*W][2].
 * pnpx_csmri_admm_backward: given grad_vars_out [B,3,H,W,2] returns grad_vars_in [B,3,H,W,2] (may not alias),
 *   grad_sigma_d [T][B] and grad_mu [T][B] (iteration-major, dense); `work` is 3*B*H*W floats of caller workspace.
 *   The denoiser weights are constants (frozen, as in the reference); y0 / mask get no gradient.  Per iteration: one
 *   masked-FFT adjoint (same three fused passes as the forward), one deterministic per-item reduction (d/d mu) and the
 *   denoiser VJP (pnpx_unet_denoise_backward's kernels).
 * Activation ring: every iteration's denoiser forward is a pnpx_unet_denoise_train call (above), so within the
 *   "train_cache_gb" budget (default 96 GiB; ~5 GiB per 48 x 256^2 iteration -- the 288 GB of an MI355X are what make
 *   this affordable) the backward pass does not re-compute the denoiser forwards (8 instead of 14.5 ms per iteration at
 *   48 x 256^2).  *ticket (host memory, written before the call returns) is iteration 0's ticket, iteration i holds
 *   ticket + i; slots that a later training forward has re-used are answered by re-computation from `saved` -- same
 *   gradients, never stale ones. */
int pnpx_csmri_admm_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                          const uint8_t* mask, const float* sigma_d, const float* mu, int param_stride, int B,
                          int H, int W, int T, float* saved, unsigned long long* ticket, void* stream);
int pnpx_csmri_admm_backward(pnpx_ctx* ctx, const float* y0, const uint8_t* mask, const float* sigma_d,
                             const float* mu, int param_stride, const float* saved, const float* grad_vars_out,
                             float* grad_vars_in, float* grad_sigma_d, float* grad_mu, float* work, int B, int H,
                             int W, int T, unsigned long long ticket, void* stream);
/* HQSSolver_CSMRI.forward (tasks/csmri/solver.py:64-89).  vars [B,2,H,W,2] = cat(x,z). */
int pnpx_csmri_hqs(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                   const uint8_t* mask, const float* sigma_d, const float* mu, int param_stride, int B,
                   int H, int W, int T, void* stream);
/* Training path of HQSSolver_CSMRI.forward, same contract as pnpx_csmri_admm_train / _backward above with vars
 * [B,2,H,W,2]: `saved` = 3*T*B*H*W floats (denoiser inputs, then the k-space images before the blend), activations parked
 * under *ticket + i; the backward returns grad_vars_in [B,2,H,W,2], grad_sigma_d and grad_mu [T][B], work = 3*B*H*W floats. */
int pnpx_csmri_hqs_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                         const uint8_t* mask, const float* sigma_d, const float* mu, int param_stride, int B,
                         int H, int W, int T, float* saved, unsigned long long* ticket, void* stream);
int pnpx_csmri_hqs_backward(pnpx_ctx* ctx, const float* y0, const uint8_t* mask, const float* sigma_d,
                            const float* mu, int param_stride, const float* saved, const float* grad_vars_out,
                            float* grad_vars_in, float* grad_sigma_d, float* grad_mu, float* work, int B, int H,
                            int W, int T, unsigned long long ticket, void* stream);
/* PGSolver_CSMRI.forward (tasks/csmri/solver.py:96-120).  vars [B,1,H,W,2] = x. */
int pnpx_csmri_pg(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                  const uint8_t* mask, const float* sigma_d, const float* tau, int param_stride, int B,
                  int H, int W, int T, void* stream);
/* Training path of PGSolver_CSMRI.forward (same contract; vars [B,1,H,W,2]): `saved` = 2*T*B*H*W floats (the denoiser inputs,
 * then the real parts of the masked-residual images ifft2c(mask * (fft2c(x_i) - y0))); grads wrt (x, sigma_d, tau). */
int pnpx_csmri_pg_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                        const uint8_t* mask, const float* sigma_d, const float* tau, int param_stride, int B,
                        int H, int W, int T, float* saved, unsigned long long* ticket, void* stream);
int pnpx_csmri_pg_backward(pnpx_ctx* ctx, const float* y0, const uint8_t* mask, const float* sigma_d,
                           const float* tau, int param_stride, const float* saved, const float* grad_vars_out,
                           float* grad_vars_in, float* grad_sigma_d, float* grad_tau, float* work, int B, int H,
                           int W, int T, unsigned long long ticket, void* stream);
/* APGSolver_CSMRI.forward (tasks/csmri/solver.py:127-165).  vars [B,2,H,W,2] = cat(x,s). */
int pnpx_csmri_apg(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                   const uint8_t* mask, const float* sigma_d, const float* tau, const float* beta,
                   int param_stride, int B, int H, int W, int T, void* stream);
/* Training path of APGSolver_CSMRI.forward (same contract; vars [B,2,H,W,2]): `saved` = 4*T*B*H*W floats (denoiser inputs,
 * real parts of the masked-residual images, x' - x_prev as complex); grads wrt (cat(x, s), sigma_d, tau, beta); work =
 * 4*B*H*W floats. */
int pnpx_csmri_apg_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                         const uint8_t* mask, const float* sigma_d, const float* tau, const float* beta,
                         int param_stride, int B, int H, int W, int T, float* saved, unsigned long long* ticket,
                         void* stream);
int pnpx_csmri_apg_backward(pnpx_ctx* ctx, const float* y0, const uint8_t* mask, const float* sigma_d,
                            const float* tau, const float* beta, int param_stride, const float* saved,
                            const float* grad_vars_out, float* grad_vars_in, float* grad_sigma_d, float* grad_tau,
                            float* grad_beta, float* work, int B, int H, int W, int T, unsigned long long ticket,
                            void* stream);
/* REDADMMSolver_CSMRI.forward (tasks/csmri/solver.py:172-204).  vars [B,3,H,W,2]. */
int pnpx_csmri_redadmm(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                       const uint8_t* mask, const float* sigma_d, const float* mu, const float* lamda,
                       int param_stride, int B, int H, int W, int T, void* stream);
/* Training path of REDADMMSolver_CSMRI.forward (same contract; vars [B,3,H,W,2]): `saved` = 7*T*B*H*W floats (denoiser
 * inputs Re x, the k-space images before the blend, r2c(xh) - x' and (z - u) - x' as complex); grads wrt (cat(x, z, u),
 * sigma_d, mu, lamda); work = 4*B*H*W floats. */
int pnpx_csmri_redadmm_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                             const uint8_t* mask, const float* sigma_d, const float* mu, const float* lamda,
                             int param_stride, int B, int H, int W, int T, float* saved, unsigned long long* ticket,
                             void* stream);
int pnpx_csmri_redadmm_backward(pnpx_ctx* ctx, const float* y0, const uint8_t* mask, const float* sigma_d,
                                const float* mu, const float* lamda, int param_stride, const float* saved,
                                const float* grad_vars_out, float* grad_vars_in, float* grad_sigma_d, float* grad_mu,
                                float* grad_lamda, float* work, int B, int H, int W, int T, unsigned long long ticket,
                                void* stream);
/* AMPSolver_CSMRI.forward (tasks/csmri/solver.py:211-250), inference only.  vars [B,2,H,W,2] = cat(x,z); sigma_d [B,T]
 * (row stride param_stride); probe [T,B,1,H,W] = the reference's torch.randn_like(r) draw of each iteration (:237).
 * The reference calls two undefined names; this entry runs its loop with them supplied: self.prox_fun (:238) is
 * self.prox_mapping (the context's denoiser), and transforms.complex_norm(z) (:230) is, per item, the square root of the
 * sum of z^2 over its [1,H,W,2] entries.  eps = max(r) / 1000 + 1e-8 is taken over all B items of the call.  Both
 * denoiser evaluations of an iteration run as one denoiser call over 2B items; eps stays on the device (capturable). */
int pnpx_csmri_amp(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const uint8_t* mask,
                   const float* sigma_d, const float* probe, int param_stride, int B, int H, int W, int T,
                   void* stream);
/* IADMMSolver_PR.forward (tasks/pr/solver.py:37-76).
 * vars [B,3,H,W,2]; y0 [B,S,H,W]; mask [B,S,H,W,2]. */
int pnpx_pr_iadmm(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0,
                  const float* mask, const float* sigma_d, const float* mu, const float* tau,
                  int param_stride, int B, int S, int H, int W, int T, void* stream);
/* Training path of IADMMSolver_PR.forward (same contract): `saved` = (2*S + 5)*T*B*H*W floats (denoiser inputs, the S
 * k-space images before the residual, g + mu (z - (x + u)) and z - (x + u) as complex); grads wrt (cat(x, z, u), sigma_d,
 * mu, tau), each hyper-parameter gradient [T][B]; work = 4*B*H*W floats.  ticket as in pnpx_csmri_admm_train. */
int pnpx_pr_iadmm_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const float* mask,
                        const float* sigma_d, const float* mu, const float* tau, int param_stride, int B, int S,
                        int H, int W, int T, float* saved, unsigned long long* ticket, void* stream);
int pnpx_pr_iadmm_backward(pnpx_ctx* ctx, const float* y0, const float* mask, const float* sigma_d, const float* mu,
                           const float* tau, int param_stride, const float* saved, const float* grad_vars_out,
                           float* grad_vars_in, float* grad_sigma_d, float* grad_mu, float* grad_tau, float* work,
                           int B, int S, int H, int W, int T, unsigned long long ticket, void* stream);
/* PGSolver_PR.forward: proximal gradient on the PR data term.  The reference's own loop (tasks/pr/solver.py:79-112) was pasted
 * from CS-MRI and raises on any PR input; this entry runs it with the gradient step IADMMSolver_PR.forward computes (:61-68):
 *   Ax = cdp_forward(x, mask);  r = (|Ax| - y0) / |Ax| * Ax  (no epsilon);  z = x - tau_i * cdp_backward(r, mask);
 *   x  = real2complex(prox_mapping(complex2real(z), sigma_d_i))
 * vars [B,1,H,W,2]; y0 [B,S,H,W]; mask [B,S,H,W,2]; sigma_d, tau [B,T] (row stride param_stride).  vars_in may carry an
 * imaginary part (the first iteration reads it); the imaginary part of vars_out is +0.  T = 0 copies the state. */
int pnpx_pr_pg(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const float* mask,
               const float* sigma_d, const float* tau, int param_stride, int B, int S, int H, int W, int T,
               void* stream);
/* Training path of PGSolver_PR.forward (same contract): `saved` = (2*S + 2)*T*B*H*W floats (the S k-space images before the
 * residual as complex, then the denoiser inputs, then Re of the data-term gradient); grads wrt (x, sigma_d, tau), each
 * hyper-parameter gradient [T][B]; work = 3*B*H*W floats.  The imaginary part of grad_vars_out is not read (the output's
 * imaginary part is a constant).  ticket as in pnpx_csmri_admm_train. */
int pnpx_pr_pg_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const float* mask,
                     const float* sigma_d, const float* tau, int param_stride, int B, int S, int H, int W, int T,
                     float* saved, unsigned long long* ticket, void* stream);
int pnpx_pr_pg_backward(pnpx_ctx* ctx, const float* y0, const float* mask, const float* sigma_d, const float* tau,
                        int param_stride, const float* saved, const float* grad_vars_out, float* grad_vars_in,
                        float* grad_sigma_d, float* grad_tau, float* work, int B, int S, int H, int W, int T,
                        unsigned long long ticket, void* stream);
/* ADMMSolver_SPI.forward (tasks/spi/solver.py:17-52).
 * vars [B,3,H,W] real; x0 [B,1,H,W]; Kmap [B,1,H,W] (K/10 broadcast, only [b,0,0,0] is read). */
int pnpx_spi_admm(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* x0,
                  const float* Kmap, const float* sigma_d, const float* mu, int param_stride, int B, int H,
                  int W, int T, void* stream);
/* Training path of ADMMSolver_SPI.forward (same contract): `saved` = 2*T*B*H*W floats (x + u and the denoiser inputs); grads
 * wrt (cat(x, z, u), sigma_d, mu), hyper-parameter gradients [T][B]; work = 3*B*H*W floats.  As in the reference the bisection
 * branch of spi_inverse carries no gradient (transforms.py:404-439), only its K1 == 0 branch does. */
int pnpx_spi_admm_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* x0, const float* Kmap,
                        const float* sigma_d, const float* mu, int param_stride, int B, int H, int W, int T,
                        float* saved, unsigned long long* ticket, void* stream);
int pnpx_spi_admm_backward(pnpx_ctx* ctx, const float* x0, const float* Kmap, const float* sigma_d, const float* mu,
                           int param_stride, const float* saved, const float* grad_vars_out, float* grad_vars_in,
                           float* grad_sigma_d, float* grad_mu, float* work, int B, int H, int W, int T,
                           unsigned long long ticket, void* stream);
/* PGSolver_SPI: proximal gradient on the SPI data term.  The reference has no counterpart (tasks/spi/solver.py stops at ADMM);
 * the step is this package's own, on the likelihood behind spi_inverse (transforms.py:404-439, func) divided by K^2:
 *   f(x) = (1 - x0) x - x0 log(1 - e^-x);   K = 10 Kmap[b,0,0,0];  x_lo = 0.5 / K^2;  x_c = max(x, x_lo);  q = -expm1(-x_c);
 *   g = 1 - x0 / q  (= f');  c = x0 (1 - q) / q^2  (= f'');  h = g / max(c, 1);  z = clamp(x - tau h, 0, 1)
 * (the gradient step where f'' < 1, the damped Newton step where f'' >= 1).
 * pnpx_spi_pg_step is that one step alone, the counterpart of pnpx_spi_inverse: x, x0 [B,1,H,W]; Kmap [B,1,H,W] (only
 * [b,0,0,0] is read); tau [B] -> out = z [B,1,H,W]. */
int pnpx_spi_pg_step(pnpx_ctx* ctx, const float* x, const float* x0, const float* Kmap, const float* tau, float* out, int B,
                     int H, int W, void* stream);
/* PGSolver_SPI.forward: per iteration i, x <- D(z(x, tau_i), sigma_d_i).  vars [B,1,H,W] real; x0, Kmap as above; sigma_d, tau
 * [B,T] (row stride param_stride >= T).  T = 0 copies the state. */
int pnpx_spi_pg(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* x0, const float* Kmap,
                const float* sigma_d, const float* tau, int param_stride, int B, int H, int W, int T, void* stream);
/* Training path of PGSolver_SPI.forward (same contract): `saved` = 2*T*B*H*W floats (x of every iteration, then the denoiser
 * inputs); grads wrt (x, sigma_d, tau), each hyper-parameter gradient [T][B] as in pnpx_pr_pg_backward; work = 3*B*H*W floats.
 * The VJP is that of the expression above with torch.clamp's rule (closed intervals pass); x0 and Kmap get no gradient; the tau
 * term is summed per item in a fixed order (no atomics: two runs give equal bytes).  ticket as in pnpx_csmri_admm_train. */
int pnpx_spi_pg_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* x0, const float* Kmap,
                      const float* sigma_d, const float* tau, int param_stride, int B, int H, int W, int T, float* saved,
                      unsigned long long* ticket, void* stream);
int pnpx_spi_pg_backward(pnpx_ctx* ctx, const float* x0, const float* Kmap, const float* sigma_d, const float* tau,
                         int param_stride, const float* saved, const float* grad_vars_out, float* grad_vars_in,
                         float* grad_sigma_d, float* grad_tau, float* work, int B, int H, int W, int T,
                         unsigned long long ticket, void* stream);

/* ---- CT: Radon pair standing in for torch_radon (tfpnp/utils/transforms.py:465-508) -------------- */
/* Parallel beam, angles = linspace(0, 179/180*pi, n_view), det = ceil(sqrt(2)*R), unit spacing
 * (transforms.py:487-491).  img [B,1,R,R] <-> sino [B,1,n_view,det].  Discretisation: DESIGN.md. */
int pnpx_radon_det_count(int R);
int pnpx_radon_forward(pnpx_ctx* ctx, const float* img, float* sino, int B, int R, int n_view, void* stream);
int pnpx_radon_backprojection(pnpx_ctx* ctx, const float* sino, float* img, int B, int R, int n_view,
                              void* stream);
/* IADMMSolver_CT.forward (tasks/ct/solver.py:17-53); opnorm = Radon_norm.opnorm (transforms.py:470-474).
 * vars [B,3,R,R] real; y0 [B,1,n_view,det]. */
int pnpx_ct_iadmm(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, int n_view,
                  float opnorm, const float* sigma_d, const float* mu, const float* tau, int param_stride,
                  int B, int R, int T, void* stream);
/* Training path of IADMMSolver_CT.forward: `saved` = 3*T*B*R*R floats; grads wrt (cat(x, z, u), sigma_d, mu, tau);
 * work = 6*B*R*R + 2*n_view floats. */
int pnpx_ct_iadmm_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, int n_view,
                        float opnorm, const float* sigma_d, const float* mu, const float* tau, int param_stride, int B,
                        int R, int T, float* saved, unsigned long long* ticket, void* stream);
int pnpx_ct_iadmm_backward(pnpx_ctx* ctx, int n_view, float opnorm, const float* sigma_d, const float* mu,
                           const float* tau, int param_stride, const float* saved, const float* grad_vars_out,
                           float* grad_vars_in, float* grad_sigma_d, float* grad_mu, float* grad_tau, float* work,
                           int B, int R, int T, unsigned long long ticket, void* stream);
/* PGSolver_CT.forward (tasks/ct/solver.py:61-87).  vars [B,1,R,R]. */
int pnpx_ct_pg(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, int n_view,
               float opnorm, const float* sigma_d, const float* tau, int param_stride, int B, int R, int T,
               void* stream);
/* Training path of PGSolver_CT.forward: `saved` = 2*T*B*R*R floats; grads wrt (x, sigma_d, tau); work = 3*B*R*R + 1 + 2*n_view
 * floats. */
int pnpx_ct_pg_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, int n_view, float opnorm,
                     const float* sigma_d, const float* tau, int param_stride, int B, int R, int T, float* saved,
                     unsigned long long* ticket, void* stream);
int pnpx_ct_pg_backward(pnpx_ctx* ctx, int n_view, float opnorm, const float* sigma_d, const float* tau,
                        int param_stride, const float* saved, const float* grad_vars_out, float* grad_vars_in,
                        float* grad_sigma_d, float* grad_tau, float* work, int B, int R, int T,
                        unsigned long long ticket, void* stream);

/* ---- CT, fan beam: flat detector, full circle (own discretisation: DESIGN.md section 7) ---------------------------------------
 * Centred pixel units (x = column - (R/2 - 0.5), y = row - (R/2 - 0.5)), e_s(b) = (cos b, sin b), e_t(b) = (-sin b, cos b).  View v
 * has beta_v = 2 pi v / n_view; the source sits at -source_distance e_t, bin j is centred at det_distance e_t + u_j e_s with
 * u_j = (j - det_count/2 + 0.5) det_spacing; D = source_distance + det_distance.
 *   forward (ray-driven): ray (v, j) is the parallel-beam ray of angle beta_v - gamma_j (tan gamma_j = u_j / D) and offset
 *     source_distance sin gamma_j, sampled at the parallel projector's n = pnpx_radon_det_count(R) unit steps (bilinear, zero outside);
 *   backprojection (pixel-driven): per pixel and view s = x cos b + y sin b, t = -x sin b + y cos b, U = source_distance + t,
 *     u = s D / U, linear interpolation at bin u / det_spacing + det_count/2 - 0.5 (zero outside), times
 *     w = sqrt(D^2 + u^2) / (U det_spacing), the reciprocal spacing of the fan's rays at the pixel: with it the pair is adjoint to
 *     1e-5 on smooth images, as the parallel pair is.
 * Refused, with a message and nothing launched: source_distance < n/2 + 1 (the source would stand inside the sampled span) and
 * det_count < 2 (or > 2^20) with PNPX_ERR_SHAPE; det_spacing <= 0, det_distance < 0, a value that is not finite, n_view <= 0,
 * R <= 0 and a struct that is NULL or not of kind PNPX_GEOM_FAN with PNPX_ERR_ARG. */
enum { PNPX_GEOM_PARALLEL = 0, PNPX_GEOM_FAN = 1 };
typedef struct pnpx_radon_geom {
  int kind;      /* PNPX_GEOM_PARALLEL: the other fields are not read */
  int n_view;
  int det_count;
  float source_distance, det_distance, det_spacing;
} pnpx_radon_geom;
/* The default bin count: the fan that just covers the sampled circle, ceil(2 D tan(asin((n/2) / source_distance)) / det_spacing).
 * 0 with a message for a geometry the entries refuse.  Host only. */
int pnpx_fan_det_count(int R, float source_distance, float det_distance, float det_spacing);
/* img [B,1,R,R] <-> sino [B,1,n_view,det_count]. */
int pnpx_fan_forward(pnpx_ctx* ctx, const float* img, float* sino, const pnpx_radon_geom* geom, int B, int R, void* stream);
int pnpx_fan_backprojection(pnpx_ctx* ctx, const float* sino, float* img, const pnpx_radon_geom* geom, int B, int R,
                            void* stream);
/* Host only, for tests: the tables the kernels read -- view_cs [n_view][2] = (cos, sin) of beta_v rounded to fp32, bins [det_count][3]
 * = (cos gamma_j, sin gamma_j, source_distance sin gamma_j) -- and *window = the bins per view and 32 x 32 tile that the LDS
 * backprojection kernel stages (0: n_view windows exceed its 60 KiB and the per-pixel gather kernel runs; same bytes).  Any
 * output may be NULL.  Refuses what the entries refuse; needs no device. */
int pnpx_fan_tables(const pnpx_radon_geom* geom, int R, float* view_cs, float* bins, int* window);
/* HQS for CT (HQSSolver_CT): state cat(x, z) [B,2,R,R], hyper-parameters (sigma_d, mu).  Per iteration x = D(z, sigma_d_i), then
 * z <- z - (A^T(A z - y0) / opnorm^2 + mu_i (z - x)) / (1 + mu_i): the reference's inexact data step (tasks/ct/solver.py:46-49)
 * without the dual, with the step 1 / (1 + mu).  geom NULL or of kind PNPX_GEOM_PARALLEL: the parallel pair, y0 [B,1,n_view,det];
 * a fan geometry (its n_view must equal n_view): y0 [B,1,n_view,det_count].  opnorm as for pnpx_ct_iadmm, of the pair in use. */
int pnpx_ct_hqs(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const pnpx_radon_geom* geom, int n_view,
                float opnorm, const float* sigma_d, const float* mu, int param_stride, int B, int R, int T, void* stream);
/* Training path: `saved` = 3*T*B*R*R floats; grads wrt (cat(x, z), sigma_d, mu), hyper-parameter gradients [T][B];
 * work = 5*B*R*R + 4 + 2*n_view floats, plus 4*det_count with a fan geometry. */
int pnpx_ct_hqs_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const pnpx_radon_geom* geom,
                      int n_view, float opnorm, const float* sigma_d, const float* mu, int param_stride, int B, int R, int T,
                      float* saved, unsigned long long* ticket, void* stream);
int pnpx_ct_hqs_backward(pnpx_ctx* ctx, const pnpx_radon_geom* geom, int n_view, float opnorm, const float* sigma_d,
                         const float* mu, int param_stride, const float* saved, const float* grad_vars_out, float* grad_vars_in,
                         float* grad_sigma_d, float* grad_mu, float* work, int B, int R, int T, unsigned long long ticket,
                         void* stream);

/* ---- CT, filtered backprojection of a fan-beam sinogram (Kak & Slaney section 3.4.2, equispaced flat detector, full circle)
 *   fbp(y)(x, y) = sum over views v of (D_so / U)^2 * lerp(q_v, pos),   U and pos as in the fan backprojection above,
 *   q_v[j] = S * sum over m, ascending, of (y_v[m] c[m]) h[j - m],   c[m] = cos gamma_m = D / sqrt(D^2 + u_m^2),
 *   h[0] = 1/4, h[odd n] = -1 / (pi n)^2, h[even n != 0] = 0 (the band-limited ramp's spatial kernel; even lags are skipped),
 *   S = pi / (n_view dp), dp = det_spacing * source_distance / D the ray spacing at the isocentre: the view step 2 pi / n_view, the
 *   factor 1/2 of a full circle and dp h / dp^2 of the sampled ramp in one constant, computed in double and applied last.
 * pnpx_radon_filter is the row filter alone: sino_in, sino_out [B,1,n_view,det].  geom NULL or of kind PNPX_GEOM_PARALLEL: the parallel
 * beam's filter, c = 1 and S = pi / n_view (Radon_norm.filter_sinogram without its FFTs), det given by the caller; a fan geometry:
 * its n_view and det_count must be the call's, and what depends on an image (the source's distance from the sampled span) is not
 * checked.  A pre-weighted row is staged in LDS: det must be in [2, 8192] (PNPX_ERR_SHAPE beyond), and sino_out == sino_in is refused
 * (PNPX_ERR_ARG).  pnpx_fan_backprojection_w is pnpx_fan_backprojection with the view weight chosen: PNPX_FAN_W_ADJOINT (the same
 * bytes) or PNPX_FAN_W_FBP, w = (D_so / U)^2.  pnpx_fan_fbp runs the two, with the filtered sinogram in the context's scratch.  The
 * refusals are those of the fan entries above. */
enum { PNPX_FAN_W_ADJOINT = 0, PNPX_FAN_W_FBP = 1 };
int pnpx_radon_filter(pnpx_ctx* ctx, const float* sino_in, float* sino_out, const pnpx_radon_geom* geom, int B, int n_view, int det,
                      void* stream);
int pnpx_fan_backprojection_w(pnpx_ctx* ctx, const float* sino, float* img, const pnpx_radon_geom* geom, int weight, int B, int R,
                              void* stream);
int pnpx_fan_fbp(pnpx_ctx* ctx, const float* sino, float* img, const pnpx_radon_geom* geom, int B, int R, void* stream);
/* pnpx_ct_iadmm / pnpx_ct_pg and their training pairs on a chosen geometry, as pnpx_ct_hqs takes it: geom NULL or of kind
 * PNPX_GEOM_PARALLEL is the entry without _geom (same bytes); a fan geometry (its n_view must equal n_view) runs the fan pair,
 * y0 [B,1,n_view,det_count], opnorm of that pair.  The backward work buffers grow with a fan geometry, whose tables stand 16-byte
 * aligned behind the image buffers: iADMM 6*B*R*R + 2*n_view + 4 + 4*det_count floats, PG 3*B*R*R + 1 + 2*n_view + 3 + 4*det_count. */
int pnpx_ct_iadmm_geom(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const pnpx_radon_geom* geom,
                       int n_view, float opnorm, const float* sigma_d, const float* mu, const float* tau, int param_stride, int B,
                       int R, int T, void* stream);
int pnpx_ct_iadmm_geom_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const pnpx_radon_geom* geom,
                             int n_view, float opnorm, const float* sigma_d, const float* mu, const float* tau, int param_stride,
                             int B, int R, int T, float* saved, unsigned long long* ticket, void* stream);
int pnpx_ct_iadmm_geom_backward(pnpx_ctx* ctx, const pnpx_radon_geom* geom, int n_view, float opnorm, const float* sigma_d,
                                const float* mu, const float* tau, int param_stride, const float* saved, const float* grad_vars_out,
                                float* grad_vars_in, float* grad_sigma_d, float* grad_mu, float* grad_tau, float* work, int B, int R,
                                int T, unsigned long long ticket, void* stream);
int pnpx_ct_pg_geom(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const pnpx_radon_geom* geom, int n_view,
                    float opnorm, const float* sigma_d, const float* tau, int param_stride, int B, int R, int T, void* stream);
int pnpx_ct_pg_geom_train(pnpx_ctx* ctx, const float* vars_in, float* vars_out, const float* y0, const pnpx_radon_geom* geom,
                          int n_view, float opnorm, const float* sigma_d, const float* tau, int param_stride, int B, int R, int T,
                          float* saved, unsigned long long* ticket, void* stream);
int pnpx_ct_pg_geom_backward(pnpx_ctx* ctx, const pnpx_radon_geom* geom, int n_view, float opnorm, const float* sigma_d,
                             const float* tau, int param_stride, const float* saved, const float* grad_vars_out,
                             float* grad_vars_in, float* grad_sigma_d, float* grad_tau, float* work, int B, int R, int T,
                             unsigned long long ticket, void* stream);

/* Host-only helpers of the Winograd F(4x4,3x3) kernel (csrc/conv3x3_winof4.hip), for tests: the 1-D matrices the weight packer and the
 * kernel use (G 6x3, B^T 6x6, A^T 4x6, row-major doubles), and the packer itself (w [cout][cin][3][3], cout % 64 == 0, cin % 8 == 0 ->
 * dst 36 * cout * cin floats: [cout/64][cin/8][stage 3][row 2][column pair 3][cout block 4][channel group 4][cout 16][k-step 2][column 2],
 * position (2 stage + row, 2 pair + column), channel 8 chunk + 2 group + k-step). */
void pnpx_winof4_matrices(double* g18, double* bt36, double* at24);
int pnpx_winof4_pack(const float* w, int cout, int cin, float* dst);
/* ... and the packer of the kernel's 32-cout instance (cout % 32 == 0): [cout/32][cin/8][stage 3][row 2][column pair 3][cout block 2]
 * [channel group 4][cout 16][k-step 2][column 2], positions and channels numbered as above. */
int pnpx_winof4_c32_pack(const float* w, int cout, int cin, float* dst);
/* ... and the plan by which an instance (0 plain, 1 two-source entry, 2 up-sampling entry, 3 32-cout) fetches one 8-channel chunk's halo
 * into LDS at image size H x W, from the tables the kernels themselves use.  Host only.  info[PNPX_WINOF4_HALO_INFO]: 0 the instance
 * gathers 16-byte units, 1 cout tile, 2 region width RW, 3 LDS row stride (floats), 4 LDS plane stride (floats), 5 first padded column of the
 * fetched window, counted from x0 for a region whose first pixel is image column x0 (the chunk's origin is channel 0, padded row y0,
 * padded column x0 + info[5]; image column x lies at padded column x + 4), 6 LDS column of halo column 0, 7 gather instructions per chunk, 8 of which 16-byte ones
 * (the first), 9 most gathers a wave issues, 10 fewest (what the waits count), 11 bytes of a halo buffer, 12 LDS offset of halo buffer
 * 0, 13 LDS bytes used, 14 weight LDS-DMA instructions every wave issues per stage, 15 staging gathers every wave issues (instance 2),
 * 16 .. 19 the vmcnt immediates: weight slice alone, + halo gathers, + staging gathers, + both (-1: the instance has none such; the
 * 32-cout instance: 0 and the halo gathers alone).  Per (instruction i, lane l), at [64 i + l]: src = byte offset of the lane's source
 * from the chunk's origin, dst = byte offset in the halo buffer, width = bytes moved, wave = issuing wave, real = 0 for a dummy lane (it
 * reads the origin and lands where nothing reads).  read[(c * 18 + hy) * (RW + 2) + hx] = byte offset in the halo buffer from which the
 * input transform reads halo element (channel c, row hy, column hx).  The arrays may all be NULL (info alone). */
#define PNPX_WINOF4_HALO_INFO 20
int pnpx_winof4_halo_plan(int inst, int H, int W, int* info, long long* src, int* dst, int* width, int* wave, int* real, int* read);

/* Single-layer probe of the fp32 3x3 convolution kernels of conv_mode 0 (csrc/conv_probe.hip), for tests: one layer's HOST weights are
 * packed by the packers pnpx_unet_load uses and ONE kernel of the chosen kind runs on DEVICE tensors the caller laid out in the denoiser's
 * internal padded planar layout: [B][C][H + 2][W + 8] fp32, pixel (y, x) at row y + 1, column x + 4, every other cell zero.  The call pads
 * and unpads nothing, allocates its own K-split scratch, and waits for its launch before it returns (the packed weights are its own).
 *   forward kinds: out = LeakyReLU_slope(conv3x3(cat(in0, in1), w [cout][C0 + C1][3][3]) + bias [cout]) (+ res, same geometry as out);
 *     pool_out (where the kind has the fused epilogue): also MaxPool2d(2) of out, [B][cout][H/2 + 2][W/2 + 8].
 *     WINO8_KSPLIT: the 8-wave kernel handed the K-split scratch (ks_rule: conv3x3_wino8.hip; 1 = the default rule); WINO8_UPS: in1 is
 *     the LOW-resolution second source [B][C1][H/2 + 2][W/2 + 8], up-sampled x2 (bilinear, align_corners) inside the kernel;
 *     WINOF4 is single-source (C1 = 0), WINOF4_2SRC the same kernel's two-source instance (C1 > 0, in1 at full resolution; takes
 *     pool_out); WINOF4_UPS is reserved (its plan is 0 for every geometry and the probe returns PNPX_ERR_SHAPE) and stays so: the
 *     instance that up-samples in1 (LOW-resolution [B][C1][H/2 + 2][W/2 + 8], like WINO8_UPS) is kind WINOF4_FUSE_UP = 11, and 10 is
 *     unknown.  WINOF4_C32 = 12 is the F(4x4,3x3) kernel's 32-cout instance: single-source, takes pool_out, W % 64 == 0.
 *   adjoint kinds: w is the FORWARD layer's [C0][cout][3][3]; in0 = the gradient of its output (C0 channels), out = the gradient of its
 *     input (cout channels, a multiple of 32) = conv_transpose(in0, w), times (mask > 0 ? 1 : slope) when mask (out's geometry) is given;
 *     no bias.
 * A geometry the kind's launcher refuses returns PNPX_ERR_SHAPE with the launcher's message and launches nothing.
 * pnpx_conv3x3_probe_plan (host only, no context): 0 when the kind refuses the geometry, else the cout-tile width (32 / 64); for
 * WINO8_KSPLIT plus 256 x the number of K-split pieces (1 = the layer does not split). */
enum pnpx_probe_kind {
  PNPX_PROBE_DIRECT = 0,
  PNPX_PROBE_WINO4 = 1,
  PNPX_PROBE_WINO8 = 2,
  PNPX_PROBE_WINO8_KSPLIT = 3,
  PNPX_PROBE_WINOF4 = 4,
  PNPX_PROBE_WINO8_UPS = 5,
  PNPX_PROBE_DIRECT_GRAD = 6,
  PNPX_PROBE_WINO8_GRAD = 7,
  PNPX_PROBE_WINOF4_2SRC = 8,   /* the F(4x4,3x3) kernel's two-source instance: in1 at full resolution, C1 > 0 */
  PNPX_PROBE_WINOF4_UPS = 9,    /* reserved before an F(4x4,3x3) instance that up-samples in1 existed: still refuses every geometry */
  /* 10 is no kind */
  PNPX_PROBE_WINOF4_FUSE_UP = 11,  /* the F(4x4,3x3) kernel's up-sampling instance: in1 at H/2 x W/2, C1 > 0, C0 >= 16; no pool_out */
  PNPX_PROBE_WINOF4_C32 = 12       /* the F(4x4,3x3) kernel's 32-cout instance: cout % 32 == 0 and % 64 != 0, C1 = 0, W % 64 == 0 */
};
int pnpx_conv3x3_probe(pnpx_ctx* ctx, int kind, const float* w_host, const float* bias_host, int cout, const float* in0, int C0,
                       const float* in1, int C1, float* out, const float* res, const float* mask, float slope, float* pool_out,
                       int ks_rule, int B, int H, int W, void* stream);
int pnpx_conv3x3_probe_plan(int kind, int C0, int C1, int cout, int H, int W, int ks_rule);
/* For tests: the separate bilinear x2 (align_corners) up-sampling launch of conv_mode 0 on device tensors in the same padded planar layout:
 * src [planes][h + 2][w + 8] -> the interior of dst [planes][2h + 2][2w + 8] (its border cells are not written).  Asynchronous on `stream`. */
int pnpx_upsample2x_probe(pnpx_ctx* ctx, const float* src, float* dst, int planes, int h, int w, void* stream);

/* Single-layer probe of the half-split convolution launcher (csrc/conv_hs_probe.hip), for tests: one layer's HOST weights are packed by
 * the library's own pack_conv_weights_hs / pack_conv_weights_hs_taps for the tile conv_hs_mt gives, uploaded with the alignment and slack
 * of pnpx_unet_load / pack_layer, and ONE launch_conv_hs call runs on DEVICE tensors the caller laid out.  The call waits for its launch
 * and frees what it allocated.  Nothing in the library calls it; it adds no option and reads no state of the context but its device.
 *   HS8 tensors: [B][C/8][H + 2][W + 2] records of 32 bytes = hi[8] f16 | lo[8] f16 with hi = f16(16 v), lo = f16(16 v - hi), zero border.
 *   w [cout][cin][9] with cin <= 8 (G0 + G1) < cin + 16 (K is zero-padded to a multiple of 16); bias [cout] (null = zeros: the gradient
 *   epilogues read none).  in0 carries in0_groups >= G0 groups per image (0 = G0) of which the layer reads the first G0; in1 carries G1
 *   groups, at (ups_h, ups_w) = (H/2, W/2) when those are set.  out / res / dmask: cout/8 groups (res: res_groups when set, critic_epi 2
 *   only); pool_out [B][cout/8][H/2 + 2][W/2 + 2].  outc_w [32], outc_b [1], first_w [32][2][9], first_b [32] are HOST arrays; x_in,
 *   out_img, out_pre, first_x [B][H][W] and first_sigma [B * first_sigma_stride] are fp32 DEVICE arrays.
 *   Every other field is the ConvHsFuse field of the same name (csrc/conv_hs.h); want_range_flag hands the kernel a cleared range-guard
 *   word whose value after the launch comes back in *range_flag_out.
 * An operand the selected path has no place for (pool_out where no pool is fused, res beside dmask, x_in without outc_w, in1 with G1 = 0,
 * ...) is refused with PNPX_ERR_ARG, never dropped; what launch_conv_hs itself refuses returns its status and message, nothing launched.
 * pnpx_conv_hs_probe_plan (host only, no context, dereferences no pointer of the descriptor: non-null = operand present) reports what
 * that call would launch at (B, H, W), as launch_conv_hs / launch_hs_cfg themselves decide it:
 *   out[0..7] = the conv_hs_kernel instance MT, NBW, MBW, NW, EPI, UPS, WREG, TAPS; out[8] = cout tile of the weight packing; out[9] =
 *   grid size; out[10] = tiles; out[11] = plain_walk.  Returns 1, or 0 (out zeroed) when the probe or the launcher refuses. */
typedef struct pnpx_conv_hs_probe_desc {
  const float *w, *bias, *outc_w, *outc_b, *first_w, *first_b;                 /* host */
  const void *in0, *in1, *res, *dmask;                                         /* device, HS8 */
  void *out, *pool_out;                                                        /* device, HS8 */
  const float *x_in, *first_x, *first_sigma;                                   /* device, fp32 */
  float *out_img, *out_pre;                                                    /* device, fp32 */
  int cin, cout, G0, G1, B, H, W;
  float slope;
  int taps, in0_groups, wreg, share, ups_h, ups_w, critic_epi;
  float alpha;
  int res_groups, first_sigma_stride;
  float first_slope;
  int want_range_flag;
  unsigned* range_flag_out;                                                    /* host, may be null */
} pnpx_conv_hs_probe_desc;
enum { PNPX_CONV_HS_PLAN_INTS = 12 };
int pnpx_conv_hs_probe(pnpx_ctx* ctx, const pnpx_conv_hs_probe_desc* desc, void* stream);
int pnpx_conv_hs_probe_plan(const pnpx_conv_hs_probe_desc* desc, int B, int H, int W, int* out);

/* Probe of the launches between the UNet VJP's adjoint convolutions (csrc/vjp_glue_probe.hip; kernels and launchers: csrc/unet_bwd.hip,
 * csrc/grad_common.h), for tests: ONE call of the launcher pnpx_unet_denoise_backward itself uses, on DEVICE tensors the caller laid out,
 * and a wait for it.  Nothing in the library calls it; it adds no option and reads no state of the context but its device.
 *   family 0: padded planar fp32 [B][C][H + 2][W + 8] (see pnpx_conv3x3_probe); family 1: HS8 records [B][C/8][H + 2][W + 2] (see
 *   pnpx_conv_hs_probe; C, Ccat and c_off multiples of 8).  Plain images are fp32 [B][H][W].  Outputs: interiors only, borders untouched.
 *   OUTC_BWD (C = 32): g = g_out [B][H][W], pre [B][H][W], w [32] (device), act = the saved activation, sc (family 1) ->
 *     out = w[c] g 1[0 <= pre <= 1] LeakyReLU'(act) (family 1: g_out times sc[0] first), out_res [B][H][W] = the masked g.
 *   UPSAMPLE_BWD: the adjoint of the bilinear x2 (align_corners) up-sampling of an H x W source into channels [c_off, c_off + C) of a
 *     concat gradient g [B][Ccat][Ht][Wt], 2H <= Ht <= 2H + 1, 2W <= Wt <= 2W + 1; out [B][C][H][W] = the adjoint times
 *     LeakyReLU'(act).  family 0 forms: 1 = one thread per source pixel, 2 = LDS window of 16 x 16 source pixels, 3 = of 16 x 64; auto
 *     takes 3 at W >= 64, else 2, and 1 when B * C > 65535 (forms 2 and 3 put a plane on gridDim.z and refuse that).  family 1 has one
 *     form; B * C/8 > 65535 runs as consecutive launches over whole images of at most 65535 / (C/8) images each (the VJP does the same),
 *     so no geometry of the denoiser is refused and no launch exceeds the grid limit.
 *   SKIP_POOL_MERGE: out [B][C][H][W] = (g [B][Ccat][H][W] channels [0, C) + the 2 x 2 max-pool routing of g_pool [B][C][H/2][W/2], null =
 *     none, to the first maximum of act in scan order) LeakyReLU'(act).  family 0 forms: 1 = one thread per pixel, 2 = one per 2 x 2
 *     block (even H and W only: auto takes it there).
 *   INPUT_GRAD: g = the gradient of the first convolution's input [B][C][H][W] (family 1: C = 32), g_res [B][H][W], sc (family 1) ->
 *     out [B][H][W] = g[:, 0] + g_res, part [B][64] = the partial sums of g[:, 1] over 64 pixel ranges, gsigma [B] = their sums
 *     (family 1: all times sc[1]).
 *   GRAD_SCALE (family 1): g = B * H * W floats -> bits = the bit pattern of max |g|, out = float2 {1 / m, m}, m = the power of two
 *     above max |g| ({0, 0} for all zeros, {1, 1} when a value is infinite; a NaN is dropped by the maximum, so it leaves the scale of
 *     the other values; a denormal maximum: m = 2^-126).
 * LeakyReLU' is 1 where act > 0, else 0.2 (so 0.2 at +0 and -0).  An operand the op has no place for, or a missing one, is refused with
 * PNPX_ERR_ARG; a size or a form the op cannot run with PNPX_ERR_SHAPE; nothing is launched then.
 * pnpx_vjp_glue_probe_plan (host only, no context, reads the sizes only): 0 when refused, else the form the call runs (form = 0: the
 * one the VJP dispatches) + 256 x (launches of the kernel - 1). */
enum pnpx_vjp_glue_op {
  PNPX_VJP_OUTC_BWD = 0,
  PNPX_VJP_UPSAMPLE_BWD = 1,
  PNPX_VJP_SKIP_POOL_MERGE = 2,
  PNPX_VJP_INPUT_GRAD = 3,
  PNPX_VJP_GRAD_SCALE = 4
};
typedef struct pnpx_vjp_glue_probe_desc {
  int op, family, form;
  int B, C, H, W, Ccat, c_off, Ht, Wt;
  const void *g, *act, *g_pool;          /* device: incoming gradient, saved activation, pooled gradient */
  const float *pre, *w, *g_res, *sc;     /* device, fp32 */
  void* out;                             /* device */
  float *out_res, *part, *gsigma;        /* device, fp32 */
  unsigned* bits;                        /* device */
} pnpx_vjp_glue_probe_desc;
int pnpx_vjp_glue_probe(pnpx_ctx* ctx, const pnpx_vjp_glue_probe_desc* desc, void* stream);
int pnpx_vjp_glue_probe_plan(const pnpx_vjp_glue_probe_desc* desc);

/* Probe of the launches between the convolutions of the two denoisers' FORWARD passes and of the DRUNet VJP's own glue
 * (csrc/fwd_glue_probe.hip; launchers: csrc/fwd_glue.h; kernels: csrc/unet.hip, csrc/conv_first.h, csrc/drunet_f32.hip, csrc/drunet.hip,
 * csrc/hs_relayout.h), for tests: ONE call of the launcher the network walks themselves use, on DEVICE tensors the caller laid out, and a
 * wait for it.  Nothing in the library calls it; it adds no option and reads no state of the context but its device.
 *   family 0: padded planar fp32 [B][C][H + 2][W + 8] (see pnpx_conv3x3_probe); family 1: HS8 records [B][C/8][H + 2][W + 2] (see
 *   pnpx_conv_hs_probe; C a multiple of 8).  Plain images are fp32 [B][H][W].  Outputs: interiors only, borders untouched.  w and bias
 *   are HOST arrays (copied to the device for the call); every other pointer is a device pointer.
 *   PREP_INPUT (C = 0): x [B][H][W], sigma [1 + (B - 1) sigma_stride] -> out, 2 channels (family 1: 16, i.e. two groups; the second is
 *     not written): channel 0 = x, channel 1 = sigma[b sigma_stride] inside the image; the border is not written.
 *   CONV_FIRST (C = cout, 32 or 64): x, sigma, sigma_stride as above, w [cout][2][9], bias [cout], slope -> out [B][cout][H][W] =
 *     act(bias + sum_t w[c][0][t] x[t] + w[c][1][t] sigma 1[t inside the image]), act(v) = max(v, slope v); family 1 writes the records of
 *     HS_ASCALE 2^-k times that (0 <= k <= 24).  family 0 needs W % 4 == 0.
 *   MAXPOOL2: src [B][C][H][W] -> out [B][C][H/2][W/2], floor semantics (H, W >= 2).
 *   UPSAMPLE2X: bilinear x2 (align_corners) of src [B][C][H][W] into the 2H x 2W corner of out [B][C][Ht][Wt], 2H <= Ht <= 2H + 1,
 *     2W <= Wt <= 2W + 1; the extra row / column is not written.  family 0 forms: 1 = one thread per output pixel, 2 = four outputs along
 *     x per thread (2W % 4 == 0 and B C <= 65535 planes only: the forward takes it there).  family 1 forms: 1 = 32 x 16 output tiles,
 *     2 = 64 x 16 (the forward takes 2 above 32 output columns); B C/8 > 65535 runs as consecutive launches over whole images of at most
 *     65535 / (C/8) images each, so no launch exceeds the grid limit.
 *   OUTC_RESIDUAL (C = 32): src = feat, x [B][H][W], w [32], bias [1] -> out_pre (may be null) = x + (sum_c w[c] feat[c] + bias),
 *     out = clamp(out_pre, 0, 1), both [B][H][W].
 *   S2D: src [B][C][H][W] (H, W even) -> out [B][4C][H/2][W/2], channel (2 dy + dx) C + c = src[c][2y + dy][2x + dx] (family 1: the same
 *     over groups of 8 channels: group (2 dy + dx) C/8 + g; record copies).  D2S: src [B][4C][H][W] -> out [B][C][2H][2W], its inverse.
 *   ADD: out = src + src2, [B][C][H][W].
 *   TAIL_OUT (family 0, C = 32): out_pre (may be null) = channel 0 of src, out = clamp(that, 0, 1), both [B][H][W].
 *   TAIL_MASK (C = 0): out = x 1[0 <= pre <= 1], all [B][H][W] (family 1: x times sc[0] first, sc a device float2).
 *   DRU_INPUT_GRAD (family 0, C >= 2): src = the gradient of the first convolution's input -> out [B][H][W] = src[:, 0], part [B][64] =
 *     the partial sums of src[:, 1] over 64 pixel ranges, gsigma [B] = their sums.
 * A field the op has no place for must be 0 / null: an operand the op has no place for, or a missing one, is refused with PNPX_ERR_ARG; a
 * size or a form the op cannot run with PNPX_ERR_SHAPE; nothing is launched then.
 * pnpx_fwd_glue_probe_plan (host only, no context, reads the sizes only): 0 when refused, else the form the call runs (form = 0: the one
 * the forward dispatches; 1 for the ops with one form) + 256 x (launches of the kernel - 1). */
enum pnpx_fwd_glue_op {
  PNPX_FWD_PREP_INPUT = 0,
  PNPX_FWD_CONV_FIRST = 1,
  PNPX_FWD_MAXPOOL2 = 2,
  PNPX_FWD_UPSAMPLE2X = 3,
  PNPX_FWD_OUTC_RESIDUAL = 4,
  PNPX_FWD_S2D = 5,
  PNPX_FWD_D2S = 6,
  PNPX_FWD_ADD = 7,
  PNPX_FWD_TAIL_OUT = 8,
  PNPX_FWD_TAIL_MASK = 9,
  PNPX_FWD_DRU_INPUT_GRAD = 10
};
typedef struct pnpx_fwd_glue_probe_desc {
  int op, family, form;
  int B, C, H, W, Ht, Wt, sigma_stride, k;
  float slope;
  const void *src, *src2;                /* device: padded tensors */
  const float *x, *sigma, *pre, *sc;     /* device, fp32 */
  const float *w, *bias;                 /* host */
  void* out;                             /* device */
  float *out_pre, *part, *gsigma;        /* device, fp32 */
} pnpx_fwd_glue_probe_desc;
int pnpx_fwd_glue_probe(pnpx_ctx* ctx, const pnpx_fwd_glue_probe_desc* desc, void* stream);
int pnpx_fwd_glue_probe_plan(const pnpx_fwd_glue_probe_desc* desc);

/* Probe of the TRAINING kernels of the two ResNet-18 networks (csrc/net_train_probe.hip; launchers: csrc/policy_grad.h, csrc/critic_grad.h;
 * kernels: csrc/policy_bn.hip, csrc/policy_grad.hip, csrc/critic_grad.hip), for tests: ONE call of the launcher(s) the network walks
 * themselves use, on DEVICE tensors the caller laid out, and a wait for it.  Nothing in the library calls it; it adds no option and reads
 * no state of the context but its device.  HS8 tensors are records [B][G][h + 2][w + 2] (see pnpx_conv_hs_probe), values times 16; cout = 8 G.
 * The probe allocates every scratch (K-split slab, partial sums, head rows, range bits) itself and fills it with NaN before the launch.
 *   BN_STATS: z0, params [4 cout] (weight, bias, running_mean, running_var), momentum, update -> fout [4][cout] = mean, biased variance,
 *     scale = weight / sqrt(var + 1e-5), shift = bias - mean scale, over the interior; update != 0 moves the running statistics in params
 *     (variance times n / (n - 1)).
 *   BN_APPLY: z0, st0 [3][cout] (mean, scale, beta) [, z1, st1] [, res] -> out and / or out2 = relu((z0 - mean) scale + beta [+ the same of
 *     z1] [+ res]); out2 is the space-to-depth copy [B][4 G][h/2 + 2][w/2 + 2] (h, w even), group (2 (y & 1) + (x & 1)) G + g.
 *   BN_BWD: g, act, z0, st0 [2][cout] (mean, var) [, z1, st1], params [4 cout per layer] [, slot (float2: s, 1 / s)] [, boost] -> grad
 *     [4 cout per layer] (weight, bias, two rows of zeros), coef [3 cout per layer], out = dz0 [, out2 = dz1] [, dy_out] [, flag |= 1
 *     where |dz| >= 4095].  dy = g [act > 0]; slot null: (1, 1); boost 0: 1 (the gradients are times 1 / (s boost)).
 *   WGRAD_PLAIN (G = 0): g [B][Gg][..] (cout = K-split GEMM rows), x [B][Xg][..], gv [B], inv_w, kind 0 / 1 / 2 (3x3 stride 1; 3x3 stride 2
 *     on the space-to-depth grid, K = 4 Cp, cin <= Cp; 1x1 shortcut, Cp = 0), cout, cin, K -> grad [cout][cin][9] ([cout][cin] for kind 2)
 *     = inv_w sum_b gv[b] corr(g, x).
 *   WGRAD_WN: the same with params = bias [cout] | weight_g [cout] | weight_v [cout][fan] and inv_b -> grad in the same layout.
 *   CLIP_MASK: act, thr (in the records' units, 16 x the activation) -> out (every record written: hi = 16 where the stored value does not
 *     exceed thr inside, zero border).
 *   ALPHA_DOT: g, x (= W m), G [, res, m with resG, mG groups] -> dout [B].
 *   FC_GRAD: act [B][64][h + 2][w + 2], gv, fin = fc.weight [512], thr (records' units) -> fout [512] = fc.weight's gradient, dout [512] =
 *     the head threshold's share per channel.
 *   ALPHA_FINISH: alpha_src (HOST int [21], each -1 or an index below 21), din [21][B], din2 [512], gv, inv_w -> grad [23]: [21] the head's
 *     threshold, [22] fc.bias.
 *   HEAD_GRAD: act = feat [B][64][..], params = the head tensors in parameter order (fc_softmax.0 weight [2][512], bias [2]; the first
 *     deterministic Linear [n1][512], [n1], n1 = spi ? 64 : n_det; with spi the second [n_det][64], [n_det]), fin = gp [B][2],
 *     fin2 = gd [B][n_det] -> fout = g_f [B][512], grad in the layout of params.
 *   GRAD_SEED: fin = g_f [B][512], boost -> fout (float2 slot), out = ga [B][64][..], fout2 = gv [B].
 * A field the op has no place for must be 0 / null (PNPX_ERR_ARG); a size the op cannot run: PNPX_ERR_SHAPE; nothing is launched then.
 * pnpx_net_train_probe_plan (host only, no context, reads the sizes only): 0 when refused, else BN_STATS / BN_BWD: the pieces of 2048
 * pixels; BN_APPLY: the workgroups; WGRAD_*: K-split pieces + 256 x chunks (of 32 pixels) per piece; HEAD_GRAD: the rows of the head
 * tensors (one workgroup each); the others: 1. */
enum pnpx_net_train_op {
  PNPX_NT_BN_STATS = 0,
  PNPX_NT_BN_APPLY = 1,
  PNPX_NT_BN_BWD = 2,
  PNPX_NT_WGRAD_PLAIN = 3,
  PNPX_NT_WGRAD_WN = 4,
  PNPX_NT_CLIP_MASK = 5,
  PNPX_NT_ALPHA_DOT = 6,
  PNPX_NT_FC_GRAD = 7,
  PNPX_NT_ALPHA_FINISH = 8,
  PNPX_NT_HEAD_GRAD = 9,
  PNPX_NT_GRAD_SEED = 10
};
typedef struct pnpx_net_train_probe_desc {
  int op;
  int B, G, h, w;
  int cout, K, cin, Cp, kind, Gg, Xg;    /* WGRAD_* */
  int resG, mG;                          /* ALPHA_DOT */
  int n_det, spi, update;
  float momentum, thr, boost, inv_w, inv_b;
  const void *z0, *z1, *g, *act, *res, *x, *m;          /* device, HS8 */
  const float *st0, *st1, *gv, *slot, *fin, *fin2;      /* device, fp32 */
  float* params;                                        /* device, fp32 (BN_STATS moves its running statistics) */
  const double *din, *din2;                             /* device */
  const int* alpha_src;                                 /* host */
  void *out, *out2, *dy_out;                            /* device, HS8 */
  float *grad, *coef, *fout, *fout2;                    /* device, fp32 */
  double* dout;                                         /* device */
  unsigned* flag;                                       /* device */
} pnpx_net_train_probe_desc;
int pnpx_net_train_probe(pnpx_ctx* ctx, const pnpx_net_train_probe_desc* desc, void* stream);
int pnpx_net_train_probe_plan(const pnpx_net_train_probe_desc* desc);

/* Host-only, for tests: which kernel a UNet decoder entry of conv_mode 0 gets (csrc/conv_f32_select.hip, conv_f32_entry) for a set of
 * options, a geometry (second source C1 > 0 at H/2 x W/2, output H x W) and the batch of the whole call.
 * opts: bit 0 "fp32_winograd", bit 1 the layer's "fp32_wino8_layers" bit, bit 2 its "fp32_winof4_layers" bit, bit 3 its
 * "fp32_winof4_entries" bit, bit 4 "fp32_fuse_up", bit 5 the layer's F(2x2) weights are packed, bit 6 its F(4x4) weights are packed,
 * bit 7 its "fp32_winof4_fuse_up" bit.
 * Returns kernel + 16 x K-split pieces + 256 x fused, kernel 0 = direct, 1 = 4-wave F(2x2), 2 = 8-wave F(2x2), 3 = F(4x4); fused = the
 * instance that up-samples the second source itself runs (else the separate up-sampling kernel runs first); -1 = a non-positive size. */
int pnpx_conv_f32_entry_plan(int opts, int ksplit, int ksplit_rule, int C0, int C1, int cout, int H, int W, int B_call);
/* ... and which kernel a plain forward layer gets (conv_f32_forward; C1 >= 0) or, with bit 7, the network's last 3x3 layer (conv_f32_last).
 * opts: bit 0 "fp32_winograd", bit 1 the layer's "fp32_wino8_layers" bit, bit 2 its "fp32_winof4_layers" bit, bit 3 its "fp32_winof4_c32"
 * bit, bit 4 its F(2x2) weights are packed, bit 5 its F(4x4) weights, bit 6 its F(4x4) weights in the 32-cout instance's layout, bit 7
 * the layer is the last one.  Same return value, kernel 4 = the F(4x4) kernel's 32-cout instance; fused = the layer's fused epilogue
 * (2x2 max-pool; last layer: out-conv) is available. */
int pnpx_conv_f32_forward_plan(int opts, int ksplit, int ksplit_rule, int C0, int C1, int cout, int H, int W, int B_call);

#ifdef __cplusplus
}
#endif
#endif /* PNPX_H */
