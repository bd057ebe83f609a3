// The launches between the convolutions of the two denoisers' forward passes, and the DRUNet VJP's own glue (kernels and launchers: unet.hip,
// drunet_f32.hip, drunet.hip; conv_first.h and hs_relayout.h hold the kernels other translation units share).  The network walks and the test
// probe (fwd_glue_probe.hip) both go through these launchers, so a form decision, a grid formula and sy / sx exist once.  The form decisions
// are host-only and need no device.  Form ids are those of include/pnpx.h (pnpx_fwd_glue_probe_desc.form); 0 = decide here.
#pragma once
#include "common.h"
#include "hs_rec.h"

namespace pnpx {

enum FwdGlueForm {
  FG_AUTO = 0,
  FG_UPS_SCALAR = 1, FG_UPS_V4 = 2,        // fp32 up-sampling: one thread per output pixel / four outputs along x per thread
  FG_UPS_HS32 = 1, FG_UPS_HS64 = 2,        // HS8 up-sampling: 32 x 16 output tiles (<32,2>) / 64 x 16 (<64,4>)
  FG_ONLY = 1                              // every other launch has one form
};
constexpr size_t FG_GRID_Z_MAX = 65535;    // gridDim.y / gridDim.z of one launch

// fp32 up-sampling of `planes` planes from width w: the v4 form stores 16 bytes (2w a multiple of 4) and puts a plane on gridDim.z
inline bool upsample2x_form_runs_f32(int form, size_t planes, int w) {
  return form == FG_UPS_SCALAR || (form == FG_UPS_V4 && (2 * w) % 4 == 0 && planes <= FG_GRID_Z_MAX);
}
inline int upsample2x_form_f32(size_t planes, int w) { return upsample2x_form_runs_f32(FG_UPS_V4, planes, w) ? FG_UPS_V4 : FG_UPS_SCALAR; }
// HS8 up-sampling: both tile shapes run every size; the forward takes the 64-wide one above 32 output columns
inline int upsample2x_form_hs(int w) { return 2 * w > 32 ? FG_UPS_HS64 : FG_UPS_HS32; }
inline bool upsample2x_form_runs_hs(int form) { return form == FG_UPS_HS32 || form == FG_UPS_HS64; }
// ... one (image, group) per gridDim.z.  nb * G above the limit runs as consecutive launches over whole images, each of at most
// FG_GRID_Z_MAX / G images (0: a single image is over the limit, the launcher refuses with PNPX_ERR_SHAPE) -- as the adjoint does
// (grad_common.h: upsample_bwd_hs_launches).
inline int upsample2x_hs_images_per_launch(int G) { return G > 0 ? (int)(FG_GRID_Z_MAX / (size_t)G) : 0; }
inline int upsample2x_hs_launches(int nb, int G) {
  const int per = upsample2x_hs_images_per_launch(G);
  return per > 0 ? (nb + per - 1) / per : 0;
}
// the fp32 first convolution stores four pixels along x per thread
inline bool conv_first_runs_f32(int W) { return W > 0 && W % 4 == 0; }

// Every launcher checks its launch and returns a PNPX status.  fp32 tensors: padded planar (common.h); HS8: records (hs_rec.h); images,
// sigma: plain fp32.
// ---- unet.hip
int launch_prep_input_f32(const float* x, const float* sigma, int sigma_stride, float* dst, int B, int H, int W, hipStream_t s);
int launch_prep_input_hs(const float* x, const float* sigma, int sigma_stride, HsRec* dst, int B, int H, int W, hipStream_t s);
// w [cout][2][9], bias [cout] (device), cout a multiple of 8; fp32: PNPX_ERR_SHAPE unless W % 4 == 0
int launch_conv_first_f32(const float* x, const float* sigma, int sigma_stride, const float* w, const float* bias, float* dst, int cout, int B,
                          int H, int W, float slope, hipStream_t s);
int launch_conv_first_hs(const float* x, const float* sigma, int sigma_stride, const float* w, const float* bias, HsRec* dst, int cout, int B,
                         int H, int W, float slope, float oscale, hipStream_t s);
// planes = B * C (fp32) or B * C / 8 (HS8) planes of H x W -> H/2 x W/2
int launch_maxpool2_f32(const float* src, float* dst, size_t planes, int H, int W, hipStream_t s);
int launch_maxpool2_hs(const HsRec* src, HsRec* dst, size_t planes, int H, int W, hipStream_t s);
// planes of h x w into the 2h x 2w corner of planes of Ht x Wt
int launch_upsample2x_f32(int form, const float* src, float* dst, size_t planes, int h, int w, int Ht, int Wt, hipStream_t s);
int launch_upsample2x_hs(int form, const HsRec* src, HsRec* dst, int nb, int G, int h, int w, int Ht, int Wt, hipStream_t s);
// feat [B][32][H][W], w [32], bias [1] (device) -> out, out_pre (may be null) [B][H][W]
int launch_outc_residual_f32(const float* feat, const float* x, const float* w, const float* bias, float* out, float* out_pre, int B, int H,
                             int W, hipStream_t s);
int launch_outc_residual_hs(const HsRec* feat, const float* x, const float* w, const float* bias, float* out, float* out_pre, int B, int H,
                            int W, hipStream_t s);
// ---- drunet_f32.hip
int launch_s2d_f32(const float* in, float* out, int B, int C, int h, int w, hipStream_t s);     // [B][C][h][w] -> [B][4C][h/2][w/2]
int launch_d2s_f32(const float* in, float* out, int B, int C, int h, int w, hipStream_t s);     // [B][4C][h][w] -> [B][C][2h][2w]
int launch_add_f32(const float* a, const float* b, float* o, size_t planes, int h, int w, hipStream_t s);
int launch_tail_out_f32(const float* t32, float* out, float* out_pre, int B, int H, int W, hipStream_t s);
int launch_tail_mask_f32(const float* g_out, const float* pre, float* g_pre, size_t n, hipStream_t s);
// gx [B][H][W], part [B][SIG_CHUNKS], gsigma [B]: the input-gradient kernel, then sigma_grad_final_kernel
int launch_dru_input_grad_f32(const float* g_in0, int Cg, float* gx, float* part, float* gsigma, int B, int H, int W, hipStream_t s);
// ---- drunet.hip
int launch_s2d_hs(const HsRec* in, HsRec* out, int B, int G, int h, int w, hipStream_t s);      // [B][G][h][w] -> [B][4G][h/2][w/2]
int launch_d2s_hs(const HsRec* in, HsRec* out, int B, int G, int h, int w, hipStream_t s);      // [B][4G][h][w] -> [B][G][2h][2w]
int launch_add_hs(const HsRec* a, const HsRec* b, HsRec* o, size_t planes, int h, int w, hipStream_t s);
int launch_tail_mask_hs(const float* g_out, const float* pre, const float2* sc, float* g_pre, size_t n, hipStream_t s);

}  // namespace pnpx
