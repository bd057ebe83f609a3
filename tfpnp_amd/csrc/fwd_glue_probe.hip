// Probe of the launches between the convolutions of the two denoisers' forward passes and of the DRUNet VJP's own glue, for tests
// (tests/test_gpu_fwd_glue.py): ONE call of a launcher of fwd_glue.h -- the very function the network walks call -- on tensors the caller
// laid out, and a wait for it.  pnpx_fwd_glue_probe_plan asks the launchers' own host-only form decisions.  Nothing in the library calls
// either; they add no option.
#include <cmath>

#include "common.h"
#include "conv_hs.h"
#include "fwd_glue.h"

using namespace pnpx;

namespace {

int bad(int code, const char* what) {
  set_error("pnpx_fwd_glue_probe: %s", what);
  return code;
}

// sizes and form: what the op cannot run.  *form_out = the form the launcher will take, *launches = kernel launches of the op's own kernel.
int validate_sizes(const pnpx_fwd_glue_probe_desc& d, int* form_out, int* launches) {
  *form_out = 0;
  *launches = 1;
  if (d.family != 0 && d.family != 1) return bad(PNPX_ERR_ARG, "family is 0 (fp32) or 1 (half-split)");
  if (d.op < PNPX_FWD_PREP_INPUT || d.op > PNPX_FWD_DRU_INPUT_GRAD) return bad(PNPX_ERR_ARG, "unknown op");
  const bool hs = d.family == 1;
  if (hs && (d.op == PNPX_FWD_TAIL_OUT || d.op == PNPX_FWD_DRU_INPUT_GRAD)) return bad(PNPX_ERR_ARG, "the op belongs to the fp32 family");
  const bool image_op = d.op == PNPX_FWD_PREP_INPUT || d.op == PNPX_FWD_TAIL_MASK;      // no channel count
  const bool first = d.op == PNPX_FWD_CONV_FIRST, ups = d.op == PNPX_FWD_UPSAMPLE2X;
  if (!ups && (d.Ht != 0 || d.Wt != 0)) return bad(PNPX_ERR_ARG, "Ht / Wt belong to the up-sampling only");
  if (!first && d.op != PNPX_FWD_PREP_INPUT && d.sigma_stride != 0) return bad(PNPX_ERR_ARG, "sigma_stride belongs to the input preparation and the first convolution");
  if (!(first && hs) && d.k != 0) return bad(PNPX_ERR_ARG, "the scale exponent belongs to the half-split first convolution");
  if (!first && d.slope != 0.f) return bad(PNPX_ERR_ARG, "the slope belongs to the first convolution");
  if (image_op && d.C != 0) return bad(PNPX_ERR_ARG, "the op has no channel count");
  if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.form < 0 || d.sigma_stride < 0 || (!image_op && d.C <= 0)) return bad(PNPX_ERR_SHAPE, "non-positive size");
  if ((long long)d.H * d.W > 0x7fffffffLL) return bad(PNPX_ERR_SHAPE, "image too large");
  if (hs && !image_op && d.C % 8) return bad(PNPX_ERR_SHAPE, "half-split channel counts are multiples of 8");
  int form = d.form ? d.form : FG_ONLY;
  const size_t zmax = FG_GRID_Z_MAX;
  switch (d.op) {
    case PNPX_FWD_PREP_INPUT:
      if (!hs && ((size_t)d.B > zmax || (size_t)d.H > zmax)) return bad(PNPX_ERR_SHAPE, "more rows or images than one launch's grid");
      break;
    case PNPX_FWD_CONV_FIRST:
      if (d.C != 32 && d.C != 64) return bad(PNPX_ERR_SHAPE, "the first convolution has 32 or 64 output channels");
      if ((size_t)d.B > zmax) return bad(PNPX_ERR_SHAPE, "more images than one launch's grid");
      if (!hs && !conv_first_runs_f32(d.W)) return bad(PNPX_ERR_SHAPE, "the fp32 first convolution needs W % 4 == 0");
      if (d.k < 0 || d.k > 24) return bad(PNPX_ERR_SHAPE, "scale exponent outside [0, 24]");
      break;
    case PNPX_FWD_MAXPOOL2:
      if (d.H < 2 || d.W < 2) return bad(PNPX_ERR_SHAPE, "nothing to pool");
      break;
    case PNPX_FWD_UPSAMPLE2X:
      if (d.Ht < 2 * d.H || d.Ht > 2 * d.H + 1 || d.Wt < 2 * d.W || d.Wt > 2 * d.W + 1) return bad(PNPX_ERR_SHAPE, "Ht x Wt is 2H or 2H + 1 by 2W or 2W + 1");
      if (hs) {
        if (!d.form) form = upsample2x_form_hs(d.W);
        *launches = upsample2x_hs_launches(d.B, d.C / 8);
        if (!upsample2x_form_runs_hs(form) || *launches <= 0) return bad(PNPX_ERR_SHAPE, "unknown form, or more channel groups per image than planes of one launch");
      } else {
        const size_t planes = (size_t)d.B * d.C;
        if (!d.form) form = upsample2x_form_f32(planes, d.W);
        if (!upsample2x_form_runs_f32(form, planes, d.W)) return bad(PNPX_ERR_SHAPE, "the form cannot run this width or this many planes, or is unknown");
      }
      break;
    case PNPX_FWD_OUTC_RESIDUAL:
    case PNPX_FWD_TAIL_OUT:
      if (d.C != 32) return bad(PNPX_ERR_SHAPE, "the tail reads 32 channels");
      if (!hs && ((size_t)d.B > zmax || (size_t)d.H > zmax)) return bad(PNPX_ERR_SHAPE, "more rows or images than one launch's grid");
      break;
    case PNPX_FWD_S2D:
      if (d.H % 2 || d.W % 2) return bad(PNPX_ERR_SHAPE, "space-to-depth needs even sizes");
      break;
    case PNPX_FWD_DRU_INPUT_GRAD:
      if (d.C < 2) return bad(PNPX_ERR_SHAPE, "the input gradient reads channels 0 and 1");
      if ((size_t)d.B > zmax) return bad(PNPX_ERR_SHAPE, "more images than one launch's grid");
      break;
    default:
      break;
  }
  if (form != FG_ONLY && !ups) return bad(PNPX_ERR_SHAPE, "the op has one form");
  *form_out = form;
  return PNPX_OK;
}

// operands: each op's own, all of them, and no other
int validate_operands(const pnpx_fwd_glue_probe_desc& d) {
  const bool hs = d.family == 1;
  // bit i: src, src2, x, sigma, pre, sc, w, bias, out, out_pre, part, gsigma
  const void* p[12] = {d.src, d.src2, d.x, d.sigma, d.pre, d.sc, d.w, d.bias, d.out, d.out_pre, d.part, d.gsigma};
  enum { SRC = 1, SRC2 = 2, X = 4, SIGMA = 8, PRE = 16, SC = 32, WT = 64, BIAS = 128, OUT = 256, OPRE = 512, PART = 1024, GSIG = 2048 };
  unsigned need = 0, may = 0;
  switch (d.op) {
    case PNPX_FWD_PREP_INPUT: need = X | SIGMA | OUT; break;
    case PNPX_FWD_CONV_FIRST: need = X | SIGMA | WT | BIAS | OUT; break;
    case PNPX_FWD_OUTC_RESIDUAL: need = SRC | X | WT | BIAS | OUT; may = OPRE; break;
    case PNPX_FWD_ADD: need = SRC | SRC2 | OUT; break;
    case PNPX_FWD_TAIL_OUT: need = SRC | OUT; may = OPRE; break;
    case PNPX_FWD_TAIL_MASK: need = X | PRE | OUT | (hs ? SC : 0); break;
    case PNPX_FWD_DRU_INPUT_GRAD: need = SRC | OUT | PART | GSIG; break;
    default: need = SRC | OUT; break;      // MAXPOOL2, UPSAMPLE2X, S2D, D2S
  }
  for (int i = 0; i < 12; ++i) {
    const unsigned bit = 1u << i;
    if ((need & bit) && !p[i]) return bad(PNPX_ERR_ARG, "an operand of the op is null");
    if (!((need | may) & bit) && p[i]) return bad(PNPX_ERR_ARG, "an operand the op has no place for");
  }
  return PNPX_OK;
}

// host weights and bias on the device for the length of one call
struct DevCopy {
  float* p = nullptr;
  ~DevCopy() {
    if (p) (void)hipFree(p);
  }
  int put(const float* w, size_t nw, const float* b, size_t nb) {
    PNPX_HIP(hipMalloc(reinterpret_cast<void**>(&p), (nw + nb) * sizeof(float)));
    PNPX_HIP(hipMemcpy(p, w, nw * sizeof(float), hipMemcpyHostToDevice));
    PNPX_HIP(hipMemcpy(p + nw, b, nb * sizeof(float), hipMemcpyHostToDevice));
    return PNPX_OK;
  }
};

}  // namespace

extern "C" int pnpx_fwd_glue_probe_plan(const pnpx_fwd_glue_probe_desc* desc) {
  if (!desc) return 0;
  int form = 0, launches = 1;
  if (validate_sizes(*desc, &form, &launches) != PNPX_OK) return 0;
  return form + 256 * (launches - 1);
}

extern "C" int pnpx_fwd_glue_probe(pnpx_ctx* ctx, const pnpx_fwd_glue_probe_desc* desc, void* stream) {
  if (!ctx || !desc) {
    set_error("pnpx_fwd_glue_probe: null context or descriptor");
    return PNPX_ERR_ARG;
  }
  const pnpx_fwd_glue_probe_desc& d = *desc;
  int form = 0, launches = 1;
  PNPX_TRY(validate_sizes(d, &form, &launches));
  PNPX_TRY(validate_operands(d));
  std::lock_guard<std::mutex> lk(ctx->mu);
  PNPX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool hs = d.family == 1;
  const float* sf = static_cast<const float*>(d.src);
  const float* s2f = static_cast<const float*>(d.src2);
  const HsRec* sh = static_cast<const HsRec*>(d.src);
  const HsRec* s2h = static_cast<const HsRec*>(d.src2);
  float* of = static_cast<float*>(d.out);
  HsRec* oh = static_cast<HsRec*>(d.out);
  DevCopy wb;
  if (d.op == PNPX_FWD_CONV_FIRST) PNPX_TRY(wb.put(d.w, (size_t)d.C * 18, d.bias, (size_t)d.C));
  if (d.op == PNPX_FWD_OUTC_RESIDUAL) PNPX_TRY(wb.put(d.w, 32, d.bias, 1));
  int rc = PNPX_OK;
  switch (d.op) {
    case PNPX_FWD_PREP_INPUT:
      rc = hs ? launch_prep_input_hs(d.x, d.sigma, d.sigma_stride, oh, d.B, d.H, d.W, s)
              : launch_prep_input_f32(d.x, d.sigma, d.sigma_stride, of, d.B, d.H, d.W, s);
      break;
    case PNPX_FWD_CONV_FIRST:
      rc = hs ? launch_conv_first_hs(d.x, d.sigma, d.sigma_stride, wb.p, wb.p + (size_t)d.C * 18, oh, d.C, d.B, d.H, d.W, d.slope,
                                     std::ldexp(HS_ASCALE, -d.k), s)
              : launch_conv_first_f32(d.x, d.sigma, d.sigma_stride, wb.p, wb.p + (size_t)d.C * 18, of, d.C, d.B, d.H, d.W, d.slope, s);
      break;
    case PNPX_FWD_MAXPOOL2:
      rc = hs ? launch_maxpool2_hs(sh, oh, (size_t)d.B * (d.C / 8), d.H, d.W, s) : launch_maxpool2_f32(sf, of, (size_t)d.B * d.C, d.H, d.W, s);
      break;
    case PNPX_FWD_UPSAMPLE2X:
      rc = hs ? launch_upsample2x_hs(d.form, sh, oh, d.B, d.C / 8, d.H, d.W, d.Ht, d.Wt, s)
              : launch_upsample2x_f32(d.form, sf, of, (size_t)d.B * d.C, d.H, d.W, d.Ht, d.Wt, s);
      break;
    case PNPX_FWD_OUTC_RESIDUAL:
      rc = hs ? launch_outc_residual_hs(sh, d.x, wb.p, wb.p + 32, of, d.out_pre, d.B, d.H, d.W, s)
              : launch_outc_residual_f32(sf, d.x, wb.p, wb.p + 32, of, d.out_pre, d.B, d.H, d.W, s);
      break;
    case PNPX_FWD_S2D:
      rc = hs ? launch_s2d_hs(sh, oh, d.B, d.C / 8, d.H, d.W, s) : launch_s2d_f32(sf, of, d.B, d.C, d.H, d.W, s);
      break;
    case PNPX_FWD_D2S:
      rc = hs ? launch_d2s_hs(sh, oh, d.B, d.C / 8, d.H, d.W, s) : launch_d2s_f32(sf, of, d.B, d.C, d.H, d.W, s);
      break;
    case PNPX_FWD_ADD:
      rc = hs ? launch_add_hs(sh, s2h, oh, (size_t)d.B * (d.C / 8), d.H, d.W, s) : launch_add_f32(sf, s2f, of, (size_t)d.B * d.C, d.H, d.W, s);
      break;
    case PNPX_FWD_TAIL_OUT:
      rc = launch_tail_out_f32(sf, of, d.out_pre, d.B, d.H, d.W, s);
      break;
    case PNPX_FWD_TAIL_MASK:
      rc = hs ? launch_tail_mask_hs(d.x, d.pre, reinterpret_cast<const float2*>(d.sc), of, (size_t)d.B * d.H * d.W, s)
              : launch_tail_mask_f32(d.x, d.pre, of, (size_t)d.B * d.H * d.W, s);
      break;
    default:
      rc = launch_dru_input_grad_f32(sf, d.C, of, d.part, d.gsigma, d.B, d.H, d.W, s);
      break;
  }
  const hipError_t e = hipStreamSynchronize(s);      // (before the weights' copy is freed)
  if (rc == PNPX_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(fwd glue probe)", __FILE__, __LINE__);
  return rc;
}
