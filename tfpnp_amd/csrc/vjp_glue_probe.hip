// Probe of the launches between the UNet VJP's adjoint convolutions, for tests (tests/test_gpu_vjp_glue.py): ONE call of a launcher of
// grad_common.h -- the very function unet_denoise_backward calls -- on tensors the caller laid out, and a wait for it.
// pnpx_vjp_glue_probe_plan asks the launchers' own host-only form decisions.  Nothing in the library calls either; they add no option.
#include "common.h"
#include "grad_common.h"

using namespace pnpx;

namespace {

int bad(int code, const char* what) {
  set_error("pnpx_vjp_glue_probe: %s", what);
  return code;
}

// sizes and form: what the op cannot run.  *form_out = the form the launcher will take, *launches = kernel launches of the op's own kernel.
int validate_sizes(const pnpx_vjp_glue_probe_desc& d, int* form_out, int* launches) {
  *form_out = 0;
  *launches = 1;
  if (d.family != 0 && d.family != 1) return bad(PNPX_ERR_ARG, "family is 0 (fp32) or 1 (half-split)");
  if (d.B <= 0 || d.C <= 0 || d.H <= 0 || d.W <= 0 || d.form < 0) return bad(PNPX_ERR_SHAPE, "non-positive size");
  const bool hs = d.family == 1;
  const bool ups = d.op == PNPX_VJP_UPSAMPLE_BWD, spm = d.op == PNPX_VJP_SKIP_POOL_MERGE;
  if (!ups && (d.c_off != 0 || d.Ht != 0 || d.Wt != 0)) return bad(PNPX_ERR_ARG, "c_off / Ht / Wt belong to the up-sampling adjoint only");
  if (!ups && !spm && d.Ccat != 0) return bad(PNPX_ERR_ARG, "Ccat belongs to the up-sampling adjoint and the skip / pool merge only");
  if (hs && d.op != PNPX_VJP_GRAD_SCALE && (d.C % 8 || d.Ccat % 8 || d.c_off % 8)) return bad(PNPX_ERR_SHAPE, "half-split channel counts are multiples of 8");
  int form = d.form ? d.form : VG_ONLY;
  switch (d.op) {
    case PNPX_VJP_OUTC_BWD:
      if (d.C != 32) return bad(PNPX_ERR_SHAPE, "the out-conv tail has 32 channels");
      break;
    case PNPX_VJP_UPSAMPLE_BWD:
      if (d.c_off < 0 || d.Ccat < d.c_off + d.C) return bad(PNPX_ERR_SHAPE, "channels [c_off, c_off + C) outside the concat");
      if (d.Ht < 2 * d.H || d.Ht > 2 * d.H + 1 || d.Wt < 2 * d.W || d.Wt > 2 * d.W + 1) return bad(PNPX_ERR_SHAPE, "Ht x Wt is 2H or 2H + 1 by 2W or 2W + 1");
      if (hs) {
        *launches = upsample_bwd_hs_launches(d.B, d.C / 8);
        if (*launches <= 0) return bad(PNPX_ERR_SHAPE, "more channel groups per image than planes of one launch");
      } else {
        if (!d.form) form = upsample_bwd_form_f32((size_t)d.B, d.C, d.W);
        if (!upsample_bwd_form_runs(form, (size_t)d.B, d.C)) return bad(PNPX_ERR_SHAPE, "the form cannot run this many planes, or is unknown");
      }
      break;
    case PNPX_VJP_SKIP_POOL_MERGE:
      if (d.Ccat < d.C) return bad(PNPX_ERR_SHAPE, "Ccat below C");
      if (!hs) {
        if (!d.form) form = skip_pool_merge_form_f32(d.H, d.W);
        if (!skip_pool_merge_form_runs(form, d.H, d.W)) return bad(PNPX_ERR_SHAPE, "the 2 x 2-block form needs even sizes, or the form is unknown");
      }
      break;
    case PNPX_VJP_INPUT_GRAD:
      if (hs ? d.C != 32 : d.C < 2) return bad(PNPX_ERR_SHAPE, "the input gradient has 32 channels (half-split) or at least 2 (fp32)");
      if ((long long)d.H * d.W > 0x7fffffffLL || d.B > 65535) return bad(PNPX_ERR_SHAPE, "image or batch too large");
      break;
    case PNPX_VJP_GRAD_SCALE:
      if (!hs) return bad(PNPX_ERR_ARG, "the gradient scale belongs to the half-split family");
      if (d.C != 1) return bad(PNPX_ERR_SHAPE, "the gradient scale reads one channel");
      break;
    default:
      return bad(PNPX_ERR_ARG, "unknown op");
  }
  if (form != VG_ONLY && (hs || (!ups && !spm))) return bad(PNPX_ERR_SHAPE, "the op has one form");
  *form_out = form;
  return PNPX_OK;
}

// operands: each op's own, all of them, and no other
int validate_operands(const pnpx_vjp_glue_probe_desc& d) {
  const bool hs = d.family == 1;
  // bit i: g, act, g_pool, pre, w, g_res, sc, out, out_res, part, gsigma, bits
  const void* p[12] = {d.g, d.act, d.g_pool, d.pre, d.w, d.g_res, d.sc, d.out, d.out_res, d.part, d.gsigma, d.bits};
  enum { G = 1, ACT = 2, GPOOL = 4, PRE = 8, WT = 16, GRES = 32, SC = 64, OUT = 128, ORES = 256, PART = 512, GSIG = 1024, BITS = 2048 };
  unsigned need = 0, may = 0;
  switch (d.op) {
    case PNPX_VJP_OUTC_BWD: need = G | ACT | PRE | WT | OUT | ORES | (hs ? SC : 0); break;
    case PNPX_VJP_UPSAMPLE_BWD: need = G | ACT | OUT; break;
    case PNPX_VJP_SKIP_POOL_MERGE: need = G | ACT | OUT; may = GPOOL; break;
    case PNPX_VJP_INPUT_GRAD: need = G | GRES | OUT | PART | GSIG | (hs ? SC : 0); break;
    default: need = G | OUT | BITS; break;
  }
  for (int i = 0; i < 12; ++i) {
    const unsigned bit = 1u << i;
    if ((need & bit) && !p[i]) return bad(PNPX_ERR_ARG, "an operand of the op is null");
    if (!((need | may) & bit) && p[i]) return bad(PNPX_ERR_ARG, "an operand the op has no place for");
  }
  return PNPX_OK;
}

}  // namespace

extern "C" int pnpx_vjp_glue_probe_plan(const pnpx_vjp_glue_probe_desc* desc) {
  if (!desc) return 0;
  int form = 0, launches = 1;
  if (validate_sizes(*desc, &form, &launches) != PNPX_OK) return 0;
  return form + 256 * (launches - 1);
}

extern "C" int pnpx_vjp_glue_probe(pnpx_ctx* ctx, const pnpx_vjp_glue_probe_desc* desc, void* stream) {
  if (!ctx || !desc) {
    set_error("pnpx_vjp_glue_probe: null context or descriptor");
    return PNPX_ERR_ARG;
  }
  const pnpx_vjp_glue_probe_desc& d = *desc;
  int form = 0, launches = 1;
  PNPX_TRY(validate_sizes(d, &form, &launches));
  PNPX_TRY(validate_operands(d));
  std::lock_guard<std::mutex> lk(ctx->mu);
  PNPX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool hs = d.family == 1;
  const float* gf = static_cast<const float*>(d.g);
  const float* af = static_cast<const float*>(d.act);
  const HsRec* gh = static_cast<const HsRec*>(d.g);
  const HsRec* ah = static_cast<const HsRec*>(d.act);
  float* of = static_cast<float*>(d.out);
  HsRec* oh = static_cast<HsRec*>(d.out);
  const float2* sc = reinterpret_cast<const float2*>(d.sc);
  int rc = PNPX_OK;
  switch (d.op) {
    case PNPX_VJP_OUTC_BWD:
      rc = hs ? launch_outc_bwd_hs(gf, d.pre, d.w, ah, oh, d.out_res, sc, d.B, d.H, d.W, s)
              : launch_outc_bwd_f32(gf, d.pre, d.w, af, of, d.out_res, d.B, d.H, d.W, s);
      break;
    case PNPX_VJP_UPSAMPLE_BWD:
      rc = hs ? launch_upsample_bwd_hs(gh, d.Ccat / 8, d.c_off / 8, ah, oh, d.B, d.C / 8, d.H, d.W, d.Ht, d.Wt, s)
              : launch_upsample_bwd_f32(d.form, gf, d.Ccat, d.c_off, af, of, d.B, d.C, d.H, d.W, d.Ht, d.Wt, s);
      break;
    case PNPX_VJP_SKIP_POOL_MERGE:
      rc = hs ? launch_skip_pool_merge_hs(gh, d.Ccat / 8, static_cast<const HsRec*>(d.g_pool), ah, oh, d.B, d.C / 8, d.H, d.W, s)
              : launch_skip_pool_merge_f32(d.form, gf, d.Ccat, static_cast<const float*>(d.g_pool), af, of, d.B, d.C, d.H, d.W, s);
      break;
    case PNPX_VJP_INPUT_GRAD:
      rc = hs ? launch_input_grad_hs(gh, d.g_res, of, d.part, sc, d.gsigma, d.B, d.H, d.W, s)
              : launch_input_grad_f32(gf, d.C, d.g_res, of, d.part, d.gsigma, d.B, d.H, d.W, s);
      break;
    default:
      rc = launch_grad_scale(gf, (size_t)d.B * d.H * d.W, d.bits, reinterpret_cast<float2*>(d.out), s);
      break;
  }
  const hipError_t e = hipStreamSynchronize(s);
  if (rc == PNPX_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(vjp glue probe)", __FILE__, __LINE__);
  return rc;
}
