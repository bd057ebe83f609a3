// Half-split convolution, input-gradient epilogue of the critic's TReLU layers: (conv [+ res]) where the saved forward
// activation lies above its threshold (critic.hip).  3x3 adjoints and the adjoint of a 2x2-window stride-2 entry on its
// space-to-depth grid (the mirrored window, tap mask 0x1B0).  Kernel template: conv_hs_kernel.h.
#include "conv_hs_kernel.h"

namespace pnpx {

int launch_conv_hs_dthr(const ConvHsArgs& a, int mt, int taps, int B, hipStream_t s) {
  if (taps == 0x1FF) return mt == 64 ? launch_hs_mt<64, EPI_DTHR>(a, B, s) : launch_hs_mt<32, EPI_DTHR>(a, B, s);
  if (taps == 0x1B0) return mt == 64 ? launch_hs_mt<64, EPI_DTHR, 0x1B0>(a, B, s) : launch_hs_mt<32, EPI_DTHR, 0x1B0>(a, B, s);
  set_error("conv_hs: no input-gradient instance for tap mask 0x%x", taps);
  return PNPX_ERR_SHAPE;
}

}  // namespace pnpx
