// Half-split convolution, TReLU epilogue max(conv + bias [+ res], alpha): the weight-normalised convolutions of the critic
// (critic.hip; tfpnp/trainer/mddpg/critic.py:11-19, 37-60) -- 3x3 layers and the 2x2-window form of the stride-2 entries (0x01B).
// Kernel template: conv_hs_kernel.h.
#include "conv_hs_kernel.h"

namespace pnpx {

int launch_conv_hs_trelu(const ConvHsArgs& a, int mt, int taps, int B, hipStream_t s) {
  if (taps == 0x1FF) return mt == 64 ? launch_hs_mt<64, EPI_TRELU>(a, B, s) : launch_hs_mt<32, EPI_TRELU>(a, B, s);
  if (taps == 0x01B) return mt == 64 ? launch_hs_mt<64, EPI_TRELU, 0x01B>(a, B, s) : launch_hs_mt<32, EPI_TRELU, 0x01B>(a, B, s);
  set_error("conv_hs: no TReLU instance for tap mask 0x%x", taps);
  return PNPX_ERR_SHAPE;
}

}  // namespace pnpx
