// Live weights shared by the actor and the critic: live_params.h.
#include "common.h"
#include "pack_desc.h"

namespace pnpx {

int LiveParams::alloc(size_t count, const char* what) {
  PNPX_TRY(alloc_dev(master, count * sizeof(float), what));
  n = count;
  return PNPX_OK;
}

int LiveParams::set_host(const float* src) {
  PNPX_HIP(hipMemcpy(master.p, src, n * sizeof(float), hipMemcpyHostToDevice));
  return PNPX_OK;
}

int LiveParams::set_device(const float* src_dev, hipStream_t s) {
  if (src_dev != master.p) PNPX_HIP(hipMemcpyAsync(master.p, src_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return PNPX_OK;
}

int LiveParams::copy_out(float* dst_dev, hipStream_t s) const {
  PNPX_HIP(hipMemcpyAsync(dst_dev, master.p, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return PNPX_OK;
}

void LiveParams::free() {
  if (master.p) (void)hipFree(master.p);
  *this = LiveParams();
}

int PackWorkspace::alloc(const void* table, size_t table_bytes, size_t chan_bytes, size_t readback_floats, const PackDims& d,
                         const char* what) {
  PNPX_TRY(alloc_dev(ws, ((table_bytes + 255) & ~(size_t)255) + chan_bytes + readback_floats * sizeof(float), what));
  void* h = nullptr;
  PNPX_HIP(hipHostMalloc(&h, readback_floats * sizeof(float), hipHostMallocDefault));
  readback = static_cast<float*>(h);
  PNPX_HIP(hipMemcpy(ws.p, table, table_bytes, hipMemcpyHostToDevice));
  dims = d;
  return PNPX_OK;
}

void PackWorkspace::free() {
  if (ws.p) (void)hipFree(ws.p);
  if (readback) (void)hipHostFree(readback);
  *this = PackWorkspace();
}

namespace {

__global__ __launch_bounds__(256) void live_copy_kernel(const CopyDesc* __restrict__ copy, const float* __restrict__ P,
                                                        const float* __restrict__ sh, float* __restrict__ blob) {
  const CopyDesc C = copy[blockIdx.y];
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i < C.n) blob[C.dst + i] = (C.space ? sh : P)[C.src + i];
}

}  // namespace

int launch_live_copy(const CopyDesc* copy_dev, dim3 grid, const float* P, const float* sh, float* blob, hipStream_t s) {
  hipLaunchKernelGGL(live_copy_kernel, grid, dim3(256), 0, s, copy_dev, P, sh, blob);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

}  // namespace pnpx
