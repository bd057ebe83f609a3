// Live weights: what the actor (policy_pack.hip) and the critic (critic.hip) keep around the flat fp32 parameter vector that
// stays on the device, and nothing that knows which network the vector belongs to.
//   LiveParams      the vector itself ("master"): every packed layout a forward reads is derived from it
//   PackWorkspace   what one device-side packing of it needs: the layer table (uploaded once, when the blob is allocated), the
//                   per-channel fold results, the block read back per refresh -- and the launch dimensions of that table, so that
//                   a refresh does not rebuild the table on the host to learn them
//   BlobCursor      the two running offsets every layout table is built with
//   LiveOptim       clip + Adam on the vector: moments, step counter, frozen ranges (kernels: live_optim.hip)
// The fold and scale kernels differ per network (weight-norm in double, BatchNorm in fp32) and stay there; so do the pointer
// carve-ups of the workspace.  The one kernel that is the same, the copy of biases and head matrices, is in live_params.hip
// (launch_live_copy, pack_desc.h).
//
// Part of common.h (included there behind DeviceBuf): include common.h, not this file.
#pragma once

namespace pnpx {

struct LiveParams {
  DeviceBuf master;   // [n] floats, in the order of the network's load entry
  size_t n = 0;
  float* p() const { return static_cast<float*>(master.p); }
  int alloc(size_t count, const char* what);                  // what: "<network> parameter", for the allocation error
  int set_host(const float* src);                             // synchronous upload of n floats
  int set_device(const float* src_dev, hipStream_t s);        // n floats on stream s; nothing if src_dev is the vector itself
  int copy_out(float* dst_dev, hipStream_t s) const;          // n floats on stream s
  void free();
};

// clip_grad_norm_ + Adam on a live vector (live_optim.hip): the moments, the step counter and the ranges of the vector the optimiser
// must not see (buffers that live in the vector next to the parameters).  The owner's driver checks its arguments, hands in the device
// slot (two floats: norm, clip coefficient) it reads back with its own refresh, and calls commit() once it has seen a finite norm.
struct FrozenRange {
  size_t first, count;   // elements [first, first + count)
};
constexpr int LIVE_OPTIM_MAX_FROZEN = 32;
constexpr int LIVE_OPTIM_PARTIALS = 1024;   // blocks of the sum-of-squares launch = doubles it writes
// sorted ranges, adjacent ones merged, empty ones dropped; PNPX_ERR_SHAPE if unsorted, overlapping, outside [0, vec_n) or too many
int live_merge_frozen(const FrozenRange* in, int n, size_t vec_n, FrozenRange* out, int* n_out);
struct LiveOptim {
  DeviceBuf state;     // exp_avg, exp_avg_sq (each padded to a multiple of four floats), then the sum-of-squares partials; allocated
                       // zero-filled by the first step
  DeviceBuf frozen;    // [nfrozen] FrozenRange, uploaded once with the network (set_frozen); none: null
  int nfrozen = 0;
  long long step = 0;  // Adam's step counter t
  int set_frozen(const FrozenRange* ranges, int n, size_t vec_n, const char* what);   // synchronous upload; merges adjacent ranges
  // sum of squares, finish (slot[0] = norm, slot[1] = min(1, max_norm / (norm + 1e-6)); norm_out, may be null, receives the norm as
  // well), the fused update of live / the moments on stream s; what: "<network> optimiser state", for the allocation error.  A norm
  // that is not finite: the update writes nothing.  The counter does not move: commit()
  int launch_step(const LiveParams& live, const float* grad, float lr, float beta1, float beta2, float eps, float max_norm, float* slot,
                  float* norm_out, const char* what, hipStream_t s);
  void commit() { ++step; }
  int copy_state(size_t n, float* exp_avg_dst, float* exp_avg_sq_dst, long long* step_host, hipStream_t s) const;   // zeros and 0 before the first step
  int reset();         // back to "before the first step" (the frozen ranges stay)
  void free();
};

struct PackDims {     // grid dimensions of the refresh launches over one table
  unsigned nchan = 0;        // output channels over all convolutions
  unsigned max_items = 0;    // largest half-split packing
  unsigned max_copy = 0;     // largest copy, of ncopy
  int ncopy = 0;
};
struct PackWorkspace {
  DeviceBuf ws;                // the table, padded to 256 bytes; the per-channel arrays; the read-back block
  float* readback = nullptr;   // pinned host copy of the read-back block
  PackDims dims;
  // ws = table | chan_bytes | readback_floats, the table uploaded; readback = readback_floats on the host
  int alloc(const void* table, size_t table_bytes, size_t chan_bytes, size_t readback_floats, const PackDims& d, const char* what);
  void free();
};

struct BlobCursor {   // offsets in floats: into the parameter vector (sources, in order) and into the blob (256-float aligned entries)
  size_t src = 0, dst = 0;
  unsigned take(size_t n) {
    const size_t r = src;
    src += n;
    return (unsigned)r;
  }
  size_t put(size_t n) {
    dst = (dst + 255) & ~(size_t)255;
    const size_t r = dst;
    dst += n;
    return r;
  }
};

}  // namespace pnpx
