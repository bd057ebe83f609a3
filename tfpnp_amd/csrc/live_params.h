// Live weights: what the actor (policy_pack.hip) and the critic (critic.hip) keep around the flat fp32 parameter vector that
// stays on the device, and nothing that knows which network the vector belongs to.
//   LiveParams      the vector itself ("master"): every packed layout a forward reads is derived from it
//   PackWorkspace   what one device-side packing of it needs: the layer table (uploaded once, when the blob is allocated), the
//                   per-channel fold results, the block read back per refresh -- and the launch dimensions of that table, so that
//                   a refresh does not rebuild the table on the host to learn them
//   BlobCursor      the two running offsets every layout table is built with
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
