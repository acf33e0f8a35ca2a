// The bad-encoding fraud proofs' device interface (befp_kernels.hip), used by api_befp.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cel_internal.hpp"

namespace cel {

// Share e of d_shares (16-byte aligned) into cell d_cell[e] of d_dense ([axes][W][512], 16-byte
// aligned), d_dmask[cell] = 1, and d_bad[cell / W] = 1 where d_ok[e] == 0; e < n_ent. The
// caller zeroes d_dmask and d_bad first. W a power of two.
hipError_t launch_befp_place(const uint8_t* d_shares, const uint32_t* d_cell, const uint8_t* d_ok, uint64_t n_ent,
                             uint32_t W, uint8_t* d_dense, uint8_t* d_dmask, uint8_t* d_bad, hipStream_t s);
// Per proof p < n: CEL_BEFP_BAD_SHARE where d_bad[p], else FRAUD / NOT_FRAUD as root record p
// of d_root_rec (96-byte records) differs from / equals the packed root at d_accused + 90 * p.
// d_rebuilt [n][90]: the record's 90 bytes, zeros for a bad share.
hipError_t launch_befp_verdict(const uint8_t* d_bad, const uint32_t* d_root_rec, const uint8_t* d_accused, uint32_t n,
                               uint8_t* d_verdict, uint8_t* d_rebuilt, hipStream_t s);
// d_ok[a] = record root0 + a of d_nodes equals the packed root at d_want + 90 * a; a < count.
hipError_t launch_befp_roots_ok(const uint32_t* d_nodes, uint64_t root0, const uint8_t* d_want, uint32_t count,
                                uint8_t* d_ok, hipStream_t s);

}  // namespace cel
