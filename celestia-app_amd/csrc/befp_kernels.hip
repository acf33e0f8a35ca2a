// Device glue of the bad-encoding fraud proofs (api_befp.cpp, layout: befp_plan.hpp): what
// keeps verify -> decode -> encode -> roots -> verdict of a batch of proofs on one stream.
//   k_befp_place    the entries' shares into their proofs' dense axes, with the presence mask
//                   and a per-proof flag for a failed entry;
//   k_befp_verdict  the verdict byte and the rebuilt root of each proof;
//   k_befp_roots_ok the producer's check of gathered trees' roots against the header's.
// Everything between them is the existing launches (nmt_verify.hip, rs_*.hip, nmt_trees.hip).
#include <hip/hip_runtime.h>

#include "befp_kernels.hpp"
#include "befp_plan.hpp"

namespace cel {

namespace {

// Entry e of the batch: share e (512 bytes, 16-byte aligned) into cell cell[e] of the dense
// axes (cell = live proof * W + position), 32 lanes of 16 bytes per share. Lane 0 of a share
// marks the cell present and, when the entry's NMT proof failed (ok[e] == 0), raises its
// proof's flag. A failed entry's share is placed all the same: the proof's verdict is fixed by
// the flag, and the decoder then always sees at least k distinct shards per axis.
__global__ __launch_bounds__(256) void k_befp_place(const uint4* __restrict__ shares, const uint32_t* __restrict__ cell,
                                                    const uint8_t* __restrict__ ok, uint64_t n_ent, uint32_t log_w,
                                                    uint4* __restrict__ dense, uint8_t* __restrict__ dmask,
                                                    uint8_t* __restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t e = t >> 5;
  const uint32_t q = (uint32_t)(t & 31);
  if (e >= n_ent) return;
  const uint32_t c = cell[e];
  dense[(uint64_t)c * (kShare / 16) + q] = shares[t];
  if (q == 0) {
    dmask[c] = 1;
    if (!ok[e]) bad[c >> log_w] = 1;  // every writer stores the same byte
  }
}

// Byte b of the 96-byte record at rec against byte b of the packed 90-byte node at want.
__device__ __forceinline__ bool node_byte_differs(const uint32_t* rec, const uint8_t* want, uint32_t b, uint8_t* got) {
  *got = reinterpret_cast<const uint8_t*>(rec)[b];
  return *got != want[b];
}

// One workgroup per live proof p, lane b < 90 one byte of the root. bad[p]: an entry failed.
// root_rec: launch_axes_roots' records; accused: the packed accused roots, proof p's at 90 * p.
// results: verdicts [n], then from rebuilt_off on the rebuilt roots [n][90] (zeros where an
// entry failed).
__global__ __launch_bounds__(128) void k_befp_verdict(const uint8_t* __restrict__ bad,
                                                      const uint32_t* __restrict__ root_rec,
                                                      const uint8_t* __restrict__ accused, uint32_t n,
                                                      uint8_t* __restrict__ verdict, uint8_t* __restrict__ rebuilt) {
  const uint32_t p = blockIdx.x, b = threadIdx.x;
  if (p >= n) return;  // uniform per workgroup
  const bool failed = bad[p] != 0;
  uint8_t got = 0;
  const bool diff = b < kNode && node_byte_differs(root_rec + (uint64_t)p * kNodeWords, accused + (uint64_t)p * kNode, b, &got);
  const int any = __syncthreads_or(diff ? 1 : 0);
  if (b < kNode) rebuilt[(uint64_t)p * kNode + b] = failed ? (uint8_t)0 : got;
  if (b == 0) verdict[p] = failed ? befp::kBadShare : any ? befp::kFraud : befp::kNotFraud;
}

// One workgroup per gathered tree a: ok[a] = its root record (record root0 + a of `nodes`)
// equals the packed header root at want + 90 * a.
__global__ __launch_bounds__(128) void k_befp_roots_ok(const uint32_t* __restrict__ nodes, uint64_t root0,
                                                       const uint8_t* __restrict__ want, uint32_t count,
                                                       uint8_t* __restrict__ ok) {
  const uint32_t a = blockIdx.x, b = threadIdx.x;
  if (a >= count) return;
  uint8_t got;
  const bool diff = b < kNode && node_byte_differs(nodes + (root0 + a) * kNodeWords, want + (uint64_t)a * kNode, b, &got);
  const int any = __syncthreads_or(diff ? 1 : 0);
  if (b == 0) ok[a] = any ? 0 : 1;
}

}  // namespace

hipError_t launch_befp_place(const uint8_t* d_shares, const uint32_t* d_cell, const uint8_t* d_ok, uint64_t n_ent,
                             uint32_t W, uint8_t* d_dense, uint8_t* d_dmask, uint8_t* d_bad, hipStream_t s) {
  if (!n_ent) return hipSuccess;
  const uint64_t blocks = (n_ent * 32 + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_befp_place, dim3((uint32_t)blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(d_shares),
                     d_cell, d_ok, n_ent, befp::log2_width(W), reinterpret_cast<uint4*>(d_dense), d_dmask, d_bad);
  return hipGetLastError();
}

hipError_t launch_befp_verdict(const uint8_t* d_bad, const uint32_t* d_root_rec, const uint8_t* d_accused, uint32_t n,
                               uint8_t* d_verdict, uint8_t* d_rebuilt, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_befp_verdict, dim3(n), dim3(128), 0, s, d_bad, d_root_rec, d_accused, n, d_verdict, d_rebuilt);
  return hipGetLastError();
}

hipError_t launch_befp_roots_ok(const uint32_t* d_nodes, uint64_t root0, const uint8_t* d_want, uint32_t count,
                                uint8_t* d_ok, hipStream_t s) {
  if (count) hipLaunchKernelGGL(k_befp_roots_ok, dim3(count), dim3(128), 0, s, d_nodes, root0, d_want, count, d_ok);
  return hipGetLastError();
}

}  // namespace cel
