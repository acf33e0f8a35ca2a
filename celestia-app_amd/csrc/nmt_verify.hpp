// The batched NMT proof verifiers' device interface (nmt_verify.hip: VerifyInclusion and
// VerifyNamespace), used by api_verify.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace cel {

// One proof of a batch, as the fold kernel reads it. Ranges are in records: the proof's
// leaves are leaf records [leaf0, leaf0 + nleaves), its nodes node records [node0, node0 +
// nnodes), its root is packed root `root` of the caller's roots (repacked into root record i).
// pad: 0 for the inclusion verifier; the namespace verifier keeps the proof's kind there.
struct VerifyProof {
  int32_t start, end;
  uint32_t nleaves, nnodes;
  uint64_t leaf0, node0;
  uint32_t root, pad;
};
static_assert(sizeof(VerifyProof) == 40, "VerifyProof layout");

// The workspace of one batch. The head [0, head_bytes) is filled by the host and uploaded
// in one copy: the proofs, a 32-byte namespace per proof (29 bytes, zero padded), and the
// proof index of every leaf. Behind it the 96-byte records of the leaves and of the nodes
// followed by one root per proof.
struct VerifyWork {
  VerifyProof* proofs;
  uint32_t* ns;
  uint32_t* leaf_proof;
  size_t head_bytes;
  uint32_t* leaf_rec;
  uint32_t* node_rec;
  size_t bytes;
};
// On a null `work` every pointer is null and `bytes` is the workspace's size.
VerifyWork verify_carve(void* work, uint64_t total_leaves, uint64_t total_nodes, uint32_t n);

enum { kVerifyRepack = 1, kVerifyLeaves = 2, kVerifyFold = 4, kVerifyAll = 7 };
// The stages of a batch whose head is in place (stages: a measurement runs them apart).
// d_leaves: 16-byte aligned shares; d_nodes, d_roots: packed 90-byte nodes, any alignment.
hipError_t launch_verify(const VerifyWork& w, const uint8_t* d_leaves, uint64_t total_leaves, const uint8_t* d_nodes,
                         uint64_t total_nodes, const uint8_t* d_roots, uint32_t n, uint8_t* d_ok, int stages,
                         hipStream_t s);
// Share d_src[t] of d_shares into cell d_dst[t] (row-major index) of d_eds, t < n.
hipError_t launch_place_shares(const uint8_t* d_shares, const uint32_t* d_src, const uint32_t* d_dst, uint32_t n,
                               uint8_t* d_eds, hipStream_t s);

// nmt Proof.VerifyNamespace for a batch (nmt_verify.hip). The table is the inclusion
// verifier's, with the proof's kind (CEL_NS_INCLUSION / CEL_NS_ABSENCE) in VerifyProof::pad.
// Behind the total_leaves leaf records lies one more record per proof, record total_leaves + i,
// where an absence proof's fold starts from its leaf hash; leaf_ok holds one byte per leaf:
// does the share start with its proof's namespace?
struct VerifyNsWork {
  VerifyWork v;
  uint8_t* leaf_ok;
  size_t bytes;
};
VerifyNsWork verify_ns_carve(void* work, uint64_t total_leaves, uint64_t total_nodes, uint32_t n);
// The stages as in launch_verify: repack (the inclusion verifier's kernel), leaves, fold.
hipError_t launch_verify_ns(const VerifyNsWork& w, const uint8_t* d_leaves, uint64_t total_leaves,
                            const uint8_t* d_nodes, uint64_t total_nodes, const uint8_t* d_roots, uint32_t n,
                            uint8_t* d_ok, int stages, hipStream_t s);

}  // namespace cel
