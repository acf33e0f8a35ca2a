// The blobs of a BlobTx as square.cpp's parser sees them, for the commitment entry points
// (api_commit.cpp). Host only, no HIP: square.cpp is also built by a plain host compiler.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/celestia_eds.h"

namespace cel {
namespace blob {

// One blob of a BlobTx, pointing into the tx bytes.
struct View {
  uint8_t ns[29];
  const uint8_t* data;
  size_t len;
  uint32_t share_version;
};
// blob.UnmarshalBlobTx as cel_square_construct applies it (square.cpp): false if tx is no
// BlobTx, else its blobs in order.
bool blob_tx_views(const uint8_t* tx, size_t n, std::vector<View>& out);

}  // namespace blob

namespace sq {

// The square without its blob bytes (cel_square_layout, include/celestia_eds.h): the width,
// the compact shares of the tx and PayForBlob namespaces as bytes, and the ascending
// segments that cover [0, k * k) exactly once.
struct Layout {
  uint32_t k = 0;
  std::vector<uint8_t> compact;
  std::vector<cel_square_segment> segs;
};
// One blob of a BlobTx among the txs, kept in the square or not (the commitments' input).
struct BlobRef {
  uint8_t ns[29];
  uint64_t off;  // byte offset of the data in the concatenated txs
  uint64_t len;
  uint32_t share_version, tx_index;
};
// cel_square_layout's body for callers inside the library (api_block.cpp): the layout, and
// in all_blobs (nullable) every blob of every BlobTx in order. Same status codes as
// cel_square_construct; the message is left in cel_square_last_error.
cel_status square_layout(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx, uint32_t max_square_size,
                         uint32_t subtree_root_threshold, uint32_t greedy, uint8_t* included, Layout& out,
                         std::vector<BlobRef>* all_blobs);

}  // namespace sq
}  // namespace cel
