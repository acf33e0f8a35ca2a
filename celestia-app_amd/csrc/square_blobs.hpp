// The blobs of a BlobTx as square.cpp's parser sees them, for the commitment entry points
// (api_commit.cpp). Host only, no HIP: square.cpp is also built by a plain host compiler.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

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
}  // namespace cel
