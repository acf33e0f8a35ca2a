// Blob share commitments from blob bytes: the device replacement of go-square
// inclusion.CreateCommitment(s) where blobtypes.ValidateBlobTx recomputes them
// (x/blob/types/blob_tx.go:96-105) for CheckTx and ProcessProposal. Like the rest of this
// package it is written against the C ABI and is not compiled in this repository.
package celestiaeds

/*
#include <stdlib.h>
#include "celestia_eds.h"
*/
import "C"

import (
	"unsafe"

	"github.com/celestiaorg/go-square/blob"
)

const commitmentSize = 32

// CreateCommitments wraps cel_create_commitments: inclusion.CreateCommitments(blobs,
// merkle.HashFromByteSlices, threshold) with every hash on the device. The blob bytes are
// packed back to back into page-locked memory (cgo may not retain Go pointers, and the
// library uploads page-locked data in place). Namespaces are hashed as given:
// ValidateBlobNamespace stays with the caller, as in ValidateBlobTx.
func (c *Context) CreateCommitments(blobs []*blob.Blob, threshold int) ([][]byte, error) {
	if len(blobs) == 0 {
		return nil, nil
	}
	total := 0
	for _, b := range blobs {
		total += len(b.Data)
	}
	data := C.cel_host_alloc(C.size_t(total + 1))
	if data == nil {
		return nil, &StatusError{Status: int(C.CEL_ENOMEM), Msg: "page-locked allocation failed"}
	}
	defer C.cel_host_free(data)
	n := len(blobs)
	offsets := C.malloc(C.size_t(8 * (n + 1)))
	nss := C.malloc(C.size_t(C.CEL_NAMESPACE_SIZE * n))
	vers := C.malloc(C.size_t(n))
	out := C.malloc(C.size_t(commitmentSize * n))
	defer C.free(offsets)
	defer C.free(nss)
	defer C.free(vers)
	defer C.free(out)
	d := unsafe.Slice((*byte)(data), total+1)
	o := unsafe.Slice((*C.uint64_t)(offsets), n+1)
	ns := unsafe.Slice((*byte)(nss), C.CEL_NAMESPACE_SIZE*n)
	v := unsafe.Slice((*byte)(vers), n)
	at := 0
	for i, b := range blobs {
		if len(b.NamespaceId) != C.CEL_NAMESPACE_SIZE-1 || b.NamespaceVersion > 255 || b.ShareVersion > 255 {
			return nil, &StatusError{Status: int(C.CEL_EINVAL), Msg: "invalid blob namespace or share version"}
		}
		o[i] = C.uint64_t(at)
		copy(d[at:], b.Data)
		at += len(b.Data)
		ns[i*C.CEL_NAMESPACE_SIZE] = byte(b.NamespaceVersion)
		copy(ns[i*C.CEL_NAMESPACE_SIZE+1:], b.NamespaceId)
		v[i] = byte(b.ShareVersion)
	}
	o[n] = C.uint64_t(at)
	if err := c.call(func() C.cel_status {
		return C.cel_create_commitments(c.ctx, (*C.uint8_t)(data), (*C.uint64_t)(offsets), C.uint32_t(n),
			(*C.uint8_t)(nss), (*C.uint8_t)(vers), C.uint32_t(threshold), (*C.uint8_t)(out))
	}); err != nil {
		return nil, err
	}
	return splitCommitments(out, n), nil
}

// BlobCommitment is one blob's share commitment and the index (in txs) of the BlobTx it
// belongs to.
type BlobCommitment struct {
	TxIndex    int
	Commitment []byte
}

// BlobTxCommitments wraps cel_blob_tx_commitments: the commitments of every blob of every
// BlobTx among txs (a block's raw txs, unmarshalled as square.Construct does), in tx and
// then blob order, from one device batch. ProcessProposal compares them with the
// ShareCommitments of each tx's MsgPayForBlobs instead of calling ValidateBlobTx's
// inclusion.CreateCommitment per blob.
func (c *Context) BlobTxCommitments(txs [][]byte, threshold int) ([]BlobCommitment, error) {
	total := 0
	for _, t := range txs {
		total += len(t)
	}
	buf := C.malloc(C.size_t(total + 1))
	lens := C.malloc(C.size_t(4 * (len(txs) + 1)))
	defer C.free(buf)
	defer C.free(lens)
	b := unsafe.Slice((*byte)(buf), total+1)
	l := unsafe.Slice((*C.uint32_t)(lens), len(txs)+1)
	off := 0
	for i, t := range txs {
		copy(b[off:], t)
		l[i] = C.uint32_t(len(t))
		off += len(t)
	}
	var n C.uint32_t
	if err := c.call(func() C.cel_status {
		return C.cel_blob_tx_commitments(c.ctx, (*C.uint8_t)(buf), (*C.uint32_t)(lens), C.uint32_t(len(txs)),
			C.uint32_t(threshold), nil, nil, 0, &n)
	}); err != nil {
		return nil, err
	}
	if n == 0 {
		return nil, nil
	}
	out := C.malloc(C.size_t(commitmentSize * int(n)))
	idx := C.malloc(C.size_t(4 * int(n)))
	defer C.free(out)
	defer C.free(idx)
	if err := c.call(func() C.cel_status {
		return C.cel_blob_tx_commitments(c.ctx, (*C.uint8_t)(buf), (*C.uint32_t)(lens), C.uint32_t(len(txs)),
			C.uint32_t(threshold), (*C.uint8_t)(out), (*C.uint32_t)(idx), n, &n)
	}); err != nil {
		return nil, err
	}
	cs := splitCommitments(out, int(n))
	ix := unsafe.Slice((*C.uint32_t)(idx), int(n))
	res := make([]BlobCommitment, int(n))
	for i := range res {
		res[i] = BlobCommitment{TxIndex: int(ix[i]), Commitment: cs[i]}
	}
	return res, nil
}

func splitCommitments(p unsafe.Pointer, n int) [][]byte {
	raw := unsafe.Slice((*byte)(p), commitmentSize*n)
	out := make([][]byte, n)
	for i := range out {
		out[i] = append([]byte(nil), raw[i*commitmentSize:(i+1)*commitmentSize]...)
	}
	return out
}
