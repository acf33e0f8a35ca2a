// Blobs out of a square: go-square's parseSparseShares over runs of ODS shares and the blobs'
// share commitments on the device, what celestia-node's blob service (GetAll, Get, Included)
// builds from the shares of a namespace. Like the rest of this package it is written against
// the C ABI and is not compiled in this repository.
package celestiaeds

/*
#include <stdlib.h>
#include "celestia_eds.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// ShareRange is [Start, End) in row-major index of the original data square.
type ShareRange struct {
	Start, End uint32
}

// RangeBlob is one blob found in a range: its namespace (29 bytes), data, share commitment,
// the ODS index of its first share and the range it was found in.
type RangeBlob struct {
	Namespace  []byte
	Data       []byte
	Commitment []byte
	Index      int
	Range      int
}

// BlobRangeError is the status of a range that does not parse (CEL_BLOB_EVERSION,
// CEL_BLOB_ENOSTART, CEL_BLOB_ESHORT).
type BlobRangeError struct {
	Range, Status int
}

func (e *BlobRangeError) Error() string {
	return fmt.Sprintf("share range %d does not parse into blobs (status %d)", e.Range, e.Status)
}

// BlobsByRange wraps cel_blobs_by_range for a square in host memory (eds: 2k*2k*512 bytes,
// row-major): upload, parse, gather and commit on the device. A range that fails yields no
// blobs and is reported in the second result; the other ranges are unaffected.
func (c *Context) BlobsByRange(eds []byte, k int, ranges []ShareRange, threshold int) ([]RangeBlob, []*BlobRangeError, error) {
	n := len(ranges)
	if n == 0 {
		return nil, nil, nil
	}
	if len(eds) != 4*k*k*int(C.CEL_SHARE_SIZE) {
		return nil, nil, &StatusError{Status: int(C.CEL_EINVAL), Msg: "eds is not 2k*2k*512 bytes"}
	}
	sq := C.cel_host_alloc(C.size_t(len(eds)))
	if sq == nil {
		return nil, nil, &StatusError{Status: int(C.CEL_ENOMEM), Msg: "page-locked allocation failed"}
	}
	defer C.cel_host_free(sq)
	copy(unsafe.Slice((*byte)(sq), len(eds)), eds)
	starts := C.malloc(C.size_t(4 * n))
	ends := C.malloc(C.size_t(4 * n))
	status := C.malloc(C.size_t(4 * n))
	defer C.free(starts)
	defer C.free(ends)
	defer C.free(status)
	s := unsafe.Slice((*C.uint32_t)(starts), n)
	e := unsafe.Slice((*C.uint32_t)(ends), n)
	for i, r := range ranges {
		s[i], e[i] = C.uint32_t(r.Start), C.uint32_t(r.End)
	}
	var nb, tb C.uint64_t
	if err := c.call(func() C.cel_status {
		return C.cel_blobs_by_range(c.ctx, (*C.uint8_t)(sq), C.uint32_t(k), C.uint32_t(n), (*C.uint32_t)(starts),
			(*C.uint32_t)(ends), 0, 0, nil, (*C.uint32_t)(status), nil, nil, C.uint32_t(threshold), &nb, &tb)
	}); err != nil {
		return nil, nil, err
	}
	var failed []*BlobRangeError
	for i, st := range unsafe.Slice((*C.uint32_t)(status), n) {
		if st != 0 {
			failed = append(failed, &BlobRangeError{Range: i, Status: int(st)})
		}
	}
	if nb == 0 {
		return nil, failed, nil
	}
	recs := C.malloc(C.size_t(nb) * C.size_t(unsafe.Sizeof(C.cel_blob_rec{})))
	data := C.malloc(C.size_t(tb))
	coms := C.malloc(C.size_t(commitmentSize) * C.size_t(nb))
	defer C.free(recs)
	defer C.free(data)
	defer C.free(coms)
	if err := c.call(func() C.cel_status {
		return C.cel_blobs_by_range(c.ctx, (*C.uint8_t)(sq), C.uint32_t(k), C.uint32_t(n), (*C.uint32_t)(starts),
			(*C.uint32_t)(ends), nb, tb, (*C.cel_blob_rec)(recs), (*C.uint32_t)(status), (*C.uint8_t)(data),
			(*C.uint8_t)(coms), C.uint32_t(threshold), &nb, &tb)
	}); err != nil {
		return nil, nil, err
	}
	rs := unsafe.Slice((*C.cel_blob_rec)(recs), int(nb))
	raw := unsafe.Slice((*byte)(data), int(tb))
	cs := splitCommitments(coms, int(nb))
	out := make([]RangeBlob, int(nb))
	for i, r := range rs {
		ns := make([]byte, C.CEL_NAMESPACE_SIZE)
		for j := range ns {
			ns[j] = byte(r.ns[j])
		}
		off := int(r.data_off)
		out[i] = RangeBlob{Namespace: ns, Data: append([]byte(nil), raw[off:off+int(r.len)]...), Commitment: cs[i],
			Index: int(r.start), Range: int(r._range)}
	}
	return out, failed, nil
}

// NamespaceODSRanges wraps cel_namespace_ods_ranges: the inclusion entries of a namespace plan
// (cel_dev_namespace_plan / cel_namespace_rows) as one ODS range per queried namespace.
func NamespaceODSRanges(k, nNamespaces int, nsIdx, rows []uint32, starts, ends []int32, kinds []byte) ([]ShareRange, error) {
	m := len(rows)
	if len(nsIdx) != m || len(starts) != m || len(ends) != m || len(kinds) != m {
		return nil, &StatusError{Status: int(C.CEL_EINVAL), Msg: "the entry arrays differ in length"}
	}
	a := make([]C.uint32_t, nNamespaces+1)
	b := make([]C.uint32_t, nNamespaces+1)
	var pi, pr *C.uint32_t
	var ps, pe *C.int32_t
	var pk *C.uint8_t
	if m > 0 {
		pi, pr = (*C.uint32_t)(unsafe.Pointer(&nsIdx[0])), (*C.uint32_t)(unsafe.Pointer(&rows[0]))
		ps, pe = (*C.int32_t)(unsafe.Pointer(&starts[0])), (*C.int32_t)(unsafe.Pointer(&ends[0]))
		pk = (*C.uint8_t)(unsafe.Pointer(&kinds[0]))
	}
	if st := C.cel_namespace_ods_ranges(C.uint32_t(k), C.uint32_t(nNamespaces), C.uint64_t(m), pi, pr, ps, pe, pk, &a[0], &b[0]); st != C.CEL_OK {
		return nil, &StatusError{Status: int(st), Msg: "the shares of a namespace are not one contiguous run of the original data square"}
	}
	out := make([]ShareRange, nNamespaces)
	for i := range out {
		out[i] = ShareRange{Start: uint32(a[i]), End: uint32(b[i])}
	}
	return out, nil
}
