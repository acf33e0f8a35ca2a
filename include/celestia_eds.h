/*
 * celestia_eds.h — C ABI of the MI355X-native extended-data-square hot path.
 *
 * This library replaces, behind an unchanged Go surface, the hot path of
 * celestia-app's pkg/da (reference /root/reference):
 *
 *   da.ExtendShares                 pkg/da/data_availability_header.go:65-75
 *   da.NewDataAvailabilityHeader    pkg/da/data_availability_header.go:44-63
 *   DataAvailabilityHeader.Hash     pkg/da/data_availability_header.go:92-108
 *   rsmt2d.Codec (LeoRSCodec)       pkg/appconsts/global_consts.go:92 (DefaultCodec)
 *   rsmt2d.Tree via wrapper         pkg/wrapper/nmt_wrapper.go:14-17,83,93-124
 *   rsmt2d ExtendedDataSquare.Repair (rsmt2d v0.14.0 [dep]; used by celestia-node)
 *
 * Every entry point returns cel_status (0 = OK) and never aborts. Buffers are
 * borrowed for the duration of the call only (cgo forbids retaining Go pointers);
 * outputs go to caller-allocated memory. A cel_ctx binds one HIP device and one
 * stream; calls on one ctx are serialised internally, so a ctx may be shared by
 * goroutines; use one ctx per device for concurrency.
 *
 * Layouts (all row-major, share = 512 B = appconsts.ShareSize):
 *   ODS   k*k shares                         (the [][]byte of da.ExtendShares, flattened)
 *   EDS   2k*2k shares                       (rsmt2d flattened square: Q0 Q1 / Q2 Q3)
 *   roots 2k entries of 90 B                 (minNs(29) || maxNs(29) || sha256(32))
 *   dah   32 B                               (RFC-6962 root of rowRoots || colRoots)
 */
#ifndef CELESTIA_EDS_H
#define CELESTIA_EDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t cel_status;

/* Status codes; each maps 1:1 onto a Go error of the reference surface. */
#define CEL_OK 0
#define CEL_EINVAL 1         /* bad argument (nil pointer, zero size)                          */
#define CEL_ENOTPOW2 2       /* "number of shares is not a power of 2: got %d" (data_availability_header.go:68) */
#define CEL_ECHUNK 3         /* chunk size not a positive multiple of 64 (rsmt2d ValidateChunkSize) */
#define CEL_ETOOBIG 4        /* square / codeword wider than the device path supports: the Go shim
                                answers these calls with the reference path instead */
#define CEL_EORDER 5         /* nmt: leaves pushed out of namespace order (nmt_wrapper_test.go:106-111) */
#define CEL_ETOOFEW 6        /* decode: fewer than k of 2k shards present                      */
#define CEL_EBYZANTINE 7     /* rsmt2d ErrByzantineData: axis fails re-encoding or root check  */
#define CEL_EUNREPAIRABLE 8  /* rsmt2d ErrUnrepairableDataSquare                               */
#define CEL_EDEVICE 9        /* HIP runtime / kernel failure                                   */
#define CEL_ENOMEM 10        /* device allocation failed                                       */
#define CEL_ESHORT 11        /* "data is too short to contain namespace ID" (nmt_wrapper.go:98) */
#define CEL_EPUSHPAST 12     /* "pushed past predetermined square size" (nmt_wrapper.go:95)     */
#define CEL_EBADROOT 13      /* rsmt2d preRepairSanityCheck "bad root input": a complete axis does
                                not match its root (a plain error, not ErrByzantineData)       */
#define CEL_ENODATA 14       /* codec: zero-length shards (klauspost reedsolomon ErrShardNoData,
                                "no shard data", which LeoRSCodec.Encode / Decode pass through) */

/* Flags for the square entry points. */
#define CEL_FLAG_ORDER_CHECK 0x1u   /* enforce the honest nmt push order (default in the Go path) */
#define CEL_FLAG_PARITY_ONLY 0x2u   /* host entry points: eds_out receives the parity cells only
                                       (Q1, Q2, Q3); its Q0 cells are not written, the caller
                                       holds the ODS already (the Go shim points Q0's cells of the
                                       imported square at the input shares): 3/4 of the PCIe bytes */
#define CEL_FLAG_CALLER_STREAM 0x4u /* cel_dev_extend_batch: the whole batch as one chunk on the
                                       caller's stream, no internal streams (a caller keeping
                                       several batches in flight on its own streams). Such
                                       batches on one ctx are chained: each starts its extension
                                       after the previous CALLER_STREAM batch's extension on that
                                       ctx has finished (an event wait, whatever stream either
                                       ran on), so its extension runs beside the previous batch's
                                       hashing. Independent pipelines that must not be ordered
                                       use one ctx each. */

#define CEL_SHARE_SIZE 512u
#define CEL_NAMESPACE_SIZE 29u
#define CEL_NMT_NODE_SIZE 90u
#define CEL_HASH_SIZE 32u

typedef struct cel_ctx cel_ctx;

/* ---------------------------------------------------------------- context */
cel_status cel_ctx_create(int device, cel_ctx** out);
void cel_ctx_destroy(cel_ctx* ctx);
const char* cel_strerror(cel_status st);
/* Go-style message of the last failing call on ctx (e.g. the exact
 * "number of shares is not a power of 2: got 5" string). */
const char* cel_last_error(const cel_ctx* ctx);
/* Name of the device (for reports). */
cel_status cel_device_name(cel_ctx* ctx, char* buf, size_t len);

/* ------------------------------------------------------- square (host I/O) */
/* da.ExtendShares + da.NewDataAvailabilityHeader in one device pass.
 * shares: n_shares * share_size bytes (n_shares must be a power of two and a
 * perfect square, i.e. k*k; replaces data_availability_header.go:65-75,44-63).
 * eds_out may be NULL (PrepareProposal/ProcessProposal discard the EDS:
 * app/prepare_proposal.go:81-83). row_roots/col_roots: 2k*90 B each; dah: 32 B. */
cel_status cel_extend_shares(cel_ctx* ctx, const uint8_t* shares, uint32_t n_shares,
                             uint32_t share_size, uint8_t* eds_out, uint8_t* row_roots,
                             uint8_t* col_roots, uint8_t* dah, uint32_t flags);

/* Batch replay: n independent k*k squares laid out back to back (config 4).
 * eds_out (nullable): n * 4k^2 * share; roots: n * 2k * 90 each; dah: n * 32.
 * status_out (nullable): per-square status (CEL_EORDER for a bad square). */
cel_status cel_extend_batch(cel_ctx* ctx, const uint8_t* ods, uint32_t n, uint32_t k,
                            uint32_t share_size, uint8_t* eds_out, uint8_t* row_roots,
                            uint8_t* col_roots, uint8_t* dah, int32_t* status_out,
                            uint32_t flags);

/* Page-locked host memory for the buffers of the host entry points (the ODS, the EDS
 * output): with it every PCIe copy of cel_extend_batch is an asynchronous DMA that
 * overlaps the other chunks' kernels. Any host memory works; pageable memory is
 * staged by the runtime. cel_host_alloc returns NULL on failure. */
void* cel_host_alloc(size_t bytes);
void cel_host_free(void* p);

/* -------------------------------------------------- square (device resident)
 * Same as cel_extend_batch with every pointer in device memory of ctx's device.
 * stream: a hipStream_t (NULL = ctx's own stream). Asynchronous: returns after
 * enqueueing. d_status: n int32 (0 or CEL_EORDER). Required d_eds: n*4k^2*share
 * (the EDS is always materialised on the device). d_work: scratch of
 * cel_dev_workspace_size(k, n) bytes. */
size_t cel_dev_workspace_size(uint32_t k, uint32_t n);
cel_status cel_dev_extend_batch(cel_ctx* ctx, const void* d_ods, uint32_t n, uint32_t k,
                                void* d_eds, void* d_row_roots, void* d_col_roots, void* d_dah,
                                int32_t* d_status, void* d_work, void* stream, uint32_t flags);
/* Input layout of the device path: d_ods == NULL means every ODS already sits in
 * quadrant Q0 of its EDS buffer (row pitch 2k shares, the flattened rsmt2d square)
 * and is extended in place. cel_dev_place_ods puts n
 * row-major ODSs (host or device memory, as da.ExtendShares receives them flattened,
 * data_availability_header.go:65-75) there with strided copies on `stream`.
 * cel_extend_batch uses this path; a separate d_ods buffer makes the row pass also
 * copy Q0 into the EDS. */
cel_status cel_dev_place_ods(cel_ctx* ctx, const void* ods, uint32_t n, uint32_t k, void* d_eds,
                             void* stream);
/* Phase entry points of the same pipeline (for profiling and the row-sharded
 * multi-GPU mode): RS extension only, and NMT roots + DAH over a resident EDS. */
cel_status cel_dev_extend_only(cel_ctx* ctx, const void* d_ods, uint32_t n, uint32_t k,
                               void* d_eds, void* stream);
cel_status cel_dev_commit_only(cel_ctx* ctx, const void* d_eds, uint32_t n, uint32_t k,
                               void* d_row_roots, void* d_col_roots, void* d_dah,
                               int32_t* d_status, void* d_work, void* stream, uint32_t flags);

/* ------------------------------------------- row-sharded square (multi-GPU)
 * One square extended by nranks processes, one per GPU (config 3).
 * Replaces, for a square too large for one device's share of the work, the same
 * da.ExtendShares + NewDataAvailabilityHeader pair (data_availability_header.go:65-75,
 * :44-63). Rank r owns ODS rows [r*k/nranks, (r+1)*k/nranks) and, after the column
 * transpose, EDS columns [r*w, (r+1)*w) with w = 2k/nranks. The two collectives (one
 * all-to-all of cells, one all-gather of node records) belong to the caller (RCCL
 * through torch.distributed); these calls are the per-rank device steps.
 * Supported for k in {256, 512} (Leopard GF(2^16)), nranks a power of two <= k.
 * Node records are 96 bytes: the 90-byte NMT node and 6 zero bytes. In a row-subtree
 * record of a Q0 row, bytes 92..95 are a little-endian 1 when the slab's last leaf in that
 * row carries the parity namespace 0xFF*29 (IgnoreMaxNamespace keeps it out of the
 * subtree's maxNs, and step 3's push-order check across slab boundaries needs it). */
#define CEL_NODE_RECORD 96u
size_t cel_dev_shard_workspace_size(uint32_t k, uint32_t nranks);
/* Step 1: row-encode this rank's k/nranks ODS rows (d_ods_rows: [k/nranks][k][512])
 * straight into the all-to-all send buffer d_send: [nranks][k/nranks][w][512]
 * (block h = the cells of columns [h*w, (h+1)*w), Q0 and Q1 alike). */
cel_status cel_dev_shard_rows(cel_ctx* ctx, const void* d_ods_rows, uint32_t k, uint32_t nranks, void* d_send,
                              void* stream);
/* Step 2 (after the all-to-all into the top half of d_slab): d_slab is [2k][w][512]
 * with rows [0, k) received in rank order. Column-encodes the slab in place (rows
 * [k, 2k)), hashes its 2k*w leaves once, and writes the w column-root records
 * (d_col_rec: [w][96]) and the 2k row-subtree records over this slab's columns
 * (d_row_sub: [2k][96]). *d_status = 0 or CEL_EORDER (within-slab push order).
 * Step 3 all-gathers one record block per rank, [2k + w + 1][96]: the row subtrees,
 * then the column roots, then a record whose first 4 bytes are the status; pointing
 * d_row_sub, d_col_rec and d_status into that block makes it the send buffer. */
cel_status cel_dev_shard_cols(cel_ctx* ctx, void* d_slab, uint32_t k, uint32_t nranks, uint32_t rank,
                              void* d_col_rec, void* d_row_sub, int32_t* d_status, void* d_work, void* stream,
                              uint32_t flags);
/* Step 3 (after all-gathering every rank's record block, rank order):
 * d_gathered [nranks][2k + w + 1][96] -> d_row_roots, d_col_roots (2k x 90 B each) and
 * d_dah (32 B). *d_status = the max over ranks of the step-2 status, or CEL_EORDER if
 * the push order breaks across slab boundaries. */
cel_status cel_dev_shard_finish(cel_ctx* ctx, const void* d_gathered, uint32_t k, uint32_t nranks, void* d_row_roots,
                                void* d_col_roots, void* d_dah, int32_t* d_status, void* d_work, void* stream,
                                uint32_t flags);

/* --------------------------------------- multi-GPU inside the library (configs 3, 4)
 * One process, one host thread, several devices: ctxs[0..ngpu) as cel_ctx_create made them.
 * The collectives run inside the library over RCCL: one communicator rank per device
 * (ncclCommInitAll), every rank's sends / receives / all-gathers issued inside
 * ncclGroupStart / ncclGroupEnd. librccl.so.1 is loaded (dlopen) by the first plan over
 * distinct devices; the single-device entry points never need it. RCCL refuses two ranks on
 * one device, so a plan whose ctxs repeat a device moves the same blocks with device copies
 * instead (transport "copy": the same schedule, e.g. N ranks rehearsed on one GPU). Distinct
 * devices without RCCL (CEL_FLAG_SHARD_PEERCOPY, or RCCL not loadable / ncclCommInitAll
 * failing at plan creation) move them with hipMemcpyPeerAsync, peer access enabled (transport
 * "peer", "peer-fallback" when RCCL failed; cel_shard_plan_note keeps RCCL's message).
 *
 * cel_extend_sharded: da.ExtendShares + da.NewDataAvailabilityHeader
 * (data_availability_header.go:65-75, :44-63) for ONE square row-sharded over ngpu devices
 * (config 3): rank r row-encodes ODS rows [r k/N, (r+1) k/N) straight into
 * the all-to-all layout, grouped ncclSend / ncclRecv transpose the column blocks (k/N x 2k/N
 * cells per peer), each rank column-encodes and commits its [2k][2k/N] slab, one ncclAllGather
 * of 96-byte record blocks, rank 0 combines the row subtrees and hashes the DAH. Same
 * arguments and outputs as cel_extend_shares (ods: k*k*512 host bytes; eds_out nullable, with
 * CEL_FLAG_PARITY_ONLY its Q0 cells are not written). k = 256 or 512 (Leopard GF(2^16)), ngpu a
 * power of two <= k. The plan (buffers, streams, communicators) is kept in ctxs[0] for the
 * next call with the same device list, k and flags; ctxs[0]'s lock serialises such calls. */
cel_status cel_extend_sharded(cel_ctx* const* ctxs, uint32_t ngpu, const uint8_t* ods, uint32_t k,
                              uint32_t share_size, uint8_t* eds_out, uint8_t* row_roots, uint8_t* col_roots,
                              uint8_t* dah, uint32_t flags);
/* The same square as an explicit plan, for callers that keep ODSs resident or several squares
 * in flight (each plan has its own streams and communicators):
 *   create   per-rank buffers, streams, tables and the communicators (the expensive part);
 *   upload   ods (k*k*512 bytes, host or device memory) -> each rank's row block;
 *   run      one square, asynchronous on the ranks' streams;
 *   wait     sync, then (each nullable) the EDS (from every rank's column slab), the roots and
 *            the DAH (rank 0); returns the square's status (CEL_EORDER) or a device error.
 * flags: CEL_FLAG_ORDER_CHECK, CEL_FLAG_PARITY_ONLY (wait's eds_out), CEL_FLAG_SHARD_EXCHANGE,
 * CEL_FLAG_SHARD_PEERCOPY. */
typedef struct cel_shard_plan cel_shard_plan;
#define CEL_FLAG_SHARD_EXCHANGE 0x8u /* the exchange through RCCL wherever it is asked for: ngpu = 1
                                        gets a one-rank RCCL communicator, a separate send buffer, the
                                        all-to-all through it (self send / receive) and the record
                                        all-gather too, instead of the row pass writing the slab in
                                        place and no collective (tests the N > 1 exchange on one GPU);
                                        ctxs repeating a device try RCCL too (which refuses them) and
                                        fall back to device copies ("copy-fallback") */
#define CEL_FLAG_SHARD_PEERCOPY 0x10u /* never RCCL: distinct devices exchange with hipMemcpyPeerAsync
                                         (transport "peer"), repeated devices with device copies */
cel_status cel_shard_plan_create(cel_ctx* const* ctxs, uint32_t ngpu, uint32_t k, uint32_t flags,
                                 cel_shard_plan** out);
void cel_shard_plan_destroy(cel_shard_plan* plan);
const char* cel_shard_plan_transport(const cel_shard_plan* plan); /* "rccl", "copy" (ctxs repeat a
                                                                      device), "peer" (distinct
                                                                      devices, peer copies), "local"
                                                                      (one rank, no collective);
                                                                      "copy-fallback" /
                                                                      "peer-fallback" when RCCL
                                                                      could not start */
const char* cel_shard_plan_note(const cel_shard_plan* plan); /* why RCCL was not used ("" if it was,
                                                               or was not asked for) */
const char* cel_shard_plan_last_error(const cel_shard_plan* plan);
cel_status cel_shard_plan_upload(cel_shard_plan* plan, const uint8_t* ods);
cel_status cel_shard_plan_run(cel_shard_plan* plan);
cel_status cel_shard_plan_wait(cel_shard_plan* plan, uint8_t* eds_out, uint8_t* row_roots, uint8_t* col_roots,
                               uint8_t* dah);
/* The plan's all-to-all alone, `reps` times back to back after one warm-up exchange: the
 * slowest rank's microseconds per exchange (a report's figure next to SURVEY.md §8e's
 * one-link estimate; CEL_EINVAL for a one-rank plan in place, which has no exchange). */
cel_status cel_shard_plan_time_exchange(cel_shard_plan* plan, uint32_t reps, double* us_per_exchange);
/* Config 4 over several devices: cel_extend_batch's arguments, the n squares split into ngpu
 * contiguous ranges (sizes differ by at most one) each extended by cel_extend_batch on ctxs[i]
 * from its own host thread, so every device's PCIe copies and kernels run side by side
 * (page-locked buffers from cel_host_alloc keep the copies asynchronous). ctxs may repeat a
 * device. Returns the first failing range's status (its message in ctxs[0]). */
cel_status cel_extend_batch_multi(cel_ctx* const* ctxs, uint32_t ngpu, const uint8_t* ods, uint32_t n, uint32_t k,
                                  uint32_t share_size, uint8_t* eds_out, uint8_t* row_roots, uint8_t* col_roots,
                                  uint8_t* dah, int32_t* status_out, uint32_t flags);

/* ------------------------------------------------------- same-run probes
 * The ceilings a report prices the hot path against, measured on ctx's device in the same
 * process (bench.py's line): cel_probe_sha256 runs the NMT kernels' SHA-256 compression
 * chained in registers on every lane with no memory traffic (G compressions/s, best of 5
 * launches) and reports the sustained shader clock over that launch (MHz, nullable: shader
 * clock ticks per constant-rate tick of every wave); cel_probe_hbm_copy streams a copy over
 * `bytes` of HBM (half read, half written; one 16-byte element per lane) and reports read +
 * write GB/s (best of 5); cel_probe_hbm_stream adds the read-only and write-only rates over
 * the same half (each nullable: HBM writes stream slower than reads, which prices a
 * write-heavy kernel such as the extension, 3 bytes written per byte read);
 * cel_probe_rs_transform runs the encode tile (GF(2^8): k = 32, 64 or 128; GF(2^16): k = 256
 * or 512) with its HBM traffic taken away and reports the microseconds one square's
 * extension (3k axis encodes) spends in the transform alone, whole chip (best of 5). */
cel_status cel_probe_sha256(cel_ctx* ctx, double* g_compressions_per_s, double* shader_mhz);
cel_status cel_probe_hbm_copy(cel_ctx* ctx, uint64_t bytes, double* gbps);
cel_status cel_probe_hbm_stream(cel_ctx* ctx, uint64_t bytes, double* copy_gbps, double* read_gbps,
                                double* write_gbps);
cel_status cel_probe_rs_transform(cel_ctx* ctx, uint32_t k, double* us_per_square);

/* ------------------------------------------------------ rsmt2d.Codec surface
 * Leopard RS (klauspost/reedsolomon v1.12.1 New(n, n, WithLeopardGF(true))):
 * GF(2^8) when 2n <= 256, GF(2^16) otherwise. len must be a positive multiple
 * of 64. data: n*len contiguous -> parity: n*len. */
cel_status cel_codec_encode(cel_ctx* ctx, const uint8_t* data, uint32_t n, uint32_t len,
                            uint8_t* parity);
/* shards: 2n*len (n data then n parity), present: 2n flags (nil shard = 0).
 * Fills every missing shard in place (rsmt2d Codec.Decode). */
cel_status cel_codec_decode(cel_ctx* ctx, uint8_t* shards, const uint8_t* present, uint32_t n,
                            uint32_t len);
/* Device-resident batch of rsmt2d Codec.Decode calls (one per axis), as the repair's
 * crossword passes issue them: d_shards [naxes][2n][len] (data then parity, filled in
 * place), d_present [naxes][2n] (0 = missing; every axis needs >= n present). n <= 1024,
 * len a positive multiple of 64. Asynchronous on stream (NULL = ctx's stream). */
cel_status cel_dev_decode(cel_ctx* ctx, void* d_shards, const void* d_present, uint32_t naxes, uint32_t n,
                          uint32_t len, void* stream);
uint64_t cel_codec_max_chunks(void);             /* 32768 * 32768 */
const char* cel_codec_name(void);                /* "Leopard" */
cel_status cel_codec_validate_chunk_size(uint32_t len);

/* ---------------------------------------------------- rsmt2d.Tree surface
 * Root of one erasured NMT axis: the 2k cells of row/column `axis_index` of a
 * square of original width k (wrapper.Push x 2k then Root,
 * pkg/wrapper/nmt_wrapper.go:93-124). cells: 2k*share contiguous. */
cel_status cel_axis_root(cel_ctx* ctx, const uint8_t* cells, uint32_t k, uint32_t axis_index,
                         uint32_t share_size, uint8_t* root_out, uint32_t flags);
/* Plain NMT root over n namespaced leaves of leaf_len bytes (ns = first 29 B). */
cel_status cel_nmt_root(cel_ctx* ctx, const uint8_t* leaves, uint32_t n, uint32_t leaf_len,
                        uint8_t* root_out, uint32_t flags);
/* DataAvailabilityHeader.Hash: RFC-6962 root over rowRoots || colRoots (w each). */
cel_status cel_dah_hash(cel_ctx* ctx, const uint8_t* row_roots, const uint8_t* col_roots,
                        uint32_t w, uint8_t* out);
/* merkle.HashFromByteSlices (RFC-6962; tendermint crypto/merkle, the hash
 * DataAvailabilityHeader.Hash applies to rowRoots || colRoots,
 * data_availability_header.go:92-108) over n byte slices of any length: slice i is
 * data[offsets[i] .. offsets[i+1]) (offsets: n + 1 entries, non-decreasing). For DAHs
 * whose roots are not all 90-byte NMT roots (FromProto accepts any length). n = 0 gives
 * SHA-256 of the empty string. */
cel_status cel_merkle_hash_slices(cel_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint32_t n,
                                  uint8_t* out);

/* ------------------------------------------------------------------ repair
 * rsmt2d ExtendedDataSquare.Repair(rowRoots, colRoots) (rsmt2d v0.14.0
 * extendeddatacrossword.go [dep]; oracle/eds.c restates it): eds is 2k*2k*share with
 * present[2k*2k] marking known cells.
 *   CEL_OK            every cell filled, present[] all ones.
 *   CEL_EBADROOT      an axis complete before the repair does not match its root
 *                     (preRepairSanityCheck "bad root input", a plain error).
 *   CEL_EBYZANTINE    rsmt2d *ErrByzantineData{Axis, Index, Shares}: *bad_axis (0 = row,
 *                     1 = col), *bad_index, and (both nullable) byz_shares (2k*share) /
 *                     byz_present (2k) = that axis's shares as rsmt2d reports them
 *                     (absent cells zero with byz_present 0). Raised by a complete axis
 *                     whose parity differs from Encode(data) (sanity check), a decoded axis
 *                     failing its re-encoding or root check, or an orthogonal axis the
 *                     decode completed failing its root or encoding.
 *   CEL_EUNREPAIRABLE ErrUnrepairableDataSquare: no progress possible.
 * On CEL_EBYZANTINE / CEL_EBADROOT present[] is the mask before the failing solve (the
 * "most-repaired square prior to the byzantine axis"); on CEL_EUNREPAIRABLE the mask of
 * the most-repaired square. Cells outside present[] are undefined. Checks are reported
 * in rsmt2d's order: sanity row i then column i; then solveCrossword's sweeps, row i then
 * column i for i = 0..2k-1, each solve followed by the orthogonal axes it completes.
 * rsmt2d runs its sanity checks in goroutines, so which failing complete axis it reports
 * first is not fixed there. */
cel_status cel_repair(cel_ctx* ctx, uint8_t* eds, uint8_t* present, uint32_t k,
                      uint32_t share_size, const uint8_t* row_roots, const uint8_t* col_roots,
                      int32_t* bad_axis, int32_t* bad_index, uint8_t* byz_shares,
                      uint8_t* byz_present);
/* Same repair over an EDS resident on ctx's device (d_eds: 2k*2k*512 bytes, filled in
 * place); present, the roots and the byzantine outputs stay host memory (the crossword
 * control loop runs on the host over the presence mask). Synchronous. */
cel_status cel_dev_repair(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t k,
                          const uint8_t* row_roots, const uint8_t* col_roots, int32_t* bad_axis,
                          int32_t* bad_index, uint8_t* byz_shares, uint8_t* byz_present);
/* Tests only: from the next repair on ctx, an idle kernel of a pseudo-random 0..max_us
 * microseconds (seeded by seed) goes in front of every operation the repair enqueues on
 * either of its two streams, so the streams interleave differently; max_us = 0 turns it
 * off. Outcomes must not change: it checks that the schedule's cross-stream dependencies
 * are complete. */
cel_status cel_debug_schedule_fuzz(cel_ctx* ctx, uint64_t seed, uint32_t max_us);
/* Tests only, host-only (no device): the plan of the byzantine replay in rsmt2d's sweep
 * order for a presence mask (2k*2k): for each solve in sequence its axis (0 row, 1 col),
 * index and level (solves of one level run together on the device; a solve's level is
 * one more than that of every earlier solve that filled a cell it reads). The outputs
 * hold up to 4k entries (each axis is solved at most once); *solved = 1 if the sweeps
 * complete the square. */
cel_status cel_debug_repair_plan(const uint8_t* present, uint32_t k, int32_t* solve_axis, int32_t* solve_index,
                                 int32_t* solve_level, uint32_t* nsolves, int32_t* solved);

/* The repair of n squares of one k in one call (a node catching up over a range of heights):
 * d_eds is [n][2k][2k][512] on ctx's device, filled in place; present [n][2k*2k], the roots
 * [n][2k][90] and the outputs are host memory. For k = 32, 64, 128 and n > 1 the squares'
 * crossword passes are merged (every solvable row of every square in one decode launch, then
 * every solvable column, ...), one commit gives all roots and one copy brings the results
 * back; any other k, and n = 1, runs cel_dev_repair square after square. Per square i,
 * status[i], present[i], bad_axis[i], bad_index[i], byz_shares[i] ([2k][512]), byz_present[i]
 * ([2k]) and every cell present[i] vouches for are what cel_dev_repair gives for that square
 * alone; one square's failure changes nothing about another. status is required; bad_axis,
 * bad_index, byz_shares and byz_present are nullable.
 * Returns CEL_OK whenever every square ran to one of CEL_OK, CEL_EBYZANTINE, CEL_EBADROOT,
 * CEL_EUNREPAIRABLE (in status[]; cel_last_error then holds the first failing square's
 * message, prefixed "square i: "). CEL_EINVAL (a nil argument, k not a power of two or above
 * 512), CEL_ENOMEM and CEL_EDEVICE are the call's own; n = 0 is CEL_OK and touches nothing.
 * Synchronous. */
cel_status cel_dev_repair_batch(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t n, uint32_t k,
                                const uint8_t* row_roots, const uint8_t* col_roots, cel_status* status,
                                int32_t* bad_axis, int32_t* bad_index, uint8_t* byz_shares,
                                uint8_t* byz_present);
/* Device scratch (bytes) the ctx holds after cel_dev_repair_batch(k, n), beside the caller's
 * squares: masks, flags, roots, entry lists and the commit workspace of n squares, on top of
 * one square's repair buffers. It grows with n; 0 for a k the repair does not take or n = 0. */
size_t cel_dev_repair_batch_scratch_size(uint32_t k, uint32_t n);
/* The same over host squares eds [n][2k][2k][share_size], in and out (uploaded before,
 * downloaded after, through n squares of ctx scratch on top of the size above). */
cel_status cel_repair_batch(cel_ctx* ctx, uint8_t* eds, uint8_t* present, uint32_t n, uint32_t k,
                            uint32_t share_size, const uint8_t* row_roots, const uint8_t* col_roots,
                            cel_status* status, int32_t* bad_axis, int32_t* bad_index,
                            uint8_t* byz_shares, uint8_t* byz_present);
/* Tests only, host-only (no device): the merged pass schedule of n presence masks
 * ([n][2k*2k], k <= 256). Global pass p has direction pass_dir[p] (0 rows, 1 columns) and
 * the entries [pass_off[p], pass_off[p + 1]): entry e is axis ent_axis[e] of square
 * ent_square[e], squares in ascending order, a square's axes ascending. pass_dir holds up to
 * 8k passes, pass_off one more, the entries up to n * 4k (each axis is solved at most once). */
cel_status cel_debug_repair_batch_plan(const uint8_t* present, uint32_t n, uint32_t k, int32_t* pass_dir,
                                       uint32_t* pass_off, uint32_t* npasses, uint32_t* ent_square,
                                       int32_t* ent_axis);

/* ------------------------------------------------------- exported trees, proofs
 * pkg/proof (proof.go:78-202, row_proof.go, share_proof.go) and the subtree-root
 * cacher (pkg/inclusion/nmt_caching.go:96-124) need inner nodes, which the reference
 * gets by rebuilding row trees on the CPU. Here the device hashes the trees and
 * returns every node; proof building only selects nodes (host, no device).
 *
 * cel_axis_trees: all nodes of the NMTs of EDS axes [first, first + count) (axis 0 =
 * rows, row i = cells (i, 0..2k-1); 1 = columns), eds = 2k*2k*share host bytes.
 * nodes_out: count * (4k - 1) nodes of 90 B; per axis level-major from the 2k leaves
 * up to the root (leaf j at [j], level-1 node j at [2k + j], ..., root last). */
cel_status cel_axis_trees(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t share_size,
                          uint32_t axis, uint32_t first, uint32_t count, uint8_t* nodes_out);
/* cel_axis_tree: all 4k - 1 nodes of the NMT of one axis from its 2k cells (contiguous
 * shares, the wrapper's pushed data), axis_index deciding the Q0 namespace rule as in
 * nmt_wrapper.go:100-107; same layout as one axis of cel_axis_trees. For
 * ErasuredNamespacedMerkleTree.ProveRange (nmt_wrapper.go:127-130) on a full axis. */
cel_status cel_axis_tree(cel_ctx* ctx, const uint8_t* cells, uint32_t k, uint32_t axis_index,
                         uint32_t share_size, uint8_t* nodes_out);
/* RFC-6962 tree over rowRoots || colRoots (w each, 2w a power of two), every level:
 * nodes_out (4w - 1) * 32 B, level 0 = the 2w leaf hashes, ..., the root last (equal to
 * cel_dah_hash). */
cel_status cel_dah_tree(cel_ctx* ctx, const uint8_t* row_roots, const uint8_t* col_roots,
                        uint32_t w, uint8_t* nodes_out);
/* nmt ProveRange(start, end) on one tree of cel_axis_trees (nleaves = 2k): the proof
 * nodes (90 B each, nmt order: maximal subtrees outside [start, end), left to right)
 * to nodes_out (nullable: count only) and their count to *nnodes. */
cel_status cel_nmt_prove_range(const uint8_t* tree_nodes, uint32_t nleaves, uint32_t start,
                               uint32_t end, uint8_t* nodes_out, uint32_t* nnodes);
/* merkle.ProofsFromByteSlices Aunts of item `index` (n items, a power of two) from a
 * cel_dah_tree table: leaf sibling first, 32 B each, count to *naunts. */
cel_status cel_merkle_aunts(const uint8_t* tree, uint32_t n, uint32_t index, uint8_t* aunts_out,
                            uint32_t* naunts);

/* ------------------------------------------------- proof verification, samples
 * nmt Proof.VerifyInclusion (nmt v0.22.0 proof.go [dep]) for n proofs in one device batch:
 * the NMT range proofs of ShareProofs (pkg/proof/share_proof.go:60-82) and of sampled
 * cells. Proof i: range [starts[i], ends[i]), namespace namespaces[29*i..], its leaves =
 * the 512-byte shares leaf_off[i]..leaf_off[i+1] of `leaves` (without namespace prefix:
 * the namespace hashed in front of a leaf is the proof's, whatever the share starts
 * with), its nodes = the 90-byte nodes node_off[i]..node_off[i+1] of `nodes` (nmt order),
 * its root = roots[90*root_idx[i]..]. ok_out[i] = 1 iff it verifies. The proofs are
 * untrusted: start < 0, end <= start, a leaf count other than end - start, a missing
 * node, unordered children are verdict 0, never an error of the call.
 * CEL_EINVAL: nil argument, decreasing offsets, root_idx[i] >= nroots. n = 0 is CEL_OK. */
cel_status cel_nmt_verify_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts, const int32_t* ends,
                                const uint8_t* namespaces, const uint8_t* leaves, const uint64_t* leaf_off,
                                const uint8_t* nodes, const uint64_t* node_off, const uint8_t* roots,
                                uint32_t nroots, const uint32_t* root_idx, uint8_t* ok_out);
/* Same with leaves (16-byte aligned), nodes, roots and ok (n bytes) in device memory; the
 * small per-proof arrays stay host. d_work: cel_dev_nmt_verify_workspace_size bytes for
 * the batch's leaves (leaf_off[n] - leaf_off[0]), nodes and proofs. Asynchronous on stream
 * (NULL = the ctx's own), in the style of cel_dev_create_commitments: the host arrays are
 * consumed before the call returns. */
size_t cel_dev_nmt_verify_workspace_size(uint64_t total_leaves, uint64_t total_nodes, uint32_t n);
cel_status cel_dev_nmt_verify_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts, const int32_t* ends,
                                    const uint8_t* namespaces, const void* d_leaves, const uint64_t* leaf_off,
                                    const void* d_nodes, const uint64_t* node_off, const void* d_roots,
                                    uint32_t nroots, const uint32_t* root_idx, void* d_ok, void* d_work,
                                    void* stream);
/* Samples into a device EDS (d_eds: 2k*2k*512 bytes; present: host, 2k*2k). Sample i is
 * cell (rows[i], cols[i]) with share shares[512*i..] and a single-leaf nmt proof (nodes
 * node_off[i]..node_off[i+1]) against row_roots[rows[i]] at leaf cols[i] (axes[i] = 0) or
 * col_roots[cols[i]] at leaf rows[i] (axes[i] = 1). The namespace follows the wrapper's
 * rule (nmt_wrapper.go:100-107): share[0:29] for row < k and col < k, else 0xFF*29.
 * ok_out[i] = the verdict. A coordinate >= 2k, or an axis > 1, is verdict 0. An accepted
 * sample whose cell is not yet present is written into d_eds and present[] set. A cell
 * already present is left as it is. Of several accepted samples for one absent cell, the
 * lowest index is written. Nothing of a rejected sample is written. Synchronous. */
cel_status cel_dev_place_samples(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t k,
                                 const uint8_t* row_roots, const uint8_t* col_roots, uint32_t n,
                                 const uint32_t* rows, const uint32_t* cols, const uint8_t* axes,
                                 const uint8_t* shares, const uint8_t* nodes, const uint64_t* node_off,
                                 uint8_t* ok_out);
/* The samples placed into a zeroed device square as above, then the repair of
 * cel_dev_repair. eds_out: 2k*2k*512. present_out: 2k*2k. The status and the byzantine
 * outputs are those of cel_repair. */
cel_status cel_repair_samples(cel_ctx* ctx, uint32_t k, const uint8_t* row_roots, const uint8_t* col_roots,
                              uint32_t n, const uint32_t* rows, const uint32_t* cols, const uint8_t* axes,
                              const uint8_t* shares, const uint8_t* nodes, const uint64_t* node_off,
                              uint8_t* ok_out, uint8_t* eds_out, uint8_t* present_out, int32_t* bad_axis,
                              int32_t* bad_index, uint8_t* byz_shares, uint8_t* byz_present);

/* ------------------------------------------------- bad-encoding fraud proofs
 * What a node does with CEL_EBYZANTINE (specs/src/specs/fraud_proofs.md:3-13, networking.md
 * "Invalid Erasure Coding", types.proto BadEncodingFraudProof; celestia-node share/eds/byzantine):
 * it builds a proof that axis (axis, index) of the square is badly encoded (axis 0 = row, 1 =
 * column), and a peer checks such a proof against the square's 2k row roots and 2k column
 * roots. A proof carries entries: a position in the accused axis, the 512-byte share there, a
 * single-leaf nmt proof of it and an entry_axis that says which tree the proof is in, in the
 * convention of cel_dev_place_samples. The cell is (index, position) of an accused row,
 * (position, index) of an accused column; entry_axis 0 proves it at leaf col of row_roots[row],
 * entry_axis 1 at leaf row of col_roots[col], the namespace by the wrapper's rule
 * (nmt_wrapper.go:100-107). The reference specification's form (shares proved in the accused
 * root) and celestia-node's (in the orthogonal roots) are both entries of this kind.
 *
 * The verdict of one proof, one byte, the rule applied in this order (celestia-node's
 * BadEncodingProof.Validate):
 *   CEL_BEFP_MALFORMED  axis > 1, index >= 2k, an entry's position >= 2k or entry_axis > 1, or
 *                       two entries with one position.
 *   CEL_BEFP_TOO_FEW    fewer than k entries.
 *   CEL_BEFP_BAD_SHARE  an entry's nmt proof does not verify (a wrong node count is such an
 *                       entry, not an error of the call).
 *   otherwise the axis is rebuilt: the entries at their positions, every other shard absent,
 *   Codec.Decode, the parity half replaced by Codec.Encode(data half), and the root taken as
 *   the wrapper tree of axis `index` (no push-order check, as the repair's root check).
 *   CEL_BEFP_FRAUD      that root differs from the accused root (row_roots[index] or
 *                       col_roots[index]).
 *   CEL_BEFP_NOT_FRAUD  it is the accused root.
 * The rule cannot prove fraud where the accused root is honest and the corrupt cell is one its
 * orthogonal root does not commit to: no entry for that cell verifies, and the others rebuild
 * the honest axis. */
#define CEL_BEFP_NOT_FRAUD 0
#define CEL_BEFP_FRAUD 1
#define CEL_BEFP_BAD_SHARE 2
#define CEL_BEFP_TOO_FEW 3
#define CEL_BEFP_MALFORMED 4
/* n proofs for squares of one k, everything in host memory (proofs arrive from peers). Proof i
 * accuses (axes[i], index[i]) and holds the entries ent_off[i]..ent_off[i+1]; entry e is
 * positions[e], ent_axes[e], the share shares[512*e..] and the 90-byte nodes
 * node_off[e]..node_off[e+1] of `nodes` in nmt order (the layout cel_nmt_verify_batch reads;
 * node_off has ent_off[n] + 1 values). row_roots / col_roots: [n][2k][90], proof i's square.
 * verdict_out[n]; rebuilt_roots_out [n][90] (nullable): the rebuilt axis's root where the
 * verdict is CEL_BEFP_FRAUD or CEL_BEFP_NOT_FRAUD, zeros elsewhere. One proof's verdict never
 * depends on another's, and nothing in a proof makes the call fail. MALFORMED and TOO_FEW are
 * decided on the host and take no device work; the rest is one upload, one chain of kernels
 * on the ctx's stream (entries verified, placed into dense axes, decoded, re-encoded, hashed,
 * compared) and one download. Synchronous.
 * CEL_EINVAL: a nil argument, decreasing offsets, k not a power of two or above 512, or more
 * than 2^31 entries or nodes; CEL_ENOMEM; CEL_EDEVICE. n = 0 is CEL_OK. */
cel_status cel_befp_verify_batch(cel_ctx* ctx, uint32_t n, uint32_t k, const uint8_t* axes,
                                 const uint32_t* index, const uint64_t* ent_off,
                                 const uint32_t* positions, const uint8_t* ent_axes,
                                 const uint8_t* shares, const uint8_t* nodes, const uint64_t* node_off,
                                 const uint8_t* row_roots, const uint8_t* col_roots,
                                 uint8_t* verdict_out, uint8_t* rebuilt_roots_out);
/* The producer, over the square a cel_dev_repair left resident (d_eds: 2k*2k*512 bytes, 16-byte
 * aligned; present: host, 2k*2k, the mask the repair returned) and the axis it reported
 * (bad_axis, bad_index). Position j of that axis becomes an entry when its cell is known, the
 * orthogonal axis j (column j of a row, row j of a column) is complete in present, and that
 * axis's root, recomputed on the device, equals its root in the header: a cell corrupted after
 * the roots were made gives no entry that would fail. Entry e, positions ascending:
 * positions_out[e], ent_axes_out[e] (the orthogonal direction), shares_out[512*e..] and its
 * log2(2k) nodes at nodes_out[90*log2(2k)*e..], the bytes cel_nmt_prove_range gives on that
 * tree. The outputs hold 2k entries; *count_out is how many there are. Fewer than k is
 * CEL_OK with the count (an outcome: the caller adds sample proofs it holds). Synchronous.
 * CEL_EINVAL: a nil argument, k not a power of two or above 512, bad_axis > 1, bad_index >= 2k. */
cel_status cel_dev_befp_build(cel_ctx* ctx, const void* d_eds, const uint8_t* present, uint32_t k,
                              const uint8_t* row_roots, const uint8_t* col_roots, uint32_t bad_axis,
                              uint32_t bad_index, uint32_t* positions_out, uint8_t* ent_axes_out,
                              uint8_t* shares_out, uint8_t* nodes_out, uint32_t* count_out);
/* The same over a square in host memory (eds: 2k*2k*512, as cel_repair leaves it). */
cel_status cel_befp_build(cel_ctx* ctx, const uint8_t* eds, const uint8_t* present, uint32_t k,
                          const uint8_t* row_roots, const uint8_t* col_roots, uint32_t bad_axis,
                          uint32_t bad_index, uint32_t* positions_out, uint8_t* ent_axes_out,
                          uint8_t* shares_out, uint8_t* nodes_out, uint32_t* count_out);

/* ------------------------------------------------- proofs in batches, tree index
 * nmt ProveRange (nmt v0.22.0 [dep], as pkg/proof/proof.go:190 calls it per row) for many
 * requests over one resident square: the range proofs of ShareProofs and of sampled cells, in
 * the layout the verifier above reads, so a producer and a verifier chain with no repacking.
 *
 * cel_dev_tree_index_build: every node of the 4k row and column NMTs of the square at d_eds
 * (2k*2k*512 bytes, any cells, codeword or not, 16-byte aligned) into d_index
 * (cel_dev_tree_index_size(k) bytes, 16-byte aligned): 96-byte records, the 2k*2k leaf
 * records [row][col] once (a cell's leaf is the same in its row tree and its column tree),
 * then level l = 1 .. log2(2k) as [4k trees][2k >> l], the 2k row trees first, then the
 * columns; a tail of 64*2k + 48 bytes belongs to the build. d_row_roots / d_col_roots
 * (2k*90 bytes each), d_dah (32 bytes, nullable) and CEL_FLAG_ORDER_CHECK as in
 * cel_dev_commit_only for one square. status (nullable): host memory, 0 or CEL_EORDER,
 * copied back on the stream: valid once the stream is synchronised (page-locked memory
 * keeps the call asynchronous). k: a power of two up to 512, rejected otherwise as the other
 * device entry points reject it; k = 1 is valid (leaves and roots).
 * cel_dev_tree_index_size is 0 for a k that is not a power of two or is above 2048. */
size_t cel_dev_tree_index_size(uint32_t k);
cel_status cel_dev_tree_index_build(cel_ctx* ctx, const void* d_eds, uint32_t k, void* d_index,
                                    void* d_row_roots, void* d_col_roots, void* d_dah,
                                    int32_t* status, uint32_t flags, void* stream);
/* Host only: where each proof's output goes. leaf_off[i] / node_off[i] (n + 1 entries each) are
 * the prefix sums of ends[i] - starts[i] and of the node count of ProveRange(starts[i],
 * ends[i]) over 2k leaves. The ranges are the caller's own, so a bad one (start < 0, end <=
 * start, end > 2k) is CEL_EINVAL, with the proof named in cel_prove_last_error (this
 * thread's last cel_prove_offsets failure). */
cel_status cel_prove_offsets(uint32_t k, uint32_t n, const int32_t* starts, const int32_t* ends,
                             uint64_t* leaf_off, uint64_t* node_off);
const char* cel_prove_last_error(void);
/* Proof i = ProveRange(starts[i], ends[i]) on row index[i] (axes[i] = 0) or column index[i]
 * (axes[i] = 1) of the square whose index is d_index. Its nodes go to d_nodes + 90 *
 * node_off[i], packed and in nmt order (the bytes cel_nmt_prove_range gives for that tree);
 * its shares to d_leaves + 512 * leaf_off[i] (d_leaves nullable: nodes only, and d_eds is
 * then not read), offsets as cel_prove_offsets gives them. d_leaves, d_eds, d_index and d_work
 * 16-byte aligned, d_nodes 2-byte aligned; d_work: cel_dev_prove_workspace_size(n) bytes.
 * The host arrays are consumed before the call returns; asynchronous on stream (NULL = the
 * ctx's own). CEL_EINVAL: nil argument, misalignment, axes[i] > 1, index[i] >= 2k, a bad
 * range. n = 0 is CEL_OK. */
size_t cel_dev_prove_workspace_size(uint32_t n);
cel_status cel_dev_prove_batch(cel_ctx* ctx, const void* d_eds, const void* d_index, uint32_t k,
                               uint32_t n, const uint8_t* axes, const uint32_t* index,
                               const int32_t* starts, const int32_t* ends, void* d_leaves,
                               void* d_nodes, void* d_work, void* stream);
/* The same for a square in host memory (eds: 2k*2k*512): upload, index, proofs, download.
 * Synchronous. cel_prove_samples: sample i is cell (rows[i], cols[i]), proved at leaf cols[i]
 * of row rows[i] (axes[i] = 0) or at leaf rows[i] of column cols[i] (axes[i] = 1), the
 * convention of cel_dev_place_samples, whose shares / nodes / node_off arguments these
 * outputs are (shares_out: n*512; nodes_out: n * log2(2k) nodes; node_off_out: n + 1). A
 * coordinate >= 2k is CEL_EINVAL. cel_prove_ranges: the arguments of cel_dev_prove_batch,
 * outputs sized by cel_prove_offsets (leaves_out nullable). */
cel_status cel_prove_samples(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n,
                             const uint32_t* rows, const uint32_t* cols, const uint8_t* axes,
                             uint8_t* shares_out, uint8_t* nodes_out, uint64_t* node_off_out);
cel_status cel_prove_ranges(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n,
                            const uint8_t* axes, const uint32_t* index, const int32_t* starts,
                            const int32_t* ends, uint8_t* leaves_out, uint8_t* nodes_out);

/* ------------------------------------------------- namespace queries
 * nmt ProveNamespace / Proof.VerifyNamespace (nmt v0.22.0 [dep]) in batches: "every share of
 * namespace N in this square, with a proof that none was left out", what celestia-node's
 * GetSharesByNamespace asks of every row whose root range holds N.
 *
 * The producer works on the row trees of the square whose index is d_index. For namespace nid
 * and a row of 2k leaves, with lt / le the number of leaves whose namespace is < nid / <= nid:
 * the row yields an entry iff root.min <= nid <= root.max and lt < 2k. le > lt: an inclusion
 * entry (CEL_NS_INCLUSION), range [lt, le), the nodes of ProveRange(lt, le), the le - lt shares.
 * Otherwise an absence entry (CEL_NS_ABSENCE): range [lt, lt + 1), the nodes of ProveRange(lt,
 * lt + 1) followed by one more 90-byte node, the leaf record of leaf lt (nmt's leafHash), and
 * no shares. nmt's empty proof for the other rows is not emitted.
 *
 * cel_dev_namespace_plan: the entries of n namespaces (host, 29 bytes each, duplicates allowed)
 * over the 2k rows, in (namespace index, row) order, into the host arrays (cap entries each;
 * leaf_off / node_off: cap + 1, the prefix sums of the entries' shares and nodes) and *n_entries.
 * Synchronous on stream: the count depends on the data. cap = 0 with every array NULL: count
 * only. cap below the count: CEL_EINVAL, both numbers in cel_last_error, *n_entries set, nothing
 * else written; n * 2k always suffices. The plan stays in d_work
 * (cel_dev_namespace_workspace_size(k, n) bytes, 16-byte aligned) for cel_dev_namespace_prove.
 * CEL_EINVAL: nil argument, misalignment, a k that is not a power of two up to 512, the parity
 * namespace (0xFF * 29, not a data namespace), n * 2k >= 2^32. n = 0 is CEL_OK.
 * cel_dev_namespace_prove: the first n_entries entries of the plan in d_work: entry e's nodes to
 * d_nodes + 90 * node_off[e] (2-byte aligned; an absence entry's leaf hash last), its shares to
 * d_leaves + 512 * leaf_off[e] (16-byte aligned; nullable: nodes only). Asynchronous on stream.
 * A batch of inclusion entries is byte for byte what cel_dev_prove_batch gives for the same
 * ranges, so it feeds cel_dev_nmt_verify_batch as well as the namespace verifier below.
 * cel_namespace_rows: the same for a square in host memory (eds: 2k*2k*512): upload, index
 * with the order check (an unordered square: CEL_EORDER), plan, proofs, download. Synchronous.
 * The totals always come back; the arrays are written when cap, leaf_cap (shares) and
 * node_cap (nodes) suffice, else CEL_EINVAL; all three 0 and every array NULL: count only. */
#define CEL_NS_INCLUSION 0
#define CEL_NS_ABSENCE 1
size_t cel_dev_namespace_workspace_size(uint32_t k, uint32_t n);
cel_status cel_dev_namespace_plan(cel_ctx* ctx, const void* d_index, uint32_t k, uint32_t n,
                                  const uint8_t* namespaces, uint64_t cap, uint32_t* ns_idx,
                                  uint32_t* rows, int32_t* starts, int32_t* ends, uint8_t* kinds,
                                  uint64_t* leaf_off, uint64_t* node_off, uint64_t* n_entries,
                                  void* d_work, void* stream);
cel_status cel_dev_namespace_prove(cel_ctx* ctx, const void* d_eds, const void* d_index, uint32_t k,
                                   uint64_t n_entries, void* d_leaves, void* d_nodes, void* d_work,
                                   void* stream);
cel_status cel_namespace_rows(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n,
                              const uint8_t* namespaces, uint64_t cap, uint64_t leaf_cap,
                              uint64_t node_cap, uint32_t* ns_idx, uint32_t* rows, int32_t* starts,
                              int32_t* ends, uint8_t* kinds, uint64_t* leaf_off, uint64_t* node_off,
                              uint8_t* leaves_out, uint8_t* nodes_out, uint64_t* n_entries,
                              uint64_t* total_leaves, uint64_t* total_nodes);
/* ------------------------------------------------- many resident squares at once
 * The index, the proofs and the namespace queries above over n squares of one width k that lie
 * back to back at d_eds (n * 2k*2k*512 bytes), as cel_dev_extend_batch, cel_dev_repair_batch and
 * a width group of cel_block_extend_batch leave them: one launch per step for all squares, one
 * request table, one plan.
 *
 * The batch index is n single-square indexes back to back: square i's starts at d_index + i *
 * cel_dev_tree_index_size(k) (a multiple of 16) and is byte for byte what
 * cel_dev_tree_index_build gives for square i, so every single-square call (cel_dev_prove_batch,
 * cel_dev_namespace_plan, cel_dev_blobs_*, cel_dev_txs_*) works on (d_eds + i * 2k*2k*512, d_index
 * + i * size). cel_dev_tree_index_batch_size is n times cel_dev_tree_index_size(k): 0 where that
 * is 0 (a k that is not a power of two or is above 2048), for n = 0, for n above 65535 and on
 * overflow. As with the single pair, the size is given for more widths than the build takes: the
 * calls below take k up to 512, the device path's limit.
 * One call takes at most 65535 squares (a launch's grid holds the square in 16 bits): more is
 * CEL_EINVAL in every call of this section, not split.
 *
 * cel_dev_tree_index_build_batch: per square exactly cel_dev_tree_index_build. d_row_roots /
 * d_col_roots: [n][2k][90] each, d_dah: n*32 (nullable: each DAH goes to its slice's tail),
 * status: host, n values (nullable), 0 or CEL_EORDER per square under CEL_FLAG_ORDER_CHECK; a
 * square that fails the check does not touch the others. Asynchronous; status is copied back on
 * the stream, in one copy, through one device array that the ctx keeps: a build that asks for
 * status waits on the device for the status copy of the ctx's previous such build, so two of
 * them on different streams of one ctx do not overlap, and the first build that needs a larger
 * array waits for that copy on the host. A build with status = NULL has no such order. CEL_EINVAL: nil argument, misalignment, a bad k, too many squares. n = 0: CEL_OK.
 *
 * cel_dev_prove_squares: proof i = ProveRange(starts[i], ends[i]) on row or column index[i] of
 * square squares[i] < n_squares. Outputs at cel_prove_offsets' prefix sums (they depend on the
 * ranges only), so a batch whose requests all name square s is byte for byte cel_dev_prove_batch
 * on slice s. Alignment, nullable d_leaves and CEL_EINVAL as there, and squares[i] >= n_squares
 * (the request is named, nothing is enqueued). d_work: cel_dev_prove_squares_workspace_size(n).
 *
 * cel_dev_namespace_plan_squares / cel_dev_namespace_prove_squares: query i is the pair
 * (squares[i], namespaces + 29*i); the entries come in (query, row) order and query_idx[e] names
 * entry e's query. Everything else as cel_dev_namespace_plan / cel_dev_namespace_prove: count
 * only with cap = 0, a cap below the count, the parity namespace, n * 2k < 2^32, the plan kept in
 * d_work (cel_dev_namespace_squares_workspace_size(k, n) bytes) for the prove call, which takes
 * the n_squares the plan was made for. A plan of one sort is nothing to the prove call of the
 * other sort. CEL_EINVAL also for squares[i] >= n_squares. n = 0 or n_squares = 0 with nothing
 * to do is CEL_OK.
 *
 * cel_prove_samples_squares / cel_namespace_rows_squares: the squares in host memory (eds:
 * n_squares * 2k*2k*512): upload, batch index, proofs, download; synchronous; cel_prove_samples'
 * and cel_namespace_rows' arguments with n_squares and squares[]. An unordered square is
 * CEL_EORDER for the namespace rows, with the square named. */
size_t cel_dev_tree_index_batch_size(uint32_t k, uint32_t n);
cel_status cel_dev_tree_index_build_batch(cel_ctx* ctx, const void* d_eds, uint32_t n, uint32_t k,
                                          void* d_index, void* d_row_roots, void* d_col_roots,
                                          void* d_dah, int32_t* status, uint32_t flags, void* stream);
size_t cel_dev_prove_squares_workspace_size(uint32_t n);
cel_status cel_dev_prove_squares(cel_ctx* ctx, const void* d_eds, const void* d_index, uint32_t k,
                                 uint32_t n_squares, uint32_t n, const uint32_t* squares,
                                 const uint8_t* axes, const uint32_t* index, const int32_t* starts,
                                 const int32_t* ends, void* d_leaves, void* d_nodes, void* d_work,
                                 void* stream);
size_t cel_dev_namespace_squares_workspace_size(uint32_t k, uint32_t n);
cel_status cel_dev_namespace_plan_squares(cel_ctx* ctx, const void* d_index, uint32_t k,
                                          uint32_t n_squares, uint32_t n, const uint32_t* squares,
                                          const uint8_t* namespaces, uint64_t cap, uint32_t* query_idx,
                                          uint32_t* rows, int32_t* starts, int32_t* ends,
                                          uint8_t* kinds, uint64_t* leaf_off, uint64_t* node_off,
                                          uint64_t* n_entries, void* d_work, void* stream);
cel_status cel_dev_namespace_prove_squares(cel_ctx* ctx, const void* d_eds, const void* d_index,
                                           uint32_t k, uint32_t n_squares, uint64_t n_entries,
                                           void* d_leaves, void* d_nodes, void* d_work, void* stream);
cel_status cel_prove_samples_squares(cel_ctx* ctx, const uint8_t* eds, uint32_t n_squares, uint32_t k,
                                     uint32_t n, const uint32_t* squares, const uint32_t* rows,
                                     const uint32_t* cols, const uint8_t* axes, uint8_t* shares_out,
                                     uint8_t* nodes_out, uint64_t* node_off_out);
cel_status cel_namespace_rows_squares(cel_ctx* ctx, const uint8_t* eds, uint32_t n_squares, uint32_t k,
                                      uint32_t n, const uint32_t* squares, const uint8_t* namespaces,
                                      uint64_t cap, uint64_t leaf_cap, uint64_t node_cap,
                                      uint32_t* query_idx, uint32_t* rows, int32_t* starts,
                                      int32_t* ends, uint8_t* kinds, uint64_t* leaf_off,
                                      uint64_t* node_off, uint8_t* leaves_out, uint8_t* nodes_out,
                                      uint64_t* n_entries, uint64_t* total_leaves,
                                      uint64_t* total_nodes);

/* nmt Proof.VerifyNamespace for n proofs: the arguments of cel_nmt_verify_batch and kinds[i]
 * (CEL_NS_INCLUSION / CEL_NS_ABSENCE; above 1: verdict 0). The leaves are whole 512-byte shares.
 * Inclusion: as cel_nmt_verify_batch, and every share starts with the namespace. Absence:
 * end = start + 1, no leaves, at least popcount(start) + 1 nodes, the last of them the leaf
 * hash, with min <= max and namespace < min, folded as the single leaf. Either kind: every
 * proof node left of the range ends below the namespace and every node right of it begins
 * above (completeness). The empty proof (inclusion, start = end, no nodes, no leaves) verifies
 * iff the namespace lies outside the root's range; any other proof with start = end does not.
 * Malformed proofs are verdict 0, never an error of the call; CEL_EINVAL as in
 * cel_nmt_verify_batch. The device form is asynchronous, its workspace
 * cel_dev_nmt_verify_namespace_workspace_size bytes. */
cel_status cel_nmt_verify_namespace_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts,
                                          const int32_t* ends, const uint8_t* kinds,
                                          const uint8_t* namespaces, const uint8_t* leaves,
                                          const uint64_t* leaf_off, const uint8_t* nodes,
                                          const uint64_t* node_off, const uint8_t* roots,
                                          uint32_t nroots, const uint32_t* root_idx, uint8_t* ok_out);
size_t cel_dev_nmt_verify_namespace_workspace_size(uint64_t total_leaves, uint64_t total_nodes,
                                                   uint32_t n);
cel_status cel_dev_nmt_verify_namespace_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts,
                                              const int32_t* ends, const uint8_t* kinds,
                                              const uint8_t* namespaces, const void* d_leaves,
                                              const uint64_t* leaf_off, const void* d_nodes,
                                              const uint64_t* node_off, const void* d_roots,
                                              uint32_t nroots, const uint32_t* root_idx, void* d_ok,
                                              void* d_work, void* stream);

/* ------------------------------------------------- blobs by range
 * go-square v1.1.0 parseSparseShares over runs of ODS shares of a resident square, and the
 * blobs' share commitments: what celestia-node's blob service (GetAll, Get, Included) builds
 * from the shares of a namespace. A range is [start, end) in row-major ODS index (share s is
 * cell (s / k, s % k) of Q0); ranges may overlap or repeat. The shares of a range in order: a
 * share version other than 0 fails the range (CEL_BLOB_EVERSION); tail padding, primary
 * reserved padding and namespace padding (a sequence start of length 0) are skipped; any other
 * sequence start opens a blob (namespace bytes 0 .. 28, length bytes 30 .. 33 big-endian,
 * payload bytes 34 .. 511); a continuation appends its bytes 30 .. 511 to the blob opened last
 * in the range, whatever its own namespace, and fails the range with none open
 * (CEL_BLOB_ENOSTART). A blob closes at the next start or the range's end; fewer bytes than
 * its length fail the range (CEL_BLOB_ESHORT), more are trimmed. A failed range has its first
 * error as status and yields no blobs; the other ranges are unaffected.
 *
 * cel_dev_blobs_plan: the blobs of n_ranges ranges (host arrays starts, ends) of the square at
 * d_eds (2k*2k*512, 16-byte aligned; only Q0 is read), in (range, position) order, into recs
 * (cap records) and range_status (n_ranges words, nullable); *n_blobs and *total_bytes, the
 * size of the data buffer: blob b's bytes go to data_off, a multiple of 16, and take len rounded
 * up to 16. recs[].shares is the number of shares the blob was found with. Synchronous on
 * stream: the count depends on the data. cap = 0 with recs NULL: count only. cap below the
 * count: CEL_EINVAL, both numbers in cel_last_error, the counts and range_status set. The plan
 * stays in d_work (cel_dev_blobs_workspace_size(total shares of the ranges, n_ranges) bytes,
 * 16-byte aligned) for cel_dev_blobs_emit, which must be the next blob call on this ctx with
 * that workspace. CEL_EINVAL: nil argument, misalignment, a k that is not a power of two up to
 * 512, start > end, end > k*k, 2^31 shares or more in all. n_ranges = 0 is CEL_OK.
 * cel_dev_blobs_emit: the bytes of the first n_blobs blobs of the plan in d_work (no more than
 * it holds) into d_data (16-byte aligned, total_bytes bytes; the bytes between a blob's end and
 * the next multiple of 16 are zero) and, with d_commitments not NULL, their share commitments
 * (32 bytes each, inclusion.CreateCommitment) from there: d_commit_work is
 * cel_dev_commitments_workspace_size(sum of recs[].shares, n_blobs) bytes. Asynchronous on
 * stream.
 * cel_blobs_by_range: the same for a square in host memory: upload, plan, emit, download.
 * The counts and range_status always come back; recs, data_out and commitments_out
 * (nullable) are written when cap and data_cap (bytes) suffice, else CEL_EINVAL; both 0 with
 * recs and data_out NULL: count only.
 * cel_namespace_ods_ranges (host only): the inclusion entries of a namespace plan
 * (cel_dev_namespace_plan's arrays) as one ODS range per queried namespace, from the first
 * entry's (row, start) to the last entry's (row, end); a namespace without one gets the empty
 * range [0, 0). CEL_EINVAL: an entry outside Q0 (row or end beyond k), an ns_idx beyond
 * n_namespaces, or entries of a namespace that are not one contiguous run of ODS shares (an
 * unordered square). */
#define CEL_BLOB_EVERSION 1 /* range status codes; 0 = ok */
#define CEL_BLOB_ENOSTART 2
#define CEL_BLOB_ESHORT 3
typedef struct cel_blob_rec { /* 64 bytes */
  uint32_t range, start, shares, share_version;
  uint32_t len, reserved;
  uint64_t data_off;
  uint8_t ns[32]; /* 29 bytes, then zeros */
} cel_blob_rec;
size_t cel_dev_blobs_workspace_size(uint64_t total_shares, uint32_t n_ranges);
cel_status cel_dev_blobs_plan(cel_ctx* ctx, const void* d_eds, uint32_t k, uint32_t n_ranges,
                              const uint32_t* starts, const uint32_t* ends, uint64_t cap,
                              cel_blob_rec* recs, uint32_t* range_status, uint64_t* n_blobs,
                              uint64_t* total_bytes, void* d_work, void* stream);
cel_status cel_dev_blobs_emit(cel_ctx* ctx, const void* d_eds, uint32_t k, uint64_t n_blobs,
                              void* d_data, void* d_commitments, uint32_t subtree_root_threshold,
                              void* d_work, void* d_commit_work, void* stream);
cel_status cel_blobs_by_range(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n_ranges,
                              const uint32_t* starts, const uint32_t* ends, uint64_t cap,
                              uint64_t data_cap, cel_blob_rec* recs, uint32_t* range_status,
                              uint8_t* data_out, uint8_t* commitments_out,
                              uint32_t subtree_root_threshold, uint64_t* n_blobs,
                              uint64_t* total_bytes);
cel_status cel_namespace_ods_ranges(uint32_t k, uint32_t n_namespaces, uint64_t n_entries,
                                    const uint32_t* ns_idx, const uint32_t* rows,
                                    const int32_t* starts, const int32_t* ends, const uint8_t* kinds,
                                    uint32_t* range_start, uint32_t* range_end);

/* ------------------------------------------------- txs by range
 * go-square v1.1.0 parseCompactShares over runs of ODS shares of a resident square: the txs of
 * the tx namespace (28 zero bytes, 0x01) and the index wrappers of the PayForBlob namespace
 * (28 zero bytes, 0x04), what shares.ParseTxs and square.Deconstruct read. Ranges are those of
 * the blob calls; they may repeat, overlap or be empty. A range's status is its first error in
 * this order, a failed range yields no units, the other ranges are unaffected:
 *   1. a share whose info byte has a version other than 0: CEL_TX_EVERSION;
 *   2. a share whose namespace is neither of the two: CEL_TX_ENAMESPACE (narrower than go-square,
 *      which would read it with another header size); both may be mixed in one range;
 *   3. the stream: a share's header size h is 38 with the sequence-start bit, else 34; the first
 *      share's reserved value R, big-endian at bytes h-4 .. h-1, gives CEL_TX_ERESERVED when
 *      R >= 512, no bytes when R == 0, else the bytes R .. 511 (also where R < h); every later
 *      share gives its bytes h .. 511 whatever its reserved value. The sequence length is not
 *      read;
 *   4. the units, from stream position p = 0: stop at the stream's end; read a uvarint from up to
 *      10 bytes at p, zeros behind the end (more than 10 bytes, or a 10th byte above 1:
 *      CEL_TX_EVARINT); with its value L and n the length of L's canonical encoding, L == 0
 *      stops (padding), L above the bytes left behind p + n stops (a cut unit is dropped without
 *      error), else the unit is the stream's bytes [p + n, p + n + L) and p += n + L.
 * range_flags (nullable, n_ranges words): CEL_TX_FHINTS where the reserved bytes of the later
 * shares disagree with that parse: up to the share in which the last unit begins, a share in
 * which a unit begins does not name the first such unit's byte, or one in which none begins
 * holds a usable value (h <= R < 512). The device finds the units share by share from these
 * values and parses such a range serially instead; the result is the same. An honest builder
 * never produces it.
 *
 * cel_tx_rec: (share, shares) are the ODS index of the share in which the unit's length prefix
 * begins and the number of shares that prefix and unit touch: cel_square_tx_range's
 * [start, end) = [share, share + shares), which counts the prefix too. share_off is the byte of
 * that share at which the prefix begins; len the unit's length; its bytes go to data_off, a
 * multiple of 16, and take len rounded up to 16.
 *
 * cel_dev_txs_plan: counts the units of n_ranges ranges of the square at d_eds (2k*2k*512,
 * 16-byte aligned; only Q0 is read): *n_units, *total_bytes, range_status and range_flags (both
 * nullable). Synchronous on stream: the counts depend on the data. The plan stays in d_work
 * (cel_dev_txs_workspace_size(total shares of the ranges, n_ranges) bytes, 16-byte aligned,
 * linear in both) for cel_dev_txs_emit, which must be the next tx call on this ctx with that
 * workspace. CEL_EINVAL as for cel_dev_blobs_plan; n_ranges = 0 is CEL_OK.
 * cel_dev_txs_emit: the records of the first n_units units of the plan (no more than it holds),
 * in (range, position) order, into d_recs (device memory, 16-byte aligned), their bytes into
 * d_data (16-byte aligned, total_bytes bytes; zeros up to the next multiple of 16) and, with
 * d_hashes not NULL, the SHA-256 of each unit's bytes (32 bytes each): the tx hash of a unit of
 * the tx namespace, the hash of the index wrapper as stored of a PayForBlob unit. Asynchronous
 * on stream.
 * cel_txs_by_range: the same for a square in host memory: upload, plan, emit, download. The
 * counts, range_status and range_flags always come back; recs, data_out and hashes_out
 * (nullable) are written when cap and data_cap (bytes) suffice, else CEL_EINVAL; both 0 with
 * recs and data_out NULL: count only. */
#define CEL_TX_EVERSION 1 /* range status codes; 0 = ok */
#define CEL_TX_ENAMESPACE 2
#define CEL_TX_ERESERVED 3
#define CEL_TX_EVARINT 4
#define CEL_TX_FHINTS 1u /* range flag */
typedef struct cel_tx_rec { /* 32 bytes */
  uint32_t range, share, share_off, shares;
  uint64_t len, data_off;
} cel_tx_rec;
size_t cel_dev_txs_workspace_size(uint64_t total_shares, uint32_t n_ranges);
cel_status cel_dev_txs_plan(cel_ctx* ctx, const void* d_eds, uint32_t k, uint32_t n_ranges,
                            const uint32_t* starts, const uint32_t* ends, uint32_t* range_status,
                            uint32_t* range_flags, uint64_t* n_units, uint64_t* total_bytes,
                            void* d_work, void* stream);
cel_status cel_dev_txs_emit(cel_ctx* ctx, const void* d_eds, uint32_t k, uint64_t n_units,
                            void* d_recs, void* d_data, void* d_hashes, void* d_work, void* stream);
cel_status cel_txs_by_range(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n_ranges,
                            const uint32_t* starts, const uint32_t* ends, uint64_t cap,
                            uint64_t data_cap, cel_tx_rec* recs, uint32_t* range_status,
                            uint32_t* range_flags, uint8_t* data_out, uint8_t* hashes_out,
                            uint64_t* n_units, uint64_t* total_bytes);

/* Blob share commitments from an EDS (pkg/inclusion).
 * cel_commitment_paths: calculateCommitmentPaths (paths.go:16-47) for a blob of
 * blob_share_len shares placed at the first aligned index >= start of a square of
 * width square_size: per subtree root, its row and its (depth, position) inside the
 * row's ODS half (the reference walk is WalkLeft then the depth bits of position,
 * most significant first). n_out = count; arrays (nullable) hold up to cap entries.
 * cel_get_commitment: GetCommitment (get_commit.go:12-30) over device-built row
 * trees: the RFC-6962 root of those subtree roots (eds = 2k*2k*share host bytes). */
cel_status cel_commitment_paths(uint32_t square_size, uint32_t start, uint32_t blob_share_len,
                                uint32_t subtree_root_threshold, uint32_t* rows, uint32_t* depths,
                                uint32_t* positions, uint32_t cap, uint32_t* n_out);
/* calculateSubTreeRootCoordinates (paths.go:95-173): leaves [start, end) of a tree of
 * depth max_depth covered left to right by the largest aligned subtrees of depth >=
 * min_depth, as (depth, position) pairs. */
cel_status cel_subtree_root_coordinates(uint32_t max_depth, uint32_t min_depth, uint32_t start,
                                        uint32_t end, uint32_t* depths, uint32_t* positions,
                                        uint32_t cap, uint32_t* n_out);
cel_status cel_get_commitment(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t share_size,
                              uint32_t start, uint32_t blob_share_len,
                              uint32_t subtree_root_threshold, uint8_t* commitment);

/* Blob share commitments from blob bytes (go-square v1.1.0 inclusion.CreateCommitment, as
 * blobtypes.ValidateBlobTx recomputes it for every blob before the square exists,
 * x/blob/types/blob_tx.go:96-105). The device splits the blobs into sparse shares on the
 * fly (shares are never written out), hashes the NMT subtree roots of each blob's merkle
 * mountain range at SubTreeWidth(shares, subtree_root_threshold) and the RFC-6962 root
 * over them. Only share version 0 exists ("unsupported share version v" otherwise);
 * namespaces are hashed as given (ValidateBlobNamespace stays with the caller); an empty
 * blob is CEL_EINVAL ("blob i has no data"), a blob above 2^20 shares CEL_ETOOBIG.
 *
 * go-square inclusion.CreateCommitments: blob i is data[offsets[i] .. offsets[i+1]),
 * namespaces: nblobs*29 (version || id), share_versions nullable (= 0).
 * commitments: nblobs*32. Page-locked data (cel_host_alloc) is uploaded in place, pageable
 * data through page-locked staging; large batches run in chunks of whole blobs. */
cel_status cel_create_commitments(cel_ctx* ctx, const uint8_t* data, const uint64_t* offsets,
                                  uint32_t nblobs, const uint8_t* namespaces,
                                  const uint8_t* share_versions, uint32_t subtree_root_threshold,
                                  uint8_t* commitments);
/* Same with data and commitments in device memory; offsets / namespaces stay host
 * (the host plans the leaf slots). Asynchronous on stream. d_work: at least
 * cel_dev_commitments_workspace_size(sum of the blobs' shares, nblobs) bytes; one call
 * holds at most 2^31 leaf slots (CEL_ETOOBIG). The kernels read d_data in whole aligned
 * dwords that hold at least one blob byte, so up to 3 bytes before d_data + offsets[0] and
 * after the last blob byte are touched (never used): the first and last aligned dword of
 * the data must be readable, which holds for any hipMalloc'd buffer. */
size_t cel_dev_commitments_workspace_size(uint64_t total_shares, uint32_t nblobs);
cel_status cel_dev_create_commitments(cel_ctx* ctx, const void* d_data, const uint64_t* offsets,
                                      uint32_t nblobs, const uint8_t* namespaces,
                                      const uint8_t* share_versions, uint32_t subtree_root_threshold,
                                      void* d_commitments, void* d_work, void* stream);
/* The block-level shape ProcessProposal needs: every blob of every BlobTx among txs (same tx
 * encoding and unmarshal rules as cel_square_construct), one device batch. commitments: cap*32,
 * tx_index[cap] = the tx each blob came from, *n_out = number of blobs (call with cap = 0 to
 * size; a cap below the count is CEL_EINVAL). The sizing call only counts: an invalid
 * blob (empty, share version other than 0, above 2^20 shares) is reported by the call
 * with cap > 0. */
cel_status cel_blob_tx_commitments(cel_ctx* ctx, const uint8_t* txs, const uint32_t* tx_lens,
                                   uint32_t ntx, uint32_t subtree_root_threshold,
                                   uint8_t* commitments, uint32_t* tx_index, uint32_t cap,
                                   uint32_t* n_out);
/* Host only: MerkleMountainRangeSizes(SparseSharesNeeded(blob_len), SubTreeWidth(...)):
 * *shares, *width (both nullable), and the subtree sizes (up to cap entries, *n_out = count). */
cel_status cel_blob_subtree_sizes(uint64_t blob_len, uint32_t subtree_root_threshold,
                                  uint32_t* shares, uint32_t* width, uint32_t* sizes,
                                  uint32_t cap, uint32_t* n_out);

/* ---------------------------------------------------- data-square construction
 * go-square v1.1.0 (host code, no device needed):
 *   greedy = 0: square.Construct (app/extend_block.go:16-25, app/process_proposal.go:121-130):
 *               normal txs must precede blob txs; a tx that does not fit is an error
 *               (CEL_ETOOBIG "not enough space to append tx at index i",
 *               CEL_EINVAL "normal transaction at index i can not be appended after blob tx");
 *   greedy = 1: square.Build (app/prepare_proposal.go:48-61): txs that do not fit are
 *               skipped (the square orders kept normal txs before kept blob txs).
 * included (nullable, ntx bytes): 0 = tx not in the square, 1 = normal tx kept,
 * 2 = blob tx kept.
 * txs: the ntx transactions concatenated, tx_lens[ntx] their lengths.
 * max_square_size / subtree_root_threshold: appconsts SquareSizeUpperBound (128) and
 * SubtreeRootThreshold (64) (pkg/appconsts/v1,v2/app_consts.go).
 * Writes k*k shares (the ODS handed to cel_extend_shares) to shares_out (capacity
 * cap_shares shares; shares_out == NULL only reports *k_out). */
cel_status cel_square_construct(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx,
                                uint32_t max_square_size, uint32_t subtree_root_threshold,
                                uint32_t greedy, uint8_t* shares_out, uint32_t cap_shares,
                                uint32_t* k_out, uint8_t* included);
/* go-square Builder.FindTxShareRange after Construct (pkg/proof/proof.go:21-48,
 * NewTxInclusionProof): the ODS shares [*start, *end) holding tx `tx_index` (a normal tx,
 * or the index wrapper of a blob tx, which lives in the PayForBlob namespace). */
cel_status cel_square_tx_range(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx,
                               uint32_t max_square_size, uint32_t subtree_root_threshold,
                               uint32_t tx_index, uint32_t* start, uint32_t* end);
/* Message of the last cel_square_construct / cel_square_tx_range / cel_square_layout failure
 * on this thread. */
const char* cel_square_last_error(void);

/* The same square as a layout, without its blob bytes (host only): where every share of the
 * k*k ODS comes from. The segments are ascending and cover share indices [0, k*k) exactly
 * once (segments of zero shares are left out):
 *   CEL_SEG_COMPACT  count shares copied from the compact shares, from share `off` on: the
 *                    tx and PayForBlob namespaces, whose re-marshalled index wrappers only
 *                    the host can produce;
 *   CEL_SEG_BLOB     the count sparse shares of one blob: namespace ns, share version,
 *                    `len` data bytes at byte `off` of the concatenated txs, from tx tx_index;
 *   CEL_SEG_PAD      count padding shares of namespace ns (namespace padding between blobs,
 *                    primary reserved padding, tail padding): ns, info byte 1, zeros. */
#define CEL_SEG_COMPACT 0u
#define CEL_SEG_BLOB 1u
#define CEL_SEG_PAD 2u
typedef struct cel_square_segment {
  uint32_t kind;          /* CEL_SEG_* */
  uint32_t start;         /* first share index of the segment */
  uint32_t count;         /* shares */
  uint32_t share_version; /* BLOB: the info byte's version */
  uint64_t off;           /* COMPACT: share offset in the compact shares; BLOB: byte offset in txs */
  uint32_t len;           /* BLOB: data bytes */
  uint32_t tx_index;      /* BLOB: the tx that carries it */
  uint8_t ns[32];         /* BLOB, PAD: the 29 namespace bytes, then 3 zero bytes */
} cel_square_segment;
/* Same inputs, status codes and cel_square_last_error strings as cel_square_construct.
 * *k_out, included[] (nullable) as there; *n_segments and *n_compact_shares always receive
 * the counts. cap_segments == 0 only sizes; otherwise segments[cap_segments] and
 * compact_out[cap_compact_shares * 512] must hold them (CEL_EINVAL if not). */
cel_status cel_square_layout(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx,
                             uint32_t max_square_size, uint32_t subtree_root_threshold,
                             uint32_t greedy, uint32_t* k_out, uint8_t* included,
                             cel_square_segment* segments, uint32_t cap_segments,
                             uint32_t* n_segments, uint8_t* compact_out,
                             uint32_t cap_compact_shares, uint32_t* n_compact_shares);

/* ------------------------------------------- block data root from txs (one upload)
 * The block path of app/process_proposal.go:107 (ValidateBlobTx's commitments), :122
 * (square.Construct), app/prepare_proposal.go:50 (square.Build) and app/extend_block.go:16
 * (square.Construct + da.ExtendShares) as one call: the host lays the square out
 * (cel_square_layout), the blob bytes cross PCIe once, the device writes every ODS share
 * straight into quadrant Q0 of the EDS (blob shares cut from the tx bytes, compact shares
 * copied, padding shares generated), extends it in place and hashes the roots; the blob
 * share commitments are hashed from the same device copy of the tx bytes.
 *
 * cel_dev_square_build: the device-resident step. d_txs: the concatenated txs in device
 * memory (the segments' BLOB offsets point into it; aligned dwords that hold at least one
 * blob byte are read, as cel_dev_create_commitments documents); segments / compact: a
 * layout of cel_square_layout (host memory); d_eds: an EDS buffer of 2k*2k*512 bytes,
 * 16-byte aligned, of which exactly quadrant Q0 is written (every byte of it).
 * Asynchronous on stream (NULL = ctx's stream). */
cel_status cel_dev_square_build(cel_ctx* ctx, const void* d_txs, const cel_square_segment* segments,
                                uint32_t n_segments, const uint8_t* compact,
                                uint32_t n_compact_shares, uint32_t k, void* d_eds, void* stream);
/* cel_block_extend: txs in, data root (and roots, commitments, optionally the EDS) out.
 * txs, tx_lens, ntx, max_square_size (up to 512; k >= 256 extends over GF(2^16)),
 * subtree_root_threshold, greedy, *k_out, included[] (nullable): as cel_square_construct.
 * row_roots / col_roots: sized for max_square_size (2 * max_square_size * 90 bytes each),
 * 2k*90 bytes of each are written; dah: 32 bytes. eds_out (nullable) with eds_cap bytes:
 * the 2k*2k*512-byte EDS (CEL_EINVAL if eds_cap is below that); with CEL_FLAG_PARITY_ONLY
 * its Q0 cells are not written. commitments / commit_tx_index / commit_cap / n_commit: the
 * share commitments of every blob of every BlobTx among txs, in order, kept in the square or
 * not, with cel_blob_tx_commitments' convention (*n_commit always receives the count;
 * commit_cap == 0 skips them; a cap below the count is CEL_EINVAL). Construction errors are
 * cel_square_construct's (text in cel_last_error), commitment errors exactly
 * cel_blob_tx_commitments' (commit_cap > 0 only), both before any device work. Page-locked
 * txs (cel_host_alloc) are uploaded in place, pageable txs through page-locked staging; with
 * greedy = 0 only the blob txs (a contiguous tail) are uploaded. */
cel_status cel_block_extend(cel_ctx* ctx, const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx,
                            uint32_t max_square_size, uint32_t subtree_root_threshold,
                            uint32_t greedy, uint32_t* k_out, uint8_t* included,
                            uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                            uint8_t* eds_out, uint64_t eds_cap, uint8_t* commitments,
                            uint32_t* commit_tx_index, uint32_t commit_cap, uint32_t* n_commit,
                            uint32_t flags);

/* ------------------------------------------- a range of blocks from txs (one call)
 * The block path for a range of heights: a node catching up holds each block's txs and needs
 * each block's data root and DAH. Blocks that construct are grouped by square width, cut into
 * chunks whose EDS bytes fit a budget, and each chunk costs one upload of its blob bytes and
 * plan, one square-build launch for all its blocks, one extension and one commit per width
 * present, one commitments batch and one download; one stream synchronise ends the call.
 *
 * cel_dev_square_build_batch: cel_dev_square_build for n_blocks blocks in one launch. d_txs:
 * device tx bytes, block b's txs starting at d_txs + tx_base[b] (its BLOB offsets count from
 * there); segments: the blocks' layouts back to back, n_segments[b] of block b; compact: their
 * compact shares back to back, n_compact_shares[b] of block b (NULL if there are none);
 * k[b]: block b's width; d_eds: one device buffer, 16-byte aligned, in which block b's EDS of
 * 2k*2k*512 bytes starts at byte eds_off[b] (a multiple of 16; the caller keeps the EDSs
 * apart). Exactly quadrant Q0 of every block's EDS is written, every byte of it. Every block's
 * layout is checked as cel_dev_square_build checks one, before any device work; the blocks
 * hold fewer than 2^27 shares in all. Asynchronous on stream (NULL = ctx's stream). */
cel_status cel_dev_square_build_batch(cel_ctx* ctx, const void* d_txs, const uint64_t* tx_base,
                                      uint32_t n_blocks, const cel_square_segment* segments,
                                      const uint32_t* n_segments, const uint8_t* compact,
                                      const uint32_t* n_compact_shares, const uint32_t* k,
                                      void* d_eds, const uint64_t* eds_off, void* stream);
/* cel_block_extend_batch: cel_block_extend for n_blocks blocks. txs: every block's txs
 * concatenated, block after block; tx_lens: their lengths; block_ntx[n_blocks]: how many of
 * them belong to each block. max_square_size, subtree_root_threshold, greedy, flags: as
 * cel_block_extend, the same for every block.
 * host_threads: the blocks are laid out on up to this many threads (0 and 1: the calling
 * thread). max_eds_bytes: the EDS bytes of one chunk (0: 2 GiB); a block above it is a chunk
 * of its own.
 * Per block i: k_out[i]; status_out[i]; included (nullable), one byte per tx in tx order
 * across blocks; dah + 32 i; row_roots / col_roots (roots_cap nodes of 90 bytes each): block
 * i's 2k roots of each start at node root_off[i], and root_off[n_blocks] is the total
 * (n_blocks * 2 * max_square_size always suffices; a cap below the total is CEL_EINVAL).
 * commitments / commit_block / commit_tx_index / commit_cap / n_commit: every blob of every
 * BlobTx of every block that constructed, flat in block order, with its block and its tx's
 * index inside the block; cel_block_extend's convention (*n_commit always receives the count,
 * commit_cap == 0 skips them, a cap below the count is CEL_EINVAL).
 * A block whose txs do not construct, or whose commitments cannot be computed, gets the
 * status cel_block_extend gives it, k 0, no roots, a zero dah, zero included bytes and no
 * commitments; it does not stop the others, whose outputs are exactly cel_block_extend's. The
 * call returns the first status in block order that is not CEL_OK, with that block's message
 * prefixed "block <i>: " in cel_last_error; cel_block_batch_error gives any block's message.
 * Argument errors, both caps among them, return before any output but *n_commit is written.
 * phase_ms (nullable, 2 floats): the host layout's wall time and the device time between
 * events around the call's enqueued work, in milliseconds. */
cel_status cel_block_extend_batch(cel_ctx* ctx, const uint8_t* txs, const uint32_t* tx_lens,
                                  const uint32_t* block_ntx, uint32_t n_blocks,
                                  uint32_t max_square_size, uint32_t subtree_root_threshold,
                                  uint32_t greedy, uint32_t host_threads, uint64_t max_eds_bytes,
                                  uint32_t* k_out, int32_t* status_out, uint8_t* included,
                                  uint8_t* row_roots, uint8_t* col_roots, uint32_t* root_off,
                                  uint64_t roots_cap, uint8_t* dah, uint8_t* commitments,
                                  uint32_t* commit_block, uint32_t* commit_tx_index,
                                  uint32_t commit_cap, uint32_t* n_commit, float* phase_ms,
                                  uint32_t flags);
/* The message of block `block` of the last cel_block_extend_batch on ctx ("" if it was
 * CEL_OK or there is no such block); valid until the next call on ctx. */
const char* cel_block_batch_error(cel_ctx* ctx, uint32_t block);

#ifdef __cplusplus
}
#endif
#endif /* CELESTIA_EDS_H */
