/* lzo_mi355x_kernels.h -- internal launch interface between the host C code
 * (lzo_host.c) and the HIP kernels (lzo1x_kernels.hip). */
#ifndef POM_LZO_MI355X_KERNELS_H
#define POM_LZO_MI355X_KERNELS_H 1

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#include "host_debug.h"         /* the debug switches the launchers read */

#ifdef __cplusplus
extern "C" {
#endif

/* status of a block lzo1x_encode_fast_kernel left to the general encoder */
#define LZO_MI355X_ENC_PENDING 0x7FFF0002
/* status of a block a speculative decoder (fast, win, lat) handed to the exact decoder */
#define LZO_MI355X_DEC_PENDING 0x7FFF0001

#define LZO_MI355X_FAST_MAX_N (1u << 24)   /* the throughput encoder's largest block (kMaxN) */

/* Throughput encoder (lzo1x_encode_fast.hip), blocks of up to 16 MiB; larger
 * blocks get status LZO_MI355X_ENC_PENDING.  With scratch (scratch_bytes of
 * device memory, lzo_mi355x_compress_scratch()) the dictionaries live there
 * and 16 blocks per CU are parsed at once; without, in LDS (4 per CU). */
int lzo_mi355x_launch_compress_fast(const uint8_t *src, const uint64_t *src_off,
                                    const uint32_t *src_len, uint8_t *dst,
                                    const uint64_t *dst_off, const uint32_t *dst_cap,
                                    uint32_t *out_len, int32_t *status, uint32_t nblocks,
                                    void *scratch, size_t scratch_bytes, hipStream_t stream);

/* General encoder (lzo1x_kernels.hip), any block size.
 * pending_only: only blocks whose status is LZO_MI355X_ENC_PENDING. */
int lzo_mi355x_launch_compress(const uint8_t *src, const uint64_t *src_off,
                               const uint32_t *src_len, uint8_t *dst,
                               const uint64_t *dst_off, const uint32_t *dst_cap,
                               uint32_t *out_len, int32_t *status, uint32_t nblocks,
                               int pending_only, hipStream_t stream);

/* Exact (grammar-serial) decoder, lzo1x_decompress_safe semantics, or with
 * `unchecked` those of the unchecked lzo1x_decompress.  fb NULL: grid entry b
 * decodes block b (ngrid = nblocks).  Otherwise the *fb blocks listed at
 * fb_ids[] are decoded by a grid of ngrid workgroups. */
int lzo_mi355x_launch_decompress_exact(const uint8_t *src, const uint64_t *src_off,
                                       const uint32_t *src_len, uint8_t *dst,
                                       const uint64_t *dst_off, const uint32_t *dst_cap,
                                       uint32_t *out_len, int32_t *status,
                                       const uint32_t *fb, const uint32_t *fb_ids,
                                       uint32_t ngrid, uint32_t nblocks, int unchecked,
                                       hipStream_t stream);

/* Exact decoder over blocks of consecutive streams (the hvfs_fwritev column
 * layout): each stream decodes with lzo1x_decompress_safe semantics right
 * after the previous one's output; out_len = the total. */
int lzo_mi355x_launch_decompress_concat(const uint8_t *src, const uint64_t *src_off,
                                        const uint32_t *src_len, uint8_t *dst,
                                        const uint64_t *dst_off, const uint32_t *dst_cap,
                                        uint32_t *out_len, int32_t *status, uint32_t nblocks,
                                        hipStream_t stream);

/* Throughput decoder (lzo1x_decode_fast.hip).  Blocks it does not finish
 * exactly are appended to fallback_ids[] (*fallback = count, must be 0 on
 * entry) and get status LZO_MI355X_DEC_PENDING until the exact decoder runs on them.
 * ops: nsets op-slot sets of lzo_mi355x_fast_ops_bytes_per_block() bytes,
 * shared by the workgroups through a pool (pool: LZO_MI355X_FAST_POOL_BYTES
 * of counters, ring: nsets u64, all zero on entry); nsets = min(nblocks,
 * lzo_mi355x_fast_resident_blocks()) keeps every resident workgroup busy. */
#define LZO_MI355X_FAST_POOL_BYTES 8192
size_t lzo_mi355x_fast_ops_bytes_per_block(void);
uint32_t lzo_mi355x_fast_resident_blocks(void);
int lzo_mi355x_launch_decompress_fast(const uint8_t *src, const uint64_t *src_off,
                                      const uint32_t *src_len, uint8_t *dst,
                                      const uint64_t *dst_off, const uint32_t *dst_cap,
                                      uint32_t *out_len, int32_t *status, uint32_t *fallback,
                                      uint32_t *fallback_ids, uint32_t *pool, void *ring,
                                      void *ops, uint32_t nsets, uint32_t nblocks,
                                      uint32_t *order, hipStream_t stream);

/* Batches with more blocks than resident workgroups start them largest first
 * (order[i] = the i-th block to start; key: src_len to compress, dst_cap to
 * decompress, in 4 KiB classes): the last blocks to start are then the
 * smallest, and the batch does not wait on a large block started last (C4,
 * mixed 4-256 KiB: decompress 37.6 -> 35.2 ms, compress 119.6 -> 117.2 ms).
 * One workgroup, a counting sort, a few tens of microseconds. */
int lzo_mi355x_launch_order_by_size(const uint32_t *key, uint32_t n, uint32_t *order,
                                    hipStream_t stream);

/* Windowed throughput decoder (lzo1x_decode_win.hip): one workgroup of 512
 * threads per block, 64 KiB LDS output ring.  Blocks it does not finish
 * exactly go to fallback_ids[] as with the fast decoder (*fallback = 0 on
 * entry). */
int lzo_mi355x_launch_decompress_win(const uint8_t *src, const uint64_t *src_off,
                                     const uint32_t *src_len, uint8_t *dst,
                                     const uint64_t *dst_off, const uint32_t *dst_cap,
                                     uint32_t *out_len, int32_t *status, uint32_t *fallback,
                                     uint32_t *fallback_ids, uint32_t nblocks, hipStream_t stream);

/* Latency decoder (lzo1x_decode_lat.hip): ONE block of z compressed bytes
 * into out (capacity cap) by a pipeline of grid-wide kernels; out_len[b] /
 * status[b] and the fallback list as above.  scratch: at least
 * lzo_mi355x_decompress_lat_scratch(z, cap) bytes of device memory (0: the
 * block is outside the decoder's range -- z or cap 0, 2z + 3 or cap over
 * 16 Mi).  Returns -1 (nothing launched) outside that range or with too little
 * scratch. */
size_t lzo_mi355x_decompress_lat_scratch(uint32_t z, uint32_t cap);
int lzo_mi355x_launch_decompress_lat(const uint8_t *in, uint32_t z, uint8_t *out, uint32_t cap,
                                     uint32_t *out_len, int32_t *status, uint32_t *fallback,
                                     uint32_t *fallback_ids, uint32_t b, void *scratch,
                                     size_t scratch_bytes, hipStream_t stream);

/* Up to 8 blocks side by side in one latency-decoder pipeline (host arrays:
 * block b is z[b] bytes at src + src_off[b] into dst + dst_off[b], capacity
 * cap[b]; results at b0 + b; src_off[b] + z[b] < 2^31).  Scratch 0: outside
 * the range. */
size_t lzo_mi355x_decompress_lat_scratch_n(const uint64_t *src_off, const uint32_t *z, const uint32_t *cap,
                                           uint32_t nb);
int lzo_mi355x_launch_decompress_lat_n(const uint8_t *src, const uint64_t *src_off, const uint32_t *z,
                                       uint8_t *dst, const uint64_t *dst_off, const uint32_t *cap, uint32_t nb,
                                       uint32_t *out_len, int32_t *status, uint32_t *fallback,
                                       uint32_t *fallback_ids, uint32_t b0, void *scratch, size_t scratch_bytes,
                                       hipStream_t stream);

/* Unchecked-decoder pre-scan: decoded length and status per block; with
 * cap_out, also min(length, cap_limit) per block (a decode's capacity). */
int lzo_mi355x_launch_decoded_length(const uint8_t *src, const uint64_t *src_off,
                                     const uint32_t *src_len, uint32_t *out_len,
                                     int32_t *status, uint32_t nblocks, uint32_t *cap_out,
                                     uint32_t cap_limit, hipStream_t stream);

/* Host side (lzo_host.c), not part of the ABI: lzo_mi355x_compress_batch
 * with on_chunk(ctx, ids, nb) called as each chunk's blocks are delivered
 * (ids: indices into the caller's arrays), from the thread running that
 * device's chunks -- concurrently when the batch is split over GPUs. */
typedef void (*pom_chunk_fn)(void *ctx, const size_t *ids, size_t nb);
int pom_compress_batch_chunked(const uint8_t *const *src, const size_t *src_len, uint8_t *const *dst,
                               size_t *dst_len, int *status, size_t nblocks, pom_chunk_fn on_chunk,
                               void *ctx);
/* lzo_mi355x_decompress_batch with pre_chunk(ctx, ids, nb) called before each
 * chunk's inputs are staged (the caller fills src[ids[i]] then). */
int pom_decompress_batch_chunked(const uint8_t *const *src, const size_t *src_len, uint8_t *const *dst,
                                 size_t *dst_len, int *status, size_t nblocks, pom_chunk_fn pre_chunk,
                                 void *ctx);

/* Host side (lzo_host.c), not part of the ABI: len[i] bytes from src[i] to
 * dst[i] for every i, split over up to 8 threads once the total is large. */
void pom_copy_parallel(uint8_t *const *dst, const uint8_t *const *src, const size_t *len, size_t n);

/* Block b's first min(len[b], cap[b]) bytes at from + from_off[b] go to
 * to + to_off[b] (offsets 16-byte aligned, regions padded to 16 bytes). */
int lzo_mi355x_launch_pack(const uint8_t *from, const uint64_t *from_off, const uint32_t *len,
                           const uint32_t *cap, const uint64_t *to_off, uint8_t *to,
                           uint32_t nblocks, hipStream_t stream);

/* The garbage collector's ITB walk (itb_scan.hip): pom_gc_scan_dev of
 * include/pom_gc.h, three launches on `stream`. */
struct pom_gc_range;
int lzo_mi355x_launch_gc_scan(const uint8_t *payload, const uint64_t *payload_off,
                              const uint32_t *payload_len, const int32_t *status,
                              const uint8_t *adepth, uint32_t nitb, uint32_t column,
                              uint32_t *live, uint32_t *nranges, uint64_t *first,
                              struct pom_gc_range *ranges, uint64_t ranges_cap, int32_t *err,
                              hipStream_t stream);

/* Host side (host_records.c), not part of the ABI: the chunk pipeline of the
 * host batches with a walk queued behind each chunk's decode (gc_scan.c,
 * readdir.c, kvlist.c).  Block b is src_len[b] bytes at src[b]: an LZO1X
 * stream decoded on the GPU with capacity cap[b] when is_lzo[b], else a
 * payload walked as staged.  Per block the decoder's status and out_len (0 and
 * src_len[b] when not is_lzo), and live, count and err as the walk's _dev call
 * gives them; recs[b] = the block's records, inside one of the per-chunk
 * buffers linked at bufs (the caller frees them with pom_walk_bufs_free).
 * Only the counts and the records are copied back. */
struct pom_walk_buf;                /* host_requests.h */
struct pom_walk_sink {
    const uint8_t *is_lzo;
    const size_t *cap;
    const uint8_t *adepth;
    int32_t *status, *err;
    uint32_t *out_len, *live;
    uint32_t *count;                /* nranges (GC scan) or dnum (listings) */
    const uint8_t **recs;           /* count[b] 16-byte ranges (GC scan) or bytes[b] bytes (listings) */
    int column;                     /* pom_gc_scan_chunked only */
    uint32_t *bytes;                /* the listings only */
    /* pom_kvlist_chunked only: */
    uint32_t *keybytes;
    uint64_t *mask;                 /* 16 words a block, or NULL: the masks stay on the device */
    uint32_t kv_op, needle_len;
    const uint8_t *needle;          /* staged once per chunk */
    int count_only;                 /* no emit launch, no record comes back (recs[b] stays NULL) */
    struct pom_walk_buf *bufs;
    pthread_mutex_t mu;             /* bufs: chunks of a multi-GPU batch finish on several threads */
};
int pom_gc_scan_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                        struct pom_walk_sink *sink);
int pom_readdir_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                        struct pom_walk_sink *sink);
int pom_kvlist_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                       struct pom_walk_sink *sink);

/* Host side (host_records.c), not part of the ABI: pom_gc_scan_chunked with the
 * merge of each chunk's ranges queued behind its walk (gc_merge.hip; gc_stat.c).
 * The per-block results are the scan's, but no range comes back (recs[b] stays
 * NULL): each delivered chunk links its merged map at maps (pad: its extents;
 * the caller frees them with pom_walk_bufs_free) and adds its ranges, and those
 * of them with high <= low, to nin and nwrapped, all under the sink's mu. */
struct pom_gc_stat_sink {
    struct pom_walk_buf *maps;
    uint64_t nin, nwrapped;
};
int pom_gc_stat_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                        struct pom_walk_sink *sink, struct pom_gc_stat_sink *maps);

/* Host side (gc_scan.c), not part of the ABI: the two halves the walks' host
 * batches share around their pom_*_chunked call.  pom_walk_out names the
 * caller's outputs: out_cap and first[] count units of `unit` bytes (16-byte
 * ranges, or bytes); dnum, keybytes, mask, len_ok and entries_ok may be NULL.
 * listing: the h.entries rule of the listings (negative: -EINVAL; 0: done, not
 * walked), their records sized by bytes[] and copied over the copy threads.
 * count_only: nothing is copied and nothing can run out of room. */
struct pom_walk_out {
    uint8_t *out;
    size_t out_cap, unit;
    size_t *first;
    uint32_t *live, *dnum, *keybytes;
    uint64_t *mask;
    int *err, *len_ok, *entries_ok;
    int listing, count_only;
};
/* The work arrays of one call: the records that go to the GPU are k = 0 ... m -
 * 1, record idx[k], and G is their sink, set up but for the operation's own
 * inputs (column; op and needle). */
struct pom_walk_batch {
    size_t n, m;
    size_t *idx, *slen, *cap, *fit;
    const uint8_t **src, **recs;
    uint8_t *flags, **to;
    int32_t *i32, *entries;
    uint32_t *u32;
    uint64_t *masks;
    struct pom_walk_sink G;
};
/* Zeroes the outputs, selects the records by their headers and sets up the
 * sink.  LZO_E_OK or LZO_E_OUT_OF_MEMORY; pom_walk_finish follows either way. */
int pom_walk_begin(struct pom_walk_batch *W, const uint8_t *const *rec, const size_t *rec_len, size_t n,
                   const struct pom_walk_out *O);
/* rc: pom_walk_begin's or the chunked call's.  A failure gives every selected
 * record LZO_E_ERROR; otherwise the results are put together in ITB order.
 * Frees everything and returns the batch's result (rc, LZO_E_OK or
 * POM_GC_E_NOSPACE). */
int pom_walk_finish(struct pom_walk_batch *W, int rc, const struct pom_walk_out *O);

/* The directory listing's ITB walk (itb_dents.hip): pom_readdir_dev of
 * include/pom_readdir.h, three launches on `stream`. */
int lzo_mi355x_launch_readdir(const uint8_t *payload, const uint64_t *payload_off,
                              const uint32_t *payload_len, const int32_t *status,
                              const uint8_t *adepth, uint32_t nitb, uint32_t *live,
                              uint32_t *dnum, uint32_t *bytes, uint64_t *first, uint8_t *out,
                              uint64_t out_cap, int32_t *err, hipStream_t stream);

/* The key/value table listing's ITB walk (itb_keys.hip): pom_kvlist_dev of
 * include/pom_kvlist.h, three launches on `stream`. */
int lzo_mi355x_launch_kvlist(const uint8_t *payload, const uint64_t *payload_off,
                             const uint32_t *payload_len, const int32_t *status,
                             const uint8_t *adepth, uint32_t nitb, uint32_t op, const uint8_t *needle,
                             uint32_t needle_len, uint32_t *live, uint32_t *dnum, uint32_t *bytes,
                             uint32_t *keybytes, uint64_t *mask, uint64_t *first, uint8_t *out,
                             uint64_t out_cap, int32_t *err, hipStream_t stream);

/* Column reads by offset and size (col_slice.hip): pom_col_slice_dev of
 * include/pom_column.h, one launch on `stream`. */
struct pom_col_req;
int lzo_mi355x_launch_col_slice(const uint8_t *data, const uint64_t *data_off,
                                const uint32_t *data_len, const int32_t *status,
                                const uint64_t *want, uint32_t ncol, const struct pom_col_req *req,
                                uint32_t nreq, uint8_t *out, const uint64_t *out_off,
                                uint32_t *out_len, int32_t *err, hipStream_t stream);

/* Host side (host_records.c), not part of the ABI: the chunk pipeline of the host
 * batches with the region copy queued behind each chunk's decode
 * (column_codec.c).  Block b is an LZO1X stream of src_len[b] bytes at src[b],
 * decoded on the GPU with capacity want[b] (concat: as consecutive streams);
 * its requests are req[req_ids[k]] for k in [req_first[b], req_first[b + 1])
 * (their col is not read: the block is the column).  Per block the decoder's
 * status; per request out_len and err as pom_col_slice_dev, and the bytes in
 * out[].  Only the slices are copied back. */
struct pom_col_sink {
    const uint64_t *want;
    const size_t *req_first, *req_ids;
    const struct pom_col_req *req;
    uint8_t *const *out;
    size_t *out_len;
    int *err;
    int32_t *status;
    int concat;
};
int pom_col_read_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                         struct pom_col_sink *sink);

/* The lookup's ITB walk (itb_find.hip): pom_lookup_dev of
 * include/pom_lookup.h, one launch on `stream`. */
struct pom_lookup_req;
int lzo_mi355x_launch_lookup(const uint8_t *payload, const uint64_t *payload_off,
                             const uint32_t *payload_len, const int32_t *status,
                             const uint8_t *adepth, uint32_t nitb, const struct pom_lookup_req *req,
                             uint32_t nreq, const uint8_t *names, uint32_t names_len, int32_t *err,
                             uint32_t *nr, uint32_t *depth, uint8_t *out, hipStream_t stream);

/* The key/value point get's ITB walk (itb_kvget.hip): pom_kvget_dev of
 * include/pom_kvget.h, three launches on `stream`. */
struct pom_kvget_req;
int lzo_mi355x_launch_kvget(const uint8_t *payload, const uint64_t *payload_off,
                            const uint32_t *payload_len, const int32_t *status,
                            const uint8_t *adepth, uint32_t nitb, const struct pom_kvget_req *req,
                            uint32_t nreq, const uint8_t *keys, uint32_t keys_len, int32_t *err,
                            uint32_t *nr, uint32_t *depth, uint32_t *len, uint64_t *lease,
                            uint64_t *first, uint8_t *out, uint64_t out_cap, hipStream_t stream);

/* Host side (host_records.c), not part of the ABI: the request operations.
 * pom_gc_scan_chunked's pipeline (LZO records decoded, stored ones walked as
 * staged) with the lookup or the get behind each chunk's decode and
 * pom_col_read_chunked's request grouping.  An ITB and all its requests travel
 * in one chunk, renumbered to the chunk's own ITB indices, with their names or
 * keys staged behind them; a decoder's code reaches the requests through err.
 * The sink (struct pom_req_sink, host_requests.h) is one for both kinds, set
 * up by pom_req_begin: a lookup's caller adds `fixed`, where the 136-byte
 * records go in request order; a get's caller adds `records` and places the
 * records recs[] points at before pom_req_finish frees their buffers.  Only
 * the kind's words and those records come back. */
struct pom_req_sink;
int pom_lookup_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                       struct pom_req_sink *sink);
int pom_kvget_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                      struct pom_req_sink *sink);

/* The ITB check (itb_check.hip): pom_itb_check_dev of include/pom_check.h, one
 * launch on `stream`; flags are the caller's to refuse. */
struct pom_check_hdr;
struct pom_check_report;
int lzo_mi355x_launch_itb_check(const uint8_t *payload, const uint64_t *payload_off,
                                const uint32_t *payload_len, const int32_t *status,
                                const uint8_t *adepth, const struct pom_check_hdr *hdr, uint32_t nitb,
                                uint32_t flags, struct pom_check_report *report, uint64_t *slot_mask,
                                uint64_t *ite_mask, int32_t *err, hipStream_t stream);

/* The ITB split (itb_split.hip): the second launch of pom_itb_split_dev of
 * include/pom_split.h, behind the check's, whose reports and err it reads.
 * payload and new_payload are 16-byte aligned; the caller has seen to hdr. */
struct pom_split_result;
int lzo_mi355x_launch_itb_split(uint8_t *payload, const uint64_t *payload_off, const uint8_t *adepth,
                                const struct pom_check_hdr *hdr, const uint8_t *split_depth, uint32_t nitb,
                                uint8_t *new_payload, const uint64_t *new_off, const uint32_t *new_cap,
                                const struct pom_check_report *ck_report, const int32_t *ck_err,
                                struct pom_split_result *result, hipStream_t stream);

/* The encoder's source lengths of 2 * nitb halves from the results on the
 * device: len[b] = old_len - 264, len[nitb + b] = new_len - 264, 0 where
 * nothing is produced. */
int lzo_mi355x_launch_itb_split_lens(const struct pom_split_result *result, uint32_t nitb, uint32_t *len,
                                     hipStream_t stream);

/* Host side (host_records.c), not part of the ABI: the check's pipeline with
 * the split and the encoder of both halves behind each chunk's decode.  Block
 * k of the call is the caller's record idx[k], whose header is rec_hdr[k] (264
 * bytes).  A delivered block gets status[k], out_len[k], its result at
 * result[idx[k]], err[idx[k]] (the result's err, or LZO_E_OUTPUT_OVERRUN when a
 * half does not fit out_cap), and, when something is produced and fits, both
 * stored records in old_out / new_out with their lengths.  A block whose chunk
 * is not delivered keeps what the caller put there.  Up go the payloads, 32
 * bytes of header facts and the split depth; back come the results and the two
 * stored payloads. */
struct pom_split_sink {
    const uint8_t *is_lzo;
    const size_t *cap;
    const uint8_t *adepth;
    const struct pom_check_hdr *hdr;    /* per block */
    const uint8_t *sd;                  /* per block: the split depth in effect */
    const uint8_t *const *rec_hdr;      /* per block */
    const size_t *idx;
    int32_t *status;
    uint32_t *out_len;
    uint8_t *delivered;                 /* per block: 1 once its chunk is delivered */
    uint8_t *const *old_out, *const *new_out;   /* the caller's, in the caller's order */
    const size_t *out_cap;
    size_t *old_len, *new_len;
    struct pom_split_result *result;
    int *err;
};
int pom_itb_split_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                          struct pom_split_sink *sink);
/* What the check needs of a record's struct itbh (check.c); is_lzo: the record is COMPR_LZO. */
void pom_check_header_facts(const uint8_t *rec, int is_lzo, struct pom_check_hdr *h);
/* itb_lzo_compress's not-smaller rule on one 264-byte header (itbsplit.c): a
 * stream of z bytes is kept when it is smaller than the payload of a record of
 * ulen bytes; len, zlen and compress_algo are set accordingly.  Returns
 * whether the stream is kept. */
int pom_itb_stored_as(uint8_t *h, uint32_t ulen, uint32_t z);

/* The ITB sweep (itb_sweep.hip): the second launch of pom_itb_sweep_dev of
 * include/pom_sweep.h, behind the check's, whose reports and err it reads.
 * payload is 16-byte aligned; the caller has seen to hdr.  budget may be
 * NULL. */
struct pom_sweep_result;
int lzo_mi355x_launch_itb_sweep(uint8_t *payload, const uint64_t *payload_off, const uint8_t *adepth,
                                const struct pom_check_hdr *hdr, const uint32_t *budget, uint32_t nitb,
                                const struct pom_check_report *ck_report, const int32_t *ck_err,
                                struct pom_sweep_result *result, hipStream_t stream);

/* The encoder's source lengths of nitb swept payloads from the results on the
 * device: len[b] = result[b].len - 264, 0 where nothing is produced. */
int lzo_mi355x_launch_itb_sweep_lens(const struct pom_sweep_result *result, uint32_t nitb, uint32_t *len,
                                     hipStream_t stream);

/* Host side (host_records.c), not part of the ABI: the split's pipeline with
 * the sweep and the encoder of the one payload behind each chunk's decode.
 * Block k of the call is the caller's record idx[k], whose header is
 * rec_hdr[k] (264 bytes).  A delivered block gets status[k], out_len[k], its
 * result at result[idx[k]], err[idx[k]] (the result's err, or
 * LZO_E_OUTPUT_OVERRUN when the record does not fit out_cap), and, when
 * something was removed and the record fits, the stored record in out with its
 * length.  A block whose chunk is not delivered keeps what the caller put
 * there.  Up go the payloads, 32 bytes of header facts and the budget; back
 * come the results and the one stored payload. */
struct pom_sweep_sink {
    const uint8_t *is_lzo;
    const size_t *cap;
    const uint8_t *adepth;
    const struct pom_check_hdr *hdr;    /* per block */
    const uint32_t *budget;             /* per block: the budget in effect */
    const uint8_t *const *rec_hdr;      /* per block */
    const size_t *idx;
    int32_t *status;
    uint32_t *out_len;
    uint8_t *delivered;                 /* per block: 1 once its chunk is delivered */
    uint8_t *const *out;                /* the caller's, in the caller's order */
    const size_t *out_cap;
    size_t *rec_len;
    struct pom_sweep_result *result;
    int *err;
};
int pom_itb_sweep_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                          struct pom_sweep_sink *sink);

/* The ITB unlink (itb_unlink.hip): the second launch of pom_itb_unlink_dev of
 * include/pom_unlink.h, behind the check's, whose reports and err it reads.
 * payload is 16-byte aligned, req and out 8-byte aligned; the caller has seen
 * to hdr. */
struct pom_unlink_result;
int lzo_mi355x_launch_itb_unlink(uint8_t *payload, const uint64_t *payload_off, const uint32_t *payload_len,
                                 const uint8_t *adepth, const struct pom_check_hdr *hdr, uint32_t nitb,
                                 int async_unlink, const struct pom_lookup_req *req, const uint32_t *req_first,
                                 uint32_t nreq, const uint8_t *names, uint32_t names_len,
                                 const struct pom_check_report *ck_report, const int32_t *ck_err, int32_t *err,
                                 uint32_t *nr, uint32_t *depth, uint32_t *what, uint8_t *out,
                                 struct pom_unlink_result *result, hipStream_t stream);

/* The encoder's source lengths of nitb payloads from the unlink's results on
 * the device: len[b] = result[b].len - 264, 0 where nothing is produced. */
int lzo_mi355x_launch_itb_unlink_lens(const struct pom_unlink_result *result, uint32_t nitb, uint32_t *len,
                                      hipStream_t stream);

/* Host side (host_records.c), not part of the ABI: the request operations'
 * pipeline (requests grouped by ITB, renumbered and staged with their names,
 * fixed results scattered into the caller's request order: K, set up by
 * pom_req_begin with the unlink's kind) with the sweep's writer half behind
 * it: the check, the unlink and the encoder of the one payload behind each
 * chunk's decode.  Block k of the call is the caller's record idx[k], whose
 * header is rec_hdr[k] (264 bytes).  A delivered block gets status[k],
 * out_len[k], its result at result[idx[k]], err[idx[k]] (the result's err, or
 * LZO_E_OUTPUT_OVERRUN when the record does not fit out_cap), and, when
 * something changed and the record fits, the stored record in out with its
 * length.  A block whose chunk is not delivered keeps what the caller put
 * there. */
struct pom_unlink_sink {
    struct pom_req_sink *K;
    int async_unlink;
    const struct pom_check_hdr *hdr;    /* per block */
    const uint8_t *const *rec_hdr;      /* per block */
    const size_t *idx;
    int32_t *status;                    /* per block: the decoder's */
    uint32_t *out_len;
    uint8_t *delivered;                 /* per block: 1 once its chunk is delivered */
    uint8_t *const *out;                /* the caller's, in the caller's order */
    const size_t *out_cap;
    size_t *rec_len;
    struct pom_unlink_result *result;
    int *err;
};
int pom_itb_unlink_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                           struct pom_unlink_sink *sink);

/* Host side (host_records.c), not part of the ABI: pom_gc_scan_chunked's
 * pipeline (LZO records decoded, stored ones checked as staged) with the check
 * behind each chunk's decode.  Block k of the call is the caller's record
 * idx[k]: its report, and its masks when the caller gave arrays for them, go
 * straight to their places in the caller's order, the per-block words to
 * status[k], out_len[k] and err[k].  A block whose chunk is not delivered reads
 * err LZO_E_ERROR.  Only 32 bytes of header facts go up besides the payloads,
 * and only the three words, the reports and the masks come back. */
struct pom_check_sink {
    const uint8_t *is_lzo;
    const size_t *cap;
    const uint8_t *adepth;
    const struct pom_check_hdr *hdr;    /* per block */
    const size_t *idx;
    uint32_t flags;
    int32_t *status, *err;
    uint32_t *out_len;
    struct pom_check_report *report;    /* the caller's, in the caller's order */
    uint64_t *slot_mask, *ite_mask;     /* the caller's, or NULL */
};
int pom_itb_check_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                          struct pom_check_sink *sink);

#ifdef __cplusplus
}
#endif

#endif
