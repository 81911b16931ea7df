/* host_requests.h -- the host arithmetic of the request operations (lookups,
 * key/value gets) around and inside their chunks: which ITBs a call's requests
 * reach, the requests grouped by ITB, a chunk's requests and blob into its
 * pinned staging, its fixed-size results into the caller's request order.
 * Plain C, neither HIP nor threads, so that tests/native/req_check.c runs it on
 * the CPU.  Internal to liblzo_mi355x.so. */
#ifndef POM_HOST_REQUESTS_H
#define POM_HOST_REQUESTS_H 1

#include "host_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The header checks every host batch over ITB records shares
 * (include/pom_gc.h pom_gc_scan_batch).  0 and the block a record stands for
 * -- its stored payload, whether that is an LZO1X stream, the decode capacity
 * h.zlen - 264 (0 when stored uncompressed), adepth and h.entries -- or
 * -EINVAL. */
struct pom_walk_block {
    const uint8_t *src;
    size_t src_len, cap;
    uint8_t is_lzo, adepth;
    int32_t entries;
};
int pom_itb_walk_header(const uint8_t *rec, size_t rec_len, struct pom_walk_block *w);

/* A chunk's records, kept until the caller has placed them (pad: the records
 * start 16-byte aligned); the walks' sinks and the gets' link them at bufs. */
struct pom_walk_buf {
    struct pom_walk_buf *next;
    uint64_t pad;
    uint8_t bytes[];
};
void pom_walk_bufs_free(struct pom_walk_buf **bufs);

/* The stable counting sort the request batches group with: request r belongs
 * to group key[r] when that is below m, else to none.  Group k's requests are
 * ids[first[k] ... first[k + 1]), in the caller's order; first has m + 1
 * entries.  Returns first[m]. */
size_t pom_group_requests(const size_t *key, size_t nreq, size_t m, size_t *first, size_t *ids);

/* The two kinds.  Lookup: namelen <= 255 and the name inside the blob; results
 * err, nr, depth and a 136-byte record.  Get: POM_KV_STR set, sklen <= 320 and
 * the key inside the blob; results err, nr, depth, len, lease and a record of
 * at most 364 bytes.  Unlink (include/pom_unlink.h): the lookup's request and
 * record; results err, nr, depth and `what`, in RW_LEN's place. */
extern const struct req_spec pom_req_lookup, pom_req_kvget, pom_req_unlink;

/* One call's requests and results as its chunks see them (pom_lookup_chunked,
 * pom_kvget_chunked): block b's requests are req[req_ids[k]] for k in
 * [req_first[b], req_first[b + 1]).  Per request the kind's words and lease
 * in the caller's request order, a fixed record at fixed + rec_fixed * r;
 * variable records come back packed per chunk, in the chunk's request order,
 * into a buffer linked at bufs, with recs[r] pointing at request r's (NULL
 * without records, or for length 0). */
struct pom_req_sink {
    const struct req_spec *spec;
    const uint8_t *is_lzo;          /* per block, as pom_walk_sink */
    const size_t *cap;
    const uint8_t *adepth;
    const size_t *req_first, *req_ids;
    const uint8_t *req;             /* POM_REQ_SIZE each */
    const uint8_t *blob;
    size_t blob_len;
    int records;                    /* variable records: 0 is lengths only, no emit launch and none comes back */
    uint32_t *word[RW_N];           /* err (an int array), nr, depth, len: those the kind has */
    uint64_t *lease;
    uint8_t *fixed;
    const uint8_t **recs;
    int32_t *status;                /* per block: 0 once its chunk is delivered */
    struct pom_walk_buf *bufs;
};

/* Block b's requests, and the blob bytes they read added to *blob_bytes: none
 * for a request refused by the kind's rule or not all inside the call's blob. */
size_t pom_req_block(const struct pom_req_sink *K, size_t b, size_t *blob_bytes);

/* The chunk's requests into staging h, in block order and then the block's
 * own, renumbered to the chunk's ITB indices, the blob repacked in that order;
 * a refused request gets no blob byte and the offset 0xFFFFFFFF, outside the
 * chunk's blob as it was outside the caller's.  -1: too many requests or blob
 * bytes for the kernels' u32. */
int pom_req_stage(const struct layout *L, uint8_t *h, const struct pom_req_sink *K);
/* The chunk's results in h into the caller's request order; its variable
 * records lie packed in bytes[0, packed). */
void pom_req_scatter(const struct layout *L, const uint8_t *h, struct pom_req_sink *K, const uint8_t *bytes,
                     size_t packed);

/* The two halves a request batch has around its pom_*_chunked call.  The ITBs
 * some request reaches and that pass the header checks go to the GPU, k = 0
 * ... m - 1 in the order of their first GPU-bound request, with their requests
 * gathered behind G.req_first[k].  The other requests are decided here:
 * -EINVAL for itb >= n or a bad header, else -ESPLIT when itbid_check is set
 * and the request's first u64 does not belong to the ITB (mds/itb.c:1754-1755).
 * A GPU-bound request reads LZO_E_ERROR until its chunk delivers. */
struct pom_req_batch {
    size_t m, ngpu;
    size_t *key, *first, *ids, *slen, *cap;
    const uint8_t **src, **recs;
    uint8_t *flags;
    int32_t *st;
    struct pom_req_sink G;          /* set up but for fixed and records */
};
/* Zeroes the results, selects and groups.  word[] and lease as in the sink.
 * LZO_E_OK or LZO_E_OUT_OF_MEMORY; pom_req_finish follows either way. */
int pom_req_begin(struct pom_req_batch *W, const struct req_spec *Q, const uint8_t *const *rec,
                  const size_t *rec_len, size_t n, int itbid_check, const void *req, size_t nreq,
                  const uint8_t *blob, size_t blob_len, uint32_t *const word[RW_N], uint64_t *lease);
/* rc: pom_req_begin's or the chunked call's.  After a delivered batch a miss
 * on an ITB that has just split becomes -ESPLIT (mds/itb.c:2030-2033).  Frees
 * everything and returns rc. */
int pom_req_finish(struct pom_req_batch *W, int rc, const uint8_t *const *rec);

#ifdef __cplusplus
}
#endif

#endif
