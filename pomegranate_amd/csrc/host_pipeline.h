/* host_pipeline.h -- the chunk pipeline of the host batches (lzo_host.c) as
 * the operations that run through it see it (the codec's in lzo_host.c, the
 * record operations' in host_records.c).  Internal to liblzo_mi355x.so. */
#ifndef POM_HOST_PIPELINE_H
#define POM_HOST_PIPELINE_H 1

#include <hip/hip_runtime_api.h>

#include "batch_split.h"
#include "host_layout.h"
#include "lzo_mi355x_kernels.h"

/* A staging slot: one stream with its device and pinned host buffers (grown
 * on demand; a host batch's chunks keep them bounded, see kChunkBudget). */
struct slot {
    hipStream_t stream;
    uint8_t *dmem;
    size_t dcap;
    uint8_t *hmem;
    size_t hcap;
};

struct tctx;
struct hbatch;

/* One operation of the host batches.  The pipeline (dev_run) cuts a device's
 * blocks into chunks and, per chunk, on the chunk's slot:
 *   layout                              where everything lies
 *   stage, H2D of [0, o_dst), kernels   queued on the slot's stream, nothing waited for
 *   collect                             once the kernels are done: the D2H that needed their results
 *   unpack                              once that is back: into the caller's arrays or sink
 * and knows nothing else about it. */
struct chunk_ops {
    const char *label;          /* debug key host_timing */
    int largest_first;          /* the compress batches' order: largest blocks first, chunks delivered as they finish */
    /* the capacity the kernels get for block b */
    size_t (*cap)(const struct hbatch *B, size_t b);
    /* what block b adds to its chunk beyond src_len + cap (requests, their results), or NULL */
    size_t (*extra_cost)(const struct hbatch *B, size_t b);
    /* block b's results as they read if its chunk is never delivered, beyond status[b], or NULL */
    void (*unreached)(const struct hbatch *B, size_t b);
    /* the chunk of blocks ids[0, nb), of which the first nlzo are LZO streams */
    void (*layout)(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B);
    /* the chunk's inputs into the pinned staging h; -1: the chunk cannot run */
    int (*stage)(const struct layout *L, uint8_t *h, const struct hbatch *B);
    /* queues the kernels, and the D2H that needs no result of theirs to be sized */
    int (*kernels)(struct slot *S, const struct layout *L, const struct hbatch *B);
    /* the kernels are done: queues the remaining D2H and returns its bytes in *packed */
    int (*collect)(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed);
    /* everything is back in S->hmem */
    int (*unpack)(struct slot *S, const struct layout *L, const struct hbatch *B);
};

/* One host batch: the caller's arrays, the capacities the kernels use, and
 * the plan (device split, largest-first order).  A caller fills ops, src,
 * src_len, status and what its operation reads of dst, dst_len, is_lzo, sink
 * and the callbacks; pom_host_batch fills the rest. */
struct hbatch {
    const struct chunk_ops *ops;
    const uint8_t *const *src;
    const size_t *src_len;
    uint8_t *const *dst;
    size_t *dst_len;
    int *status;
    const uint8_t *is_lzo;  /* per block, or NULL: every block is an LZO stream.  Given, a chunk's stored
                             * blocks ride along behind its LZO blocks */
    void *sink;             /* the operation's own inputs and results */
    pom_chunk_fn on_chunk;  /* called with each delivered chunk's block ids, or NULL */
    pom_chunk_fn pre_chunk; /* called with a chunk's block ids before its inputs are staged */
    void *cb_ctx;
    const size_t *cap;
    const size_t *cost;
    size_t budget;
    struct pom_plan plan;
    const int *devs;        /* plan device d runs on HIP device devs[d] */
    struct tctx *t;
    uint32_t enc_lds_max;   /* chunks of at most this many blocks: LDS dictionaries */
    int nslots;             /* chunks in flight per device (<= kSlots) */
    int ooo;                /* deliver chunks in completion order (compress batches) */
    int small_first;        /* smallest blocks first (every other batch) */
};

/* Runs the batch of nblocks blocks; LZO_E_OK, or an LZO_E_ code with the
 * undelivered blocks' status LZO_E_ERROR. */
int pom_host_batch(struct hbatch *B, size_t nblocks);

/* Pack/unpack copies between caller buffers and the pinned staging, split over
 * threads once they are large. */
struct copy_job {
    uint8_t *dst;
    const uint8_t *src;
    size_t len;
};
void pom_copy_jobs(const struct copy_job *jobs, size_t n);

/* The stage every operation starts with: per block its offsets, src_len and
 * capacity (0 for a stored block, which takes no output slot) into the
 * layout's shared arrays, and its input bytes behind o_src.  Returns 0 (an
 * operation with nothing else to stage has it as its stage). */
int pom_stage_inputs(const struct layout *L, uint8_t *h, const struct hbatch *B);

/* Queues the decoders over the chunk's LZO blocks: out_len and status at
 * o_outlen and o_status, the decoded bytes in the slots behind o_dst.  concat:
 * each block is a run of consecutive streams (the hvfs_fwritev column layout). */
int pom_decode_lzo_blocks(struct slot *S, const struct layout *L, int concat);

#endif
