/* host_pipeline.h -- the chunk pipeline of the host batches (lzo_host.c) as
 * the operations that run through it see it (the codec's in lzo_host.c, the
 * record operations' in host_records.c), and the per-thread, per-device
 * contexts (host_ctx.c) that it and the single calls (host_single.c) run on.
 * Internal to liblzo_mi355x.so. */
#ifndef POM_HOST_PIPELINE_H
#define POM_HOST_PIPELINE_H 1

#include <time.h>

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

/* A host thread's resources on one device (host_ctx.c): kSlots slots, so that
 * several chunks are in flight (copies and kernels of some while others are
 * packed or unpacked on the host). */
enum { kSlots = 4, kMaxDev = 16 };

struct dctx {
    int ready;
    struct slot s[kSlots];
};

struct tctx;
struct hbatch;

/* The calling thread's contexts (freed at its exit); NULL without a usable GPU. */
struct tctx *pom_tctx_get(void);
/* Its context on `device`, which must be its current device. */
struct dctx *pom_dctx_get(struct tctx *t, int device);
/* At least dbytes of device and hbytes of pinned host staging in the slot. */
int pom_slot_reserve(struct slot *t, size_t dbytes, size_t hbytes);
/* The slot lone single calls use: slot 0 on the calling thread's current device. */
struct slot *pom_single_slot(void);

/* The latency decoder (lzo1x_decode_lat.hip: the whole GPU on a few blocks)
 * over nb blocks, when there are at most kLatGroup of them, each of at least
 * sc_lat_min (debug key, default 2048) compressed bytes, and their scratch
 * fits: one pipeline, the blocks side by side in every kernel, on the
 * device's shared scratch.  src_off, z, dst_off and cap are host arrays; the
 * fallback list (count at fb, ids) must be zero on the stream before it.
 * Blocks it hands over get status LZO_MI355X_DEC_PENDING: the caller runs the
 * exact decoder behind it.  1 launched, 0 not eligible (nothing launched: the
 * caller's other decoders), -1 on a launch error. */
enum { kLatGroup = 8 };
int pom_lat_decode(const uint8_t *src, const uint64_t *src_off, const uint32_t *z, uint8_t *dst,
                   const uint64_t *dst_off, const uint32_t *cap, uint32_t nb, uint32_t *out_len,
                   int32_t *status, uint32_t *fb, uint32_t *ids, hipStream_t s);

static inline double pom_now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

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
