/*
 * lzo_host.c -- the batch API of lzo_mi355x.h on top of the HIP kernels, in C
 * like the reference: the device-resident entry points, and the host batches'
 * chunk pipeline with the codec's three operations.  Every codec call runs on
 * the GPU; there is no CPU codec in this library.  The threads' contexts are
 * host_ctx.c's, the minilzo.h single calls host_single.c's, the record
 * operations host_records.c's, the debug keys host_debug.c's.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <hip/hip_runtime_api.h>

#include "host_pipeline.h"
#include "lzo_mi355x.h"
#include "minilzo.h"

#define ALIGN_UP(x, a) POM_ALIGN_UP(x, a)

size_t lzo_mi355x_worst_compress(size_t n)
{
    return n + n / 16 + 64 + 3;
}

/* ------------------------------------------------------------------------ */
/* Device-resident batch entry points                                       */
/* ------------------------------------------------------------------------ */
int lzo_mi355x_compress_dev(const uint8_t *src, const uint64_t *src_off,
                            const uint32_t *src_len, uint8_t *dst,
                            const uint64_t *dst_off, const uint32_t *dst_cap,
                            uint32_t *out_len, int32_t *status, uint32_t nblocks,
                            void *scratch, void *stream)
{
    /* blocks up to 16 MiB: the throughput encoder; larger ones are left
     * pending for the general encoder, whose other workgroups exit at once */
    hipStream_t s = (hipStream_t)stream;
    if (nblocks == 0)
        return 0;
    if (lzo_mi355x_launch_compress_fast(src, src_off, src_len, dst, dst_off, dst_cap, out_len,
                                        status, nblocks, scratch,
                                        scratch ? lzo_mi355x_compress_scratch(nblocks) : 0, s) != 0)
        return -1;
    return lzo_mi355x_launch_compress(src, src_off, src_len, dst, dst_off, dst_cap, out_len,
                                      status, nblocks, 1, s);
}

/* Scratch (256-byte aligned parts):
 *   [0]     fallback count u32
 *   [256]   op-set pool counters (LZO_MI355X_FAST_POOL_BYTES)
 *   then    op-set return ring, u64 per set
 *   then    the fast decoder's fallback list, u32 per block
 *   then    (more blocks than resident workgroups) the start order, u32 per block
 *   then    the op-slot sets, one per workgroup resident at once
 * Only the fallback list and the start order grow with nblocks (4 bytes a
 * block each). */
enum { SCR_POOL = 256, SCR_RING = SCR_POOL + LZO_MI355X_FAST_POOL_BYTES };

static size_t scr_sets(uint32_t nblocks)
{
    const uint32_t r = lzo_mi355x_fast_resident_blocks();
    return nblocks < r ? nblocks : r;
}

static size_t scr_head(uint32_t nblocks)
{
    return ALIGN_UP(SCR_RING + 8 * scr_sets(nblocks), 256);
}

static size_t scr_order_bytes(uint32_t nblocks)
{
    return nblocks > lzo_mi355x_fast_resident_blocks() ? ALIGN_UP(4 * (size_t)nblocks, 256) : 0;
}

static size_t scr_order_off(uint32_t nblocks)
{
    return scr_head(nblocks) + ALIGN_UP(4 * (size_t)nblocks, 256);
}

static size_t scr_ops_off(uint32_t nblocks)
{
    return scr_order_off(nblocks) + scr_order_bytes(nblocks);
}

size_t lzo_mi355x_decompress_scratch(uint32_t nblocks)
{
    return scr_ops_off(nblocks) + scr_sets(nblocks) * lzo_mi355x_fast_ops_bytes_per_block();
}

/* Which throughput decoder a batch uses: the op-set decoder
 * (lzo1x_decode_fast.hip: 16 blocks per CU) or the windowed one
 * (lzo1x_decode_win.hip: 2 blocks per CU, a 64 KiB LDS output ring, never
 * reads its own output back).  Debug key decoder=fast|win forces one;
 * single calls always use the windowed one (host_single.c). */
enum { DEC_FAST = 0, DEC_WIN = 1 };
static int use_win_decoder(uint32_t nblocks)
{
    char buf[16];
    const char *e = pom_dbg_str("decoder", buf, sizeof buf);
    if (e)
        return strcmp(e, "win") == 0 ? DEC_WIN : DEC_FAST;
    /* default: the windowed decoder while the batch fits two workgroups per
     * CU (one round; lone blocks decode 1.3-1.5x faster there), the op-set
     * decoder for larger batches (16 blocks per CU) */
    const uint32_t cus = lzo_mi355x_fast_resident_blocks() / 16u;
    return nblocks <= 2u * (cus ? cus : 256u);
}

/* Throughput decoder over the whole batch, then the exact decoder over the blocks
 * it refused (malformed input, capacity/lookbehind errors, pathological
 * streams).  Without scratch every block takes the exact decoder.
 * unchecked: the exact decoder follows the unchecked lzo1x_decompress (the
 * fast decoder only ever finishes streams on which both agree). */
static int decompress_dev(const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                          uint8_t *dst, const uint64_t *dst_off, const uint32_t *dst_cap,
                          uint32_t *out_len, int32_t *status, uint32_t nblocks, void *scratch,
                          int unchecked, hipStream_t s)
{
    if (nblocks == 0)
        return 0;
    if (!scratch)
        return lzo_mi355x_launch_decompress_exact(src, src_off, src_len, dst, dst_off, dst_cap,
                                                  out_len, status, NULL, NULL, nblocks, nblocks,
                                                  unchecked, s);
    uint8_t *scr = scratch;
    const uint32_t nsets = (uint32_t)scr_sets(nblocks);
    uint32_t *fb = (uint32_t *)scr, *ids = (uint32_t *)(scr + scr_head(nblocks));
    if (use_win_decoder(nblocks)) {
        /* the windowed decoder: no op sets,
         * only the fallback list */
        if (hipMemsetAsync(scr, 0, 256, s) != hipSuccess)
            return -1;
        if (lzo_mi355x_launch_decompress_win(src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, fb,
                                             ids, nblocks, s) != 0)
            return -1;
    } else {
        if (hipMemsetAsync(scr, 0, SCR_RING + 8 * (size_t)nsets, s) != hipSuccess)
            return -1;
        if (lzo_mi355x_launch_decompress_fast(src, src_off, src_len, dst, dst_off, dst_cap,
                                              out_len, status, fb, ids,
                                              (uint32_t *)(scr + SCR_POOL), scr + SCR_RING,
                                              scr + scr_ops_off(nblocks), nsets, nblocks,
                                              scr_order_bytes(nblocks)
                                                  ? (uint32_t *)(scr + scr_order_off(nblocks))
                                                  : NULL,
                                              s) != 0)
            return -1;
    }
    const uint32_t ngrid = nblocks < 512 ? nblocks : 512;
    return lzo_mi355x_launch_decompress_exact(src, src_off, src_len, dst, dst_off, dst_cap,
                                              out_len, status, fb, ids, ngrid, nblocks, unchecked,
                                              s);
}

int lzo_mi355x_decompress_dev(const uint8_t *src, const uint64_t *src_off,
                              const uint32_t *src_len, uint8_t *dst,
                              const uint64_t *dst_off, const uint32_t *dst_cap,
                              uint32_t *out_len, int32_t *status, uint32_t nblocks,
                              void *scratch, void *stream)
{
    return decompress_dev(src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, nblocks,
                          scratch, 0, (hipStream_t)stream);
}

int lzo_mi355x_decompress_fallbacks(const void *scratch, uint32_t *count, void *stream)
{
    /* the fallback count at scratch byte 0, once the stream has reached it */
    if (!scratch || !count)
        return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(count, scratch, sizeof *count, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return -1;
    return 0;
}

int lzo_mi355x_decoded_length_dev(const uint8_t *src, const uint64_t *src_off,
                                  const uint32_t *src_len, uint32_t *out_len,
                                  int32_t *status, uint32_t nblocks, void *stream)
{
    return lzo_mi355x_launch_decoded_length(src, src_off, src_len, out_len, status, nblocks, NULL,
                                            0xFFFFFFFFu, (hipStream_t)stream);
}

/* ------------------------------------------------------------------------ */
/* Host-resident batches: pack -> H2D -> kernels -> D2H -> unpack           */
/* ------------------------------------------------------------------------ */
/* Pack/unpack copies between caller buffers and the pinned staging: split
 * over up to kCopyThreads threads by bytes once a batch is large enough for
 * one memcpy stream to be the bottleneck (the host side of config C5). */
struct copy_range {
    const struct copy_job *jobs;
    size_t lo, hi;
};

enum { kCopyThreads = 8 };
static const size_t kCopyParallelBytes = 8u << 20;

static void *copy_worker(void *arg)
{
    const struct copy_range *r = arg;
    for (size_t i = r->lo; i < r->hi; i++)
        if (r->jobs[i].len)
            memcpy(r->jobs[i].dst, r->jobs[i].src, r->jobs[i].len);
    return NULL;
}

void pom_copy_jobs(const struct copy_job *jobs, size_t n)
{
    size_t total = 0;
    for (size_t i = 0; i < n; i++)
        total += jobs[i].len;
    struct copy_range r[kCopyThreads];
    pthread_t th[kCopyThreads];
    int nt = total >= kCopyParallelBytes && n > 1 ? kCopyThreads : 1;
    /* contiguous job ranges of about total / nt bytes each */
    size_t i = 0, acc = 0;
    int k = 0;
    for (; k < nt && i < n; k++) {
        r[k].jobs = jobs;
        r[k].lo = i;
        const size_t goal = total / (size_t)nt * (size_t)(k + 1);
        while (i < n && (acc < goal || k == nt - 1)) {
            acc += jobs[i].len;
            i++;
        }
        r[k].hi = i;
    }
    int started = 0;
    for (int j = 1; j < k; j++)
        if (pthread_create(&th[j], NULL, copy_worker, &r[j]) == 0)
            started |= 1 << j;
        else
            copy_worker(&r[j]);
    if (k > 0)
        copy_worker(&r[0]);
    for (int j = 1; j < k; j++)
        if (started & (1 << j))
            pthread_join(th[j], NULL);
}

void pom_copy_parallel(uint8_t *const *dst, const uint8_t *const *src, const size_t *len, size_t n)
{
    struct copy_job *jobs = malloc(n * sizeof(*jobs));
    if (!jobs) {
        for (size_t i = 0; i < n; i++)
            if (len[i])
                memcpy(dst[i], src[i], len[i]);
        return;
    }
    for (size_t i = 0; i < n; i++) {
        jobs[i].dst = dst[i];
        jobs[i].src = src[i];
        jobs[i].len = len[i];
    }
    pom_copy_jobs(jobs, n);
    free(jobs);
}

/* Staging layout of one codec chunk (identical on host and device, so one copy
 * each way; pom_layout_codec):
 *   [src_off u64][dst_off u64][src_len u32][dst_cap u32][out_len u32][status i32]
 *   [packed offset u64]
 *   [src bytes, 16-B aligned per block][dst bytes, 16-B aligned per block]
 *   [device only: scratch of the kernels the batch runs][device only: packed output]
 * The kernels write each block into its capacity-sized dst slot; only the
 * produced bytes come back, packed (pack kernel), in one D2H copy into the
 * host's dst region.  Block i of the chunk is the caller's block ids[i]. */
int pom_stage_inputs(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    uint64_t *so = (uint64_t *)(h + L->o_srcoff);
    uint64_t *dof = (uint64_t *)(h + L->o_dstoff);
    uint32_t *sl = (uint32_t *)(h + L->o_srclen);
    uint32_t *dc = (uint32_t *)(h + L->o_dstcap);
    size_t s = 0, d = 0;
    struct copy_job *jobs = malloc(L->nb * sizeof(*jobs));
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        so[i] = s;
        dof[i] = d;
        sl[i] = (uint32_t)B->src_len[b];
        dc[i] = i < L->nlzo ? (uint32_t)B->cap[b] : 0;
        if (jobs) {
            jobs[i].dst = h + L->o_src + s;
            jobs[i].src = B->src[b];
            jobs[i].len = B->src_len[b];
        } else if (B->src_len[b]) {
            memcpy(h + L->o_src + s, B->src[b], B->src_len[b]);
        }
        s += ALIGN_UP(B->src_len[b], 16);
        d += ALIGN_UP((size_t)dc[i], 16);
    }
    if (jobs) {
        pom_copy_jobs(jobs, L->nb);
        free(jobs);
    }
    return 0;
}

/* debug key host_timing=1: per-batch and per-chunk wall times on stderr (diagnostic) */
#define g_timing (pom_dbg_int("host_timing", 0) == 1)

/* The chunk's blocks as the kernels take them: pointers into the device staging. */
struct dev_blocks {
    const uint8_t *src;
    uint8_t *dst;
    const uint64_t *so, *dof;
    const uint32_t *sl, *dc;
    uint32_t *ol;
    int32_t *st;
};

static struct dev_blocks dev_blocks(const struct slot *S, const struct layout *L)
{
    uint8_t *d = S->dmem;
    const struct dev_blocks D = {d + L->o_src, d + L->o_dst, (const uint64_t *)(d + L->o_srcoff),
                                 (const uint64_t *)(d + L->o_dstoff), (const uint32_t *)(d + L->o_srclen),
                                 (const uint32_t *)(d + L->o_dstcap), (uint32_t *)(d + L->o_outlen),
                                 (int32_t *)(d + L->o_status)};
    return D;
}

int pom_decode_lzo_blocks(struct slot *S, const struct layout *L, int concat)
{
    const struct dev_blocks D = dev_blocks(S, L);
    const uint32_t n = (uint32_t)L->nlzo;
    if (concat)
        return lzo_mi355x_launch_decompress_concat(D.src, D.so, D.sl, D.dst, D.dof, D.dc, D.ol, D.st, n, S->stream);
    return decompress_dev(D.src, D.so, D.sl, D.dst, D.dof, D.dc, D.ol, D.st, n, S->dmem + L->o_scr, 0, S->stream);
}

/* ------------------------------------------------------------------------ */
/* The codec's operations: compress, decompress, decompress_concat          */
/* ------------------------------------------------------------------------ */
static size_t compress_cap(const struct hbatch *B, size_t b)
{
    return lzo_mi355x_worst_compress(B->src_len[b]);
}

static size_t decompress_cap(const struct hbatch *B, size_t b)
{
    return B->dst_len[b];
}

static void codec_unreached(const struct hbatch *B, size_t b)
{
    B->dst_len[b] = 0;
}

static void compress_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    (void)nlzo;
    pom_layout_codec(L, ids, nb, B->src_len, B->cap, lzo_mi355x_compress_scratch((uint32_t)nb));
}

static void decompress_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    (void)nlzo;
    pom_layout_codec(L, ids, nb, B->src_len, B->cap, lzo_mi355x_decompress_scratch((uint32_t)nb));
}

/* The D2H of the lengths and codes, queued behind the kernels. */
static int codec_lengths_back(struct slot *S, const struct layout *L, int rc)
{
    if (rc != 0)
        return -1;
    return hipMemcpyAsync(S->hmem + L->u.codec.res_off, S->dmem + L->u.codec.res_off, L->u.codec.res_bytes,
                          hipMemcpyDeviceToHost, S->stream) == hipSuccess ? 0 : -1;
}

static int compress_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    /* lzo_mi355x_compress_dev, with the general encoder's pass only when a
     * block of the chunk needs it: that kernel's workgroups take 64 KB of
     * LDS each, and behind the other slots' encoders a pass with nothing to
     * do waited ~0.75 ms for LDS to free up (C5 trace) */
    const struct dev_blocks D = dev_blocks(S, L);
    const uint32_t nb = (uint32_t)L->nb;
    void *scr = nb <= B->enc_lds_max ? NULL : S->dmem + L->o_scr;
    int big = 0;
    for (size_t i = 0; i < L->nb; i++)
        big |= B->src_len[L->ids[i]] > LZO_MI355X_FAST_MAX_N;
    int rc = lzo_mi355x_launch_compress_fast(D.src, D.so, D.sl, D.dst, D.dof, D.dc, D.ol, D.st, nb, scr,
                                             scr ? lzo_mi355x_compress_scratch(nb) : 0, S->stream);
    if (rc == 0 && big)
        rc = lzo_mi355x_launch_compress(D.src, D.so, D.sl, D.dst, D.dof, D.dc, D.ol, D.st, nb, 1, S->stream);
    return codec_lengths_back(S, L, rc);
}

static int decompress_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    (void)B;
    /* a chunk of a few large blocks: the latency decoder (pom_lat_decode takes
     * the host side's arrays), its fallback list at the scratch's head zeroed
     * first, with the exact decoder behind it for the blocks it hands over;
     * every other chunk: the throughput decoders */
    const struct dev_blocks D = dev_blocks(S, L);
    const uint8_t *h = S->hmem;
    const uint32_t nb = (uint32_t)L->nb;
    uint8_t *scr = S->dmem + L->o_scr;
    uint32_t *fb = (uint32_t *)scr, *ids = (uint32_t *)(scr + scr_head(nb));
    int rc = hipMemsetAsync(scr, 0, 256, S->stream) == hipSuccess ? 0 : -1;
    if (rc == 0)
        rc = pom_lat_decode(D.src, (const uint64_t *)(h + L->o_srcoff), (const uint32_t *)(h + L->o_srclen), D.dst,
                            (const uint64_t *)(h + L->o_dstoff), (const uint32_t *)(h + L->o_dstcap), nb, D.ol,
                            D.st, fb, ids, S->stream);
    if (rc > 0)
        rc = lzo_mi355x_launch_decompress_exact(D.src, D.so, D.sl, D.dst, D.dof, D.dc, D.ol, D.st, fb, ids, nb, nb,
                                                0, S->stream);
    else if (rc == 0)
        rc = pom_decode_lzo_blocks(S, L, 0);
    return codec_lengths_back(S, L, rc);
}

static int concat_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    (void)B;
    return codec_lengths_back(S, L, pom_decode_lzo_blocks(S, L, 1));
}

/* The lengths are back: the pack kernel and the D2H of exactly the produced bytes. */
static int codec_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed_out)
{
    (void)B;
    uint8_t *d = S->dmem, *h = S->hmem;
    hipStream_t s = S->stream;
    const uint32_t *hol = (const uint32_t *)(h + L->o_outlen);
    const uint32_t *hdc = (const uint32_t *)(h + L->o_dstcap);
    uint64_t *poff = (uint64_t *)(h + L->u.codec.o_poff);
    size_t packed = 0;
    for (size_t i = 0; i < L->nb; i++) {
        poff[i] = packed;
        packed += ALIGN_UP((size_t)(hol[i] < hdc[i] ? hol[i] : hdc[i]), 16);
    }
    if (packed &&
        (hipMemcpyAsync(d + L->u.codec.o_poff, poff, 8 * L->nb, hipMemcpyHostToDevice, s) != hipSuccess ||
         lzo_mi355x_launch_pack(d + L->o_dst, (const uint64_t *)(d + L->o_dstoff),
                                (const uint32_t *)(d + L->o_outlen),
                                (const uint32_t *)(d + L->o_dstcap),
                                (const uint64_t *)(d + L->u.codec.o_poff), d + L->u.codec.o_pack,
                                (uint32_t)L->nb, s) != 0 ||
         hipMemcpyAsync(h + L->o_dst, d + L->u.codec.o_pack, packed, hipMemcpyDeviceToHost, s) !=
             hipSuccess))
        return -1;
    *packed_out = packed;
    return 0;
}

/* Lengths, codes and bytes into the caller's arrays. */
static int codec_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const uint8_t *h = S->hmem;
    const uint32_t *hol = (const uint32_t *)(h + L->o_outlen);
    const int32_t *hst = (const int32_t *)(h + L->o_status);
    const uint64_t *poff = (const uint64_t *)(h + L->u.codec.o_poff);
    struct copy_job *jobs = malloc(L->nb * sizeof(*jobs));
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        const size_t n = hol[i] < B->cap[b] ? hol[i] : B->cap[b];
        if (jobs) {
            jobs[i].dst = B->dst[b];
            jobs[i].src = h + L->o_dst + poff[i];
            jobs[i].len = n;
        } else if (n) {
            memcpy(B->dst[b], h + L->o_dst + poff[i], n);
        }
        B->dst_len[b] = hol[i];
        B->status[b] = hst[i];
    }
    if (jobs) {
        pom_copy_jobs(jobs, L->nb);
        free(jobs);
    }
    return 0;
}

/* A host batch is cut into chunks of at most kChunkBudget bytes of input plus
 * output capacity (a larger block is a chunk of its own), pipelined through
 * the device's kSlots slots: chunk k is staged and its copies and kernels are
 * queued as soon as chunk k - kSlots has been waited for and unpacked, so the
 * copies, the kernels of several chunks and the host-side packing overlap.
 * The first chunk gets a quarter of the budget: for compress batches it holds
 * the largest blocks, whose long serial LZ chains start while the rest of the
 * batch is still being copied up; decode batches go smallest first (dev_run).  Debug key chunk_mb overrides the budget. */
static const size_t kChunkBudget = (size_t)128 << 20;
/* compress batches: their chains are long (a 536 KB ITB is ~6 ms on one CU),
 * so their chunks are delivered in completion order (hbatch.ooo): a chunk of
 * smaller blocks that finishes while the largest blocks' chunk still runs
 * frees its slot for the next chunk and is handed to on_chunk (the append
 * file) at once.  In launch order, 128 MiB chunks left the slots waiting on
 * the first chunk (C5 compress 13.4-14.7 against 16.4-17.7 GiB/s with 256
 * MiB); in completion order they compress as fast and the fused write gains
 * (profiles/r04e/c5_ooo/) */
static const size_t kChunkBudgetCompress = (size_t)128 << 20;
static const size_t kChunkBlocks = (size_t)1 << 20;
/* below this many bytes per device a batch stays on one device */
static const size_t kSplitMinBytes = (size_t)64 << 20;

static const struct chunk_ops compress_ops = {
    "compress", 1, compress_cap, NULL, codec_unreached, compress_layout,
    pom_stage_inputs, compress_kernels, codec_collect, codec_unpack};
static const struct chunk_ops decompress_ops = {
    "decompress", 0, decompress_cap, NULL, codec_unreached, decompress_layout,
    pom_stage_inputs, decompress_kernels, codec_collect, codec_unpack};
static const struct chunk_ops concat_ops = {
    "decompress", 0, decompress_cap, NULL, codec_unreached, decompress_layout,
    pom_stage_inputs, concat_kernels, codec_collect, codec_unpack};

/* Chunk on slot S: inputs into pinned staging, H2D, kernels, D2H of what needs
 * no sizing -- all queued on the slot's stream, nothing waited for. */
static int chunk_launch(struct slot *S, struct layout *L, const struct hbatch *B)
{
    if (pom_slot_reserve(S, L->dtotal, L->htotal) != 0)
        return -1;
    const double t0 = g_timing ? pom_now_ms() : 0;
    if (B->ops->stage(L, S->hmem, B) != 0)
        return -1;
    if (g_timing)
        fprintf(stderr, "  chunk n=%zu: fill %.2f ms (%zu B)\n", L->nb, pom_now_ms() - t0, L->htotal);
    if (hipMemcpyAsync(S->dmem, S->hmem, L->o_dst, hipMemcpyHostToDevice, S->stream) != hipSuccess)
        return -1;
    return B->ops->kernels(S, L, B);
}

/* Waits for the chunk's kernels, then queues the D2H that needed their
 * results (codec chunks: the pack kernel and exactly the produced bytes).
 * Once per chunk: the delivery of the chunk before may have done it already. */
static int chunk_collect(struct slot *S, struct layout *L, const struct hbatch *B)
{
    if (L->collected)
        return 0;
    if (hipStreamSynchronize(S->stream) != hipSuccess || B->ops->collect(S, L, B, &L->packed) != 0)
        return -1;
    L->collected = 1;
    return 0;
}

/* Waits for the chunk's results and hands them to the caller's arrays or
 * sink.  The next chunk (nS/nL, may be NULL) is collected first (its kernels
 * waited for, its D2H queued), so that its copy runs while this one is
 * unpacked.  (Polling it with hipStreamQuery instead never found it done
 * here.) */
static int chunk_deliver(struct slot *S, struct layout *L, const struct hbatch *B,
                         struct slot *nS, struct layout *nL)
{
    const double t0 = g_timing ? pom_now_ms() : 0;
    if (chunk_collect(S, L, B) != 0 || hipStreamSynchronize(S->stream) != hipSuccess)
        return -1;
    if (nS && chunk_collect(nS, nL, B) != 0)
        return -1;
    const double t1 = g_timing ? pom_now_ms() : 0;
    const int rc = B->ops->unpack(S, L, B);
    if (g_timing)
        fprintf(stderr, "  deliver n=%zu: wait %.2f (%zu B) unpack %.2f ms\n", L->nb, t1 - t0,
                L->packed, pom_now_ms() - t1);
    return rc;
}

/* ids[0, nb): the LZO blocks to the front (any order inside either part).
 * Returns how many there are. */
static size_t lzo_blocks_first(size_t *ids, size_t nb, const uint8_t *is_lzo)
{
    size_t lo = 0, hi = nb;
    while (lo < hi) {
        if (is_lzo[ids[lo]]) {
            lo++;
        } else {
            const size_t t = ids[lo];
            ids[lo] = ids[--hi];
            ids[hi] = t;
        }
    }
    return lo;
}

/* Completion order (compress batches, hbatch.ooo): the first live slot whose
 * stream is done, polling every 20 us; a failed stream counts as done (its
 * delivery reports the error). */
static int wait_any_done(struct dctx *c, const int *live, int nslots)
{
    for (;;) {
        for (int i = 0; i < nslots; i++)
            if (live[i] && hipStreamQuery(c->s[i].stream) != hipErrorNotReady)
                return i;
        const struct timespec ts = {0, 20000};
        nanosleep(&ts, NULL);
    }
}

static int dev_run(void *arg, int d)
{
    const struct hbatch *B = arg;
    const int device = B->devs[d];
    int prev_dev = -1;
    if (hipGetDevice(&prev_dev) != hipSuccess)
        return -1;
    if (prev_dev != device && hipSetDevice(device) != hipSuccess)
        return -1;
    int rc = 0;
    struct dctx *c = pom_dctx_get(B->t, device);
    if (!c) {
        rc = -1;
    } else {
        const size_t *ids = B->plan.by_dev + B->plan.dev_off[d];
        const size_t nids = B->plan.dev_off[d + 1] - B->plan.dev_off[d];
        /* decode batches go smallest first: a decoded chunk's D2H copy is the
         * long pole (PCIe), and the first chunk's kernels -- the smallest
         * blocks -- finish early, so the copies start early and run back to
         * back while the chunks of the largest blocks decode (debug key
         * dec_small_first=0: largest first, as compress batches) */
        size_t *rev = NULL;
        if (B->small_first && nids > 1 && (rev = malloc(nids * sizeof(*rev))) != NULL) {
            for (size_t i = 0; i < nids; i++)
                rev[i] = ids[nids - 1 - i];
            ids = rev;
        }
        /* chunks with stored blocks put their LZO blocks first (lzo_blocks_first): in a copy of the ids */
        if (B->is_lzo && !rev) {
            if ((rev = malloc(nids * sizeof(*rev))) != NULL) {
                memcpy(rev, ids, nids * sizeof(*rev));
                ids = rev;
            } else {
                rc = -1;
            }
        }
        struct layout L[kSlots];
        int live[kSlots] = {0};                /* slot holds a launched chunk */
        size_t from = 0;
        /* (tests: debug key fail_chunk=K makes this device's K-th delivery fail
         * as a failed GPU stream would) */
        const long fail_at = pom_dbg_int("fail_chunk", -1);
        long ndeliv = 0;
        for (int k = 0;; k++) {
            int cur = k % B->nslots;
            const int nxt = (k + 1) % B->nslots;
            const size_t *done_ids = NULL;     /* the chunk delivered now, for on_chunk */
            size_t done_nb = 0;
            int dj = -1;                       /* slot to deliver now, if any */
            if (!B->ooo) {
                if (live[cur])                 /* chunk k - nslots: wait, unpack */
                    dj = cur;
            } else {
                /* completion order: launch into a free slot; when there is
                 * none, or nothing is left to launch, deliver whichever chunk
                 * finishes first */
                cur = -1;
                for (int j = 0; j < B->nslots && cur < 0; j++)
                    if (!live[j])
                        cur = j;
                int any = 0;
                for (int j = 0; j < B->nslots; j++)
                    any |= live[j];
                if (any && (cur < 0 || from >= nids || rc != 0))
                    dj = wait_any_done(c, live, B->nslots);
            }
            if (dj >= 0) {
                const int ahead = !B->ooo && live[nxt] && nxt != dj;
                const int fail = fail_at >= 0 && ndeliv++ == fail_at;
                if (fail || chunk_deliver(&c->s[dj], &L[dj], B, ahead ? &c->s[nxt] : NULL, &L[nxt]) != 0) {
                    rc = -1;
                    for (int j = 0; j < B->nslots; j++)
                        hipStreamSynchronize(c->s[j].stream);
                } else {
                    done_ids = L[dj].ids;      /* (points into the plan, not the layout) */
                    done_nb = L[dj].nb;
                }
                live[dj] = 0;
                if (cur < 0)
                    cur = dj;
            }
            const int more = from < nids && rc == 0 && cur >= 0;
            if (more) {
                const size_t end = pom_chunk_end(ids, from, nids, B->cost,
                                                 k ? B->budget : B->budget / 4, kChunkBlocks);
                const size_t nb = end - from;
                B->ops->layout(&L[cur], ids + from, nb,
                               B->is_lzo ? lzo_blocks_first(rev + from, nb, B->is_lzo) : nb, B);
                /* the caller may produce the chunk's inputs now (e.g. read them),
                 * while the chunks in flight are copied and decoded */
                if (B->pre_chunk)
                    B->pre_chunk(B->cb_ctx, ids + from, nb);
                if (chunk_launch(&c->s[cur], &L[cur], B) != 0) {
                    rc = -1;
                    hipStreamSynchronize(c->s[cur].stream);
                } else {
                    live[cur] = 1;
                }
                from = end;
            }
            /* the caller's per-chunk work runs while the launched chunks' copies
             * and kernels are in flight */
            if (done_ids && B->on_chunk) {
                const double tc = g_timing ? pom_now_ms() : 0;
                B->on_chunk(B->cb_ctx, done_ids, done_nb);
                if (g_timing)
                    fprintf(stderr, "  on_chunk n=%zu: %.2f ms\n", done_nb, pom_now_ms() - tc);
            }
            if (!(from < nids && rc == 0)) {
                int any = 0;
                for (int j = 0; j < B->nslots; j++)
                    any |= live[j];
                if (!any)
                    break;
            }
        }
        free(rev);
    }
    if (prev_dev != device)
        hipSetDevice(prev_dev);
    return rc;
}

/* Devices a host batch may use: POM_LZO_DEVICES ("0,2,3"; default every
 * visible device; parsed by pom_parse_devices, duplicates dropped).
 * Processes that run one rank per GPU set it to their own. */
static int batch_devices(int *devs)
{
    const int count = lzo_mi355x_device_count();
    int n = 0;
    const char *e = getenv("POM_LZO_DEVICES");
    if (e && *e) {
        n = pom_parse_devices(e, count, kMaxDev, devs);
    } else {
        for (int d = 0; d < count && d < kMaxDev; d++)
            devs[n++] = d;
    }
    /* the caller's current device first: a one-device batch runs there */
    int cur = -1;
    if (n > 1 && hipGetDevice(&cur) == hipSuccess)
        for (int i = 1; i < n; i++)
            if (devs[i] == cur) {
                devs[i] = devs[0];
                devs[0] = cur;
                break;
            }
    return n;
}

int pom_host_batch(struct hbatch *B, size_t nblocks)
{
    const struct chunk_ops *ops = B->ops;
    const double t0 = g_timing ? pom_now_ms() : 0;
    B->t = pom_tctx_get();
    if (!B->t)
        return LZO_E_ERROR;
    if (nblocks == 0)
        return LZO_E_OK;
    if (nblocks > 0xFFFFFFFFu)
        return LZO_E_ERROR;
    int devs[kMaxDev];
    const int ndev = batch_devices(devs);
    if (ndev <= 0)
        return LZO_E_ERROR;
    size_t *cap = malloc(nblocks * sizeof(size_t));
    size_t *cost = malloc(nblocks * sizeof(size_t));
    if (!cap || !cost) {
        free(cap);
        free(cost);
        return LZO_E_OUT_OF_MEMORY;
    }
    for (size_t b = 0; b < nblocks; b++) {
        if (B->src_len[b] > 0xFFFFFFF0u) {
            free(cap);
            free(cost);
            return LZO_E_ERROR;
        }
        cap[b] = ops->cap(B, b);
        if (cap[b] > 0xFFFFFFF0u)
            cap[b] = 0xFFFFFFF0u;
        cost[b] = B->src_len[b] + cap[b] + (ops->extra_cost ? ops->extra_cost(B, b) : 0);
    }
    B->cap = cap;
    B->cost = cost;
    B->budget = ops->largest_first ? kChunkBudgetCompress : kChunkBudget;
    B->plan = (struct pom_plan){0, 1, NULL, NULL};
    B->devs = devs;
    B->nslots = kSlots;
    B->ooo = ops->largest_first && pom_dbg_int("ooo", 1) != 0;
    B->small_first = !ops->largest_first && pom_dbg_int("dec_small_first", 1) != 0;
    /* compress chunks that fit the LDS encoder's 4 blocks per CU at once use
     * it: a block alone on its CU finishes twice as fast as with the
     * dictionaries in HBM (that encoder wins only on full GPUs: 16 per CU) */
    B->enc_lds_max = (uint32_t)pom_dbg_int("enc_lds_max", (long)(lzo_mi355x_fast_resident_blocks() / 4));
    const long ns = pom_dbg_int("slots", kSlots);
    if (ns >= 1 && ns <= kSlots)
        B->nslots = (int)ns;
    const long mb = pom_dbg_int("chunk_mb", 0);
    if (mb > 0)
        B->budget = (size_t)mb << 20;
    int rc = LZO_E_OUT_OF_MEMORY;
    if (pom_plan_make(&B->plan, nblocks, cost, ndev, kSplitMinBytes) == 0) {
        /* blocks a failed device leaves untouched read as errors */
        for (size_t b = 0; b < nblocks; b++) {
            B->status[b] = LZO_E_ERROR;
            if (ops->unreached)
                ops->unreached(B, b);
        }
        rc = pom_run_devices(B->plan.ndev, dev_run, B) == 0 ? LZO_E_OK : LZO_E_ERROR;
        if (g_timing)
            fprintf(stderr, "pom host %s n=%zu devices=%d: %.2f ms\n", ops->label, nblocks, B->plan.ndev,
                    pom_now_ms() - t0);
        pom_plan_free(&B->plan);
    }
    free(cap);
    free(cost);
    return rc;
}

static int codec_batch(const struct chunk_ops *ops, const uint8_t *const *src, const size_t *src_len,
                       uint8_t *const *dst, size_t *dst_len, int *status, size_t nblocks,
                       pom_chunk_fn on_chunk, pom_chunk_fn pre_chunk, void *cb_ctx)
{
    struct hbatch B = {.ops = ops, .src = src, .src_len = src_len, .dst = dst, .dst_len = dst_len,
                       .status = status, .on_chunk = on_chunk, .pre_chunk = pre_chunk, .cb_ctx = cb_ctx};
    return pom_host_batch(&B, nblocks);
}

/* lzo_mi355x_decompress_batch with pre_chunk(ctx, ids, nb) called before each
 * chunk's inputs are staged: the caller fills src[ids[i]] (src_len is known
 * up front) while earlier chunks are on the GPU.  Same threads as
 * pom_compress_batch_chunked. */
int pom_decompress_batch_chunked(const uint8_t *const *src, const size_t *src_len, uint8_t *const *dst,
                                 size_t *dst_len, int *status, size_t nblocks, pom_chunk_fn pre_chunk,
                                 void *ctx)
{
    return codec_batch(&decompress_ops, src, src_len, dst, dst_len, status, nblocks, NULL, pre_chunk, ctx);
}

/* lzo_mi355x_compress_batch with on_chunk(ctx, ids, nb) called as each chunk's
 * blocks (ids into the caller's arrays) are delivered -- from the thread
 * running that device's chunks, so concurrently for batches split over
 * several GPUs. */
int pom_compress_batch_chunked(const uint8_t *const *src, const size_t *src_len, uint8_t *const *dst,
                               size_t *dst_len, int *status, size_t nblocks, pom_chunk_fn on_chunk,
                               void *ctx)
{
    return codec_batch(&compress_ops, src, src_len, dst, dst_len, status, nblocks, on_chunk, NULL, ctx);
}

int lzo_mi355x_compress_batch(const uint8_t *const *src, const size_t *src_len,
                              uint8_t *const *dst, size_t *dst_len, int *status,
                              size_t nblocks)
{
    return codec_batch(&compress_ops, src, src_len, dst, dst_len, status, nblocks, NULL, NULL, NULL);
}

int lzo_mi355x_decompress_batch(const uint8_t *const *src, const size_t *src_len,
                                uint8_t *const *dst, size_t *dst_len, int *status,
                                size_t nblocks)
{
    return codec_batch(&decompress_ops, src, src_len, dst, dst_len, status, nblocks, NULL, NULL, NULL);
}

int lzo_mi355x_decompress_concat_batch(const uint8_t *const *src, const size_t *src_len,
                                       uint8_t *const *dst, size_t *dst_len, int *status,
                                       size_t nblocks)
{
    return codec_batch(&concat_ops, src, src_len, dst, dst_len, status, nblocks, NULL, NULL, NULL);
}
