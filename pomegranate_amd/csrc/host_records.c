/*
 * host_records.c -- the record operations of the host batches: what runs
 * behind the decode of a chunk's LZO blocks, through the chunk pipeline of
 * lzo_host.c (host_pipeline.h).  The three walks -- the GC scan
 * (itb_scan.hip), the directory listing (itb_dents.hip), the key/value
 * listing (itb_keys.hip) -- share one layout, one staging and one delivery,
 * told apart by their list of result words and their record unit; the GC data
 * stat is the GC scan with the merge of the chunk's ranges behind it
 * (gc_merge.hip) and the merged map in the records' place; the column
 * read (col_slice.hip), the lookup (itb_find.hip) and the key/value get
 * (itb_kvget.hip) carry requests, the last two as one operation told apart by
 * a descriptor (struct req_spec) and their kernels; the ITB check
 * (itb_check.hip) has the walks' partition and fixed-size results; the ITB
 * split (itb_split.hip) has the check's partition, writes, and runs the encoder
 * over both halves behind it; the ITB sweep (itb_sweep.hip) is the split with
 * one payload and no second half; the ITB unlink (itb_unlink.hip) is the
 * request operations' staging and scatter with the sweep's writer half.  Their
 * callers (gc_scan.c, gc_stat.c, readdir.c, kvlist.c, column_codec.c, lookup.c,
 * kvget.c, check.c, itbsplit.c, itbsweep.c, unlink.c) select the blocks and put
 * the results in the caller's order.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "host_pipeline.h"
#include "host_requests.h"
#include "lzo_mi355x.h"
#include "minilzo.h"
#include "pom_check.h"
#include "pom_column.h"
#include "pom_gc.h"
#include "pom_itb.h"
#include "pom_kvget.h"
#include "pom_kvlist.h"
#include "pom_lookup.h"
#include "pom_split.h"
#include "pom_sweep.h"
#include "pom_unlink.h"

/* Per block of a chunk with stored blocks: where the walk finds the payload
 * (decoded behind o_dst, or stored as staged behind o_src), the decoders'
 * status and out_len, which the walk reads and which are set here for a
 * stored payload, and adepth.  Behind pom_stage_inputs. */
static void stage_scan(const struct layout *L, const struct scan_layout *K, uint8_t *h, const uint8_t *adepth)
{
    const uint64_t *so = (const uint64_t *)(h + L->o_srcoff);
    const uint64_t *dof = (const uint64_t *)(h + L->o_dstoff);
    const uint32_t *sl = (const uint32_t *)(h + L->o_srclen);
    uint64_t *sco = (uint64_t *)(h + K->o_scanoff);
    int32_t *st = (int32_t *)(h + L->o_status);
    uint32_t *ol = (uint32_t *)(h + L->o_outlen);
    uint8_t *ad = h + K->o_adepth;
    for (size_t i = 0; i < L->nb; i++) {
        const int lzo = i < L->nlzo;
        sco[i] = lzo ? L->o_dst + dof[i] : L->o_src + so[i];
        st[i] = 0;
        ol[i] = lzo ? 0 : sl[i];
        ad[i] = adepth[L->ids[i]];
    }
}

/* The one D2H of results whose size is known at the launch (column reads,
 * lookups), queued once the chunk's kernels are done. */
static int results_back(struct slot *S, size_t o_hres, size_t o_res, size_t bytes, size_t *packed)
{
    if (bytes && hipMemcpyAsync(S->hmem + o_hres, S->dmem + o_res, bytes, hipMemcpyDeviceToHost, S->stream) !=
                     hipSuccess)
        return -1;
    *packed = bytes;
    return 0;
}

/* A chunk's records join the call's buffers until the caller has placed them
 * (the chunks of a multi-GPU batch finish on several threads). */
static void keep_records(struct pom_walk_buf **bufs, pthread_mutex_t *mu, struct pom_walk_buf *buf)
{
    pthread_mutex_lock(mu);
    buf->next = *bufs;
    *bufs = buf;
    pthread_mutex_unlock(mu);
}

/* ------------------------------------------------------------------------ */
/* The walks: decode, walk, counts and records back                          */
/* ------------------------------------------------------------------------ */
/* A chunk's blocks are its LZO records first (the decoders run over that
 * prefix alone), then the records stored uncompressed, which are walked where
 * they are staged.  Staging (host and device alike up to the inputs' end;
 * pom_layout_walk):
 *   [src_off u64][dst_off u64][scan_off u64][first u64, nb + 1][src_len u32][dst_cap u32]
 *   [the operation's result words, u32 or i32 per block each]    <- D2H, one copy
 *   [adepth u8]
 *   [kvlist: needle, 256 bytes]
 *   [src bytes, 16-B aligned per block]
 *   host:   [kvlist: masks, 128 bytes per block, when asked for] <- D2H behind the counts
 *           [the chunk's records, unless count-only]             <- D2H, sized after the first
 *   device: [decoded payloads][decoder scratch][kvlist: masks][records, room for every ITE the payloads can hold]
 * The result words:
 *   GC scan   [status i32][out_len u32][live u32][nranges u32][err i32], records: 16-byte ranges
 *   readdir   [status i32][out_len u32][live u32][dnum u32][bytes u32][err i32], records: bytes, 272 an ITE
 *   kvlist    [status i32][out_len u32][live u32][dnum u32][bytes u32][keybytes u32][err i32], 324 an ITE;
 *             the call's needle is staged once per chunk, the emit masks stay on the
 *             device unless the caller asked for them, a count-only call has no records
 * No other decoded byte leaves the device.
 * The GC data stat is the GC scan with the merge of the chunk's ranges behind it
 * (pom_layout_gcstat): its result words are followed by the chunk's struct
 * pom_gc_stat in the same D2H, the device staging by the merge's scratch and the
 * merged map, and the second D2H brings exactly stat.nout extents; no range
 * leaves the device. */
static const uint8_t gc_words[] = {WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_ERR};
static const uint8_t rd_words[] = {WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_BYTES, WW_ERR};
static const uint8_t kv_words[] = {WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_BYTES, WW_KEYBYTES, WW_ERR};

static const struct walk_spec gc_spec = {gc_words, sizeof gc_words, sizeof(struct pom_gc_range),
                                         sizeof(struct pom_gc_range), 0, 0, 0, 1};
static const struct walk_spec rd_spec = {rd_words, sizeof rd_words, POM_DENT_HDR + POM_ITE_NAME_MAX, 1, 0, 0, 0, 1};

/* One call of a walk: B->sink. */
struct walk_call {
    struct pom_walk_sink *G;
    struct walk_spec spec;
};

/* The sink's array for each result word of the call, in the spec's order. */
static void sink_words(const struct walk_call *C, uint32_t *to[WW_N])
{
    const struct pom_walk_sink *G = C->G;
    uint32_t *const all[WW_N] = {(uint32_t *)G->status, G->out_len, G->live, G->count, G->bytes, G->keybytes,
                                 (uint32_t *)G->err};
    for (size_t w = 0; w < C->spec.nwords; w++)
        to[w] = all[C->spec.words[w]];
}

static size_t walk_cap(const struct hbatch *B, size_t b)
{
    const struct walk_call *C = B->sink;
    return C->G->cap[b];
}

static void walk_unreached(const struct hbatch *B, size_t b)
{
    const struct walk_call *C = B->sink;
    C->G->err[b] = LZO_E_ERROR;
}

static void walk_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    const struct walk_call *C = B->sink;
    pom_layout_walk(L, ids, nb, nlzo, B->src_len, B->cap, &C->spec, lzo_mi355x_decompress_scratch((uint32_t)nlzo));
}

static int walk_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct walk_call *C = B->sink;
    pom_stage_inputs(L, h, B);
    stage_scan(L, &L->u.walk.scan, h, C->G->adepth);
    if (C->spec.needle) {
        memset(h + L->u.walk.o_needle, 0, 256);
        if (C->G->needle_len)
            memcpy(h + L->u.walk.o_needle, C->G->needle, C->G->needle_len);
    }
    return 0;
}

/* Device pointer of a result word. */
static uint32_t *dword(const struct slot *S, const struct layout *L, enum walk_word w)
{
    return (uint32_t *)(S->dmem + L->u.walk.o_word[w]);
}

/* Behind a walk's kernels: the D2H of the result words, and of the masks when asked for. */
static int walk_words_back(struct slot *S, const struct layout *L, const struct walk_call *C, int rc)
{
    const struct walk_layout *K = &L->u.walk;
    if (rc != 0 ||
        hipMemcpyAsync(S->hmem + K->res_off, S->dmem + K->res_off, K->res_bytes, hipMemcpyDeviceToHost, S->stream) !=
            hipSuccess)
        return -1;
    if (C->spec.host_masks && hipMemcpyAsync(S->hmem + K->o_hmask, S->dmem + K->o_mask, 8 * POM_KV_MASK_WORDS * L->nb,
                                             hipMemcpyDeviceToHost, S->stream) != hipSuccess)
        return -1;
    return 0;
}

static int gc_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct walk_call *C = B->sink;
    const struct walk_layout *K = &L->u.walk;
    uint8_t *d = S->dmem;
    int rc = pom_decode_lzo_blocks(S, L, 0);
    if (rc == 0)
        rc = lzo_mi355x_launch_gc_scan(d, (const uint64_t *)(d + K->scan.o_scanoff), dword(S, L, WW_OUTLEN),
                                       (const int32_t *)dword(S, L, WW_STATUS), d + K->scan.o_adepth, (uint32_t)L->nb,
                                       (uint32_t)C->G->column, dword(S, L, WW_LIVE), dword(S, L, WW_COUNT),
                                       (uint64_t *)(d + K->o_first), (struct pom_gc_range *)(d + K->o_pack),
                                       K->rcap / sizeof(struct pom_gc_range), (int32_t *)dword(S, L, WW_ERR),
                                       S->stream);
    return walk_words_back(S, L, C, rc);
}

static int rd_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct walk_layout *K = &L->u.walk;
    uint8_t *d = S->dmem;
    int rc = pom_decode_lzo_blocks(S, L, 0);
    if (rc == 0)
        rc = lzo_mi355x_launch_readdir(d, (const uint64_t *)(d + K->scan.o_scanoff), dword(S, L, WW_OUTLEN),
                                       (const int32_t *)dword(S, L, WW_STATUS), d + K->scan.o_adepth, (uint32_t)L->nb,
                                       dword(S, L, WW_LIVE), dword(S, L, WW_COUNT), dword(S, L, WW_BYTES),
                                       (uint64_t *)(d + K->o_first), d + K->o_pack, K->rcap,
                                       (int32_t *)dword(S, L, WW_ERR), S->stream);
    return walk_words_back(S, L, B->sink, rc);
}

static int kv_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct walk_call *C = B->sink;
    const struct walk_layout *K = &L->u.walk;
    uint8_t *d = S->dmem;
    int rc = pom_decode_lzo_blocks(S, L, 0);
    if (rc == 0)
        rc = lzo_mi355x_launch_kvlist(d, (const uint64_t *)(d + K->scan.o_scanoff), dword(S, L, WW_OUTLEN),
                                      (const int32_t *)dword(S, L, WW_STATUS), d + K->scan.o_adepth, (uint32_t)L->nb,
                                      C->G->kv_op, d + K->o_needle, C->G->needle_len, dword(S, L, WW_LIVE),
                                      dword(S, L, WW_COUNT), dword(S, L, WW_BYTES), dword(S, L, WW_KEYBYTES),
                                      (uint64_t *)(d + K->o_mask), (uint64_t *)(d + K->o_first), d + K->o_pack,
                                      C->spec.host_records ? K->rcap : 0, (int32_t *)dword(S, L, WW_ERR), S->stream);
    return walk_words_back(S, L, C, rc);
}

/* The host's copy of the word that counts a block's records, in the spec's unit. */
static const uint32_t *records_word(const struct slot *S, const struct layout *L, const struct walk_spec *W)
{
    return (const uint32_t *)(S->hmem + L->u.walk.o_word[W->unit == 1 ? WW_BYTES : WW_COUNT]);
}

/* Once the counts are back: the D2H of exactly the chunk's records (a count-only chunk has none). */
static int walk_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    const struct walk_call *C = B->sink;
    const struct walk_layout *K = &L->u.walk;
    size_t total = 0;
    if (C->spec.host_records) {
        const uint32_t *n = records_word(S, L, &C->spec);
        for (size_t i = 0; i < L->nb; i++)
            total += n[i] * C->spec.unit;
        if (total > K->rcap)
            return -1;
        if (total && hipMemcpyAsync(S->hmem + K->o_hrec, S->dmem + K->o_pack, total, hipMemcpyDeviceToHost,
                                    S->stream) != hipSuccess)
            return -1;
    }
    *packed = total;
    return 0;
}

/* The chunk's records into a buffer of their own (the chunks reorder the
 * blocks, so the caller places each block's records itself), block by block
 * over the copy threads: a listing is megabytes. */
static int walk_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct walk_call *C = B->sink;
    const struct walk_layout *K = &L->u.walk;
    struct pom_walk_sink *G = C->G;
    const uint8_t *h = S->hmem;
    const uint32_t *n = records_word(S, L, &C->spec);
    uint32_t *to[WW_N];
    const uint32_t *from[WW_N];
    sink_words(C, to);
    for (size_t w = 0; w < C->spec.nwords; w++)
        from[w] = (const uint32_t *)(h + K->o_word[C->spec.words[w]]);
    struct pom_walk_buf *buf = malloc(sizeof(*buf) + L->packed);
    if (!buf)
        return -1;
    struct copy_job *jobs = malloc((L->nb + 1) * sizeof(*jobs));
    if (!jobs)
        memcpy(buf->bytes, h + K->o_hrec, L->packed);
    size_t at = 0;
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        const size_t nbytes = C->spec.host_records ? n[i] * C->spec.unit : 0;
        for (size_t w = 0; w < C->spec.nwords; w++)
            to[w][b] = from[w][i];
        G->recs[b] = C->spec.host_records ? buf->bytes + at : NULL;
        if (C->spec.host_masks)
            memcpy(G->mask + POM_KV_MASK_WORDS * b, h + K->o_hmask + 8 * POM_KV_MASK_WORDS * i, 8 * POM_KV_MASK_WORDS);
        if (jobs) {
            jobs[i].dst = buf->bytes + at;
            jobs[i].src = h + K->o_hrec + at;
            jobs[i].len = nbytes;
        }
        at += nbytes;
    }
    if (jobs) {
        pom_copy_jobs(jobs, L->nb);
        free(jobs);
    }
    keep_records(&G->bufs, &G->mu, buf);
    return 0;
}

static const struct chunk_ops gc_ops = {"gc scan", 0, walk_cap, NULL, walk_unreached, walk_layout,
                                        walk_stage, gc_kernels, walk_collect, walk_unpack};
static const struct chunk_ops rd_ops = {"readdir", 0, walk_cap, NULL, walk_unreached, walk_layout,
                                        walk_stage, rd_kernels, walk_collect, walk_unpack};
static const struct chunk_ops kv_ops = {"kvlist", 0, walk_cap, NULL, walk_unreached, walk_layout,
                                        walk_stage, kv_kernels, walk_collect, walk_unpack};

static int walk_batch(const struct chunk_ops *ops, const struct walk_spec *spec, const uint8_t *const *src,
                      const size_t *src_len, size_t nblocks, struct pom_walk_sink *sink)
{
    struct walk_call C = {sink, *spec};
    uint32_t *to[WW_N];
    sink_words(&C, to);
    for (size_t b = 0; b < nblocks; b++) {
        for (size_t w = 0; w < spec->nwords; w++)
            if (spec->words[w] != WW_STATUS && spec->words[w] != WW_ERR)
                to[w][b] = 0;
        sink->recs[b] = NULL;
    }
    struct hbatch B = {.ops = ops, .src = src, .src_len = src_len, .status = sink->status, .is_lzo = sink->is_lzo,
                       .sink = &C};
    return pom_host_batch(&B, nblocks);
}

int pom_gc_scan_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks, struct pom_walk_sink *sink)
{
    return walk_batch(&gc_ops, &gc_spec, src, src_len, nblocks, sink);
}

/* The GC data stat.  The merge runs over all nmerge places of the ranges' room,
 * which is zeroed before the scan: a place the scan leaves is {0, 0}, a dropped
 * range, and the chunk's nwrapped is corrected for them once the counts are back
 * (the number of ranges is known on the device only, the number of launches
 * must follow from what the host knows). */
struct gcstat_call {
    struct walk_call C;             /* first: the walks' callbacks see their call */
    struct pom_gc_stat_sink *M;
};

static size_t gs_max_ranges(const struct hbatch *B, size_t b)
{
    const struct walk_call *C = B->sink;
    return pom_gc_max_ranges(C->G->is_lzo[b] ? C->G->cap[b] : B->src_len[b], C->G->adepth[b]);
}

/* the chunk budget counts a range's place, its extent's, and the sort's two buffers */
static size_t gs_extra_cost(const struct hbatch *B, size_t b)
{
    return gs_max_ranges(B, b) * (2 * sizeof(struct pom_gc_range) + 32 + 8);
}

static void gs_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    const struct walk_call *C = B->sink;
    size_t nm = 0;
    for (size_t i = 0; i < nb; i++)
        nm += gs_max_ranges(B, ids[i]);
    /* (a chunk past the merge's bound gets no scratch, and its kernels refuse to run) */
    pom_layout_gcstat(L, ids, nb, nlzo, B->src_len, B->cap, &C->spec, lzo_mi355x_decompress_scratch((uint32_t)nlzo),
                      nm, nm <= POM_GC_MERGE_MAX ? pom_gc_merge_scratch((uint32_t)nm) : 0);
}

static int gs_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct walk_call *C = B->sink;
    const struct gcstat_layout *G = &L->u.gcstat;
    const struct walk_layout *K = &G->walk;
    uint8_t *d = S->dmem;
    struct pom_gc_range *ranges = (struct pom_gc_range *)(d + K->o_pack);
    if (G->nmerge > POM_GC_MERGE_MAX)
        return -1;
    int rc = pom_decode_lzo_blocks(S, L, 0);
    if (rc == 0 && K->rcap && hipMemsetAsync(ranges, 0, K->rcap, S->stream) != hipSuccess)
        rc = -1;
    if (rc == 0)
        rc = lzo_mi355x_launch_gc_scan(d, (const uint64_t *)(d + K->scan.o_scanoff), dword(S, L, WW_OUTLEN),
                                       (const int32_t *)dword(S, L, WW_STATUS), d + K->scan.o_adepth, (uint32_t)L->nb,
                                       (uint32_t)C->G->column, dword(S, L, WW_LIVE), dword(S, L, WW_COUNT),
                                       (uint64_t *)(d + K->o_first), ranges, G->nmerge,
                                       (int32_t *)dword(S, L, WW_ERR), S->stream);
    if (rc == 0)
        rc = pom_gc_merge_dev(ranges, (uint32_t)G->nmerge, d + G->o_mscr, G->mscr_bytes,
                              (struct pom_gc_range *)(d + G->o_merged), G->nmerge,
                              (struct pom_gc_stat *)(d + G->o_stat), S->stream);
    return walk_words_back(S, L, C, rc);
}

/* Once the counts and the chunk's stat are back: the D2H of exactly its extents. */
static int gs_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    const struct gcstat_layout *G = &L->u.gcstat;
    const struct pom_gc_stat *st = (const struct pom_gc_stat *)(S->hmem + G->o_stat);
    (void)B;
    if (st->nout > G->nmerge)
        return -1;
    const size_t total = (size_t)st->nout * sizeof(struct pom_gc_range);
    if (total && hipMemcpyAsync(S->hmem + G->walk.o_hrec, S->dmem + G->o_merged, total, hipMemcpyDeviceToHost,
                                S->stream) != hipSuccess)
        return -1;
    *packed = total;
    return 0;
}

static int gs_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct gcstat_call *Y = B->sink;
    const struct walk_call *C = &Y->C;
    const struct gcstat_layout *G = &L->u.gcstat;
    struct pom_walk_sink *W = C->G;
    const uint8_t *h = S->hmem;
    const struct pom_gc_stat *st = (const struct pom_gc_stat *)(h + G->o_stat);
    const uint32_t *n = (const uint32_t *)(h + G->walk.o_word[WW_COUNT]);
    uint32_t *to[WW_N];
    sink_words(C, to);
    struct pom_walk_buf *buf = malloc(sizeof(*buf) + L->packed);
    if (!buf)
        return -1;
    uint64_t nin = 0;
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        for (size_t w = 0; w < C->spec.nwords; w++)
            to[w][b] = ((const uint32_t *)(h + G->walk.o_word[C->spec.words[w]]))[i];
        W->recs[b] = NULL;
        nin += n[i];
    }
    /* every place of the ranges' room the scan left was counted as a dropped range */
    if (nin > G->nmerge || st->nin != G->nmerge || st->nwrapped < G->nmerge - nin) {
        free(buf);
        return -1;
    }
    memcpy(buf->bytes, h + G->walk.o_hrec, L->packed);
    buf->pad = st->nout;
    pthread_mutex_lock(&W->mu);
    buf->next = Y->M->maps;
    Y->M->maps = buf;
    Y->M->nin += nin;
    Y->M->nwrapped += st->nwrapped - (G->nmerge - nin);
    pthread_mutex_unlock(&W->mu);
    return 0;
}

static const struct chunk_ops gs_ops = {"gc stat", 0, walk_cap, gs_extra_cost, walk_unreached, gs_layout,
                                        walk_stage, gs_kernels, gs_collect, gs_unpack};

int pom_gc_stat_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                        struct pom_walk_sink *sink, struct pom_gc_stat_sink *maps)
{
    struct gcstat_call Y = {{sink, gc_spec}, maps};
    uint32_t *to[WW_N];
    sink_words(&Y.C, to);
    for (size_t b = 0; b < nblocks; b++) {
        for (size_t w = 0; w < gc_spec.nwords; w++)
            if (gc_spec.words[w] != WW_STATUS && gc_spec.words[w] != WW_ERR)
                to[w][b] = 0;
        sink->recs[b] = NULL;
    }
    struct hbatch B = {.ops = &gs_ops, .src = src, .src_len = src_len, .status = sink->status, .is_lzo = sink->is_lzo,
                       .sink = &Y};
    return pom_host_batch(&B, nblocks);
}

int pom_readdir_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks, struct pom_walk_sink *sink)
{
    return walk_batch(&rd_ops, &rd_spec, src, src_len, nblocks, sink);
}

int pom_kvlist_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks, struct pom_walk_sink *sink)
{
    const struct walk_spec spec = {kv_words, sizeof kv_words, 4 + POM_KV_VALUE_MAX, 1,
                                   1, 1, sink->mask != NULL, !sink->count_only};
    return walk_batch(&kv_ops, &spec, src, src_len, nblocks, sink);
}

/* ------------------------------------------------------------------------ */
/* Column reads: decode, region copy (col_slice.hip), slices back             */
/* ------------------------------------------------------------------------ */
/* A column and all its requests are in one chunk; request j of the chunk is
 * the j-th in block order, then in the block's own order.  The recorded
 * length, the offset and the size are all known here, so every request's
 * clamped length and its 16-byte-aligned place among the chunk's slices are
 * known before the launch: one copy of a known size brings back codes and
 * slices, with no sizing round trip between two copies (the bytes of a request
 * that ends in an error are copied and ignored).  That copy is queued once the
 * chunk's kernels are done, as the codec chunks queue their own (collect).
 * Queued with the launch, the chunks' decodes ran one after another instead
 * of side by side (64 columns of 4 MiB, 32 reads each: 83 ms a call against 36
 * ms) -- as if the copy, waiting for its chunk's decode, held up
 * the next chunks' copies to the device, and with them their kernels.  Staging
 * (host and device alike up to the inputs' end; pom_layout_col):
 *   [src_off u64][dst_off u64][want u64][out_off u64, nreq][requests, nreq][src_len u32][dst_cap u32]
 *   [src bytes, 16-B aligned per block]
 *   device: [decoded columns, 16-B aligned][decoder scratch]
 *   both:   [status i32][out_len u32][slice len u32, nreq][slice err i32, nreq][slices]  <- D2H, one copy
 * No other decoded byte leaves the device. */
static size_t cr_slot(const struct pom_col_sink *C, size_t b, size_t k)
{
    const struct pom_col_req *q = &C->req[C->req_ids[k]];
    const uint64_t w = C->want[b];
    const uint64_t n = q->offset > w ? 0 : q->size < w - q->offset ? q->size : w - q->offset;
    return POM_ALIGN_UP((size_t)n, 16);
}

static size_t cr_cap(const struct hbatch *B, size_t b)
{
    const struct pom_col_sink *C = B->sink;
    return (size_t)C->want[b];
}

/* the chunk budget counts the slices too */
static size_t cr_extra_cost(const struct hbatch *B, size_t b)
{
    const struct pom_col_sink *C = B->sink;
    size_t n = 0;
    for (size_t k = C->req_first[b]; k < C->req_first[b + 1]; k++)
        n += cr_slot(C, b, k);
    return n;
}

static void cr_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    const struct pom_col_sink *C = B->sink;
    size_t nreq = 0, slices = 0;
    (void)nlzo;
    for (size_t i = 0; i < nb; i++) {
        nreq += C->req_first[ids[i] + 1] - C->req_first[ids[i]];
        slices += cr_extra_cost(B, ids[i]);
    }
    pom_layout_col(L, ids, nb, B->src_len, B->cap, nreq, slices, lzo_mi355x_decompress_scratch((uint32_t)nb));
}

static int cr_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct pom_col_sink *C = B->sink;
    const struct col_layout *K = &L->u.col;
    if (K->nreq > 0xFFFFFFFFu)
        return -1;
    uint64_t *wt = (uint64_t *)(h + K->o_want);
    uint64_t *oo = (uint64_t *)(h + K->o_outoff);
    struct pom_col_req *rq = (struct pom_col_req *)(h + K->o_req);
    size_t j = 0, at = 0;
    pom_stage_inputs(L, h, B);
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        wt[i] = C->want[b];
        for (size_t k = C->req_first[b]; k < C->req_first[b + 1]; k++, j++) {
            const struct pom_col_req *q = &C->req[C->req_ids[k]];
            rq[j].offset = q->offset;
            rq[j].size = q->size;
            rq[j].col = (uint32_t)i;            /* the chunk's own column index */
            rq[j].pad = 0;
            oo[j] = at;
            at += cr_slot(C, b, k);
        }
    }
    return 0;
}

static int cr_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct pom_col_sink *C = B->sink;
    const struct col_layout *K = &L->u.col;
    uint8_t *d = S->dmem, *res = d + K->o_res;
    if (pom_decode_lzo_blocks(S, L, C->concat) != 0)
        return -1;
    return lzo_mi355x_launch_col_slice(d + L->o_dst, (const uint64_t *)(d + L->o_dstoff),
                                       (const uint32_t *)(d + L->o_outlen), (const int32_t *)(d + L->o_status),
                                       (const uint64_t *)(d + K->o_want), (uint32_t)L->nb,
                                       (const struct pom_col_req *)(d + K->o_req), (uint32_t)K->nreq,
                                       res + K->res_hdr, (const uint64_t *)(d + K->o_outoff),
                                       (uint32_t *)(res + K->r_len), (int32_t *)(res + K->r_err), S->stream);
}

static int cr_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    (void)B;
    return results_back(S, L->u.col.o_hres, L->u.col.o_res, L->u.col.res_bytes, packed);
}

static int cr_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    struct pom_col_sink *C = B->sink;
    const struct col_layout *K = &L->u.col;
    const uint8_t *res = S->hmem + K->o_hres;
    const uint64_t *oo = (const uint64_t *)(S->hmem + K->o_outoff);
    const int32_t *hst = (const int32_t *)(res + K->r_status);
    const uint32_t *hrl = (const uint32_t *)(res + K->r_len);
    const int32_t *hre = (const int32_t *)(res + K->r_err);
    struct copy_job *jobs = malloc((K->nreq + 1) * sizeof(*jobs));
    size_t j = 0;
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        C->status[b] = hst[i];
        for (size_t k = C->req_first[b]; k < C->req_first[b + 1]; k++, j++) {
            const size_t r = C->req_ids[k];
            const size_t n = hre[j] == 0 ? hrl[j] : 0;
            C->err[r] = hre[j];
            C->out_len[r] = n;
            if (jobs) {
                jobs[j].dst = C->out[r];
                jobs[j].src = res + K->res_hdr + oo[j];
                jobs[j].len = n;
            } else if (n) {
                memcpy(C->out[r], res + K->res_hdr + oo[j], n);
            }
        }
    }
    if (jobs) {
        pom_copy_jobs(jobs, K->nreq);
        free(jobs);
    }
    return 0;
}

/* (a column read's requests: set by the caller, so nothing to mark unreached) */
static const struct chunk_ops cr_ops = {"column read", 0, cr_cap, cr_extra_cost, NULL, cr_layout,
                                        cr_stage, cr_kernels, cr_collect, cr_unpack};

int pom_col_read_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                         struct pom_col_sink *sink)
{
    struct hbatch B = {.ops = &cr_ops, .src = src, .src_len = src_len, .status = sink->status, .sink = sink};
    return pom_host_batch(&B, nblocks);
}

/* ------------------------------------------------------------------------ */
/* Requests: decode, chain walk (itb_find.hip, itb_kvget.hip), results back   */
/* ------------------------------------------------------------------------ */
/* The walks' partition (LZO records first, stored ones walked as staged) with
 * the column reads' requests: an ITB and all its requests are in one chunk;
 * request j of the chunk is the j-th in block order, then in the block's own
 * order, renumbered to the chunk's ITB index, its name or string key staged in
 * a blob of the chunk's own.  A request the kind refuses (host_requests.h: a
 * name or key the caller's blob does not hold, a namelen above 255, a get that
 * is no string get or has sklen above 320) gets no blob bytes and an offset
 * past the chunk's blob: where the kernel reads it, its rule 4 refuses it,
 * behind rules 1 to 3 as everywhere.  The decoder's status reaches the host
 * through the requests' err.  Fixed-size results come back in one copy of a
 * known size, queued once the chunk's kernels are done (the column reads say
 * why).  Variable-length records come back as the walks' do: the fixed-size
 * results and the chunk's record total in one copy queued behind the kernels,
 * exactly that many record bytes in a second one sized once the first is back.
 * Staging (host and device alike up to the inputs' end; pom_layout_req):
 *   [src_off u64][dst_off u64][scan_off u64][requests, nreq][src_len u32][dst_cap u32]
 *   [status i32][out_len u32][adepth u8]
 *   [src bytes, 16-B aligned per block][blob]
 *   device: [decoded payloads][decoder scratch][get: first u64, nreq]
 *   both:   [the kind's results, nreq each]                          <- D2H, one copy
 *           [get: the chunk's records, packed, unless lengths only]  <- D2H, sized after the first
 * The results:
 *   lookup  [err i32][nr u32][depth u32][records, 136 each]
 *   get     [total u64][err i32][nr u32][depth u32][len u32][lease u64]; the total is first[nreq]
 * No other decoded byte leaves the device. */
struct req_call {
    struct pom_req_sink *K;
    pthread_mutex_t mu;             /* K->bufs: chunks of a multi-GPU batch finish on several threads */
};

static size_t req_cap(const struct hbatch *B, size_t b)
{
    const struct req_call *C = B->sink;
    return C->K->cap[b];
}

/* the chunk budget counts the requests, their blob bytes, their results and their records' room */
static size_t req_extra_cost(const struct hbatch *B, size_t b)
{
    const struct req_call *C = B->sink;
    const struct req_spec *Q = C->K->spec;
    size_t blob = 0;
    const size_t nreq = pom_req_block(C->K, b, &blob);
    return nreq * (POM_REQ_SIZE + 4 * Q->nwords + (Q->lease ? 8 : 0) + Q->rec_fixed +
                   (Q->rec_max ? 8 + (C->K->records ? Q->rec_max : 0) : 0)) + blob;
}

static void req_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    const struct req_call *C = B->sink;
    size_t nreq = 0, blob = 0;
    for (size_t i = 0; i < nb; i++)
        nreq += pom_req_block(C->K, ids[i], &blob);
    pom_layout_req(L, ids, nb, nlzo, B->src_len, B->cap, C->K->spec, nreq, blob, C->K->records,
                   lzo_mi355x_decompress_scratch((uint32_t)nlzo));
}

static int req_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct req_call *C = B->sink;
    if (pom_req_stage(L, h, C->K) != 0)
        return -1;
    pom_stage_inputs(L, h, B);
    stage_scan(L, &L->u.req.scan, h, C->K->adepth);
    return 0;
}

static int lk_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct req_layout *Y = &L->u.req;
    uint8_t *d = S->dmem, *res = d + Y->o_res;
    (void)B;
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    return lzo_mi355x_launch_lookup(d, (const uint64_t *)(d + Y->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                                    (const int32_t *)(d + L->o_status), d + Y->scan.o_adepth, (uint32_t)L->nb,
                                    (const struct pom_lookup_req *)(d + Y->o_req), (uint32_t)Y->nreq,
                                    d + Y->o_blob, (uint32_t)Y->blob_bytes, (int32_t *)(res + Y->r_word[RW_ERR]),
                                    (uint32_t *)(res + Y->r_word[RW_NR]), (uint32_t *)(res + Y->r_word[RW_DEPTH]),
                                    res + Y->res_hdr, S->stream);
}

static int kg_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct req_layout *Y = &L->u.req;
    uint8_t *d = S->dmem, *res = d + Y->o_res;
    size_t queued;
    (void)B;
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    if (lzo_mi355x_launch_kvget(d, (const uint64_t *)(d + Y->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                                (const int32_t *)(d + L->o_status), d + Y->scan.o_adepth, (uint32_t)L->nb,
                                (const struct pom_kvget_req *)(d + Y->o_req), (uint32_t)Y->nreq, d + Y->o_blob,
                                (uint32_t)Y->blob_bytes, (int32_t *)(res + Y->r_word[RW_ERR]),
                                (uint32_t *)(res + Y->r_word[RW_NR]), (uint32_t *)(res + Y->r_word[RW_DEPTH]),
                                (uint32_t *)(res + Y->r_word[RW_LEN]), (uint64_t *)(res + Y->r_lease),
                                (uint64_t *)(d + Y->o_first), d + Y->o_pack, Y->rcap, S->stream) != 0)
        return -1;
    return results_back(S, Y->o_hres, Y->o_res, Y->res_bytes, &queued);
}

/* Fixed records: the one copy.  Variable ones, once the lengths are back: the
 * D2H of exactly the chunk's records. */
static int req_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    const struct req_call *C = B->sink;
    const struct req_layout *Y = &L->u.req;
    uint64_t total;
    if (!C->K->spec->rec_max)
        return results_back(S, Y->o_hres, Y->o_res, Y->res_bytes, packed);
    memcpy(&total, S->hmem + Y->o_hres, 8);
    if (!C->K->records)
        total = 0;
    if (total > Y->rcap)
        return -1;
    if (total && hipMemcpyAsync(S->hmem + Y->o_hrec, S->dmem + Y->o_pack, total, hipMemcpyDeviceToHost, S->stream) !=
                     hipSuccess)
        return -1;
    *packed = total;
    return 0;
}

/* The fixed-size results go to their places in the caller's request order;
 * variable records stay in a buffer of the sink until the caller knows the
 * call's own first[]. */
static int req_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    struct req_call *C = B->sink;
    struct pom_walk_buf *buf = NULL;
    if (C->K->spec->rec_max) {
        buf = malloc(sizeof(*buf) + L->packed);
        if (!buf)
            return -1;
        memcpy(buf->bytes, S->hmem + L->u.req.o_hrec, L->packed);
    }
    pom_req_scatter(L, S->hmem, C->K, buf ? buf->bytes : NULL, L->packed);
    if (buf)
        keep_records(&C->K->bufs, &C->mu, buf);
    return 0;
}

/* (a request's results: set by the caller, so nothing to mark unreached) */
static const struct chunk_ops lk_ops = {"lookup", 0, req_cap, req_extra_cost, NULL, req_layout,
                                        req_stage, lk_kernels, req_collect, req_unpack};
static const struct chunk_ops kg_ops = {"kvget", 0, req_cap, req_extra_cost, NULL, req_layout,
                                        req_stage, kg_kernels, req_collect, req_unpack};

static int req_batch(const struct chunk_ops *ops, const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                     struct pom_req_sink *sink)
{
    struct req_call C = {sink, PTHREAD_MUTEX_INITIALIZER};
    struct hbatch B = {.ops = ops, .src = src, .src_len = src_len, .status = sink->status, .is_lzo = sink->is_lzo,
                       .sink = &C};
    const int rc = pom_host_batch(&B, nblocks);
    pthread_mutex_destroy(&C.mu);
    return rc;
}

int pom_lookup_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks, struct pom_req_sink *sink)
{
    return req_batch(&lk_ops, src, src_len, nblocks, sink);
}

int pom_kvget_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks, struct pom_req_sink *sink)
{
    return req_batch(&kg_ops, src, src_len, nblocks, sink);
}

/* ------------------------------------------------------------------------ */
/* The ITB check: decode, check (itb_check.hip), reports back                 */
/* ------------------------------------------------------------------------ */
/* The walks' partition (LZO records first, stored ones checked as staged)
 * without their record room: every result has a fixed size, so one copy of a
 * size known at the launch brings everything back, queued once the chunk's
 * kernels are done (the column reads say why).  Staging (host and device alike
 * up to the inputs' end; pom_layout_check):
 *   [src_off u64][dst_off u64][scan_off u64][header facts, 32 bytes per block]
 *   [src_len u32][dst_cap u32][status i32][out_len u32][adepth u8]
 *   [src bytes, 16-B aligned per block]
 *   device: [decoded payloads][decoder scratch]
 *   both:   [status i32][out_len u32][err i32][reports, 48 bytes per block]
 *           [slot masks, 256 per block][ITE masks, 128 per block]      <- D2H, one copy
 * The masks have room only when the caller asked for them.  The decoders'
 * status and out_len are copied into the results on the device, so that
 * nothing of the results is uploaded.  No decoded byte leaves the device. */
static size_t ck_cap(const struct hbatch *B, size_t b)
{
    const struct pom_check_sink *C = B->sink;
    return C->cap[b];
}

static int ck_masks(const struct pom_check_sink *C)
{
    return C->slot_mask != NULL || C->ite_mask != NULL;
}

/* the chunk budget counts the header facts and the results */
static size_t ck_extra_cost(const struct hbatch *B, size_t b)
{
    (void)b;
    return sizeof(struct pom_check_hdr) + 12 + sizeof(struct pom_check_report) +
           (ck_masks(B->sink) ? 8 * (POM_CK_SLOT_MASK_WORDS + POM_CK_ITE_MASK_WORDS) : 0);
}

static void ck_unreached(const struct hbatch *B, size_t b)
{
    const struct pom_check_sink *C = B->sink;
    C->err[b] = LZO_E_ERROR;
}

static void ck_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    pom_layout_check(L, ids, nb, nlzo, B->src_len, B->cap, ck_masks(B->sink),
                     lzo_mi355x_decompress_scratch((uint32_t)nlzo));
}

static int ck_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct pom_check_sink *C = B->sink;
    struct pom_check_hdr *hd = (struct pom_check_hdr *)(h + L->u.check.o_hdr);
    pom_stage_inputs(L, h, B);
    stage_scan(L, &L->u.check.scan, h, C->adepth);
    for (size_t i = 0; i < L->nb; i++)
        hd[i] = C->hdr[L->ids[i]];
    return 0;
}

static int ck_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct pom_check_sink *C = B->sink;
    const struct itb_check_layout *K = &L->u.check;
    uint8_t *d = S->dmem, *res = d + K->o_res;
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    if (lzo_mi355x_launch_itb_check(d, (const uint64_t *)(d + K->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                                    (const int32_t *)(d + L->o_status), d + K->scan.o_adepth,
                                    (const struct pom_check_hdr *)(d + K->o_hdr), (uint32_t)L->nb, C->flags,
                                    (struct pom_check_report *)(res + K->r_report),
                                    K->masks ? (uint64_t *)(res + K->r_smask) : NULL,
                                    K->masks ? (uint64_t *)(res + K->r_imask) : NULL, (int32_t *)(res + K->r_err),
                                    S->stream) != 0)
        return -1;
    /* status, then out_len: adjacent among the inputs and among the results */
    return hipMemcpyAsync(res + K->r_status, d + L->o_status, 8 * L->nb, hipMemcpyDeviceToDevice, S->stream) ==
                   hipSuccess ? 0 : -1;
}

static int ck_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    (void)B;
    return results_back(S, L->u.check.o_hres, L->u.check.o_res, L->u.check.res_bytes, packed);
}

static int ck_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct pom_check_sink *C = B->sink;
    const struct itb_check_layout *K = &L->u.check;
    const uint8_t *res = S->hmem + K->o_hres;
    const int32_t *st = (const int32_t *)(res + K->r_status), *er = (const int32_t *)(res + K->r_err);
    const uint32_t *ol = (const uint32_t *)(res + K->r_outlen);
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i], to = C->idx[b];
        C->status[b] = st[i];
        C->out_len[b] = ol[i];
        C->err[b] = er[i];
        memcpy(&C->report[to], res + K->r_report + sizeof(struct pom_check_report) * i, sizeof(struct pom_check_report));
        if (C->slot_mask)
            memcpy(C->slot_mask + POM_CK_SLOT_MASK_WORDS * to, res + K->r_smask + 8 * POM_CK_SLOT_MASK_WORDS * i,
                   8 * POM_CK_SLOT_MASK_WORDS);
        if (C->ite_mask)
            memcpy(C->ite_mask + POM_CK_ITE_MASK_WORDS * to, res + K->r_imask + 8 * POM_CK_ITE_MASK_WORDS * i,
                   8 * POM_CK_ITE_MASK_WORDS);
    }
    return 0;
}

static const struct chunk_ops ck_ops = {"itb check", 0, ck_cap, ck_extra_cost, ck_unreached, ck_layout,
                                        ck_stage, ck_kernels, ck_collect, ck_unpack};

int pom_itb_check_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                          struct pom_check_sink *sink)
{
    struct hbatch B = {.ops = &ck_ops, .src = src, .src_len = src_len, .status = sink->status, .is_lzo = sink->is_lzo,
                       .sink = sink};
    return pom_host_batch(&B, nblocks);
}

/* ------------------------------------------------------------------------ */
/* The ITB split: decode, check and split (itb_split.hip), encode both halves */
/* ------------------------------------------------------------------------ */
/* The check's partition (LZO records decoded, stored ones split where they
 * are staged), and the first operation that writes.  Kernels on the chunk's
 * stream: the decoders; pom_itb_split_dev, which rewrites each old payload's
 * bitmap and index in place and writes the new payloads beside them; the
 * gather of the encoder's 2 * nb source lengths from the results;
 * lzo_mi355x_compress_dev over the 2 * nb halves where they lie.  The results
 * (the decoders' words, the 48-byte results, the encoder's out_len and status)
 * come back in one copy queued behind the kernels.  Once they are back the
 * host applies itb_lzo_compress's not-smaller rule to each half, and the pack
 * kernel gathers exactly what is delivered -- the stream, or the payload of a
 * half that did not compress -- for the second D2H.  Staging:
 * pom_layout_split (host_layout.h).  No decoded byte leaves the device unless
 * a half does not compress. */
static size_t sp_cap(const struct hbatch *B, size_t b)
{
    const struct pom_split_sink *C = B->sink;
    return C->cap[b];
}

static size_t sp_dl(const struct hbatch *B, size_t b)
{
    const struct pom_split_sink *C = B->sink;
    return C->is_lzo[b] ? B->cap[b] : B->src_len[b];
}

/* the chunk budget counts the new payload, the two stream slots, the delivered halves and the small arrays */
static size_t sp_extra_cost(const struct hbatch *B, size_t b)
{
    const struct pom_split_sink *C = B->sink;
    const size_t dl = C->is_lzo[b] ? C->cap[b] : B->src_len[b];
    return 3 * dl + 2 * pom_split_stream_room(dl) + 256;
}

static void sp_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    pom_layout_split(L, ids, nb, nlzo, B->src_len, B->cap, lzo_mi355x_decompress_scratch((uint32_t)nlzo),
                     pom_itb_split_scratch((uint32_t)nb), lzo_mi355x_compress_scratch((uint32_t)(2 * nb)));
}

static int sp_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct pom_split_sink *C = B->sink;
    const struct itb_split_layout *K = &L->u.split;
    const size_t nb = L->nb;
    struct pom_check_hdr *hd = (struct pom_check_hdr *)(h + K->o_hdr);
    uint64_t *no = (uint64_t *)(h + K->o_newoff), *eso = (uint64_t *)(h + K->o_esrcoff);
    uint64_t *edo = (uint64_t *)(h + K->o_edstoff);
    uint32_t *nc = (uint32_t *)(h + K->o_newcap), *edc = (uint32_t *)(h + K->o_edstcap);
    const uint64_t *sco = (const uint64_t *)(h + K->scan.o_scanoff);
    size_t at = 0, z = 0;
    if (2 * nb > 0xFFFFFFFFu)
        return -1;
    pom_stage_inputs(L, h, B);
    stage_scan(L, &K->scan, h, C->adepth);
    memset(h + K->o_pfrom, 0, 16 * nb);
    memset(h + K->o_pto, 0, 16 * nb);
    memset(h + K->o_plen, 0, 8 * nb);
    for (size_t i = 0; i < nb; i++) {
        const size_t b = L->ids[i], dl = sp_dl(B, b);
        hd[i] = C->hdr[b];
        h[K->o_sd + i] = C->sd[b];
        no[i] = K->o_new + at;
        nc[i] = (uint32_t)dl;
        at += POM_ALIGN_UP(dl, 16);
        eso[i] = sco[i];
        eso[nb + i] = no[i];
    }
    for (size_t k = 0; k < 2 * nb; k++) {
        const size_t room = pom_split_stream_room(sp_dl(B, L->ids[k % nb]));
        edo[k] = K->o_z + z;
        edc[k] = (uint32_t)room;
        z += room;
    }
    return 0;
}

static int sp_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct itb_split_layout *K = &L->u.split;
    uint8_t *d = S->dmem, *res = d + K->o_res;
    const uint32_t nb = (uint32_t)L->nb;
    struct pom_split_result *result = (struct pom_split_result *)(res + K->r_result);
    (void)B;
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    if (pom_itb_split_dev(d, (const uint64_t *)(d + K->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                          (const int32_t *)(d + L->o_status), d + K->scan.o_adepth,
                          (const struct pom_check_hdr *)(d + K->o_hdr), d + K->o_sd, nb, d,
                          (const uint64_t *)(d + K->o_newoff), (const uint32_t *)(d + K->o_newcap), result,
                          d + K->o_sscr, S->stream) != 0)
        return -1;
    if (lzo_mi355x_launch_itb_split_lens(result, nb, (uint32_t *)(d + K->o_esrclen), S->stream) != 0)
        return -1;
    if (lzo_mi355x_compress_dev(d, (const uint64_t *)(d + K->o_esrcoff), (const uint32_t *)(d + K->o_esrclen), d,
                                (const uint64_t *)(d + K->o_edstoff), (const uint32_t *)(d + K->o_edstcap),
                                (uint32_t *)(res + K->r_elen), (int32_t *)(res + K->r_est), 2 * nb, d + K->o_escr,
                                S->stream) != 0)
        return -1;
    /* status, then out_len: adjacent among the inputs and among the results */
    if (hipMemcpyAsync(res + K->r_status, d + L->o_status, 8 * L->nb, hipMemcpyDeviceToDevice, S->stream) != hipSuccess)
        return -1;
    return hipMemcpyAsync(S->hmem + K->o_hres, res, K->res_bytes, hipMemcpyDeviceToHost, S->stream) == hipSuccess
               ? 0 : -1;
}

/* Half k (0 ... 2 * nb) of the chunk as it is delivered: the bytes, and whether they are its stream. */
static size_t sp_half(const struct layout *L, const uint8_t *h, size_t k, int *lzo)
{
    const struct itb_split_layout *K = &L->u.split;
    const uint8_t *res = h + K->o_hres;
    const size_t i = k % L->nb;
    struct pom_split_result r;
    memcpy(&r, res + K->r_result + sizeof r * i, sizeof r);
    const uint32_t ulen = k < L->nb ? r.old_len : r.new_len;
    const uint32_t z = ((const uint32_t *)(res + K->r_elen))[k];
    *lzo = 0;
    if (r.err != 0 || r.moved == 0 || ulen < POM_ITB_SIZE)
        return 0;
    *lzo = z < ulen - (POM_ITB_SIZE - POM_ITB_ITE_OFF);
    return *lzo ? z : ulen - (POM_ITB_SIZE - POM_ITB_ITE_OFF);
}

static int sp_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    const struct itb_split_layout *K = &L->u.split;
    uint8_t *d = S->dmem, *h = S->hmem;
    const size_t nb = L->nb;
    uint64_t *pf = (uint64_t *)(h + K->o_pfrom), *pt = (uint64_t *)(h + K->o_pto);
    uint32_t *pl = (uint32_t *)(h + K->o_plen);
    const uint64_t *eso = (const uint64_t *)(h + K->o_esrcoff), *edo = (const uint64_t *)(h + K->o_edstoff);
    const int32_t *est = (const int32_t *)(h + K->o_hres + K->r_est);
    size_t total = 0;
    (void)B;
    for (size_t k = 0; k < 2 * nb; k++) {
        int lzo;
        const size_t n = sp_half(L, h, k, &lzo);
        if (n && est[k] != 0)
            return -1;                              /* (the slots hold any stream: the encoder cannot fail) */
        pf[k] = lzo ? edo[k] : eso[k];
        pt[k] = total;
        pl[k] = (uint32_t)n;
        total += POM_ALIGN_UP(n, 16);
    }
    if (total > K->pcap)
        return -1;
    if (total &&
        (hipMemcpyAsync(d + K->o_pfrom, pf, 32 * nb, hipMemcpyHostToDevice, S->stream) != hipSuccess ||
         hipMemcpyAsync(d + K->o_plen, pl, 8 * nb, hipMemcpyHostToDevice, S->stream) != hipSuccess ||
         lzo_mi355x_launch_pack(d, (const uint64_t *)(d + K->o_pfrom), (const uint32_t *)(d + K->o_plen),
                                (const uint32_t *)(d + K->o_plen), (const uint64_t *)(d + K->o_pto), d + K->o_pack,
                                (uint32_t)(2 * nb), S->stream) != 0 ||
         hipMemcpyAsync(h + K->o_hrec, d + K->o_pack, total, hipMemcpyDeviceToHost, S->stream) != hipSuccess))
        return -1;
    *packed = total;
    return 0;
}

static int sp_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct pom_split_sink *C = B->sink;
    const struct itb_split_layout *K = &L->u.split;
    const uint8_t *h = S->hmem, *res = h + K->o_hres;
    const size_t nb = L->nb;
    const int32_t *st = (const int32_t *)(res + K->r_status);
    const uint32_t *ol = (const uint32_t *)(res + K->r_outlen);
    const uint64_t *pt = (const uint64_t *)(h + K->o_pto);
    for (size_t i = 0; i < nb; i++) {
        const size_t b = L->ids[i], to = C->idx[b];
        struct pom_split_result *r = &C->result[to];
        int lzo_o, lzo_n;
        const size_t no = sp_half(L, h, i, &lzo_o), nn = sp_half(L, h, nb + i, &lzo_n);
        C->status[b] = st[i];
        C->out_len[b] = ol[i];
        C->delivered[b] = 1;
        memcpy(r, res + K->r_result + sizeof *r * i, sizeof *r);
        C->err[to] = r->err;
        C->old_len[to] = C->new_len[to] = 0;
        if (r->err != 0 || r->moved == 0)
            continue;
        if (POM_ITBH_SIZE + no > C->out_cap[to] || POM_ITBH_SIZE + nn > C->out_cap[to]) {
            C->err[to] = LZO_E_OUTPUT_OVERRUN;
            continue;
        }
        if (pom_itb_split_headers(C->rec_hdr[b], C->sd[b], r, lzo_o ? (uint32_t)no : POM_SPLIT_NO_STREAM,
                                  lzo_n ? (uint32_t)nn : POM_SPLIT_NO_STREAM, C->old_out[to], C->new_out[to]) < 0)
            return -1;
        memcpy(C->old_out[to] + POM_ITBH_SIZE, h + K->o_hrec + pt[i], no);
        memcpy(C->new_out[to] + POM_ITBH_SIZE, h + K->o_hrec + pt[nb + i], nn);
        C->old_len[to] = POM_ITBH_SIZE + no;
        C->new_len[to] = POM_ITBH_SIZE + nn;
    }
    return 0;
}

/* (an undelivered ITB: the caller sees it in `delivered`) */
static const struct chunk_ops sp_ops = {"itb split", 0, sp_cap, sp_extra_cost, NULL, sp_layout,
                                        sp_stage, sp_kernels, sp_collect, sp_unpack};

int pom_itb_split_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                          struct pom_split_sink *sink)
{
    struct hbatch B = {.ops = &sp_ops, .src = src, .src_len = src_len, .status = sink->status, .is_lzo = sink->is_lzo,
                       .sink = sink};
    return pom_host_batch(&B, nblocks);
}

/* ------------------------------------------------------------------------ */
/* The ITB sweep: decode, check and sweep (itb_sweep.hip), encode           */
/* ------------------------------------------------------------------------ */
/* The split's partition and order with one payload a block.  Kernels on the
 * chunk's stream: the decoders; pom_itb_sweep_dev, which rewrites each
 * payload's bitmap and index in place; the gather of the encoder's nb source
 * lengths from the results; lzo_mi355x_compress_dev over the payloads where
 * they lie.  The results (the decoders' words, the 32-byte results, the
 * encoder's out_len and status) come back in one copy queued behind the
 * kernels.  Once they are back the host applies itb_lzo_compress's
 * not-smaller rule, and the pack kernel gathers exactly what is delivered --
 * the stream, or the payload when it did not compress -- for the second D2H.
 * A block nothing was removed from delivers nothing: its stored record is
 * still right.  Staging: pom_layout_sweep (host_layout.h). */
static size_t sw_cap(const struct hbatch *B, size_t b)
{
    const struct pom_sweep_sink *C = B->sink;
    return C->cap[b];
}

static size_t sw_dl(const struct hbatch *B, size_t b)
{
    const struct pom_sweep_sink *C = B->sink;
    return C->is_lzo[b] ? B->cap[b] : B->src_len[b];
}

/* the chunk budget counts the stream slot, the delivered payload (device and host) and the small arrays */
static size_t sw_extra_cost(const struct hbatch *B, size_t b)
{
    const struct pom_sweep_sink *C = B->sink;
    const size_t dl = C->is_lzo[b] ? C->cap[b] : B->src_len[b];
    return 2 * dl + pom_split_stream_room(dl) + 256;
}

static void sw_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    pom_layout_sweep(L, ids, nb, nlzo, B->src_len, B->cap, lzo_mi355x_decompress_scratch((uint32_t)nlzo),
                     pom_itb_sweep_scratch((uint32_t)nb), lzo_mi355x_compress_scratch((uint32_t)nb));
}

static int sw_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct pom_sweep_sink *C = B->sink;
    const struct itb_sweep_layout *K = &L->u.sweep;
    const size_t nb = L->nb;
    struct pom_check_hdr *hd = (struct pom_check_hdr *)(h + K->o_hdr);
    uint64_t *edo = (uint64_t *)(h + K->o_edstoff);
    uint32_t *edc = (uint32_t *)(h + K->o_edstcap), *bud = (uint32_t *)(h + K->o_budget);
    size_t z = 0;
    if (nb > 0xFFFFFFFFu)
        return -1;
    pom_stage_inputs(L, h, B);
    stage_scan(L, &K->scan, h, C->adepth);
    memset(h + K->o_pfrom, 0, 8 * nb);
    memset(h + K->o_pto, 0, 8 * nb);
    memset(h + K->o_plen, 0, 4 * nb);
    for (size_t i = 0; i < nb; i++) {
        const size_t b = L->ids[i], room = pom_split_stream_room(sw_dl(B, b));
        hd[i] = C->hdr[b];
        bud[i] = C->budget[b];
        edo[i] = K->o_z + z;
        edc[i] = (uint32_t)room;
        z += room;
    }
    return 0;
}

static int sw_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct itb_sweep_layout *K = &L->u.sweep;
    uint8_t *d = S->dmem, *res = d + K->o_res;
    const uint32_t nb = (uint32_t)L->nb;
    struct pom_sweep_result *result = (struct pom_sweep_result *)(res + K->r_result);
    (void)B;
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    if (pom_itb_sweep_dev(d, (const uint64_t *)(d + K->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                          (const int32_t *)(d + L->o_status), d + K->scan.o_adepth,
                          (const struct pom_check_hdr *)(d + K->o_hdr), (const uint32_t *)(d + K->o_budget), nb, result,
                          d + K->o_sscr, S->stream) != 0)
        return -1;
    if (lzo_mi355x_launch_itb_sweep_lens(result, nb, (uint32_t *)(d + K->o_esrclen), S->stream) != 0)
        return -1;
    if (lzo_mi355x_compress_dev(d, (const uint64_t *)(d + K->scan.o_scanoff), (const uint32_t *)(d + K->o_esrclen), d,
                                (const uint64_t *)(d + K->o_edstoff), (const uint32_t *)(d + K->o_edstcap),
                                (uint32_t *)(res + K->r_elen), (int32_t *)(res + K->r_est), nb, d + K->o_escr,
                                S->stream) != 0)
        return -1;
    /* status, then out_len: adjacent among the inputs and among the results */
    if (hipMemcpyAsync(res + K->r_status, d + L->o_status, 8 * L->nb, hipMemcpyDeviceToDevice, S->stream) != hipSuccess)
        return -1;
    return hipMemcpyAsync(S->hmem + K->o_hres, res, K->res_bytes, hipMemcpyDeviceToHost, S->stream) == hipSuccess
               ? 0 : -1;
}

/* Block i of the chunk as it is delivered: the bytes, and whether they are its stream. */
static size_t sw_payload(const struct layout *L, const uint8_t *h, size_t i, int *lzo)
{
    const struct itb_sweep_layout *K = &L->u.sweep;
    const uint8_t *res = h + K->o_hres;
    struct pom_sweep_result r;
    memcpy(&r, res + K->r_result + sizeof r * i, sizeof r);
    const uint32_t z = ((const uint32_t *)(res + K->r_elen))[i];
    *lzo = 0;
    if (r.err != 0 || r.removed == 0 || r.len < POM_ITB_SIZE)
        return 0;
    *lzo = z < r.len - (POM_ITB_SIZE - POM_ITB_ITE_OFF);
    return *lzo ? z : r.len - (POM_ITB_SIZE - POM_ITB_ITE_OFF);
}

static int sw_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    const struct itb_sweep_layout *K = &L->u.sweep;
    uint8_t *d = S->dmem, *h = S->hmem;
    const size_t nb = L->nb;
    uint64_t *pf = (uint64_t *)(h + K->o_pfrom), *pt = (uint64_t *)(h + K->o_pto);
    uint32_t *pl = (uint32_t *)(h + K->o_plen);
    const uint64_t *eso = (const uint64_t *)(h + K->scan.o_scanoff), *edo = (const uint64_t *)(h + K->o_edstoff);
    const int32_t *est = (const int32_t *)(h + K->o_hres + K->r_est);
    size_t total = 0;
    (void)B;
    for (size_t i = 0; i < nb; i++) {
        int lzo;
        const size_t n = sw_payload(L, h, i, &lzo);
        if (n && est[i] != 0)
            return -1;                              /* (the slots hold any stream: the encoder cannot fail) */
        pf[i] = lzo ? edo[i] : eso[i];
        pt[i] = total;
        pl[i] = (uint32_t)n;
        total += POM_ALIGN_UP(n, 16);
    }
    if (total > K->pcap)
        return -1;
    if (total &&
        (hipMemcpyAsync(d + K->o_pfrom, pf, 16 * nb, hipMemcpyHostToDevice, S->stream) != hipSuccess ||
         hipMemcpyAsync(d + K->o_plen, pl, 4 * nb, hipMemcpyHostToDevice, S->stream) != hipSuccess ||
         lzo_mi355x_launch_pack(d, (const uint64_t *)(d + K->o_pfrom), (const uint32_t *)(d + K->o_plen),
                                (const uint32_t *)(d + K->o_plen), (const uint64_t *)(d + K->o_pto), d + K->o_pack,
                                (uint32_t)nb, S->stream) != 0 ||
         hipMemcpyAsync(h + K->o_hrec, d + K->o_pack, total, hipMemcpyDeviceToHost, S->stream) != hipSuccess))
        return -1;
    *packed = total;
    return 0;
}

static int sw_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct pom_sweep_sink *C = B->sink;
    const struct itb_sweep_layout *K = &L->u.sweep;
    const uint8_t *h = S->hmem, *res = h + K->o_hres;
    const size_t nb = L->nb;
    const int32_t *st = (const int32_t *)(res + K->r_status);
    const uint32_t *ol = (const uint32_t *)(res + K->r_outlen);
    const uint64_t *pt = (const uint64_t *)(h + K->o_pto);
    for (size_t i = 0; i < nb; i++) {
        const size_t b = L->ids[i], to = C->idx[b];
        struct pom_sweep_result *r = &C->result[to];
        int lzo;
        const size_t n = sw_payload(L, h, i, &lzo);
        C->status[b] = st[i];
        C->out_len[b] = ol[i];
        C->delivered[b] = 1;
        memcpy(r, res + K->r_result + sizeof *r * i, sizeof *r);
        C->err[to] = r->err;
        C->rec_len[to] = 0;
        if (r->err != 0 || r->removed == 0)
            continue;
        if (POM_ITBH_SIZE + n > C->out_cap[to]) {
            C->err[to] = LZO_E_OUTPUT_OVERRUN;
            continue;
        }
        if (pom_itb_sweep_header(C->rec_hdr[b], r, lzo ? (uint32_t)n : POM_SPLIT_NO_STREAM, C->out[to]) < 0)
            return -1;
        memcpy(C->out[to] + POM_ITBH_SIZE, h + K->o_hrec + pt[i], n);
        C->rec_len[to] = POM_ITBH_SIZE + n;
    }
    return 0;
}

/* (an undelivered ITB: the caller sees it in `delivered`) */
static const struct chunk_ops sw_ops = {"itb sweep", 0, sw_cap, sw_extra_cost, NULL, sw_layout,
                                        sw_stage, sw_kernels, sw_collect, sw_unpack};

int pom_itb_sweep_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                          struct pom_sweep_sink *sink)
{
    struct hbatch B = {.ops = &sw_ops, .src = src, .src_len = src_len, .status = sink->status, .is_lzo = sink->is_lzo,
                       .sink = sink};
    return pom_host_batch(&B, nblocks);
}

/* ------------------------------------------------------------------------ */
/* The ITB unlink: decode, check and unlink (itb_unlink.hip), encode          */
/* ------------------------------------------------------------------------ */
/* The request operations' partition, staging and scatter (an ITB and all its
 * requests are in one chunk, the requests in block order and then the caller's
 * own, renumbered to the chunk's ITB index, their names in a blob of the
 * chunk's own) with the sweep's writer half.  Kernels on the chunk's stream:
 * the decoders; pom_itb_unlink_dev, which applies each block's requests in
 * order and rewrites its payload in place; the gather of the encoder's nb
 * source lengths from the results; lzo_mi355x_compress_dev over the payloads
 * where they lie.  The results (the decoders' words, the 32-byte results, the
 * encoder's out_len and status, four words and a 136-byte record a request)
 * come back in one copy queued behind the kernels.  Once they are back the
 * host applies itb_lzo_compress's not-smaller rule, and the pack kernel
 * gathers exactly what is delivered -- the stream, or the payload when it did
 * not compress -- for the second D2H.  A block no request changed delivers no
 * payload: its stored record is still right.  Staging: pom_layout_unlink
 * (host_layout.h). */
static size_t ul_cap(const struct hbatch *B, size_t b)
{
    const struct pom_unlink_sink *U = B->sink;
    return U->K->cap[b];
}

static size_t ul_dl(const struct hbatch *B, size_t b)
{
    const struct pom_unlink_sink *U = B->sink;
    return U->K->is_lzo[b] ? B->cap[b] : B->src_len[b];
}

/* the chunk budget counts the sweep's part and the requests' */
static size_t ul_extra_cost(const struct hbatch *B, size_t b)
{
    const struct pom_unlink_sink *U = B->sink;
    const struct pom_req_sink *K = U->K;
    const size_t dl = K->is_lzo[b] ? K->cap[b] : B->src_len[b];
    size_t blob = 0;
    const size_t nreq = pom_req_block(K, b, &blob);
    return 2 * dl + pom_split_stream_room(dl) + 256 + nreq * (POM_REQ_SIZE + 4 * K->spec->nwords + K->spec->rec_fixed) +
           blob;
}

static void ul_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    const struct pom_unlink_sink *U = B->sink;
    size_t nreq = 0, blob = 0;
    for (size_t i = 0; i < nb; i++)
        nreq += pom_req_block(U->K, ids[i], &blob);
    pom_layout_unlink(L, ids, nb, nlzo, B->src_len, B->cap, U->K->spec, nreq, blob,
                      lzo_mi355x_decompress_scratch((uint32_t)nlzo), pom_itb_unlink_scratch((uint32_t)nb),
                      lzo_mi355x_compress_scratch((uint32_t)nb));
}

static int ul_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct pom_unlink_sink *U = B->sink;
    const struct itb_unlink_layout *K = &L->u.unlink;
    const size_t nb = L->nb;
    struct pom_check_hdr *hd = (struct pom_check_hdr *)(h + K->o_hdr);
    uint64_t *edo = (uint64_t *)(h + K->o_edstoff);
    uint32_t *edc = (uint32_t *)(h + K->o_edstcap), *rf = (uint32_t *)(h + K->o_reqfirst);
    size_t z = 0, at = 0;
    if (nb > 0xFFFFFFFFu || pom_req_stage(L, h, U->K) != 0)
        return -1;
    pom_stage_inputs(L, h, B);
    stage_scan(L, &K->req.scan, h, U->K->adepth);
    memset(h + K->o_pfrom, 0, 8 * nb);
    memset(h + K->o_pto, 0, 8 * nb);
    memset(h + K->o_plen, 0, 4 * nb);
    for (size_t i = 0; i < nb; i++) {
        const size_t b = L->ids[i], room = pom_split_stream_room(ul_dl(B, b));
        hd[i] = U->hdr[b];
        rf[i] = (uint32_t)at;
        at += U->K->req_first[b + 1] - U->K->req_first[b];
        edo[i] = K->o_z + z;
        edc[i] = (uint32_t)room;
        z += room;
    }
    rf[nb] = (uint32_t)at;
    return 0;
}

static int ul_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct pom_unlink_sink *U = B->sink;
    const struct itb_unlink_layout *K = &L->u.unlink;
    const struct req_layout *Y = &K->req;
    uint8_t *d = S->dmem, *res = d + Y->o_res;
    const uint32_t nb = (uint32_t)L->nb;
    struct pom_unlink_result *result = (struct pom_unlink_result *)(res + K->r_result);
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    if (pom_itb_unlink_dev(d, (const uint64_t *)(d + Y->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                           (const int32_t *)(d + L->o_status), d + Y->scan.o_adepth,
                           (const struct pom_check_hdr *)(d + K->o_hdr), nb, U->async_unlink,
                           (const struct pom_lookup_req *)(d + Y->o_req), (const uint32_t *)(d + K->o_reqfirst),
                           (uint32_t)Y->nreq, d + Y->o_blob, (uint32_t)Y->blob_bytes,
                           (int32_t *)(res + Y->r_word[RW_ERR]), (uint32_t *)(res + Y->r_word[RW_NR]),
                           (uint32_t *)(res + Y->r_word[RW_DEPTH]), (uint32_t *)(res + Y->r_word[RW_LEN]),
                           res + Y->res_hdr, result, d + K->o_sscr, S->stream) != 0)
        return -1;
    if (lzo_mi355x_launch_itb_unlink_lens(result, nb, (uint32_t *)(d + K->o_esrclen), S->stream) != 0)
        return -1;
    if (lzo_mi355x_compress_dev(d, (const uint64_t *)(d + Y->scan.o_scanoff), (const uint32_t *)(d + K->o_esrclen), d,
                                (const uint64_t *)(d + K->o_edstoff), (const uint32_t *)(d + K->o_edstcap),
                                (uint32_t *)(res + K->r_elen), (int32_t *)(res + K->r_est), nb, d + K->o_escr,
                                S->stream) != 0)
        return -1;
    /* status, then out_len: adjacent among the inputs and among the results */
    if (hipMemcpyAsync(res + K->r_status, d + L->o_status, 8 * L->nb, hipMemcpyDeviceToDevice, S->stream) != hipSuccess)
        return -1;
    return hipMemcpyAsync(S->hmem + Y->o_hres, res, Y->res_bytes, hipMemcpyDeviceToHost, S->stream) == hipSuccess
               ? 0 : -1;
}

/* Block i of the chunk as it is delivered: the bytes, and whether they are its stream. */
static size_t ul_payload(const struct layout *L, const uint8_t *h, size_t i, int *lzo)
{
    const struct itb_unlink_layout *K = &L->u.unlink;
    const uint8_t *res = h + K->req.o_hres;
    struct pom_unlink_result r;
    memcpy(&r, res + K->r_result + sizeof r * i, sizeof r);
    const uint32_t z = ((const uint32_t *)(res + K->r_elen))[i];
    *lzo = 0;
    if (r.err != 0 || r.changed == 0 || r.len < POM_ITB_SIZE)
        return 0;
    *lzo = z < r.len - (POM_ITB_SIZE - POM_ITB_ITE_OFF);
    return *lzo ? z : r.len - (POM_ITB_SIZE - POM_ITB_ITE_OFF);
}

static int ul_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    const struct itb_unlink_layout *K = &L->u.unlink;
    uint8_t *d = S->dmem, *h = S->hmem;
    const size_t nb = L->nb;
    uint64_t *pf = (uint64_t *)(h + K->o_pfrom), *pt = (uint64_t *)(h + K->o_pto);
    uint32_t *pl = (uint32_t *)(h + K->o_plen);
    const uint64_t *eso = (const uint64_t *)(h + K->req.scan.o_scanoff), *edo = (const uint64_t *)(h + K->o_edstoff);
    const int32_t *est = (const int32_t *)(h + K->req.o_hres + K->r_est);
    size_t total = 0;
    (void)B;
    for (size_t i = 0; i < nb; i++) {
        int lzo;
        const size_t n = ul_payload(L, h, i, &lzo);
        if (n && est[i] != 0)
            return -1;                              /* (the slots hold any stream: the encoder cannot fail) */
        pf[i] = lzo ? edo[i] : eso[i];
        pt[i] = total;
        pl[i] = (uint32_t)n;
        total += POM_ALIGN_UP(n, 16);
    }
    if (total > K->pcap)
        return -1;
    if (total &&
        (hipMemcpyAsync(d + K->o_pfrom, pf, 16 * nb, hipMemcpyHostToDevice, S->stream) != hipSuccess ||
         hipMemcpyAsync(d + K->o_plen, pl, 4 * nb, hipMemcpyHostToDevice, S->stream) != hipSuccess ||
         lzo_mi355x_launch_pack(d, (const uint64_t *)(d + K->o_pfrom), (const uint32_t *)(d + K->o_plen),
                                (const uint32_t *)(d + K->o_plen), (const uint64_t *)(d + K->o_pto), d + K->o_pack,
                                (uint32_t)nb, S->stream) != 0 ||
         hipMemcpyAsync(h + K->o_hrec, d + K->o_pack, total, hipMemcpyDeviceToHost, S->stream) != hipSuccess))
        return -1;
    *packed = total;
    return 0;
}

static int ul_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct pom_unlink_sink *U = B->sink;
    const struct itb_unlink_layout *K = &L->u.unlink;
    const uint8_t *h = S->hmem, *res = h + K->req.o_hres;
    const size_t nb = L->nb;
    const int32_t *st = (const int32_t *)(res + K->r_status);
    const uint32_t *ol = (const uint32_t *)(res + K->r_outlen);
    const uint64_t *pt = (const uint64_t *)(h + K->o_pto);
    pom_req_scatter(L, h, U->K, NULL, 0);
    for (size_t i = 0; i < nb; i++) {
        const size_t b = L->ids[i], to = U->idx[b];
        struct pom_unlink_result *r = &U->result[to];
        int lzo;
        const size_t n = ul_payload(L, h, i, &lzo);
        U->status[b] = st[i];
        U->out_len[b] = ol[i];
        U->delivered[b] = 1;
        memcpy(r, res + K->r_result + sizeof *r * i, sizeof *r);
        U->err[to] = r->err;
        U->rec_len[to] = 0;
        if (r->err != 0 || r->changed == 0)
            continue;
        if (POM_ITBH_SIZE + n > U->out_cap[to]) {
            U->err[to] = LZO_E_OUTPUT_OVERRUN;
            continue;
        }
        if (pom_itb_unlink_header(U->rec_hdr[b], r, lzo ? (uint32_t)n : POM_SPLIT_NO_STREAM, U->out[to]) < 0)
            return -1;
        memcpy(U->out[to] + POM_ITBH_SIZE, h + K->o_hrec + pt[i], n);
        U->rec_len[to] = POM_ITBH_SIZE + n;
    }
    return 0;
}

/* (an undelivered ITB: the caller sees it in `delivered`; its requests keep what pom_req_begin put there) */
static const struct chunk_ops ul_ops = {"itb unlink", 0, ul_cap, ul_extra_cost, NULL, ul_layout,
                                        ul_stage, ul_kernels, ul_collect, ul_unpack};

int pom_itb_unlink_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                           struct pom_unlink_sink *sink)
{
    struct hbatch B = {.ops = &ul_ops, .src = src, .src_len = src_len, .status = sink->K->status,
                       .is_lzo = sink->K->is_lzo, .sink = sink};
    return pom_host_batch(&B, nblocks);
}
