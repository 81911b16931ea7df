/*
 * host_records.c -- the record operations of the host batches: what runs
 * behind the decode of a chunk's LZO blocks, through the chunk pipeline of
 * lzo_host.c (host_pipeline.h).  The three walks -- the GC scan
 * (itb_scan.hip), the directory listing (itb_dents.hip), the key/value
 * listing (itb_keys.hip) -- share one layout, one staging and one delivery,
 * told apart by their list of result words and their record unit; the column
 * read (col_slice.hip), the lookup (itb_find.hip) and the key/value get
 * (itb_kvget.hip) carry requests.  Their callers (gc_scan.c, readdir.c,
 * kvlist.c, column_codec.c, lookup.c, kvget.c) select
 * the blocks and put the results in the caller's order.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "host_pipeline.h"
#include "lzo_mi355x.h"
#include "minilzo.h"
#include "pom_column.h"
#include "pom_kvget.h"
#include "pom_kvlist.h"
#include "pom_lookup.h"

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
 * No other decoded byte leaves the device. */
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

/* A chunk's records, kept until the caller has placed them (pad: the records start 16-byte aligned). */
struct pom_walk_buf {
    struct pom_walk_buf *next;
    uint64_t pad;
    uint8_t bytes[];
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
    pthread_mutex_lock(&G->mu);
    buf->next = G->bufs;
    G->bufs = buf;
    pthread_mutex_unlock(&G->mu);
    return 0;
}

void pom_walk_sink_free(struct pom_walk_sink *sink)
{
    while (sink->bufs) {
        struct pom_walk_buf *next = sink->bufs->next;
        free(sink->bufs);
        sink->bufs = next;
    }
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
/* Lookups: decode, chain walk (itb_find.hip), matched MDUs back              */
/* ------------------------------------------------------------------------ */
/* The walks' partition (LZO records first, stored ones walked as staged) with
 * the column reads' requests: an ITB and all its requests are in one chunk;
 * request j of the chunk is the j-th in block order, then in the block's own
 * order, renumbered to the chunk's ITB index, its name staged in a blob of the
 * chunk's own.  A request whose name the caller's blob does not hold, or whose
 * namelen is above 255, gets no name bytes and a name_off past the chunk's
 * blob: the kernel's rule 4 refuses it, behind rules 1 to 3 as everywhere.
 * Every result has a fixed size, so one copy of a known size brings them back,
 * queued once the chunk's kernels are done (the column reads say why).  The
 * decoder's status reaches the host through the requests' err.  Staging (host
 * and device alike up to the inputs' end; pom_layout_lookup):
 *   [src_off u64][dst_off u64][scan_off u64][requests, nreq][src_len u32][dst_cap u32]
 *   [status i32][out_len u32][adepth u8]
 *   [src bytes, 16-B aligned per block][names]
 *   device: [decoded payloads][decoder scratch]
 *   both:   [err i32, nreq][nr u32, nreq][depth u32, nreq][records, 136 * nreq]  <- D2H, one copy
 * No other decoded byte leaves the device. */
static int lk_name_ok(const struct pom_lookup_sink *K, const struct pom_lookup_req *q)
{
    return q->namelen <= 255 && (size_t)q->name_off + q->namelen <= K->names_len;
}

static size_t lk_name_bytes(const struct pom_lookup_sink *K, const struct pom_lookup_req *q)
{
    return lk_name_ok(K, q) ? q->namelen : 0;
}

static size_t lk_cap(const struct hbatch *B, size_t b)
{
    const struct pom_lookup_sink *K = B->sink;
    return K->cap[b];
}

static size_t lk_names(const struct pom_lookup_sink *K, size_t b)
{
    size_t n = 0;
    for (size_t k = K->req_first[b]; k < K->req_first[b + 1]; k++)
        n += lk_name_bytes(K, &K->req[K->req_ids[k]]);
    return n;
}

/* the chunk budget counts the requests, their names and their results (err, nr, depth, record) */
static size_t lk_extra_cost(const struct hbatch *B, size_t b)
{
    const struct pom_lookup_sink *K = B->sink;
    return (K->req_first[b + 1] - K->req_first[b]) *
               (sizeof(struct pom_lookup_req) + 3 * sizeof(uint32_t) + POM_LK_REC_SIZE) + lk_names(K, b);
}

static void lk_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    const struct pom_lookup_sink *K = B->sink;
    size_t nreq = 0, names = 0;
    for (size_t i = 0; i < nb; i++) {
        nreq += K->req_first[ids[i] + 1] - K->req_first[ids[i]];
        names += lk_names(K, ids[i]);
    }
    pom_layout_lookup(L, ids, nb, nlzo, B->src_len, B->cap, nreq, names,
                      lzo_mi355x_decompress_scratch((uint32_t)nlzo));
}

static int lk_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct pom_lookup_sink *K = B->sink;
    const struct lookup_layout *Y = &L->u.lk;
    if (Y->nreq > 0xFFFFFFFFu || Y->names_bytes > 0xFFFFFFF0u)
        return -1;
    struct pom_lookup_req *rq = (struct pom_lookup_req *)(h + Y->o_req);
    uint8_t *nm = h + Y->o_names;
    size_t j = 0, at = 0;
    pom_stage_inputs(L, h, B);
    stage_scan(L, &Y->scan, h, K->adepth);
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        for (size_t k = K->req_first[b]; k < K->req_first[b + 1]; k++, j++) {
            const struct pom_lookup_req *q = &K->req[K->req_ids[k]];
            const size_t n = lk_name_bytes(K, q);
            rq[j] = *q;
            rq[j].itb = (uint32_t)i;            /* the chunk's own ITB index */
            if (lk_name_ok(K, q)) {
                rq[j].name_off = (uint32_t)at;
                if (n)
                    memcpy(nm + at, K->names + q->name_off, n);
                at += n;
            } else {
                rq[j].name_off = 0xFFFFFFFFu;   /* outside the chunk's blob, as it was outside the caller's */
            }
        }
    }
    return 0;
}

static int lk_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct lookup_layout *Y = &L->u.lk;
    uint8_t *d = S->dmem, *res = d + Y->o_res;
    (void)B;
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    return lzo_mi355x_launch_lookup(d, (const uint64_t *)(d + Y->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                                    (const int32_t *)(d + L->o_status), d + Y->scan.o_adepth, (uint32_t)L->nb,
                                    (const struct pom_lookup_req *)(d + Y->o_req), (uint32_t)Y->nreq,
                                    d + Y->o_names, (uint32_t)Y->names_bytes, (int32_t *)(res + Y->r_err),
                                    (uint32_t *)(res + Y->r_nr), (uint32_t *)(res + Y->r_depth), res + Y->res_hdr,
                                    S->stream);
}

static int lk_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    (void)B;
    return results_back(S, L->u.lk.o_hres, L->u.lk.o_res, L->u.lk.res_bytes, packed);
}

/* The results go to their places in the caller's request order. */
static int lk_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    struct pom_lookup_sink *K = B->sink;
    const struct lookup_layout *Y = &L->u.lk;
    const uint8_t *res = S->hmem + Y->o_hres;
    const int32_t *he = (const int32_t *)(res + Y->r_err);
    const uint32_t *hn = (const uint32_t *)(res + Y->r_nr);
    const uint32_t *hd = (const uint32_t *)(res + Y->r_depth);
    const uint8_t *recs = res + Y->res_hdr;
    size_t j = 0;
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        K->status[b] = 0;                       /* delivered; the decoder's code is in the requests' err */
        for (size_t k = K->req_first[b]; k < K->req_first[b + 1]; k++, j++) {
            const size_t r = K->req_ids[k];
            K->err[r] = he[j];
            K->nr[r] = hn[j];
            K->depth[r] = hd[j];
            memcpy(K->out + POM_LK_REC_SIZE * r, recs + POM_LK_REC_SIZE * j, POM_LK_REC_SIZE);
        }
    }
    return 0;
}

/* (a lookup's requests: set by the caller, so nothing to mark unreached) */
static const struct chunk_ops lk_ops = {"lookup", 0, lk_cap, lk_extra_cost, NULL, lk_layout,
                                        lk_stage, lk_kernels, lk_collect, lk_unpack};

int pom_lookup_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                       struct pom_lookup_sink *sink)
{
    struct hbatch B = {.ops = &lk_ops, .src = src, .src_len = src_len, .status = sink->status,
                       .is_lzo = sink->is_lzo, .sink = sink};
    return pom_host_batch(&B, nblocks);
}

/* ------------------------------------------------------------------------ */
/* Key/value gets: decode, chain walk and copy (itb_kvget.hip), values back   */
/* ------------------------------------------------------------------------ */
/* The lookups' partition, request order and staging, with the string keys in
 * the names' place: a string request whose key the caller's blob does not
 * hold gets no key bytes and a skey_off past the chunk's blob (the kernel's
 * rule 4 refuses it); one with sklen above 320 gets no key bytes either and
 * matches nothing.  The records are variable-length, so they come back as the
 * walks' do: the fixed-size results and the chunk's record total in one copy
 * queued behind the kernels, exactly that many record bytes in a second one
 * sized once the first is back.  Staging (host and device alike up to the
 * inputs' end; pom_layout_kvget):
 *   [src_off u64][dst_off u64][scan_off u64][requests, nreq][src_len u32][dst_cap u32]
 *   [status i32][out_len u32][adepth u8]
 *   [src bytes, 16-B aligned per block][keys]
 *   device: [decoded payloads][decoder scratch][first u64, nreq]
 *   both:   [total u64][err i32][nr u32][depth u32][len u32][lease u64], nreq each  <- D2H, one copy
 *           [the chunk's records, packed, unless lengths only]                    <- D2H, sized after the first
 * No other decoded byte leaves the device. */
struct pom_kvget_buf {
    struct pom_kvget_buf *next;
    uint64_t pad;
    uint8_t bytes[];
};

static int kg_key_ok(const struct pom_kvget_sink *K, const struct pom_kvget_req *q)
{
    return (q->kvflag & POM_KV_STR) && q->sklen <= POM_KV_VALUE_MAX && (size_t)q->skey_off + q->sklen <= K->keys_len;
}

static size_t kg_key_bytes(const struct pom_kvget_sink *K, const struct pom_kvget_req *q)
{
    return kg_key_ok(K, q) ? q->sklen : 0;
}

static size_t kg_cap(const struct hbatch *B, size_t b)
{
    const struct pom_kvget_sink *K = B->sink;
    return K->cap[b];
}

static size_t kg_keys(const struct pom_kvget_sink *K, size_t b)
{
    size_t n = 0;
    for (size_t k = K->req_first[b]; k < K->req_first[b + 1]; k++)
        n += kg_key_bytes(K, &K->req[K->req_ids[k]]);
    return n;
}

/* the chunk budget counts the requests, their keys, their results and their records' room */
static size_t kg_extra_cost(const struct hbatch *B, size_t b)
{
    const struct pom_kvget_sink *K = B->sink;
    return (K->req_first[b + 1] - K->req_first[b]) *
               (sizeof(struct pom_kvget_req) + 4 * sizeof(uint32_t) + 2 * sizeof(uint64_t) +
                (K->lengths_only ? 0 : POM_KG_REC_MAX)) + kg_keys(K, b);
}

static void kg_layout(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const struct hbatch *B)
{
    const struct pom_kvget_sink *K = B->sink;
    size_t nreq = 0, keys = 0;
    for (size_t i = 0; i < nb; i++) {
        nreq += K->req_first[ids[i] + 1] - K->req_first[ids[i]];
        keys += kg_keys(K, ids[i]);
    }
    pom_layout_kvget(L, ids, nb, nlzo, B->src_len, B->cap, nreq, keys, !K->lengths_only,
                     lzo_mi355x_decompress_scratch((uint32_t)nlzo));
}

static int kg_stage(const struct layout *L, uint8_t *h, const struct hbatch *B)
{
    const struct pom_kvget_sink *K = B->sink;
    const struct kvget_layout *Y = &L->u.kg;
    if (Y->nreq > 0xFFFFFFFFu / POM_KG_REC_MAX || Y->keys_bytes > 0xFFFFFFF0u)
        return -1;
    struct pom_kvget_req *rq = (struct pom_kvget_req *)(h + Y->o_req);
    uint8_t *ky = h + Y->o_keys;
    size_t j = 0, at = 0;
    pom_stage_inputs(L, h, B);
    stage_scan(L, &Y->scan, h, K->adepth);
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        for (size_t k = K->req_first[b]; k < K->req_first[b + 1]; k++, j++) {
            const struct pom_kvget_req *q = &K->req[K->req_ids[k]];
            const size_t n = kg_key_bytes(K, q);
            rq[j] = *q;
            rq[j].itb = (uint32_t)i;            /* the chunk's own ITB index */
            if (kg_key_ok(K, q)) {
                rq[j].skey_off = (uint32_t)at;
                if (n)
                    memcpy(ky + at, K->keys + q->skey_off, n);
                at += n;
            } else {
                rq[j].skey_off = 0xFFFFFFFFu;   /* outside the chunk's blob (read by string gets of sklen <= 320 only) */
            }
        }
    }
    return 0;
}

static int kg_kernels(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    const struct kvget_layout *Y = &L->u.kg;
    uint8_t *d = S->dmem, *res = d + Y->o_res;
    size_t queued;
    (void)B;
    if (pom_decode_lzo_blocks(S, L, 0) != 0)
        return -1;
    if (lzo_mi355x_launch_kvget(d, (const uint64_t *)(d + Y->scan.o_scanoff), (const uint32_t *)(d + L->o_outlen),
                                (const int32_t *)(d + L->o_status), d + Y->scan.o_adepth, (uint32_t)L->nb,
                                (const struct pom_kvget_req *)(d + Y->o_req), (uint32_t)Y->nreq, d + Y->o_keys,
                                (uint32_t)Y->keys_bytes, (int32_t *)(res + Y->r_err), (uint32_t *)(res + Y->r_nr),
                                (uint32_t *)(res + Y->r_depth), (uint32_t *)(res + Y->r_len),
                                (uint64_t *)(res + Y->r_lease), (uint64_t *)(d + Y->o_first), d + Y->o_pack, Y->rcap,
                                S->stream) != 0)
        return -1;
    return results_back(S, Y->o_hres, Y->o_res, Y->res_bytes, &queued);
}

/* Once the lengths are back: the D2H of exactly the chunk's records. */
static int kg_collect(struct slot *S, const struct layout *L, const struct hbatch *B, size_t *packed)
{
    const struct pom_kvget_sink *K = B->sink;
    const struct kvget_layout *Y = &L->u.kg;
    uint64_t total;
    memcpy(&total, S->hmem + Y->o_hres, 8);
    if (K->lengths_only)
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
 * the records stay in a buffer of the sink until the caller knows the call's
 * own first[]. */
static int kg_unpack(struct slot *S, const struct layout *L, const struct hbatch *B)
{
    struct pom_kvget_sink *K = B->sink;
    const struct kvget_layout *Y = &L->u.kg;
    const uint8_t *res = S->hmem + Y->o_hres;
    const int32_t *he = (const int32_t *)(res + Y->r_err);
    const uint32_t *hn = (const uint32_t *)(res + Y->r_nr);
    const uint32_t *hd = (const uint32_t *)(res + Y->r_depth);
    const uint32_t *hl = (const uint32_t *)(res + Y->r_len);
    const uint64_t *hs = (const uint64_t *)(res + Y->r_lease);
    struct pom_kvget_buf *buf = malloc(sizeof(*buf) + L->packed);
    if (!buf)
        return -1;
    memcpy(buf->bytes, S->hmem + Y->o_hrec, L->packed);
    size_t j = 0, at = 0;
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i];
        K->status[b] = 0;                       /* delivered; the decoder's code is in the requests' err */
        for (size_t k = K->req_first[b]; k < K->req_first[b + 1]; k++, j++) {
            const size_t r = K->req_ids[k];
            K->err[r] = he[j];
            K->nr[r] = hn[j];
            K->depth[r] = hd[j];
            K->len[r] = hl[j];
            K->lease[r] = hs[j];
            K->recs[r] = !K->lengths_only && hl[j] && at + hl[j] <= L->packed ? buf->bytes + at : NULL;
            at += hl[j];
        }
    }
    pthread_mutex_lock(&K->mu);
    buf->next = K->bufs;
    K->bufs = buf;
    pthread_mutex_unlock(&K->mu);
    return 0;
}

void pom_kvget_sink_free(struct pom_kvget_sink *sink)
{
    while (sink->bufs) {
        struct pom_kvget_buf *next = sink->bufs->next;
        free(sink->bufs);
        sink->bufs = next;
    }
}

/* (a get's requests: set by the caller, so nothing to mark unreached) */
static const struct chunk_ops kg_ops = {"kvget", 0, kg_cap, kg_extra_cost, NULL, kg_layout,
                                        kg_stage, kg_kernels, kg_collect, kg_unpack};

int pom_kvget_chunked(const uint8_t *const *src, const size_t *src_len, size_t nblocks,
                      struct pom_kvget_sink *sink)
{
    struct hbatch B = {.ops = &kg_ops, .src = src, .src_len = src_len, .status = sink->status,
                       .is_lzo = sink->is_lzo, .sink = sink};
    return pom_host_batch(&B, nblocks);
}
