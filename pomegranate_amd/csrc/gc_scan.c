/*
 * gc_scan.c -- the MDSL garbage collector's data scan (include/pom_gc.h): per
 * ITB the decode switch and the bitmap walk of mdsl_gc_data_round
 * (mdsl/gc.c:945-993), batched.  The reassembly is here (the header checks
 * are host_requests.c's pom_itb_walk_header), and with it the front and back halves the three walks' batches share
 * (pom_walk_begin, pom_walk_finish); the chunks -- compressed payloads up, the
 * decoders, the walk (itb_scan.hip), counts and ranges back -- go through the
 * host batches' pipeline (host_records.c, gc_ops).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "host_requests.h"
#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_gc.h"
#include "pom_kvlist.h"
#include "pom_itb.h"

int pom_walk_begin(struct pom_walk_batch *W, const uint8_t *const *rec, const size_t *rec_len, size_t n,
                   const struct pom_walk_out *O)
{
    memset(W, 0, sizeof *W);
    pthread_mutex_init(&W->G.mu, NULL);
    W->n = n;
    W->idx = malloc((n + 1) * sizeof(*W->idx));
    W->src = malloc((n + 1) * sizeof(*W->src));
    W->slen = malloc((n + 1) * sizeof(*W->slen));
    W->cap = malloc((n + 1) * sizeof(*W->cap));
    W->flags = malloc(2 * n + 1);                               /* is_lzo[m], adepth[m] */
    W->i32 = malloc((3 * n + 1) * sizeof(*W->i32));             /* status[m], err[m], entries[m] */
    W->u32 = malloc((5 * n + 1) * sizeof(*W->u32));             /* out_len[m], live[m], count[m], bytes[m], keybytes[m] */
    W->recs = malloc((n + 1) * sizeof(*W->recs));
    W->to = malloc((n + 1) * sizeof(*W->to));                   /* the reassembly's copies: to[m], from recs[m] */
    W->fit = malloc((n + 1) * sizeof(*W->fit));
    W->masks = O->mask ? malloc((POM_KV_MASK_WORDS * n + 1) * sizeof(*W->masks)) : NULL;
    if (!W->idx || !W->src || !W->slen || !W->cap || !W->flags || !W->i32 || !W->u32 || !W->recs || !W->to ||
        !W->fit || (O->mask && !W->masks))
        return LZO_E_OUT_OF_MEMORY;
    uint8_t *is_lzo = W->flags, *adepth = W->flags + n;
    W->entries = W->i32 + 2 * n;
    size_t m = 0;
    for (size_t b = 0; b < n; b++) {
        O->live[b] = 0;
        O->err[b] = -EINVAL;
        if (O->dnum)
            O->dnum[b] = 0;
        if (O->keybytes)
            O->keybytes[b] = 0;
        if (O->mask)
            memset(O->mask + POM_KV_MASK_WORDS * b, 0, 8 * POM_KV_MASK_WORDS);
        if (O->len_ok)
            O->len_ok[b] = 0;
        if (O->entries_ok)
            O->entries_ok[b] = 0;
        struct pom_walk_block w;
        if (pom_itb_walk_header(rec[b], rec_len[b], &w) != 0 || (O->listing && w.entries < 0))
            continue;
        if (O->listing && w.entries == 0) {
            /* mds/itb.c:2540-2544 and 2479-2482: the reference leaves before the bitmap */
            O->err[b] = 0;
            if (O->entries_ok)
                O->entries_ok[b] = 1;
            continue;
        }
        W->idx[m] = b;
        W->src[m] = w.src;
        W->slen[m] = w.src_len;
        is_lzo[m] = w.is_lzo;
        W->cap[m] = w.cap;
        adepth[m] = w.adepth;
        W->entries[m] = w.entries;
        m++;
    }
    W->m = m;
    W->G.is_lzo = is_lzo;
    W->G.cap = W->cap;
    W->G.adepth = adepth;
    W->G.status = W->i32;
    W->G.err = W->i32 + n;
    W->G.out_len = W->u32;
    W->G.live = W->u32 + n;
    W->G.count = W->u32 + 2 * n;
    W->G.bytes = W->u32 + 3 * n;
    W->G.keybytes = W->u32 + 4 * n;
    W->G.mask = W->masks;
    W->G.recs = W->recs;
    return LZO_E_OK;
}

int pom_walk_finish(struct pom_walk_batch *W, int rc, const struct pom_walk_out *O)
{
    const struct pom_walk_sink *G = &W->G;
    const size_t n = W->n, m = W->m;
    if (rc != LZO_E_OK) {                       /* (pom_walk_begin's own: m is 0) */
        for (size_t k = 0; k < m; k++)
            O->err[W->idx[k]] = LZO_E_ERROR;
        goto out;
    }
    /* the chunks reordered the blocks: the global first[] and each ITB's records
     * in ITB order are put together here */
    size_t total = 0, k = 0;
    for (size_t b = 0; b < n; b++) {
        O->first[b] = total;
        if (k == m || W->idx[k] != b)
            continue;
        const int e = O->err[b] = G->status[k] != 0 ? G->status[k] : G->err[k];
        O->live[b] = G->live[k];
        if (O->len_ok)
            O->len_ok[b] = !G->is_lzo[k] || (G->status[k] == 0 && G->out_len[k] == W->cap[k]);
        if (O->entries_ok)
            O->entries_ok[b] = e == 0 && (int64_t)O->live[b] == W->entries[k];
        const size_t nr = e != 0 ? 0 : O->listing ? G->bytes[k] : G->count[k];
        if (O->dnum)
            O->dnum[b] = e == 0 ? G->count[k] : 0;
        if (O->keybytes)
            O->keybytes[b] = e == 0 ? G->keybytes[k] : 0;
        if (O->mask && e == 0)
            memcpy(O->mask + POM_KV_MASK_WORDS * b, W->masks + POM_KV_MASK_WORDS * k, 8 * POM_KV_MASK_WORDS);
        W->to[k] = O->out + O->unit * (total < O->out_cap ? total : O->out_cap);
        W->fit[k] = O->unit * (total >= O->out_cap ? 0 : nr < O->out_cap - total ? nr : O->out_cap - total);
        total += nr;
        k++;
    }
    O->first[n] = total;
    if (!O->listing) {
        for (k = 0; k < m; k++)
            if (W->fit[k])
                memcpy(W->to[k], G->recs[k], W->fit[k]);
    } else if (!O->count_only) {
        pom_copy_parallel(W->to, G->recs, W->fit, m);
    }
    rc = !O->count_only && total > O->out_cap ? POM_GC_E_NOSPACE : LZO_E_OK;
out:
    pom_walk_bufs_free(&W->G.bufs);
    pthread_mutex_destroy(&W->G.mu);
    free(W->idx);
    free(W->src);
    free(W->slen);
    free(W->cap);
    free(W->flags);
    free(W->i32);
    free(W->u32);
    free(W->recs);
    free(W->to);
    free(W->fit);
    free(W->masks);
    return rc;
}

int pom_gc_scan_dev(const uint8_t *payload, const uint64_t *payload_off,
                    const uint32_t *payload_len, const int32_t *status,
                    const uint8_t *adepth, uint32_t nitb, int column,
                    uint32_t *live, uint32_t *nranges, uint64_t *first,
                    struct pom_gc_range *ranges, uint64_t ranges_cap, int32_t *err,
                    void *stream)
{
    if (column < 0 || column >= (int)POM_ITE_COLUMNS)
        return -1;
    return lzo_mi355x_launch_gc_scan(payload, payload_off, payload_len, status, adepth, nitb,
                                     (uint32_t)column, live, nranges, first, ranges, ranges_cap, err,
                                     (hipStream_t)stream);
}

int pom_gc_scan_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int column,
                      struct pom_gc_range *ranges, size_t ranges_cap, size_t *first,
                      uint32_t *live, int *err, int *len_ok, int *entries_ok)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    if (column < 0 || column >= (int)POM_ITE_COLUMNS)
        return -EINVAL;
    /* no entries rule when selecting; the ranges are few: a plain memcpy each */
    const struct pom_walk_out O = {.out = (uint8_t *)ranges, .out_cap = ranges_cap, .unit = sizeof(*ranges),
                                   .first = first, .live = live, .err = err, .len_ok = len_ok,
                                   .entries_ok = entries_ok};
    struct pom_walk_batch W;
    int rc = pom_walk_begin(&W, rec, rec_len, n, &O);
    if (rc == LZO_E_OK) {
        W.G.column = column;
        rc = pom_gc_scan_chunked(W.src, W.slen, W.m, &W.G);
    }
    return pom_walk_finish(&W, rc, &O);
}
