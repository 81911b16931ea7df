/*
 * gc_scan.c -- the MDSL garbage collector's data scan (include/pom_gc.h): per
 * ITB the decode switch and the bitmap walk of mdsl_gc_data_round
 * (mdsl/gc.c:945-993), batched.  The header checks and the reassembly are
 * here; the chunks -- compressed payloads up, the decoders, the walk
 * (itb_scan.hip), counts and ranges back -- go through the host batches'
 * pipeline (lzo_host.c, OP_GC_SCAN).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_gc.h"
#include "pom_itb.h"

static uint32_t rd32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

static uint16_t rd16(const uint8_t *p)
{
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}

int pom_itb_walk_header(const uint8_t *rec, size_t rec_len, struct pom_walk_block *w)
{
    if (rec_len < POM_ITBH_SIZE)
        return -EINVAL;
    const uint32_t len = rd32(rec + POM_ITBH_LEN_OFF), zlen = rd32(rec + POM_ITBH_ZLEN_OFF);
    const uint16_t algo = rd16(rec + POM_ITBH_ALGO_OFF);
    const uint8_t ad = rec[POM_ITBH_ADEPTH_OFF];
    if (len < POM_ITBH_SIZE || len > rec_len || (algo != POM_COMPR_NONE && algo != POM_COMPR_LZO) ||
        ad == 0 || ad > POM_ITB_ADEPTH_MAX)
        return -EINVAL;
    if (algo == POM_COMPR_LZO &&
        (zlen <= POM_ITBH_SIZE || zlen - POM_ITBH_SIZE > POM_ITB_PAYLOAD_MAX))
        return -EINVAL;
    w->src = rec + POM_ITBH_SIZE;
    w->src_len = len - POM_ITBH_SIZE;
    w->is_lzo = algo == POM_COMPR_LZO;
    w->cap = w->is_lzo ? zlen - POM_ITBH_SIZE : 0;
    w->adepth = ad;
    w->entries = (int32_t)rd32(rec + POM_ITBH_ENTRIES_OFF);
    return 0;
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
    /* the records that pass the header checks, k = 0 ... m - 1: record idx[k] */
    size_t *idx = malloc((n + 1) * sizeof(*idx));
    const uint8_t **src = malloc((n + 1) * sizeof(*src));
    size_t *slen = malloc((n + 1) * sizeof(*slen));
    size_t *cap = malloc((n + 1) * sizeof(*cap));
    uint8_t *flags = malloc(2 * n + 1);            /* is_lzo[m], adepth[m] */
    int32_t *i32 = malloc((2 * n + 1) * sizeof(*i32));       /* status[m], err[m] */
    uint32_t *u32 = malloc((3 * n + 1) * sizeof(*u32));      /* out_len[m], live[m], nranges[m] */
    const struct pom_gc_range **rng = malloc((n + 1) * sizeof(*rng));
    struct pom_gc_sink G;
    memset(&G, 0, sizeof G);
    pthread_mutex_init(&G.mu, NULL);
    int rc = LZO_E_OUT_OF_MEMORY;
    if (!idx || !src || !slen || !cap || !flags || !i32 || !u32 || !rng)
        goto out;
    uint8_t *is_lzo = flags, *adepth = flags + n;
    size_t m = 0;
    for (size_t b = 0; b < n; b++) {
        live[b] = 0;
        err[b] = -EINVAL;
        if (len_ok)
            len_ok[b] = 0;
        if (entries_ok)
            entries_ok[b] = 0;
        struct pom_walk_block w;
        if (pom_itb_walk_header(rec[b], rec_len[b], &w) != 0)
            continue;
        idx[m] = b;
        src[m] = w.src;
        slen[m] = w.src_len;
        is_lzo[m] = w.is_lzo;
        cap[m] = w.cap;
        adepth[m] = w.adepth;
        m++;
    }
    G.is_lzo = is_lzo;
    G.cap = cap;
    G.adepth = adepth;
    G.column = column;
    G.status = i32;
    G.err = i32 + n;
    G.out_len = u32;
    G.live = u32 + n;
    G.nranges = u32 + 2 * n;
    G.rng = rng;
    rc = pom_gc_scan_chunked(src, slen, m, &G);
    if (rc != LZO_E_OK) {
        for (size_t k = 0; k < m; k++)
            err[idx[k]] = LZO_E_ERROR;
        goto out;
    }
    /* the chunks reordered the blocks: the global first[] and each ITB's ranges
     * in ITB order are put together here */
    size_t total = 0, k = 0;
    for (size_t b = 0; b < n; b++) {
        first[b] = total;
        if (k == m || idx[k] != b)
            continue;
        err[b] = G.status[k] != 0 ? G.status[k] : G.err[k];
        live[b] = G.live[k];
        if (len_ok)
            len_ok[b] = !is_lzo[k] || (G.status[k] == 0 && G.out_len[k] == cap[k]);
        if (entries_ok)
            entries_ok[b] = err[b] == 0 && (int64_t)live[b] == (int32_t)rd32(rec[b] + POM_ITBH_ENTRIES_OFF);
        const size_t nr = err[b] == 0 ? G.nranges[k] : 0;
        if (nr && total < ranges_cap) {
            const size_t fit = nr < ranges_cap - total ? nr : ranges_cap - total;
            memcpy(ranges + total, G.rng[k], fit * sizeof(*ranges));
        }
        total += nr;
        k++;
    }
    first[n] = total;
    rc = total > ranges_cap ? POM_GC_E_NOSPACE : LZO_E_OK;
out:
    pom_gc_sink_free(&G);
    pthread_mutex_destroy(&G.mu);
    free(idx);
    free(src);
    free(slen);
    free(cap);
    free(flags);
    free(i32);
    free(u32);
    free(rng);
    return rc;
}
