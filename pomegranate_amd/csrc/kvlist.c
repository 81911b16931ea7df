/*
 * kvlist.c -- the MDS key/value table listing (include/pom_kvlist.h): per ITB
 * the decode and the INDEX_KV branch of itb_readdir (mds/itb.c:2472-2534),
 * batched.  The header checks (readdir.c's) and the reassembly in ITB order
 * are here; the chunks -- compressed payloads and the needle up, the decoders,
 * the key walk (itb_keys.hip), counts, masks and records back -- go through
 * the host batches' pipeline (lzo_host.c, OP_KVLIST).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_kvlist.h"

int pom_kvlist_dev(const uint8_t *payload, const uint64_t *payload_off,
                   const uint32_t *payload_len, const int32_t *status,
                   const uint8_t *adepth, uint32_t nitb, uint32_t op,
                   const uint8_t *needle, uint32_t needle_len,
                   uint32_t *live, uint32_t *dnum, uint32_t *bytes, uint32_t *keybytes,
                   uint64_t *mask, uint64_t *first, uint8_t *out, uint64_t out_cap,
                   int32_t *err, void *stream)
{
    return lzo_mi355x_launch_kvlist(payload, payload_off, payload_len, status, adepth, nitb, op, needle,
                                    needle_len, live, dnum, bytes, keybytes, mask, first, out, out_cap, err,
                                    (hipStream_t)stream);
}

int pom_kvlist_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                     uint32_t op, const uint8_t *needle, uint32_t needle_len,
                     uint8_t *out, size_t out_cap, size_t *first,
                     uint32_t *live, uint32_t *dnum, uint32_t *keybytes, uint64_t *mask,
                     int *err, int *len_ok, int *entries_ok)
{
    if (op > POM_KV_OP_GREP_CNT || needle_len > POM_KV_NEEDLE_MAX)
        return -EINVAL;
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    if (!out)
        out_cap = 0;
    /* the records that go to the GPU, k = 0 ... m - 1: record idx[k] */
    size_t *idx = malloc((n + 1) * sizeof(*idx));
    const uint8_t **src = malloc((n + 1) * sizeof(*src));
    size_t *slen = malloc((n + 1) * sizeof(*slen));
    size_t *cap = malloc((n + 1) * sizeof(*cap));
    uint8_t *flags = malloc(2 * n + 1);            /* is_lzo[m], adepth[m] */
    int32_t *i32 = malloc((3 * n + 1) * sizeof(*i32));       /* status[m], err[m], entries[m] */
    uint32_t *u32 = malloc((5 * n + 1) * sizeof(*u32));      /* out_len[m], live[m], dnum[m], bytes[m], keybytes[m] */
    uint64_t *masks = mask ? malloc((POM_KV_MASK_WORDS * n + 1) * sizeof(*masks)) : NULL;
    const uint8_t **keys = malloc((n + 1) * sizeof(*keys));
    uint8_t **to = malloc((n + 1) * sizeof(*to));            /* the reassembly's copies: to[m], from keys[m] */
    size_t *fit = malloc((n + 1) * sizeof(*fit));
    struct pom_gc_sink G;
    memset(&G, 0, sizeof G);
    pthread_mutex_init(&G.mu, NULL);
    int rc = LZO_E_OUT_OF_MEMORY;
    if (!idx || !src || !slen || !cap || !flags || !i32 || !u32 || (mask && !masks) || !keys || !to || !fit)
        goto out;
    uint8_t *is_lzo = flags, *adepth = flags + n;
    int32_t *entries = i32 + 2 * n;
    size_t m = 0;
    for (size_t b = 0; b < n; b++) {
        live[b] = dnum[b] = 0;
        err[b] = -EINVAL;
        if (keybytes)
            keybytes[b] = 0;
        if (mask)
            memset(mask + POM_KV_MASK_WORDS * b, 0, 8 * POM_KV_MASK_WORDS);
        if (len_ok)
            len_ok[b] = 0;
        if (entries_ok)
            entries_ok[b] = 0;
        struct pom_walk_block w;
        if (pom_itb_walk_header(rec[b], rec_len[b], &w) != 0 || w.entries < 0)
            continue;
        if (w.entries == 0) {
            /* mds/itb.c:2479-2482: the reference leaves before the bitmap */
            err[b] = 0;
            if (entries_ok)
                entries_ok[b] = 1;
            continue;
        }
        idx[m] = b;
        src[m] = w.src;
        slen[m] = w.src_len;
        is_lzo[m] = w.is_lzo;
        cap[m] = w.cap;
        adepth[m] = w.adepth;
        entries[m] = w.entries;
        m++;
    }
    G.is_lzo = is_lzo;
    G.cap = cap;
    G.adepth = adepth;
    G.status = i32;
    G.err = i32 + n;
    G.out_len = u32;
    G.live = u32 + n;
    G.nranges = u32 + 2 * n;
    G.bytes = u32 + 3 * n;
    G.keybytes = u32 + 4 * n;
    G.mask = masks;
    G.dents = keys;
    G.kv_op = op;
    G.needle = needle;
    G.needle_len = needle_len;
    G.count_only = out == NULL;
    rc = pom_kvlist_chunked(src, slen, m, &G);
    if (rc != LZO_E_OK) {
        for (size_t k = 0; k < m; k++)
            err[idx[k]] = LZO_E_ERROR;
        goto out;
    }
    /* the chunks reordered the blocks: the global first[] and each ITB's records
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
            entries_ok[b] = err[b] == 0 && (int64_t)live[b] == entries[k];
        const size_t nb = err[b] == 0 ? G.bytes[k] : 0;
        dnum[b] = err[b] == 0 ? G.nranges[k] : 0;
        if (keybytes)
            keybytes[b] = err[b] == 0 ? G.keybytes[k] : 0;
        if (mask && err[b] == 0)
            memcpy(mask + POM_KV_MASK_WORDS * b, masks + POM_KV_MASK_WORDS * k, 8 * POM_KV_MASK_WORDS);
        to[k] = out + (total < out_cap ? total : out_cap);
        fit[k] = !out || total >= out_cap ? 0 : nb < out_cap - total ? nb : out_cap - total;
        total += nb;
        k++;
    }
    first[n] = total;
    if (out)
        pom_copy_parallel(to, G.dents, fit, m);
    rc = out && total > out_cap ? POM_GC_E_NOSPACE : LZO_E_OK;
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
    free(masks);
    free(keys);
    free(to);
    free(fit);
    return rc;
}
