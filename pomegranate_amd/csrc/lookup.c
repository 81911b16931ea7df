/*
 * lookup.c -- the MDS lookup (include/pom_lookup.h): per request the decode of
 * its ITB and the INDEX_LOOKUP branch of itb_search (mds/itb.c:1738-2053),
 * batched.  The header checks (gc_scan.c's), the header's two rules (the
 * itbid check and the JUST_SPLIT miss) and the grouping of the requests by
 * ITB are here; the chunks -- compressed payloads, requests and names up, the
 * decoders, the chain walk (itb_find.hip), codes and records back in request
 * order -- go through the host batches' pipeline (host_records.c, lk_ops).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_lookup.h"

int pom_lookup_dev(const uint8_t *payload, const uint64_t *payload_off,
                   const uint32_t *payload_len, const int32_t *status,
                   const uint8_t *adepth, uint32_t nitb,
                   const struct pom_lookup_req *req, uint32_t nreq,
                   const uint8_t *names, uint32_t names_len,
                   int32_t *err, uint32_t *nr, uint32_t *depth, uint8_t *out, void *stream)
{
    return lzo_mi355x_launch_lookup(payload, payload_off, payload_len, status, adepth, nitb, req, nreq, names,
                                    names_len, err, nr, depth, out, (hipStream_t)stream);
}

/* mds/itb.c:1754-1755 in u64: the request's hash belongs to this ITB. */
static int itbid_matches(const uint8_t *rec, uint64_t hash)
{
    const uint8_t depth = rec[POM_ITBH_DEPTH_OFF];
    uint64_t itbid;
    memcpy(&itbid, rec + POM_ITBH_ITBID_OFF, 8);
    const uint64_t mask = depth >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << depth) - 1;
    return ((hash >> POM_ITB_ADEPTH_MAX) & mask) == itbid;
}

/* The ITBs some request reaches and that pass the header checks go to the
 * GPU, k = slot[ITB] = 0 ... m - 1, with its requests gathered behind
 * first[k].  The other requests are decided here. */
int pom_lookup_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int itbid_check,
                     const struct pom_lookup_req *req, size_t nreq,
                     const uint8_t *names, size_t names_len,
                     uint8_t *out, int *err, uint32_t *nr, uint32_t *depth)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    if (nreq == 0)
        return LZO_E_OK;
    size_t *slot = malloc((n + 1) * sizeof(*slot));          /* ITB -> k, or a code below */
    size_t *first = calloc(n + 2, sizeof(*first));
    size_t *fill = malloc((n + 1) * sizeof(*fill));
    size_t *ids = malloc(nreq * sizeof(*ids));
    const uint8_t **src = malloc((n + 1) * sizeof(*src));
    size_t *slen = malloc((n + 1) * sizeof(*slen));
    size_t *cap = malloc((n + 1) * sizeof(*cap));
    uint8_t *flags = malloc(2 * n + 1);                      /* is_lzo[m], adepth[m] */
    int32_t *st = malloc((n + 1) * sizeof(*st));
    int rc = LZO_E_OUT_OF_MEMORY;
    if (!slot || !first || !fill || !ids || !src || !slen || !cap || !flags || !st)
        goto out;
    uint8_t *is_lzo = flags, *adepth = flags + n;
    const size_t kUnseen = (size_t)-1, kBadHeader = (size_t)-2, kGood = (size_t)-3;
    for (size_t b = 0; b < n; b++)
        slot[b] = kUnseen;
    /* a request goes to the GPU when its ITB's header is good and the itbid check lets it walk */
    size_t m = 0, ngpu = 0;
    for (size_t r = 0; r < nreq; r++) {
        const size_t b = req[r].itb;
        nr[r] = depth[r] = 0;
        err[r] = -EINVAL;
        struct pom_walk_block w;
        if (b < n && slot[b] == kUnseen)
            slot[b] = pom_itb_walk_header(rec[b], rec_len[b], &w) == 0 ? kGood : kBadHeader;
        if (b < n && slot[b] != kBadHeader && itbid_check && !itbid_matches(rec[b], req[r].hash))
            err[r] = POM_LK_E_SPLIT;
        if (b >= n || slot[b] == kBadHeader || err[r] == POM_LK_E_SPLIT) {
            memset(out + POM_LK_REC_SIZE * r, 0, POM_LK_REC_SIZE);       /* decided here */
            continue;
        }
        if (slot[b] == kGood) {
            pom_itb_walk_header(rec[b], rec_len[b], &w);
            slot[b] = m;
            src[m] = w.src;
            slen[m] = w.src_len;
            is_lzo[m] = w.is_lzo;
            cap[m] = w.cap;
            adepth[m] = w.adepth;
            m++;
        }
        first[slot[b] + 1]++;
        err[r] = LZO_E_ERROR;                   /* until its chunk delivers */
        ngpu++;
    }
    rc = LZO_E_OK;
    if (ngpu == 0)
        goto out;
    for (size_t k = 0; k < m; k++) {
        first[k + 1] += first[k];
        fill[k] = first[k];
    }
    for (size_t r = 0; r < nreq; r++)
        if (err[r] == LZO_E_ERROR)
            ids[fill[slot[req[r].itb]]++] = r;
    struct pom_lookup_sink K = {is_lzo, cap, adepth, first, ids, req, names, names_len, out, err, nr, depth, st};
    rc = pom_lookup_chunked(src, slen, m, &K);
    if (rc != LZO_E_OK) {
        /* the requests of chunks that were not delivered keep LZO_E_ERROR */
        for (size_t j = 0; j < ngpu; j++)
            if (err[ids[j]] == LZO_E_ERROR)
                memset(out + POM_LK_REC_SIZE * ids[j], 0, POM_LK_REC_SIZE);
        goto out;
    }
    /* mds/itb.c:2030-2033: a miss on an ITB that has just split */
    for (size_t j = 0; j < ngpu; j++) {
        const size_t r = ids[j];
        if (err[r] == POM_LK_E_NOENT && rec[req[r].itb][POM_ITBH_FLAG_OFF] == POM_ITB_JUST_SPLIT)
            err[r] = POM_LK_E_SPLIT;
    }
out:
    free(slot);
    free(first);
    free(fill);
    free(ids);
    free(src);
    free(slen);
    free(cap);
    free(flags);
    free(st);
    return rc;
}
