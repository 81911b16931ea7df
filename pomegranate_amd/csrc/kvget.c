/*
 * kvget.c -- the MDS key/value point get (include/pom_kvget.h): per request
 * the decode of its ITB and the INDEX_KV branches of itb_search
 * (mds/itb.c:1095-1116, :1808-1810), batched.  The header checks (gc_scan.c's),
 * the header's two rules (the itbid check and the JUST_SPLIT miss), the
 * grouping of the requests by ITB (as lookup.c) and the placing of the
 * records at the call's own first[] are here; the chunks go through the host
 * batches' pipeline (host_records.c, kg_ops).
 */
#include <errno.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_kvget.h"

int pom_kvget_dev(const uint8_t *payload, const uint64_t *payload_off,
                  const uint32_t *payload_len, const int32_t *status,
                  const uint8_t *adepth, uint32_t nitb,
                  const struct pom_kvget_req *req, uint32_t nreq,
                  const uint8_t *keys, uint32_t keys_len,
                  int32_t *err, uint32_t *nr, uint32_t *depth, uint32_t *len, uint64_t *lease,
                  uint64_t *first, uint8_t *out, uint64_t out_cap, void *stream)
{
    return lzo_mi355x_launch_kvget(payload, payload_off, payload_len, status, adepth, nitb, req, nreq, keys,
                                   keys_len, err, nr, depth, len, lease, first, out, out_cap, (hipStream_t)stream);
}

/* mds/itb.c:1754-1755 in u64: the request's key belongs to this ITB. */
static int itbid_matches(const uint8_t *rec, uint64_t key)
{
    const uint8_t depth = rec[POM_ITBH_DEPTH_OFF];
    uint64_t itbid;
    memcpy(&itbid, rec + POM_ITBH_ITBID_OFF, 8);
    const uint64_t mask = depth >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << depth) - 1;
    return ((key >> POM_ITB_ADEPTH_MAX) & mask) == itbid;
}

/* The ITBs some request reaches and that pass the header checks go to the
 * GPU, k = slot[ITB] = 0 ... m - 1, with its requests gathered behind
 * gfirst[k].  The other requests are decided here. */
int pom_kvget_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int itbid_check,
                    const struct pom_kvget_req *req, size_t nreq,
                    const uint8_t *keys, size_t keys_len,
                    uint8_t *out, size_t out_cap, size_t *first,
                    int *err, uint32_t *nr, uint32_t *depth, uint32_t *len, uint64_t *lease)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    first[0] = 0;
    if (nreq == 0)
        return LZO_E_OK;
    size_t *slot = malloc((n + 1) * sizeof(*slot));          /* ITB -> k, or a code below */
    size_t *gfirst = calloc(n + 2, sizeof(*gfirst));
    size_t *fill = malloc((n + 1) * sizeof(*fill));
    size_t *ids = malloc(nreq * sizeof(*ids));
    const uint8_t **src = malloc((n + 1) * sizeof(*src));
    size_t *slen = malloc((n + 1) * sizeof(*slen));
    size_t *cap = malloc((n + 1) * sizeof(*cap));
    uint8_t *flags = malloc(2 * n + 1);                      /* is_lzo[m], adepth[m] */
    int32_t *st = malloc((n + 1) * sizeof(*st));
    const uint8_t **recs = calloc(nreq, sizeof(*recs));
    struct pom_kvget_sink K;
    memset(&K, 0, sizeof K);
    int rc = LZO_E_OUT_OF_MEMORY, have_mu = 0;
    if (!slot || !gfirst || !fill || !ids || !src || !slen || !cap || !flags || !st || !recs)
        goto out;
    uint8_t *is_lzo = flags, *adepth = flags + n;
    const size_t kUnseen = (size_t)-1, kBadHeader = (size_t)-2, kGood = (size_t)-3;
    for (size_t b = 0; b < n; b++)
        slot[b] = kUnseen;
    /* a request goes to the GPU when its ITB's header is good and the itbid check lets it walk */
    size_t m = 0, ngpu = 0;
    for (size_t r = 0; r < nreq; r++) {
        const size_t b = req[r].itb;
        nr[r] = depth[r] = len[r] = 0;
        lease[r] = 0;
        err[r] = -EINVAL;
        struct pom_walk_block w;
        if (b < n && slot[b] == kUnseen)
            slot[b] = pom_itb_walk_header(rec[b], rec_len[b], &w) == 0 ? kGood : kBadHeader;
        if (b < n && slot[b] != kBadHeader && itbid_check && !itbid_matches(rec[b], req[r].key))
            err[r] = POM_LK_E_SPLIT;
        if (b >= n || slot[b] == kBadHeader || err[r] == POM_LK_E_SPLIT)
            continue;                           /* decided here */
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
        gfirst[slot[b] + 1]++;
        err[r] = LZO_E_ERROR;                   /* until its chunk delivers */
        ngpu++;
    }
    rc = LZO_E_OK;
    if (ngpu != 0) {
        for (size_t k = 0; k < m; k++) {
            gfirst[k + 1] += gfirst[k];
            fill[k] = gfirst[k];
        }
        for (size_t r = 0; r < nreq; r++)
            if (err[r] == LZO_E_ERROR)
                ids[fill[slot[req[r].itb]]++] = r;
        K = (struct pom_kvget_sink){is_lzo, cap, adepth, gfirst, ids, req, keys, keys_len, out == NULL,
                                    err, nr, depth, len, lease, recs, st, NULL, PTHREAD_MUTEX_INITIALIZER};
        have_mu = 1;
        rc = pom_kvget_chunked(src, slen, m, &K);
        /* (the requests of chunks that were not delivered keep LZO_E_ERROR and no record) */
        if (rc == LZO_E_OK)
            /* mds/itb.c:2030-2033: a miss on an ITB that has just split */
            for (size_t j = 0; j < ngpu; j++) {
                const size_t r = ids[j];
                if (err[r] == POM_LK_E_NOENT && rec[req[r].itb][POM_ITBH_FLAG_OFF] == POM_ITB_JUST_SPLIT)
                    err[r] = POM_LK_E_SPLIT;
            }
    }
    /* the call's own first[], and each record to its place below out_cap */
    for (size_t r = 0; r < nreq; r++) {
        first[r + 1] = first[r] + len[r];
        if (out && recs[r] && first[r] < out_cap)
            memcpy(out + first[r], recs[r], first[r + 1] <= out_cap ? len[r] : out_cap - first[r]);
    }
    if (rc == LZO_E_OK && out && first[nreq] > out_cap)
        rc = POM_GC_E_NOSPACE;
out:
    if (have_mu) {
        pom_kvget_sink_free(&K);
        pthread_mutex_destroy(&K.mu);
    }
    free(slot);
    free(gfirst);
    free(fill);
    free(ids);
    free(src);
    free(slen);
    free(cap);
    free(flags);
    free(st);
    free(recs);
    return rc;
}
