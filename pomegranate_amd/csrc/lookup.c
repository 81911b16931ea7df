/*
 * lookup.c -- the MDS lookup (include/pom_lookup.h): per request the decode of
 * its ITB and the INDEX_LOOKUP branch of itb_search (mds/itb.c:1738-2053),
 * batched.  The header checks, the header's two rules (the itbid check and the
 * JUST_SPLIT miss) and the grouping of the requests by ITB are
 * host_requests.c's pom_req_begin and pom_req_finish; the chunks -- compressed
 * payloads, requests and names up, the decoders, the chain walk
 * (itb_find.hip), codes and records back in request order -- go through the
 * host batches' pipeline (host_records.c, the request operation).
 */
#include <string.h>

#include "host_requests.h"
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

/* The selection, the grouping and the header's two rules are the request
 * batches' shared halves (host_requests.c); here are only the records of the
 * requests no chunk answered: 136 zero bytes. */
int pom_lookup_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int itbid_check,
                     const struct pom_lookup_req *req, size_t nreq,
                     const uint8_t *names, size_t names_len,
                     uint8_t *out, int *err, uint32_t *nr, uint32_t *depth)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    if (nreq == 0)
        return LZO_E_OK;
    uint32_t *const word[RW_N] = {(uint32_t *)err, nr, depth};
    struct pom_req_batch W;
    int rc = pom_req_begin(&W, &pom_req_lookup, rec, rec_len, n, itbid_check, req, nreq, names, names_len, word, NULL);
    if (rc == LZO_E_OK) {
        for (size_t r = 0; r < nreq; r++)
            if (err[r] != LZO_E_ERROR)
                memset(out + POM_LK_REC_SIZE * r, 0, POM_LK_REC_SIZE);       /* decided on the host */
        W.G.fixed = out;
        if (W.ngpu)
            rc = pom_lookup_chunked(W.src, W.slen, W.m, &W.G);
        if (rc != LZO_E_OK)
            /* the requests of chunks that were not delivered keep LZO_E_ERROR */
            for (size_t r = 0; r < nreq; r++)
                if (err[r] == LZO_E_ERROR)
                    memset(out + POM_LK_REC_SIZE * r, 0, POM_LK_REC_SIZE);
    }
    return pom_req_finish(&W, rc, rec);
}
