/*
 * kvget.c -- the MDS key/value point get (include/pom_kvget.h): per request
 * the decode of its ITB and the INDEX_KV branches of itb_search
 * (mds/itb.c:1095-1116, :1808-1810), batched.  The header checks, the header's
 * two rules (the itbid check and the JUST_SPLIT miss) and the grouping of the
 * requests by ITB are host_requests.c's pom_req_begin and pom_req_finish, as
 * for lookup.c; the placing of the records at the call's own first[] is here;
 * the chunks go through the host batches' pipeline (host_records.c, the
 * request operation).
 */
#include <string.h>

#include "host_requests.h"
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

/* The selection, the grouping and the header's two rules are the request
 * batches' shared halves (host_requests.c); here are the call's own first[]
 * and the placing of the records. */
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
    uint32_t *const word[RW_N] = {(uint32_t *)err, nr, depth, len};
    struct pom_req_batch W;
    int rc = pom_req_begin(&W, &pom_req_kvget, rec, rec_len, n, itbid_check, req, nreq, keys, keys_len, word, lease);
    if (rc != LZO_E_OK)
        return pom_req_finish(&W, rc, rec);
    W.G.records = out != NULL;
    if (W.ngpu)
        rc = pom_kvget_chunked(W.src, W.slen, W.m, &W.G);
    /* (the requests of chunks that were not delivered keep LZO_E_ERROR and no record)
     * the call's own first[], and each record to its place below out_cap */
    for (size_t r = 0; r < nreq; r++) {
        first[r + 1] = first[r] + len[r];
        if (out && W.recs[r] && first[r] < out_cap)
            memcpy(out + first[r], W.recs[r], first[r + 1] <= out_cap ? len[r] : out_cap - first[r]);
    }
    rc = pom_req_finish(&W, rc, rec);
    if (rc == LZO_E_OK && out && first[nreq] > out_cap)
        rc = POM_GC_E_NOSPACE;
    return rc;
}
