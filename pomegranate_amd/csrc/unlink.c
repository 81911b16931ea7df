/*
 * unlink.c -- the ITB unlink (include/pom_unlink.h): the device entry, which
 * queues the check (itb_check.hip) into the caller's scratch and the unlink
 * (itb_unlink.hip) behind it on the same stream; the header unlinks leave,
 * built on the host in plain C with the split's not-smaller rule
 * (pom_itb_stored_as, itbsplit.c); and the batch over stored records: the
 * selection, the grouping and the header's two rules are the request batches'
 * shared halves (host_requests.c), the header facts and the ITBs' results here,
 * the chunks through the host batches' pipeline (host_records.c, ul_ops).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "host_requests.h"
#include "lzo_mi355x.h"
#include "minilzo.h"

#include "lzo_mi355x_kernels.h"
#include "pom_gc.h"
#include "pom_itb.h"
#include "pom_lookup.h"
#include "pom_unlink.h"

/* scratch: [reports, 48 bytes per ITB][err i32 per ITB] */
size_t pom_itb_unlink_scratch(uint32_t nitb)
{
    return (((size_t)nitb * (sizeof(struct pom_check_report) + 4)) + 255) & ~(size_t)255;
}

int pom_itb_unlink_dev(uint8_t *payload, const uint64_t *payload_off,
                       const uint32_t *payload_len, const int32_t *status,
                       const uint8_t *adepth, const struct pom_check_hdr *hdr, uint32_t nitb,
                       int async_unlink, const struct pom_lookup_req *req, const uint32_t *req_first,
                       uint32_t nreq, const uint8_t *names, uint32_t names_len,
                       int32_t *err, uint32_t *nr, uint32_t *depth, uint32_t *what, uint8_t *out,
                       struct pom_unlink_result *result, void *scratch, void *stream)
{
    if (!hdr || ((uintptr_t)payload & 15) || ((uintptr_t)scratch & 7) || ((uintptr_t)req & 7) || ((uintptr_t)out & 7))
        return -EINVAL;
    struct pom_check_report *report = scratch;
    int32_t *ck_err = (int32_t *)((uint8_t *)scratch + (size_t)nitb * sizeof(struct pom_check_report));
    if (lzo_mi355x_launch_itb_check(payload, payload_off, payload_len, status, adepth, hdr, nitb, 0, report, NULL, NULL,
                                    ck_err, (hipStream_t)stream) != 0)
        return -1;
    return lzo_mi355x_launch_itb_unlink(payload, payload_off, payload_len, adepth, hdr, nitb, async_unlink, req,
                                        req_first, nreq, names, names_len, report, ck_err, err, nr, depth, what, out,
                                        result, (hipStream_t)stream);
}

static void put32(uint8_t *h, size_t off, uint32_t v)
{
    memcpy(h + off, &v, 4);
}

int pom_itb_unlink_header(const uint8_t *old_hdr, const struct pom_unlink_result *r, uint32_t z, uint8_t *out)
{
    uint8_t h[POM_ITBH_SIZE];
    if (r->err != 0 || r->changed == 0 || r->len < POM_ITBH_SIZE)
        return -EINVAL;
    memcpy(h, old_hdr, POM_ITBH_SIZE);
    put32(h, POM_ITBH_ENTRIES_OFF, (uint32_t)r->entries);
    put32(h, POM_ITBH_MAX_OFFSET_OFF, (uint32_t)r->max_offset);
    put32(h, POM_ITBH_PSEUDO_CONFLICTS_OFF, (uint32_t)r->pseudo_conflicts);
    memcpy(h + POM_ITBH_ITU_OFF, &r->itu, 2);
    const int lzo = pom_itb_stored_as(h, r->len, z);
    memcpy(out, h, POM_ITBH_SIZE);
    return lzo;
}

static uint32_t rd32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

int pom_itb_unlink_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int itbid_check,
                         int async_unlink, const struct pom_lookup_req *req, size_t nreq,
                         const uint8_t *names, size_t names_len, uint8_t *rec_out,
                         int *err, uint32_t *nr, uint32_t *depth, uint32_t *what,
                         uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                         struct pom_unlink_result *result, int *itb_err, int *len_ok)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    /* every ITB as one no request reaches; a refused header shows all the same */
    for (size_t b = 0; b < n; b++) {
        struct pom_walk_block w;
        memset(&result[b], 0, sizeof result[b]);
        out_len[b] = 0;
        itb_err[b] = pom_itb_walk_header(rec[b], rec_len[b], &w) != 0 ? -EINVAL : 0;
        if (len_ok)
            len_ok[b] = 0;
    }
    if (nreq == 0)
        return LZO_E_OK;
    uint32_t *const word[RW_N] = {(uint32_t *)err, nr, depth, what};
    struct pom_req_batch W;
    int rc = pom_req_begin(&W, &pom_req_unlink, rec, rec_len, n, itbid_check, req, nreq, names, names_len, word, NULL);
    /* per GPU-bound ITB k: the caller's record, its header facts, what the chunk leaves */
    size_t *idx = NULL;
    const uint8_t **hdrs = NULL;
    struct pom_check_hdr *hdr = NULL;
    int32_t *status = NULL;
    uint32_t *dlen = NULL;
    uint8_t *delivered = NULL;
    if (rc == LZO_E_OK) {
        idx = malloc((W.m + 1) * sizeof(*idx));
        hdrs = malloc((W.m + 1) * sizeof(*hdrs));
        hdr = malloc((W.m + 1) * sizeof(*hdr));
        status = malloc((W.m + 1) * sizeof(*status));
        dlen = malloc((W.m + 1) * sizeof(*dlen));
        delivered = calloc(W.m + 1, 1);
        if (!idx || !hdrs || !hdr || !status || !dlen || !delivered)
            rc = LZO_E_OUT_OF_MEMORY;
    }
    if (rc == LZO_E_OK) {
        for (size_t r = 0; r < nreq; r++)
            memset(rec_out + POM_LK_REC_SIZE * r, 0, POM_LK_REC_SIZE);      /* decided on the host, or not delivered */
        for (size_t k = 0; k < W.m; k++) {
            /* (a GPU-bound ITB has a request: its first one names the record) */
            const size_t b = rd32((const uint8_t *)req + POM_REQ_SIZE * W.ids[W.first[k]] +
                                  offsetof(struct pom_lookup_req, itb));
            idx[k] = b;
            hdrs[k] = rec[b];
            status[k] = 0;
            dlen[k] = 0;
            pom_check_header_facts(rec[b], W.G.is_lzo[k], &hdr[k]);
            itb_err[b] = LZO_E_ERROR;                                       /* until its chunk delivers */
        }
        W.G.fixed = rec_out;
        struct pom_unlink_sink U = {.K = &W.G, .async_unlink = async_unlink, .hdr = hdr, .rec_hdr = hdrs, .idx = idx,
                                    .status = status, .out_len = dlen, .delivered = delivered, .out = out,
                                    .out_cap = out_cap, .rec_len = out_len, .result = result, .err = itb_err};
        if (W.ngpu)
            rc = pom_itb_unlink_chunked(W.src, W.slen, W.m, &U);
        if (len_ok)
            for (size_t k = 0; k < W.m; k++)
                len_ok[idx[k]] = delivered[k] && (!W.G.is_lzo[k] || (status[k] == 0 && dlen[k] == W.cap[k]));
    }
    free(idx);
    free(hdrs);
    free(hdr);
    free(status);
    free(dlen);
    free(delivered);
    return pom_req_finish(&W, rc, rec);
}
