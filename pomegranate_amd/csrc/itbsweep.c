/*
 * itbsweep.c -- the ITB sweep (include/pom_sweep.h): the device entry, which
 * queues the check (itb_check.hip) into the caller's scratch and the sweep
 * (itb_sweep.hip) behind it on the same stream; the header a sweep leaves,
 * built on the host in plain C with the split's not-smaller rule
 * (pom_itb_stored_as, itbsplit.c); and the batch over stored records: the
 * selection (pom_itb_walk_header), the header facts and the results' order
 * here, the chunks through the host batches' pipeline (host_records.c,
 * sw_ops).
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
#include "pom_sweep.h"

/* scratch: [reports, 48 bytes per ITB][err i32 per ITB] */
size_t pom_itb_sweep_scratch(uint32_t nitb)
{
    return (((size_t)nitb * (sizeof(struct pom_check_report) + 4)) + 255) & ~(size_t)255;
}

int pom_itb_sweep_dev(uint8_t *payload, const uint64_t *payload_off,
                      const uint32_t *payload_len, const int32_t *status,
                      const uint8_t *adepth, const struct pom_check_hdr *hdr,
                      const uint32_t *budget, uint32_t nitb,
                      struct pom_sweep_result *result, void *scratch, void *stream)
{
    if (!hdr || ((uintptr_t)payload & 15) || ((uintptr_t)scratch & 7))
        return -EINVAL;
    struct pom_check_report *report = scratch;
    int32_t *err = (int32_t *)((uint8_t *)scratch + (size_t)nitb * sizeof(struct pom_check_report));
    if (lzo_mi355x_launch_itb_check(payload, payload_off, payload_len, status, adepth, hdr, nitb, 0, report, NULL, NULL,
                                    err, (hipStream_t)stream) != 0)
        return -1;
    return lzo_mi355x_launch_itb_sweep(payload, payload_off, adepth, hdr, budget, nitb, report, err, result,
                                       (hipStream_t)stream);
}

static void put32(uint8_t *h, size_t off, uint32_t v)
{
    memcpy(h + off, &v, 4);
}

int pom_itb_sweep_header(const uint8_t *old_hdr, const struct pom_sweep_result *r, uint32_t z, uint8_t *out)
{
    uint8_t h[POM_ITBH_SIZE];
    if (r->err != 0 || r->removed == 0 || r->len < POM_ITBH_SIZE)
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

int pom_itb_sweep_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                        const uint32_t *budget, uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                        struct pom_sweep_result *result, int *err, int *len_ok)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    size_t *idx = malloc((n + 1) * sizeof(*idx));
    size_t *slen = malloc((n + 1) * sizeof(*slen));
    size_t *cap = malloc((n + 1) * sizeof(*cap));
    const uint8_t **src = malloc((n + 1) * sizeof(*src));
    const uint8_t **hdrs = malloc((n + 1) * sizeof(*hdrs));
    uint8_t *bytes = malloc(3 * n + 1);                             /* is_lzo[m], adepth[m], delivered[m] */
    int32_t *status = malloc((n + 1) * sizeof(*status));
    uint32_t *dlen = malloc((n + 1) * sizeof(*dlen));
    uint32_t *bud = malloc((n + 1) * sizeof(*bud));
    struct pom_check_hdr *hdr = malloc((n + 1) * sizeof(*hdr));
    int rc = LZO_E_OUT_OF_MEMORY;
    if (idx && slen && cap && src && hdrs && bytes && status && dlen && bud && hdr) {
        uint8_t *is_lzo = bytes, *adepth = bytes + n, *delivered = bytes + 2 * n;
        size_t m = 0;
        for (size_t b = 0; b < n; b++) {
            struct pom_walk_block w;
            err[b] = -EINVAL;
            memset(&result[b], 0, sizeof result[b]);
            out_len[b] = 0;
            if (len_ok)
                len_ok[b] = 0;
            if (pom_itb_walk_header(rec[b], rec_len[b], &w) != 0)
                continue;
            idx[m] = b;
            src[m] = w.src;
            hdrs[m] = rec[b];
            slen[m] = w.src_len;
            cap[m] = w.cap;
            is_lzo[m] = w.is_lzo;
            adepth[m] = w.adepth;
            status[m] = 0;
            dlen[m] = 0;
            delivered[m] = 0;
            bud[m] = budget ? budget[b] : POM_SWEEP_NO_BUDGET;
            pom_check_header_facts(rec[b], w.is_lzo, &hdr[m]);
            err[b] = LZO_E_ERROR;                                   /* until its chunk delivers */
            m++;
        }
        struct pom_sweep_sink G = {.is_lzo = is_lzo, .cap = cap, .adepth = adepth, .hdr = hdr, .budget = bud,
                                   .rec_hdr = hdrs, .idx = idx, .status = status, .out_len = dlen,
                                   .delivered = delivered, .out = out, .out_cap = out_cap, .rec_len = out_len,
                                   .result = result, .err = err};
        rc = pom_itb_sweep_chunked(src, slen, m, &G);
        if (len_ok)
            for (size_t k = 0; k < m; k++)
                len_ok[idx[k]] = delivered[k] && (!is_lzo[k] || (status[k] == 0 && dlen[k] == cap[k]));
    }
    free(idx);
    free(slen);
    free(cap);
    free(src);
    free(hdrs);
    free(bytes);
    free(status);
    free(dlen);
    free(bud);
    free(hdr);
    return rc;
}
