/*
 * itbsplit.c -- the ITB split (include/pom_split.h): the device entry, which
 * queues the check (itb_check.hip) into the caller's scratch and the split
 * (itb_split.hip) behind it on the same stream; the two headers a split
 * leaves, built on the host in plain C; and the batch over stored records:
 * the selection (pom_itb_walk_header), the header facts and the results'
 * order here, the chunks through the host batches' pipeline (host_records.c,
 * sp_ops).
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
#include "pom_split.h"

/* scratch: [reports, 48 bytes per ITB][err i32 per ITB] */
size_t pom_itb_split_scratch(uint32_t nitb)
{
    return (((size_t)nitb * (sizeof(struct pom_check_report) + 4)) + 255) & ~(size_t)255;
}

int pom_itb_split_dev(uint8_t *payload, const uint64_t *payload_off,
                      const uint32_t *payload_len, const int32_t *status,
                      const uint8_t *adepth, const struct pom_check_hdr *hdr,
                      const uint8_t *split_depth, uint32_t nitb,
                      uint8_t *new_payload, const uint64_t *new_off, const uint32_t *new_cap,
                      struct pom_split_result *result, void *scratch, void *stream)
{
    if (!hdr || (((uintptr_t)payload | (uintptr_t)new_payload) & 15) || ((uintptr_t)scratch & 7))
        return -EINVAL;
    struct pom_check_report *report = scratch;
    int32_t *err = (int32_t *)((uint8_t *)scratch + (size_t)nitb * sizeof(struct pom_check_report));
    if (lzo_mi355x_launch_itb_check(payload, payload_off, payload_len, status, adepth, hdr, nitb, 0, report, NULL, NULL,
                                    err, (hipStream_t)stream) != 0)
        return -1;
    return lzo_mi355x_launch_itb_split(payload, payload_off, adepth, hdr, split_depth, nitb, new_payload, new_off,
                                       new_cap, report, err, result, (hipStream_t)stream);
}

static void put32(uint8_t *h, size_t off, uint32_t v)
{
    memcpy(h + off, &v, 4);
}

static void put16(uint8_t *h, size_t off, uint16_t v)
{
    memcpy(h + off, &v, 2);
}

/* itb_lzo_compress's rule (mds/itb.c:2904-2945) on one header: the stream is
 * kept when it is smaller than the payload.  Returns whether it is.  (The
 * sweep's header builder, itbsweep.c, calls it too.) */
int pom_itb_stored_as(uint8_t *h, uint32_t ulen, uint32_t z)
{
    const int lzo = z < ulen - POM_ITBH_SIZE;
    put32(h, POM_ITBH_LEN_OFF, lzo ? POM_ITBH_SIZE + z : ulen);
    put32(h, POM_ITBH_ZLEN_OFF, lzo ? ulen : 0);
    put16(h, POM_ITBH_ALGO_OFF, lzo ? POM_COMPR_LZO : POM_COMPR_NONE);
    return lzo;
}

int pom_itb_split_headers(const uint8_t *old_hdr, uint8_t sd, const struct pom_split_result *r,
                          uint32_t old_z, uint32_t new_z, uint8_t *old_out, uint8_t *new_out)
{
    uint8_t o[POM_ITBH_SIZE], n[POM_ITBH_SIZE];
    uint64_t itbid;
    if (sd < 1 || sd > POM_SPLIT_DEPTH_MAX || r->err != 0 || r->moved == 0 || r->old_len < POM_ITBH_SIZE ||
        r->new_len < POM_ITBH_SIZE)
        return -EINVAL;
    memcpy(o, old_hdr, POM_ITBH_SIZE);
    o[POM_ITBH_DEPTH_OFF] = sd;
    put32(o, POM_ITBH_ENTRIES_OFF, (uint32_t)r->old_entries);
    put32(o, POM_ITBH_MAX_OFFSET_OFF, (uint32_t)r->old_max_offset);
    put32(o, POM_ITBH_PSEUDO_CONFLICTS_OFF, (uint32_t)r->old_pseudo);
    put16(o, POM_ITBH_ITU_OFF, r->old_itu);
    const int old_lzo = pom_itb_stored_as(o, r->old_len, old_z);

    memcpy(n, o, POM_ITBH_SIZE);
    n[POM_ITBH_FLAG_OFF] = POM_ITB_JUST_SPLIT;
    n[POM_ITBH_STATE_OFF] = POM_ITB_STATE_DIRTY;
    memcpy(&itbid, n + POM_ITBH_ITBID_OFF, 8);
    itbid |= 1ull << (sd - 1);
    memcpy(n + POM_ITBH_ITBID_OFF, &itbid, 8);
    put32(n, POM_ITBH_ENTRIES_OFF, (uint32_t)r->new_entries);
    put32(n, POM_ITBH_MAX_OFFSET_OFF, (uint32_t)r->new_max_offset);
    put32(n, POM_ITBH_CONFLICTS_OFF, 0);
    put32(n, POM_ITBH_PSEUDO_CONFLICTS_OFF, (uint32_t)r->new_pseudo);
    put16(n, POM_ITBH_INF_OFF, r->new_inf);
    put16(n, POM_ITBH_ITU_OFF, r->new_itu);
    const int new_lzo = pom_itb_stored_as(n, r->new_len, new_z);
    memset(n + POM_ITBH_TWIN_OFF, 0, 8);
    memset(n + POM_ITBH_SPLIT_RLINK_OFF, 0, 8);

    memcpy(old_out, o, POM_ITBH_SIZE);
    memcpy(new_out, n, POM_ITBH_SIZE);
    return old_lzo | new_lzo << 1;
}

int pom_itb_split_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                        const uint8_t *split_depth, uint8_t *const *old_out, uint8_t *const *new_out,
                        const size_t *out_cap, size_t *old_len, size_t *new_len,
                        struct pom_split_result *result, int *err, int *len_ok)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    size_t *idx = malloc((n + 1) * sizeof(*idx));
    size_t *slen = malloc((n + 1) * sizeof(*slen));
    size_t *cap = malloc((n + 1) * sizeof(*cap));
    const uint8_t **src = malloc((n + 1) * sizeof(*src));
    const uint8_t **hdrs = malloc((n + 1) * sizeof(*hdrs));
    uint8_t *bytes = malloc(4 * n + 1);                             /* is_lzo[m], adepth[m], sd[m], delivered[m] */
    int32_t *status = malloc((n + 1) * sizeof(*status));
    uint32_t *out_len = malloc((n + 1) * sizeof(*out_len));
    struct pom_check_hdr *hdr = malloc((n + 1) * sizeof(*hdr));
    int rc = LZO_E_OUT_OF_MEMORY;
    if (idx && slen && cap && src && hdrs && bytes && status && out_len && hdr) {
        uint8_t *is_lzo = bytes, *adepth = bytes + n, *sd = bytes + 2 * n, *delivered = bytes + 3 * n;
        size_t m = 0;
        for (size_t b = 0; b < n; b++) {
            struct pom_walk_block w;
            err[b] = -EINVAL;
            memset(&result[b], 0, sizeof result[b]);
            old_len[b] = new_len[b] = 0;
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
            out_len[m] = 0;
            delivered[m] = 0;
            pom_check_header_facts(rec[b], w.is_lzo, &hdr[m]);
            /* (a depth of 255 has no next one: 0 is refused by the split's rule 2) */
            sd[m] = split_depth ? split_depth[b] : (uint8_t)(hdr[m].depth + 1u);
            err[b] = LZO_E_ERROR;                                   /* until its chunk delivers */
            m++;
        }
        struct pom_split_sink G = {.is_lzo = is_lzo, .cap = cap, .adepth = adepth, .hdr = hdr, .sd = sd,
                                   .rec_hdr = hdrs, .idx = idx, .status = status, .out_len = out_len,
                                   .delivered = delivered, .old_out = old_out, .new_out = new_out,
                                   .out_cap = out_cap, .old_len = old_len, .new_len = new_len, .result = result,
                                   .err = err};
        rc = pom_itb_split_chunked(src, slen, m, &G);
        if (len_ok)
            for (size_t k = 0; k < m; k++)
                len_ok[idx[k]] = delivered[k] && (!is_lzo[k] || (status[k] == 0 && out_len[k] == cap[k]));
    }
    free(idx);
    free(slen);
    free(cap);
    free(src);
    free(hdrs);
    free(bytes);
    free(status);
    free(out_len);
    free(hdr);
    return rc;
}
