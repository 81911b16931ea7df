/*
 * check.c -- the ITB check (include/pom_check.h): per record the decode switch
 * of mdsl_gc_data_round (mdsl/gc.c:945-960) and the check of the bitmap, the
 * index table and the header's counters against each other, batched.  Here are
 * the selection (the header checks are host_requests.c's pom_itb_walk_header;
 * a record with h.entries == 0 is checked like any other), the header facts the
 * check takes from each record, and the results' order; the chunks --
 * compressed payloads and header facts up, the decoders, the check
 * (itb_check.hip), codes, reports and masks back -- go through the host
 * batches' pipeline (host_records.c, ck_ops).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "host_requests.h"
#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_check.h"
#include "pom_itb.h"

int pom_itb_check_dev(const uint8_t *payload, const uint64_t *payload_off,
                      const uint32_t *payload_len, const int32_t *status,
                      const uint8_t *adepth, const struct pom_check_hdr *hdr,
                      uint32_t nitb, uint32_t flags,
                      struct pom_check_report *report, uint64_t *slot_mask, uint64_t *ite_mask,
                      int32_t *err, void *stream)
{
    if (flags & ~POM_CK_ITBID)
        return -EINVAL;
    return lzo_mi355x_launch_itb_check(payload, payload_off, payload_len, status, adepth, hdr, nitb, flags, report,
                                       slot_mask, ite_mask, err, (hipStream_t)stream);
}

/* What the check needs of a record's struct itbh. */
void pom_check_header_facts(const uint8_t *rec, int is_lzo, struct pom_check_hdr *h)
{
    uint32_t len;
    memset(h, 0, sizeof *h);
    memcpy(&h->entries, rec + POM_ITBH_ENTRIES_OFF, 4);
    memcpy(&h->max_offset, rec + POM_ITBH_MAX_OFFSET_OFF, 4);
    memcpy(&h->pseudo_conflicts, rec + POM_ITBH_PSEUDO_CONFLICTS_OFF, 4);
    memcpy(&len, rec + (is_lzo ? POM_ITBH_ZLEN_OFF : POM_ITBH_LEN_OFF), 4);
    h->ulen = len;
    memcpy(&h->inf, rec + POM_ITBH_INF_OFF, 2);
    memcpy(&h->itu, rec + POM_ITBH_ITU_OFF, 2);
    h->depth = rec[POM_ITBH_DEPTH_OFF];
    memcpy(&h->itbid, rec + POM_ITBH_ITBID_OFF, 8);
}

int pom_itb_check_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, uint32_t flags,
                        struct pom_check_report *report, uint64_t *slot_mask, uint64_t *ite_mask,
                        int *err, int *len_ok)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    if (flags & ~POM_CK_ITBID)
        return -EINVAL;
    size_t *idx = malloc((n + 1) * sizeof(*idx));
    size_t *slen = malloc((n + 1) * sizeof(*slen));
    size_t *cap = malloc((n + 1) * sizeof(*cap));
    const uint8_t **src = malloc((n + 1) * sizeof(*src));
    uint8_t *bytes = malloc(2 * n + 1);                             /* is_lzo[m], adepth[m] */
    int32_t *i32 = malloc((2 * n + 1) * sizeof(*i32));              /* status[m], err[m] */
    uint32_t *out_len = malloc((n + 1) * sizeof(*out_len));
    struct pom_check_hdr *hdr = malloc((n + 1) * sizeof(*hdr));
    int rc = LZO_E_OUT_OF_MEMORY;
    if (idx && slen && cap && src && bytes && i32 && out_len && hdr) {
        uint8_t *is_lzo = bytes, *adepth = bytes + n;
        int32_t *status = i32, *kerr = i32 + n;
        size_t m = 0;
        for (size_t b = 0; b < n; b++) {
            struct pom_walk_block w;
            err[b] = -EINVAL;
            memset(&report[b], 0, sizeof report[b]);
            if (slot_mask)
                memset(slot_mask + POM_CK_SLOT_MASK_WORDS * b, 0, 8 * POM_CK_SLOT_MASK_WORDS);
            if (ite_mask)
                memset(ite_mask + POM_CK_ITE_MASK_WORDS * b, 0, 8 * POM_CK_ITE_MASK_WORDS);
            if (len_ok)
                len_ok[b] = 0;
            if (pom_itb_walk_header(rec[b], rec_len[b], &w) != 0)
                continue;
            idx[m] = b;
            src[m] = w.src;
            slen[m] = w.src_len;
            cap[m] = w.cap;
            is_lzo[m] = w.is_lzo;
            adepth[m] = w.adepth;
            status[m] = 0;
            kerr[m] = LZO_E_ERROR;                                  /* until its chunk delivers */
            out_len[m] = 0;
            pom_check_header_facts(rec[b], w.is_lzo, &hdr[m]);
            m++;
        }
        struct pom_check_sink G = {.is_lzo = is_lzo, .cap = cap, .adepth = adepth, .hdr = hdr, .idx = idx,
                                   .flags = flags, .status = status, .err = kerr, .out_len = out_len,
                                   .report = report, .slot_mask = slot_mask, .ite_mask = ite_mask};
        rc = pom_itb_check_chunked(src, slen, m, &G);
        /* (the kernel's rule 1 has put a decoder's code into err) */
        for (size_t k = 0; k < m; k++) {
            err[idx[k]] = kerr[k];
            if (len_ok)
                len_ok[idx[k]] = kerr[k] != LZO_E_ERROR && (!is_lzo[k] || (status[k] == 0 && out_len[k] == cap[k]));
        }
    }
    free(idx);
    free(slen);
    free(cap);
    free(src);
    free(bytes);
    free(i32);
    free(out_len);
    free(hdr);
    return rc;
}
