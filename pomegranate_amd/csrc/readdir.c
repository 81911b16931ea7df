/*
 * readdir.c -- the MDS directory listing (include/pom_readdir.h): per ITB the
 * decode and the FS branch of itb_readdir (mds/itb.c:2536-2589), batched.  The
 * header checks (plus h.entries) and the reassembly in ITB order are gc_scan.c's
 * pom_walk_begin and pom_walk_finish; the chunks -- compressed payloads up, the
 * decoders, the dentry walk (itb_dents.hip), counts and records back -- go
 * through the host batches' pipeline (host_records.c, rd_ops).
 */
#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_readdir.h"

int pom_readdir_dev(const uint8_t *payload, const uint64_t *payload_off,
                    const uint32_t *payload_len, const int32_t *status,
                    const uint8_t *adepth, uint32_t nitb,
                    uint32_t *live, uint32_t *dnum, uint32_t *bytes, uint64_t *first,
                    uint8_t *out, uint64_t out_cap, int32_t *err, void *stream)
{
    return lzo_mi355x_launch_readdir(payload, payload_off, payload_len, status, adepth, nitb, live, dnum,
                                     bytes, first, out, out_cap, err, (hipStream_t)stream);
}

int pom_readdir_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                      uint8_t *out, size_t out_cap, size_t *first,
                      uint32_t *live, uint32_t *dnum, int *err, int *len_ok, int *entries_ok)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    const struct pom_walk_out O = {.out = out, .out_cap = out_cap, .unit = 1, .first = first, .live = live,
                                   .dnum = dnum, .err = err, .len_ok = len_ok, .entries_ok = entries_ok,
                                   .listing = 1};
    struct pom_walk_batch W;
    int rc = pom_walk_begin(&W, rec, rec_len, n, &O);
    if (rc == LZO_E_OK)
        rc = pom_readdir_chunked(W.src, W.slen, W.m, &W.G);
    return pom_walk_finish(&W, rc, &O);
}
