/*
 * kvlist.c -- the MDS key/value table listing (include/pom_kvlist.h): per ITB
 * the decode and the INDEX_KV branch of itb_readdir (mds/itb.c:2472-2534),
 * batched.  The header checks (readdir.c's) and the reassembly in ITB order
 * are gc_scan.c's pom_walk_begin and pom_walk_finish; the chunks -- compressed
 * payloads and the needle up, the decoders, the key walk (itb_keys.hip),
 * counts, masks and records back -- go through the host batches' pipeline
 * (host_records.c, kv_ops).
 */
#include <errno.h>

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
    /* out == NULL: count-only */
    const struct pom_walk_out O = {.out = out, .out_cap = out ? out_cap : 0, .unit = 1, .first = first,
                                   .live = live, .dnum = dnum, .keybytes = keybytes, .mask = mask, .err = err,
                                   .len_ok = len_ok, .entries_ok = entries_ok, .listing = 1, .count_only = !out};
    struct pom_walk_batch W;
    int rc = pom_walk_begin(&W, rec, rec_len, n, &O);
    if (rc == LZO_E_OK) {
        W.G.kv_op = op;
        W.G.needle = needle;
        W.G.needle_len = needle_len;
        W.G.count_only = !out;
        rc = pom_kvlist_chunked(W.src, W.slen, W.m, &W.G);
    }
    return pom_walk_finish(&W, rc, &O);
}
