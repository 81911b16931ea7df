/*
 * itb_rules.h -- what the ITB record codec decides once the LZO batch has come
 * back from the GPU: which record is kept, what its header says, which code is
 * reported.  Pure host code without a GPU call, shared by itb_codec.c and
 * xnet_frame.c and driven alone by tests/native/itb_rules_host.cc.
 *
 *   compress    itb_lzo_compress    mds/itb.c:2904-2945
 *   decompress  itb_lzo_decompress  mds/itb.c:2949-2980, mdsl/gc.c:755-786
 */
#ifndef POM_ITB_RULES_H
#define POM_ITB_RULES_H 1

#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pom_itb.h"

static inline uint32_t itb_rules_rd32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

static inline void itb_rules_wr32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
static inline void itb_rules_wr16(uint8_t *p, uint16_t v) { memcpy(p, &v, 2); }

/* The payload bytes a record's header announces (0 below the header size). */
static inline size_t itb_rules_payload_len(const uint8_t *rec)
{
    const uint32_t len = itb_rules_rd32(rec + POM_ITBH_LEN_OFF);
    return len >= POM_ITBH_SIZE ? len - POM_ITBH_SIZE : 0;
}

/* Whether the encoder may write a payload of slen bytes straight to tmp + 264:
 * only when tmp holds the worst case (`worst` = lzo_mi355x_worst_compress(slen));
 * otherwise it writes to a side buffer of `worst` bytes. */
static inline int itb_rules_direct(size_t tmp_cap, size_t worst)
{
    return tmp_cap >= POM_ITBH_SIZE && tmp_cap - POM_ITBH_SIZE >= worst;
}

/* Finish of a compress (mds/itb.c:2923-2944).  `z` holds the dlen compressed
 * bytes of the slen-byte payload: tmp + 264 itself, or a side buffer.  `st` is
 * the encoder's LZO_E_* code.  *oi = in (kept) or tmp (compressed); *err = 0,
 * -EINVAL (h.len below the header size) or st.
 * The record is kept uncompressed when the stream is not smaller than the
 * payload (the reference's rule) or when header + stream do not fit tmp_cap
 * (the column codec's rule, column_codec.c).  No byte at or past tmp + tmp_cap
 * is written: nothing at all when tmp_cap < 264, at most the header when the
 * record is kept. */
static inline void itb_rules_finish_compress(uint8_t *in, uint8_t *tmp, size_t tmp_cap, const uint8_t *z,
                                             size_t slen, size_t dlen, int st, uint8_t **oi, int *err)
{
    *oi = in;
    *err = 0;
    if (itb_rules_rd32(in + POM_ITBH_LEN_OFF) < POM_ITBH_SIZE) {
        *err = -EINVAL;
        return;
    }
    if (tmp_cap >= POM_ITBH_SIZE)
        memcpy(tmp, in, POM_ITBH_SIZE);                       /* the itb header */
    if (st != 0) {
        *err = st;
        return;
    }
    if (dlen >= slen)                                         /* impossible to compress */
        return;
    if (tmp_cap < POM_ITBH_SIZE || tmp_cap - POM_ITBH_SIZE < dlen)
        return;                                               /* no room: as if it did not pay */
    if (z != tmp + POM_ITBH_SIZE)
        memcpy(tmp + POM_ITBH_SIZE, z, dlen);
    itb_rules_wr32(tmp + POM_ITBH_ZLEN_OFF, itb_rules_rd32(tmp + POM_ITBH_LEN_OFF));
    itb_rules_wr32(tmp + POM_ITBH_LEN_OFF, (uint32_t)(POM_ITBH_SIZE + dlen));
    itb_rules_wr16(tmp + POM_ITBH_ALGO_OFF, POM_COMPR_LZO);
    *oi = tmp;
}

/* Finish of a decompress (mds/itb.c:2966-2979): `st` is the decoder's LZO_E_*
 * code and `produced` the bytes it wrote after the header `hdr` (264 bytes,
 * still holding the stored zlen).  *err = st; *len_ok (may be NULL) = the
 * decode succeeded and produced zlen - 264 bytes.  Always: compress_algo =
 * COMPR_NONE, len = 264 + produced.  Returns the new len. */
static inline uint32_t itb_rules_finish_decompress(uint8_t *hdr, int st, size_t produced, int *err, int *len_ok)
{
    const uint32_t zlen = itb_rules_rd32(hdr + POM_ITBH_ZLEN_OFF);
    const uint32_t len = (uint32_t)(produced + POM_ITBH_SIZE);
    *err = st;
    if (len_ok)
        *len_ok = st == 0 && produced + POM_ITBH_SIZE == zlen;
    itb_rules_wr16(hdr + POM_ITBH_ALGO_OFF, POM_COMPR_NONE);  /* clear the compress flag */
    itb_rules_wr32(hdr + POM_ITBH_LEN_OFF, len);
    return len;
}

#endif /* POM_ITB_RULES_H */
