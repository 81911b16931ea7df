/*
 * pom_readdir.h -- the MDS directory listing on the MI355X (liblzo_mi355x.so):
 * decode ITBs and return only their dentries, so that neither the fixed 12 KiB
 * of an ITB nor the rest of its ITEs has to leave the GPU.
 *
 * Per ITB of a directory, cbht_itb_hit (mds/cbht.c:899-907, INDEX_BY_ITB)
 * calls itb_readdir (mds/itb.c:2464-2593), whose FS branch (:2536-2589) keeps
 * {uuid, mode, namelen} and the name of every live, active, non-KV ITE.  These
 * entry points batch the decode and that walk:
 *
 *   pom_readdir_dev    <- the bitmap walk and the dentry_info records
 *                         mds/itb.c:2567-2585 (payloads in HBM)
 *   pom_readdir_batch  <- the same over stored records, decoded on the GPU
 *                         (records in host memory)
 *
 * The INDEX_KV branch (mds/itb.c:2472-2534: "%ld" keys and the strstr filter;
 * there is no regex on that path) is pom_kvlist.h's.  The INDEX_DTRIG triggers
 * (itb_readdir_dtriggered) stay with the caller, as do the reply's allocation
 * and its zero tail (see pom_readdir_batch).
 */
#ifndef POM_READDIR_H
#define POM_READDIR_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_gc.h"     /* the ITB layout, POM_GC_E_TRUNCATED, POM_GC_E_NOSPACE */

#ifdef __cplusplus
extern "C" {
#endif

/* Layout (LP64, the reference's build flags).  struct ite, include/ite.h:78-114: */
#define POM_ITE_UUID_OFF 8u         /* u64 uuid */
#define POM_ITE_FLAG_OFF 16u        /* u32 flag */
#define POM_ITE_NAMELEN_OFF 20u     /* u32 namelen */
#define POM_ITE_MODE_OFF 36u        /* u16 s.mdu.mode */
#define POM_ITE_NAME_OFF 104u       /* char s.name[256] */
#define POM_ITE_NAME_MAX 256u
#define POM_ITE_STATE_MASK 7u       /* ITE_STATE_MASK; ITE_ACTIVE is state 0 */
#define POM_ITE_FLAG_KV 0x01000000u /* ITE_FLAG_KV */
/* struct dentry_info, include/mds_api.h:171-178: */
#define POM_DENT_HDR 16u            /* sizeof: [u64 uuid][u16 mode][u16 namelen][u32 0] */
#define POM_DENT_MODE_OFF 8u
#define POM_DENT_NAMELEN_OFF 10u

/* Per-ITB code besides 0, -EINVAL, POM_GC_E_TRUNCATED and the decoder's
 * LZO_E_* codes.  NAME: an emitted ITE has namelen > 256; the ITB then yields
 * no record (the reference would copy past s.name into the columns and cut
 * namelen to 16 bits). */
#define POM_RD_E_NAME (-4099)

/* A record is what mds/itb.c:2575-2582 writes into its zeroed buffer:
 *   [u64 uuid][u16 mode][u16 namelen][u32 0][name, namelen bytes]
 * little-endian, records packed with no padding between them.
 *
 * Rules for one ITB (payload p of n bytes, its header's adepth); the first
 * that applies decides:
 *   1. status[b] != 0            -> err = that code, live = dnum = bytes = 0
 *   2. adepth 0 or above 10      -> -EINVAL, live = dnum = bytes = 0
 *   3. n < 3712                  -> POM_GC_E_TRUNCATED, live = dnum = bytes = 0
 *   4. live = the set bitmap bits below 1 << adepth.  A live ITE that ends
 *      past n -> POM_GC_E_TRUNCATED, dnum = bytes = 0 (the highest live bit
 *      decides, as in pom_gc_scan_dev)
 *   5. a live ITE is emitted iff (flag & 7) == ITE_ACTIVE and !(flag &
 *      ITE_FLAG_KV) (mds/itb.c:2569-2574); a skipped ITE's namelen is not
 *      examined
 *   6. an emitted ITE with namelen > 256 -> POM_RD_E_NAME, dnum = bytes = 0
 *   7. else err = 0, dnum = the ITEs emitted, bytes = the sum of 16 + namelen,
 *      records in ascending bit order; namelen 0 gives a 16-byte record.
 */

/* The walk over nitb decoded payloads in device memory; enqueue only, like
 * pom_gc_scan_dev.  Payload b is payload_len[b] bytes at payload +
 * payload_off[b], at any byte alignment (entries may repeat).  No byte at or
 * past a payload's end is loaded, and none outside a live ITE that lies
 * inside the payload, except the bitmap.  status may be NULL.  first (u64,
 * nitb + 1 entries): first[b] = the byte offset of ITB b's first record,
 * first[nitb] = the total.  ITB b's bytes go to out + first[b] ...; only
 * offsets below out_cap are written, so a record may be cut by the cap in its
 * header or in its name, and no byte outside [first[b], min(first[b] +
 * bytes[b], out_cap)) is written on behalf of ITB b.  out may have any byte
 * alignment and may be NULL when out_cap is 0.  Every pointer is device
 * memory.  Returns 0, or -1 when a launch failed. */
int pom_readdir_dev(const uint8_t *payload, const uint64_t *payload_off,
                    const uint32_t *payload_len, const int32_t *status,
                    const uint8_t *adepth, uint32_t nitb,
                    uint32_t *live, uint32_t *dnum, uint32_t *bytes, uint64_t *first,
                    uint8_t *out, uint64_t out_cap, int32_t *err, void *stream);

/* The same for n ITB records in host memory: rec[b] is a record as stored,
 * [struct itbh][payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes readable;
 * records are not modified.  The header checks, the decode (safe semantics,
 * capacity h.zlen - 264, a decoder code becomes err[b]), len_ok[b] and the
 * treatment of uncompressed records are exactly pom_gc_scan_batch's, with two
 * more header rules: h.entries < 0 is -EINVAL, and a record with h.entries ==
 * 0 is not sent to the GPU and yields err = 0, live = dnum = 0 and no bytes
 * (the reference returns before it looks at the bitmap, mds/itb.c:2540-2544).
 * live[b], dnum[b] and err[b] as pom_readdir_dev; entries_ok[b]: err[b] == 0
 * and live[b] == h.entries.  len_ok and entries_ok may be NULL.  Records come
 * out in ITB order, then bit order: first[b] (n + 1 entries) = the byte
 * offset of ITB b's first record, first[n] = the total, so ITB b's bytes are
 * first[b + 1] - first[b].  When the total exceeds out_cap the call returns
 * POM_GC_E_NOSPACE with first[], live[], dnum[] and err[] complete and only
 * out[0, out_cap) written: size the buffer by first[n] and call again.
 *
 * The reference's reply for ITB b with err[b] == 0 and entries_ok[b], where
 * bytes = first[b + 1] - first[b] (mds/itb.c:2540-2587):
 *   hmr->len  = 16 * h.entries + (bytes - 16 * dnum[b])
 *   hmr->dnum = h.entries - (live[b] - dnum[b])
 *   hmr->data = ITB b's records followed by zeros up to hmr->len
 *
 * Only the compressed payloads go to the GPU; only the per-ITB counts and
 * exactly first[n] bytes of records come back.  Returns 0, POM_GC_E_NOSPACE,
 * LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path is unusable (always,
 * without a GPU). */
int pom_readdir_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                      uint8_t *out, size_t out_cap, size_t *first,
                      uint32_t *live, uint32_t *dnum, int *err, int *len_ok, int *entries_ok);

#ifdef __cplusplus
}
#endif

#endif /* POM_READDIR_H */
