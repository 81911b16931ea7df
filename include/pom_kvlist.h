/*
 * pom_kvlist.h -- the MDS key/value table listing on the MI355X
 * (liblzo_mi355x.so): decode ITBs, scan or grep their entries and return only
 * the keys, so that neither the fixed 12 KiB of an ITB nor the values that
 * were searched have to leave the GPU.
 *
 * Per ITB of an xTable key/value table, hvfs_list (api/api.c:3272-3447)
 * reaches mds_list (mds/c2m.c:782-872) and with it the INDEX_KV branch of
 * itb_readdir (mds/itb.c:2472-2534), which keeps a 4-byte length and the key
 * of every live entry that passes __readdir_filter (mds/itb.c:2422-2458): one
 * strstr of a needle of at most 255 bytes in a string that starts inside
 * v.value[320].  These entry points batch the decode, that search and that
 * walk:
 *
 *   pom_kvlist_dev    <- the bitmap walk, the filter and the key records
 *                        mds/itb.c:2508-2532 (payloads in HBM)
 *   pom_kvlist_batch  <- the same over stored records, decoded on the GPU
 *                        (records in host memory)
 *
 * The INDEX_DTRIG triggers (itb_readdir_dtriggered) and the reply's allocation
 * and its zero tail stay with the caller.  The INDEX_KV branches of ite_match
 * and of the lookup's copy (mds/itb.c:1095-1116, :1808-1810: hvfs_get /
 * hvfs_sget) are pom_kvget.h's.
 */
#ifndef POM_KVLIST_H
#define POM_KVLIST_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_readdir.h"    /* the ITE layout, POM_RD_E_NAME; pom_gc.h's ITB layout and codes */

#ifdef __cplusplus
extern "C" {
#endif

/* Layout (LP64, the reference's build flags).  struct kv inside struct ite,
 * include/ite.h: */
#define POM_KV_FLAGS_OFF 24u        /* u32 v.flags (the same word as mdu.flags) */
#define POM_KV_LEN_OFF 28u          /* u32 v.len */
#define POM_KV_KEY_OFF 32u          /* u64 v.key */
#define POM_KV_KLEN_OFF 40u         /* u32 v.klen */
#define POM_KV_VALUE_OFF 44u        /* u8 v.value[320] */
#define POM_KV_VALUE_MAX 320u
#define POM_KV_SIZE 344u            /* sizeof(struct kv) */
#define POM_KV_HEADER_LEN 20u       /* KV_HEADER_LEN */
#define POM_KV_NORMAL 0x8000u       /* HVFS_KV_NORMAL */
#define POM_KV_STR 0x4000u          /* HVFS_KV_STR */
#define POM_KV_OP_SCAN 0u           /* KV_OP_SCAN */
#define POM_KV_OP_SCAN_CNT 1u       /* KV_OP_SCAN_CNT */
#define POM_KV_OP_GREP 2u           /* KV_OP_GREP */
#define POM_KV_OP_GREP_CNT 3u       /* KV_OP_GREP_CNT */
#define POM_KV_NEEDLE_MAX 255u      /* hi->namelen is a u8 */
#define POM_KV_TEXT_MAX 20u         /* snprintf("%ld") of INT64_MIN */
#define POM_KV_MASK_WORDS 16u       /* u64 words of an ITB's emit mask */

/* Per-ITB code besides 0, -EINVAL, POM_GC_E_TRUNCATED, POM_RD_E_NAME and the
 * decoder's LZO_E_* codes.  KEY: a live HVFS_KV_STR entry has klen > 320; the
 * ITB then lists nothing (the reference would copy on into the columns and
 * the next ITE). */
#define POM_KV_E_KEY (-4101)

/* A record is what mds/itb.c:2510-2530 writes into its zeroed buffer:
 *   [u32 keylen][key, keylen bytes]
 * little-endian, records packed with no padding between them.  A zero-length
 * key yields a 4-byte record; the reference client's parse loop stops at such
 * a record (api/api.c:3413-3415), so what follows it in a reply is not seen
 * by hvfs_list's callers.
 *
 * Rules for one ITB (payload p of n bytes, its header's adepth); the first
 * that applies decides:
 *   1. status[b] != 0            -> err = that code, every count 0
 *   2. adepth 0 or above 10      -> -EINVAL
 *   3. n < 3712                  -> POM_GC_E_TRUNCATED
 *   4. live = the set bitmap bits below 1 << adepth.  A live ITE that ends
 *      past n -> POM_GC_E_TRUNCATED with nothing emitted (as pom_gc_scan_dev)
 *   5. every live ITE takes part; ite.flag (state, ITE_FLAG_KV) is not
 *      examined, as in the reference.  Its kind comes from v.flags: NORMAL if
 *      flags & 0x8000, else STR if flags & 0x4000, else NAME
 *   6. its key: NORMAL -- the decimal text of v.key read as int64, 1 to 20
 *      bytes, as "%ld" prints it; STR -- v.klen bytes from v.value; NAME --
 *      namelen bytes of s.name.  A live STR entry with klen > 320 ->
 *      POM_KV_E_KEY, a live NAME entry with namelen > 256 -> POM_RD_E_NAME;
 *      either way the ITB lists nothing.  Both tests apply to every live
 *      entry, whether or not the filter would drop it; with both in one ITB
 *      POM_KV_E_KEY wins
 *   7. the filter: op 0 or 1 emits every live entry.  op 2 or 3 emits a
 *      NORMAL or STR entry iff the needle occurs in its haystack, and every
 *      NAME entry (the copy loop does not filter those).  The needle is the
 *      needle_len bytes (0 ... 255) up to but excluding their first zero byte
 *      (the reference copies hi->namelen bytes and NUL-terminates them); an
 *      empty needle matches every entry.  The haystack starts at ITE byte 44
 *      for NORMAL and at 44 + klen for STR and runs to the first zero byte,
 *      or to ITE byte 364 where there is none.  That bound is the one place
 *      the reference is undefined: ite_create does not terminate values, so a
 *      value of 320 non-zero bytes lets strstr read on into the columns.
 *      Wherever a zero byte lies inside v.value the result is the reference's
 *   8. with err 0: dnum = the entries emitted, bytes = the sum of 4 + keylen
 *      over them, keybytes = the sum of keylen over ALL live entries, mask =
 *      sixteen u64 words, bit l of word r set when ITE 64r + l was emitted
 *      (all zero with any error), records in ascending bit order.
 */

/* The walk over nitb decoded payloads in device memory; enqueue only, like
 * pom_readdir_dev.  Payload b is payload_len[b] bytes at payload +
 * payload_off[b]; payloads, needle and out may sit at any byte alignment.  No
 * byte at or past a payload's end is loaded, none outside a live ITE that
 * lies inside the payload except the bitmap, and none outside [needle, needle
 * + needle_len).  status may be NULL; needle may be NULL when needle_len is
 * 0.  live, dnum, bytes, keybytes: u32 per ITB; mask: 16 u64 per ITB, or NULL
 * (the call then keeps the masks in device memory of its own, allocated and
 * freed in stream order); first (u64, nitb + 1 entries) = the exclusive
 * prefix of bytes.  ITB b's records go to out + first[b] ...; only offsets of
 * out below out_cap are written, so the cap may cut a length word or a key.
 * out may be NULL when out_cap is 0.  Every pointer is device memory.
 * Returns 0, or -1 for op > 3, needle_len > 255 or a failed launch. */
int pom_kvlist_dev(const uint8_t *payload, const uint64_t *payload_off,
                   const uint32_t *payload_len, const int32_t *status,
                   const uint8_t *adepth, uint32_t nitb, uint32_t op,
                   const uint8_t *needle, uint32_t needle_len,
                   uint32_t *live, uint32_t *dnum, uint32_t *bytes, uint32_t *keybytes,
                   uint64_t *mask, uint64_t *first, uint8_t *out, uint64_t out_cap,
                   int32_t *err, void *stream);

/* The same for n ITB records in host memory, as stored ([struct itbh]
 * [payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes readable; not
 * modified).  The header checks, the decode, len_ok[b] and entries_ok[b] are
 * exactly pom_readdir_batch's: h.entries < 0 is -EINVAL, and a record with
 * h.entries == 0 is answered on the host with err = 0 and every count 0 (the
 * reference leaves at mds/itb.c:2479-2482, before the bitmap).  Records come
 * out in ITB order, then bit order; first[b] (n + 1 entries) is the byte
 * offset of ITB b's first record, first[n] the total.  mask (16 u64 per
 * record), keybytes, len_ok and entries_ok may be NULL; the masks are copied
 * back from the GPU only when asked for.
 *
 * out == NULL makes the call count-only: nothing is emitted and no record
 * byte is copied back; it returns 0 with first[] and every count complete.
 * This serves LIST_OP_COUNT and LIST_OP_GREP_COUNT, for which the reference
 * ships every key to the client.  Otherwise, when the total exceeds out_cap
 * the call returns POM_GC_E_NOSPACE with first[] and the counts complete and
 * only out[0, out_cap) written: size the buffer by first[n] and call again.
 *
 * The reference's reply for ITB b with err[b] == 0 and entries_ok[b]
 * (mds/itb.c:2478-2534):
 *   hmr->len  = 4 * h.entries + keybytes[b]
 *   hmr->dnum = h.entries
 *   hmr->data = ITB b's records followed by zeros up to hmr->len
 *
 * Only the compressed payloads and the needle go to the GPU; only the per-ITB
 * counts, the masks when asked for and exactly first[n] bytes of records come
 * back.  Returns 0, POM_GC_E_NOSPACE, -EINVAL for op > 3 or needle_len > 255,
 * LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path is unusable (always,
 * without a GPU). */
int pom_kvlist_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                     uint32_t op, const uint8_t *needle, uint32_t needle_len,
                     uint8_t *out, size_t out_cap, size_t *first,
                     uint32_t *live, uint32_t *dnum, uint32_t *keybytes, uint64_t *mask,
                     int *err, int *len_ok, int *entries_ok);

#ifdef __cplusplus
}
#endif

#endif /* POM_KVLIST_H */
