/*
 * pom_lookup.h -- the MDS lookup on the MI355X (liblzo_mi355x.so): decode ITBs
 * and return only the matched MDUs, so that neither the fixed 12 KiB of an ITB
 * nor the rest of its ITEs has to leave the GPU.
 *
 * A cold lookup loads the ITB, decodes all of it (itb_lzo_decompress,
 * mds/itb.c:2949-2980) and walks one hash chain of the index table
 * (itb_search, mds/itb.c:1738-2053, "the very HOT path").  Of the payload it
 * keeps hi->uuid, HVFS_MDU_SIZE bytes and optionally one struct column
 * (:1800-1814, __data_column_hook :1645-1668).  These entry points batch the
 * decode and the read-only INDEX_LOOKUP branch of that walk, for file-system
 * entries matched by name or by uuid (ite_match, mds/itb.c:1092-1149):
 *
 *   pom_lookup_dev    <- the chain walk, ite_match and the MDU copy
 *                        mds/itb.c:1769-1814 (payloads in HBM)
 *   pom_lookup_batch  <- the same over stored records, decoded on the GPU,
 *                        with the header's two rules (:1753-1767, :2030-2033)
 *
 * Everything that writes stays with the caller: create, unlink, update, link,
 * the lease acquire and release and the INDEX_INTENT_* lease setup; so does
 * itb_search_dtriggered.  The INDEX_KV branches are pom_kvget.h's.  The lease word mdu.dtime is
 * inside the returned MDU bytes (record byte 8 + POM_MDU_DTIME_OFF), so the
 * caller runs ite_lease_check_setup's read-only tests (:1688-1708) on the
 * record.
 */
#ifndef POM_LOOKUP_H
#define POM_LOOKUP_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_readdir.h"    /* the ITB and ITE layout, POM_GC_E_TRUNCATED */

#ifdef __cplusplus
extern "C" {
#endif

/* Layout (LP64, the reference's build flags).  struct itb_index,
 * include/xtable.h:104-116, a little-endian u32:
 *   entry = bits 0 ... 14, conflict = bits 15 ... 29, flag = bits 30 ... 31 */
#define POM_ITB_INDEX_ENTRIES 2048u /* 2 << ITB_DEPTH; itb_search's `total` */
#define POM_ITB_INDEX_SIZE 4u
#define POM_IDX_ENTRY_BITS 15u
#define POM_IDX_FLAG_SHIFT 30u
#define POM_IDX_FREE 0u             /* ITB_INDEX_FREE */
#define POM_IDX_UNIQUE 1u           /* ITB_INDEX_UNIQUE */
#define POM_IDX_CONFLICT 2u         /* ITB_INDEX_CONFLICT */
#define POM_IDX_OVERFLOW 3u         /* ITB_INDEX_OVERFLOW */
/* struct ite, include/ite.h:78-114: */
#define POM_ITE_HASH_OFF 0u         /* u64 hash */
#define POM_ITE_MD_OFF 24u          /* the union: s (sdt_md), g (gdt_md), v (kv) */
#define POM_MDU_SIZE 104u           /* HVFS_MDU_SIZE: struct mdu and three u64 */
#define POM_MDU_DTIME_OFF 56u       /* u64 mdu.dtime, the lease word, from POM_ITE_MD_OFF */
#define POM_ITE_UNLINKED 1u         /* ITE_UNLINKED */
#define POM_ITE_SHADOW 3u           /* ITE_SHADOW */
/* struct itbh, include/xtable.h:43-102: */
#define POM_ITBH_FLAG_OFF 0u        /* u8 flag */
#define POM_ITBH_DEPTH_OFF 2u       /* u8 depth */
#define POM_ITBH_ITBID_OFF 136u     /* u64 itbid */
#define POM_ITB_JUST_SPLIT 2u       /* ITB_JUST_SPLIT */

/* Request flags, hvfs_index.flag's values (include/mds_api.h:57-94).  Any
 * other bit is -EINVAL. */
#define POM_LK_BY_NAME 0x1u         /* INDEX_BY_NAME */
#define POM_LK_BY_UUID 0x2u         /* INDEX_BY_UUID, tested before BY_NAME */
#define POM_LK_LOOKUP 0x10u         /* INDEX_LOOKUP: accepted, the call is a lookup anyway */
#define POM_LK_COLUMN 0x40u         /* INDEX_COLUMN: the record's struct column is filled */
#define POM_LK_ITE_ACTIVE 0x01000000u   /* INDEX_ITE_ACTIVE */
#define POM_LK_ITE_SHADOW 0x02000000u   /* INDEX_ITE_SHADOW */

struct pom_lookup_req {          /* 32 bytes */
    uint64_t hash;               /* hi->hash */
    uint64_t uuid;               /* hi->uuid, BY_UUID */
    uint32_t itb;                /* which ITB of the call */
    uint32_t flag;               /* POM_LK_* */
    uint32_t name_off;           /* into the call's name blob, any alignment */
    uint16_t namelen;            /* hi->namelen is a u8: 0 ... 255 */
    uint16_t column;             /* hi->column, with POM_LK_COLUMN: 0 ... 5 */
};

/* One record per request:
 *   [u64 uuid][POM_MDU_SIZE bytes from &ite.g][24 bytes struct column]
 * little-endian; the column is zeros without POM_LK_COLUMN. */
#define POM_LK_REC_SIZE 136u

/* Per-request codes besides 0, -EINVAL, POM_GC_E_TRUNCATED and the decoder's
 * LZO_E_* codes.  LOOP: the chain walk made 2048 ite_match calls and would
 * make another.  An acyclic chain visits each of the 2048 index slots at most
 * once, so the chain is cyclic; the reference would spin forever there. */
#define POM_LK_E_LOOP (-4100)
#define POM_LK_E_NOENT (-2)         /* -ENOENT */
#define POM_LK_E_SPLIT (-1028)      /* -ESPLIT, include/hvfs_const.h:92 */

/* Rules for one request against payload p of n bytes with header adepth; the
 * first that applies decides.  A request that does not end in 0 gets 136 zero
 * bytes and nr = 0; depth counts the non-free slots visited up to then.
 *   0. req.itb >= nitb            -> -EINVAL
 *   1. status[itb] != 0           -> that code
 *   2. adepth 0 or above 10       -> -EINVAL
 *   3. n < 11904 (the index table is not all there) -> POM_GC_E_TRUNCATED
 *   4. a flag bit outside the six above, namelen > 255, POM_LK_COLUMN with
 *      column > 5, or name_off + namelen > names_len -> -EINVAL
 *   5. the walk (mds/itb.c:1769-1797) starts at offset = hash & ((1 << adepth)
 *      - 1).  While offset < 2048: a FREE slot ends it as a miss; else depth++
 *      and ite[entry] is matched.  A hit ends the walk.  A miss on a UNIQUE
 *      slot ends it as a miss; a miss on a CONFLICT or OVERFLOW slot goes on at
 *      offset = conflict (up to 32,767; 2048 or above ends the loop as a miss,
 *      as in the C).  The bitmap is not consulted, as in the reference.
 *   6. ite[entry] ends past n (entry can be up to 32,767) -> POM_GC_E_TRUNCATED
 *      for this request, with that slot counted in depth; no byte at or past n
 *      is loaded.
 *   7. the match is ite_match :1119-1148: with ITE_SHADOW only SHADOW and
 *      UNLINKED entries, with ITE_ACTIVE only ACTIVE ones, and an UNLINKED
 *      entry only with ITE_SHADOW; then BY_UUID (uuid and hash both equal), else
 *      BY_NAME (namelen == e->namelen and the first namelen bytes of s.name
 *      equal; the hash is not compared; namelen 0 matches any entry whose
 *      namelen is 0), else every compare misses.
 *   8. miss -> -ENOENT.  Hit -> 0, nr = entry and the record.  A walk about to
 *      make its 2049th compare -> POM_LK_E_LOOP with depth 2048.
 */

/* nreq lookups over nitb decoded payloads in device memory; enqueue only, like
 * pom_readdir_dev.  Payload b is payload_len[b] bytes at payload +
 * payload_off[b], at any byte alignment; requests may name the ITBs in any
 * order and any number of times.  status may be NULL.  req is 8-byte aligned
 * (it holds u64 fields).  names is the requests'
 * name blob of names_len bytes, at any byte alignment (NULL when names_len is
 * 0).  Nothing outside [0, names_len) of the blob or outside a payload is
 * loaded.  err, nr and depth have nreq entries; request r's record goes to out
 * + 136 * r, every record written in full, out at any byte alignment.  Nothing
 * outside out[0, 136 * nreq) and the three result arrays is written.  Every
 * pointer is device memory.  Returns 0, or -1 when a launch failed. */
int pom_lookup_dev(const uint8_t *payload, const uint64_t *payload_off,
                   const uint32_t *payload_len, const int32_t *status,
                   const uint8_t *adepth, uint32_t nitb,
                   const struct pom_lookup_req *req, uint32_t nreq,
                   const uint8_t *names, uint32_t names_len,
                   int32_t *err, uint32_t *nr, uint32_t *depth, uint8_t *out, void *stream);

/* The same for n ITB records in host memory: rec[b] is a record as stored,
 * [struct itbh][payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes readable;
 * records are not modified.  The header checks and the decode (safe semantics,
 * capacity h.zlen - 264) are pom_gc_scan_batch's: a request against a record
 * that fails them gets -EINVAL, and a decoder code becomes the err of every
 * request of that ITB.  Two more rules come from the header, after those
 * checks and before the walk's:
 *   itbid_check != 0 and ((hash >> 10) & ((1 << h.depth) - 1)) != h.itbid
 *     (in u64; every bit for h.depth >= 64) -> -ESPLIT, depth 0, no walk
 *     (mds/itb.c:1753-1767)
 *   a miss on a record whose h.flag == ITB_JUST_SPLIT -> -ESPLIT instead of
 *     -ENOENT (:2030-2033)
 * An ITB that no request reaches is neither uploaded nor decoded.  Only the
 * compressed payloads, the requests and their names go to the GPU; exactly
 * nreq codes, numbers, depths and records come back.  Returns 0,
 * LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path is unusable (always,
 * without a GPU). */
int pom_lookup_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int itbid_check,
                     const struct pom_lookup_req *req, size_t nreq,
                     const uint8_t *names, size_t names_len,
                     uint8_t *out, int *err, uint32_t *nr, uint32_t *depth);

#ifdef __cplusplus
}
#endif

#endif /* POM_LOOKUP_H */
