/*
 * pom_kvget.h -- the MDS key/value point get on the MI355X
 * (liblzo_mi355x.so): decode ITBs, match by key and return only the values, so
 * that neither the fixed 12 KiB of an ITB nor the rest of its ITEs has to
 * leave the GPU.
 *
 * hvfs_get and hvfs_sget (xtable_get / xtable_sget, mds/capi.c:200-272,
 * :495-570) reach the INDEX_KV branches of itb_search: ite_match compares
 * v.key, and for a string get v.klen and the key bytes in front of the value
 * (mds/itb.c:1095-1116); the hit's struct kv header and value are copied
 * (:1808-1810), with one struct column when asked for (__data_column_hook,
 * :1650-1661), and become the reply's hmr->data (mds/cbht.c:929-972).  These
 * entry points batch the decode, that walk and that copy:
 *
 *   pom_kvget_dev    <- the chain walk, the KV match and the record copy
 *                       (payloads in HBM)
 *   pom_kvget_batch  <- the same over stored records, decoded on the GPU, with
 *                       the header's two rules (:1753-1767, :2030-2033)
 *
 * Everything that writes (xtable_put, update, del, the INDEX_INTENT_* lease
 * setup), itb_search_dtriggered and the decision of the lease test stay with
 * the caller.
 */
#ifndef POM_KVGET_H
#define POM_KVGET_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_kvlist.h"     /* struct kv inside struct ite */
#include "pom_lookup.h"     /* the index table, the walk's codes */

#ifdef __cplusplus
extern "C" {
#endif

/* Request flags, hvfs_index.flag's values (include/mds_api.h:57-99).  Any
 * other bit is -EINVAL. */
#define POM_KG_LOOKUP 0x10u         /* INDEX_LOOKUP: accepted, the call is a lookup anyway */
#define POM_KG_COLUMN 0x40u         /* INDEX_COLUMN: the record ends with column[kvflag & 0xFFF] */
#define POM_KG_KV 0x40000000u       /* INDEX_KV: accepted, the call is a KV get anyway */
/* hvfs_index.kvflag: HVFS_KV_NORMAL or HVFS_KV_STR (POM_KV_*) and the column */
#define POM_KG_MAX_COLUMN 0xFFFu    /* HVFS_KV_MAX_COLUMN */
#define POM_KG_KVFLAG_MASK 0xCFFFu  /* the two kinds and the column number */
#define POM_KG_LEASE_OFF 80u        /* ITE byte of the lease word: s.mdu.dtime = v.value[36 ... 43] */
#define POM_KG_REC_MAX 364u         /* KV_HEADER_LEN + 320 + sizeof(struct column) */

struct pom_kvget_req {           /* 32 bytes */
    uint64_t key;                /* hi->hash */
    uint32_t itb;                /* which ITB of the call */
    uint32_t flag;               /* POM_KG_* */
    uint32_t kvflag;             /* hi->kvflag verbatim */
    uint32_t skey_off;           /* into the call's key blob, any alignment */
    uint32_t sklen;              /* a string get: what the reference carries in hi->uuid */
    uint32_t reserved;           /* ignored */
};

/* Per-request code besides 0, -EINVAL, -ENOENT, -ESPLIT, POM_LK_E_LOOP,
 * POM_GC_E_TRUNCATED and the decoder's LZO_E_* codes.  VALUE: the hit has
 * v.len > 320 (the reference would copy on into the columns). */
#define POM_KG_E_VALUE (-4102)

/* A record is the reference's hmr->data: ITE bytes [24, 44 + v.len) -- v.flags,
 * v.len, v.key, v.klen, v.value -- then, with POM_KG_COLUMN, the 24 bytes of
 * column[kvflag & 0xFFF].  Its length len = 20 + v.len (+ 24) is hmr->len.
 * Records are packed in request order with no padding: record r starts at out
 * + first[r], first being the exclusive prefix of len.
 *
 * Rules for one request against payload p of n bytes with header adepth; the
 * first that applies decides.  A request that does not end in 0 gets nr = 0,
 * len = 0, lease = 0 and no bytes; depth counts the non-free slots visited.
 *   0. req.itb >= nitb            -> -EINVAL
 *   1. status[itb] != 0           -> that code
 *   2. adepth 0 or above 10       -> -EINVAL
 *   3. n < 11904                  -> POM_GC_E_TRUNCATED
 *   4. a flag bit outside the three above, a kvflag bit outside 0xCFFF,
 *      POM_KG_COLUMN with kvflag & 0xFFF above 5 (the reference lets column
 *      numbers up to 4,095 through and reads past the ITE), or a string get
 *      with sklen <= 320 whose skey_off + sklen exceeds keys_len -> -EINVAL
 *   5. the walk is pom_lookup.h's rules 5 and 6 from key & ((1 << adepth) - 1),
 *      POM_LK_E_LOOP at the 2,049th compare and POM_GC_E_TRUNCATED for an
 *      entry whose ITE ends past n included
 *   6. the match (mds/itb.c:1095-1116): ite.flag, the ITE's state and the
 *      entry's own v.flags are not examined.  With HVFS_KV_STR in kvflag:
 *      v.key == key, v.klen == sklen and the first sklen bytes of v.value
 *      equal the blob's; sklen > 320 matches nothing and still walks.
 *      Otherwise (NORMAL, the default): v.key == key.  A string request
 *      always has a key, possibly of length 0: a caller with hi->data == NULL
 *      answers -ENOENT itself
 *   7. a miss -> -ENOENT.  A hit whose v.flags has neither 0x8000 nor 0x4000
 *      -> -EINVAL (mds/cbht.c:974-977).  A hit with v.len > 320 ->
 *      POM_KG_E_VALUE.  Otherwise 0, nr = entry, len as above and lease = ITE
 *      bytes 80 ... 87: itb_search runs ite_lease_check_setup on KV entries
 *      too (:1800-1805), and the record holds those bytes only when v.len >=
 *      44.  The test depends on hmo.tick and stays with the caller.
 */

/* nreq gets over nitb decoded payloads in device memory; enqueue only, like
 * pom_lookup_dev.  Payload b is payload_len[b] bytes at payload +
 * payload_off[b]; payloads, the key blob and out may sit at any byte
 * alignment; req is 8-byte aligned.  status may be NULL, keys may be NULL when
 * keys_len is 0, out when out_cap is 0.  No byte at or past a payload's end is
 * loaded and none outside [0, keys_len) of the blob.  err, nr, depth, len
 * (u32) and lease (u64) have nreq entries, first nreq + 1.  Only offsets of
 * out below out_cap are written (the cap may cut a record anywhere); with
 * out_cap == 0 nothing is emitted.  Nothing outside the six result arrays and
 * out[0, min(first[nreq], out_cap)) is written.  Every pointer is device
 * memory.  Returns 0, or -1 when a launch failed. */
int pom_kvget_dev(const uint8_t *payload, const uint64_t *payload_off,
                  const uint32_t *payload_len, const int32_t *status,
                  const uint8_t *adepth, uint32_t nitb,
                  const struct pom_kvget_req *req, uint32_t nreq,
                  const uint8_t *keys, uint32_t keys_len,
                  int32_t *err, uint32_t *nr, uint32_t *depth, uint32_t *len, uint64_t *lease,
                  uint64_t *first, uint8_t *out, uint64_t out_cap, void *stream);

/* The same for n ITB records in host memory, as stored ([struct itbh]
 * [payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes readable; not
 * modified).  The header checks, the decode, the itbid check (with key in the
 * place of hash), the JUST_SPLIT miss and "an ITB no request reaches is
 * neither uploaded nor decoded" are pom_lookup_batch's.  first has nreq + 1
 * entries.  out == NULL returns lengths only: no record is emitted or copied
 * back.  Otherwise, when first[nreq] exceeds out_cap the call returns
 * POM_GC_E_NOSPACE with first[] and the per-request arrays complete and only
 * out[0, out_cap) written: size the buffer by first[nreq] and call again.
 *
 * The reference's reply for request r with err[r] == 0: hmr->len = len[r],
 * hmr->data = the record, hmr->flag = MD_REPLY_WITH_KV.
 *
 * Only the compressed payloads, the requests and their keys go to the GPU;
 * the five fixed-size results per request and exactly the chunks' record bytes
 * come back.  Returns 0, POM_GC_E_NOSPACE, LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR
 * when the GPU path is unusable (always, without a GPU). */
int pom_kvget_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int itbid_check,
                    const struct pom_kvget_req *req, size_t nreq,
                    const uint8_t *keys, size_t keys_len,
                    uint8_t *out, size_t out_cap, size_t *first,
                    int *err, uint32_t *nr, uint32_t *depth, uint32_t *len, uint64_t *lease);

#ifdef __cplusplus
}
#endif

#endif /* POM_KVGET_H */
