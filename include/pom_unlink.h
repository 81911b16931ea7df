/*
 * pom_unlink.h -- the ITB unlink on the MI355X (liblzo_mi355x.so): find an
 * entry of a decoded ITB as the lookup does, return its MDU, and unlink it on
 * the GPU, so that a cold ITB whose entries are unlinked does not have to come
 * back to host memory.
 *
 * itb_search with INDEX_UNLINK (mds/itb.c:1769-1797 the walk, :1889-1911 the
 * branch, :2029-2033 the miss) walks the chain of the request's home slot with
 * ite_match, sets hi->uuid, copies HVFS_MDU_SIZE bytes from &ite.g -- before
 * the unlink, so the reply shows the old nlink -- and calls ite_unlink
 * (:676-735), which changes at most the flag word and nlink of that one ITE
 * and, where the delete is synchronous, cuts one slot out of one chain
 * (itb_del_ite, :602-671, with __ite_unlink, :567-592):
 *
 *   pom_itb_unlink_dev     <- the check, then the requests of each ITB in
 *                             order, over decoded payloads in HBM
 *   pom_itb_unlink_batch   <- the same over stored records: decoded, unlinked
 *                             and encoded on the GPU
 *   pom_itb_unlink_header  <- the ITB's struct itbh from the old one and the
 *                             result, on the host
 *
 * With hmo.conf.async_unlink set, an entry whose nlink reached 0 is only
 * marked ITE_UNLINKED; pom_sweep.h removes those later.  Together the two are
 * the delete life cycle.
 *
 * What stays with the caller: itb_dirty and the copy on write; the index
 * lock; listing the ITB on hmo.async_unlink when something was marked; the
 * directory delta (txg_add_rdir, txg_add_update_ddelta: reported per request
 * as POM_UL_DELTA); prof.cbht.aentry -= removed.  Key/value deletes (hvfs_del,
 * matched by key) are not served here.
 */
#ifndef POM_UNLINK_H
#define POM_UNLINK_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_lookup.h"     /* struct pom_lookup_req, the POM_LK_* flags, POM_LK_REC_SIZE */
#include "pom_sweep.h"      /* POM_SPLIT_E_DAMAGED, struct pom_check_hdr, the delete's counters */

#ifdef __cplusplus
extern "C" {
#endif

/* Requests are struct pom_lookup_req as they stand; `column` must be 0.
 * Request flags: POM_LK_BY_NAME, POM_LK_BY_UUID, POM_LK_ITE_ACTIVE,
 * POM_LK_ITE_SHADOW and: */
#define POM_UL_UNLINK 0x00200000u   /* INDEX_UNLINK: accepted, the call is an unlink anyway */
/* Any other bit is -EINVAL: POM_LK_LOOKUP, POM_LK_COLUMN and INDEX_KV too. */

/* The ITE flag bits ite_unlink reads (include/ite.h:91-99) besides
 * POM_ITE_FLAG_KV, and the mode bit it tests. */
#define POM_ITE_FLAG_NORMAL 0x80000000u /* ITE_FLAG_NORMAL */
#define POM_ITE_FLAG_LS 0x40000000u     /* ITE_FLAG_LS */
#define POM_ITE_FLAG_SDT 0x10000000u    /* ITE_FLAG_SDT */
#define POM_ITE_FLAG_SYM 0x02000000u    /* ITE_FLAG_SYM */
#define POM_ITE_NLINK_OFF 38u           /* u16 s.mdu.nlink */
#define POM_UL_MODE_DIR 0x4000u         /* S_IFDIR (0040000) as a bit: block devices and sockets have it too */

/* A request's fourth result word: what ite_unlink did to the ITE that hit,
 * or-ed with POM_UL_DELTA when the directory delta is owed. */
#define POM_UL_NONE 0u              /* the flag has none of NORMAL, SYM, LS, KV: nothing changed */
#define POM_UL_SHADOWED 1u          /* nlink left above 0: state ITE_SHADOW */
#define POM_UL_MARKED 2u            /* nlink 0, async_unlink: state ITE_UNLINKED */
#define POM_UL_DELETED 3u           /* itb_del_ite */
#define POM_UL_WHAT_MASK 0xFFu
#define POM_UL_DELTA 0x100u

struct pom_unlink_result {           /* 32 bytes per ITB */
    int32_t  err;                    /* 0, or the first ITB rule that applies */
    uint32_t changed;                /* requests whose `what` is not POM_UL_NONE */
    uint32_t removed;                /* __ite_unlink calls */
    uint32_t len;                    /* uncompressed record length after the unlinks; 0 when nothing is produced */
    int32_t  entries, max_offset, pseudo_conflicts;
    uint16_t itu;
    uint16_t hits;                   /* requests that ended 0 (65535: that many or more) */
};

/* ITBs are independent.  The requests of one ITB apply in the caller's request
 * order, and each sees everything the earlier ones of that ITB left: flags,
 * nlink, the chain, the bitmap and the counters.
 *
 * ITB rules; the first that applies decides, and every request of the ITB then
 * reads that code:
 *   1. the check's err (pom_check.h rules 1 ... 4)
 *   2. payload_off[b] not a multiple of 16           -> -EINVAL
 *   3. any finding other than kind 15                -> POM_SPLIT_E_DAMAGED; a
 *      table the check refuses is never walked or edited.  (Every walk has a
 *      hard bound of 1025 slots all the same, every slot and ITE number is
 *      range-checked before it is an index, and itb_del_ite's trailing
 *      needswap case -- a head that no slot followed -- requires a UNIQUE
 *      home slot; what fails any of these is POM_SPLIT_E_DAMAGED for the ITB
 *      and all its requests, with nothing stored.  A table the check passes
 *      cannot get there.)
 * With err != 0 nothing but result[b] and the requests' results is written,
 * and result[b]'s other fields are zero.  With err == 0 and changed == 0 every
 * field but err and hits is zero and no payload byte is written.  A record is
 * produced exactly when err == 0 and changed > 0.
 *
 * Request rules; the first that applies decides.  A request that does not end
 * in 0 gets 136 zero bytes and nr = what = 0; depth counts the non-free slots
 * visited up to then.
 *   0. req.itb is not the number of the group the request lies in -> -EINVAL
 *   1. the ITB's code, when it is not 0
 *   4. a flag bit outside the five above, namelen > 255, column != 0 or
 *      name_off + namelen > names_len                            -> -EINVAL
 *   5. the walk (mds/itb.c:1769-1797) from offset = hash & ((1 << adepth) -
 *      1): a FREE slot ends it as a miss; else depth++ and ite[entry] is
 *      matched.  A hit ends the walk; a miss on a UNIQUE slot ends it as a
 *      miss, a miss on a CONFLICT slot goes on at `conflict`.
 *   7. the match is ite_match (pom_lookup.h rule 7) on the ITE's flag as the
 *      earlier requests left it.
 *   8. miss -> -ENOENT.
 *   9. hit on an ITE whose flag has ITE_FLAG_KV together with NORMAL, SYM or
 *      LS -> -EINVAL, nothing changed (the reference would call itb_del_ite
 *      twice, the second time on a slot that may hold another entry by then;
 *      itb_add_ite never writes such a flag, :364-372).
 *  10. hit -> 0, nr = entry, the record
 *        [u64 uuid][104 bytes from &ite.g as they were before this unlink][24 zero bytes]
 *      (the unlink branch has no __data_column_hook), and ite_unlink on flag,
 *      nlink (u16) and mode with `async_unlink`, one int for the call:
 *        A. flag & (NORMAL | SYM): nlink-- in u16 (0 wraps to 65535), again
 *           when mode & 0040000.  nlink == 0: state ITE_UNLINKED with
 *           async_unlink (POM_UL_MARKED), else itb_del_ite (POM_UL_DELETED).
 *           nlink != 0: state ITE_SHADOW (POM_UL_SHADOWED).
 *        B. else flag & LS: nlink = 0, itb_del_ite (POM_UL_DELETED).
 *        C. else flag & KV: itb_del_ite (POM_UL_DELETED).
 *        else POM_UL_NONE.
 *      POM_UL_DELTA is or-ed in when flag & SDT and either flag & KV or the
 *      nlink left in the ITE is 0.
 * itb_del_ite(offset: the slot that hit, pos: the home slot): a UNIQUE home
 * slot that is the target is unlinked; else the chain is walked from pos.  A
 * target behind the head is cut out (the tail: its predecessor becomes UNIQUE;
 * a middle one: its predecessor's conflict skips it).  A target that is the
 * head swaps entries with the next slot, and that slot is deleted instead.
 * __ite_unlink is pom_sweep.h's.  The deleted ITE's bytes stay behind, with
 * the nlink that A or B wrote.
 */

/* The unlinks of nreq requests over nitb decoded payloads in device memory;
 * enqueue only.  It runs pom_itb_check_dev first into `scratch` (with hdr,
 * without POM_CK_ITBID).  Payload b is payload_len[b] bytes at payload +
 * payload_off[b] and is modified in place: only its 128 bitmap bytes, its 8192
 * index bytes and bytes 16-19 and 38-39 of ITEs that a request hit may change.
 * ITB b's requests are req[req_first[b] ... req_first[b + 1]) in application
 * order; req_first has nitb + 1 non-decreasing u32 entries, req_first[0] == 0
 * and req_first[nitb] == nreq (a request outside every group is not answered).
 * `payload` is 16-byte aligned; hdr is required (8-byte aligned); req and out
 * are 8-byte aligned; err, nr, depth, what (nreq entries each), req_first and
 * result are 4-byte aligned; names is the requests' name blob of names_len
 * bytes at any alignment (NULL when names_len is 0).  Request r's record goes
 * to out + 136 * r, every record written in full.  scratch:
 * pom_itb_unlink_scratch(nitb) bytes, 8-byte aligned, no initial contents
 * required.  status may be NULL.  No two ITBs of a call may share payload
 * bytes.  Every pointer is device memory.  Returns 0, -EINVAL for a NULL hdr,
 * a payload that is not 16-byte aligned, or req, out or scratch not 8-byte
 * aligned (nothing is queued then), or -1 when a launch failed. */
int pom_itb_unlink_dev(uint8_t *payload, const uint64_t *payload_off,
                       const uint32_t *payload_len, const int32_t *status,
                       const uint8_t *adepth, const struct pom_check_hdr *hdr, uint32_t nitb,
                       int async_unlink, const struct pom_lookup_req *req, const uint32_t *req_first,
                       uint32_t nreq, const uint8_t *names, uint32_t names_len,
                       int32_t *err, uint32_t *nr, uint32_t *depth, uint32_t *what, uint8_t *out,
                       struct pom_unlink_result *result, void *scratch, void *stream);
size_t pom_itb_unlink_scratch(uint32_t nitb);

/* The ITB's header after unlinks that changed something (r->err == 0 and
 * r->changed > 0), as itb_lzo_compress leaves it in the stored record; plain C
 * on the host.  old_hdr: the 264-byte struct itbh before.  z: the size of the
 * payload's LZO1X-1 stream (POM_SPLIT_NO_STREAM: there is none).  The output
 * is a copy with entries, max_offset, pseudo_conflicts and itu from r, and
 * len, zlen and compress_algo by the not-smaller rule pom_itb_sweep_header
 * uses.  It is valid when r->removed == 0 too: with async_unlink only ITE
 * bytes changed, and the stream is still a new one.  Every other byte is the
 * old header's, `state` included.  out may be old_hdr.  Returns 1 when the
 * record is stored compressed and 0 when not, or -EINVAL for r->err != 0,
 * r->changed == 0 or a length below 264 (nothing is written then). */
int pom_itb_unlink_header(const uint8_t *old_hdr, const struct pom_unlink_result *r, uint32_t z, uint8_t *out);

/* The unlinks of nreq requests over n ITB records in host memory: rec[b] is a
 * record as stored, rec_len[b] bytes readable; records are not modified.
 * Selection, the stable grouping of the requests by ITB, the header checks,
 * the host-side -ESPLIT for itbid_check and -ESPLIT instead of -ENOENT for a
 * miss on an ITB_JUST_SPLIT record are pom_lookup_batch's.  An ITB that no
 * request reaches is neither uploaded nor decoded, and reads out_len 0, a
 * zeroed result and itb_err 0 (-EINVAL when its header is refused).  On the
 * GPU each chunk is decoded, checked, unlinked and encoded where it lies: up
 * go the compressed payloads, 32 bytes of header facts, the requests and their
 * names; back come four words and 136 bytes a request (err, nr, depth, what,
 * rec_out + 136 * r), 32 bytes an ITB and the one stored payload of each
 * changed ITB.  itb_err[b] is result[b].err, else LZO_E_OUTPUT_OVERRUN when
 * the record does not fit.  With itb_err[b] == 0 and result[b].changed > 0,
 * out[b] holds the record as itb_lzo_compress would store it and out_len[b]
 * its length; else out_len[b] is 0 and out[b] is untouched.  out_cap[b] bounds
 * out[b]; a capacity equal to the input's uncompressed record length always
 * suffices.  The requests' results stand whether or not the record fits.
 * len_ok is pom_itb_sweep_batch's (may be NULL).  Returns 0,
 * LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path is unusable (always,
 * without a GPU: nothing is written then); after a failed chunk every ITB that
 * was not delivered reads LZO_E_ERROR with a zeroed result, a zero length and
 * an untouched buffer, and its requests LZO_E_ERROR with a zero record. */
int pom_itb_unlink_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int itbid_check,
                         int async_unlink, const struct pom_lookup_req *req, size_t nreq,
                         const uint8_t *names, size_t names_len, uint8_t *rec_out,
                         int *err, uint32_t *nr, uint32_t *depth, uint32_t *what,
                         uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                         struct pom_unlink_result *result, int *itb_err, int *len_ok);

#ifdef __cplusplus
}
#endif

#endif /* POM_UNLINK_H */
