/*
 * pom_split.h -- the ITB split on the MI355X (liblzo_mi355x.so): move the
 * upper half of an ITB's entries into a new ITB on the GPU, so that a decoded
 * ITB that has to be split does not have to come back to host memory.
 *
 * The split (itb_split_local, mds/xtable.c:41-268) is the one whole-ITB
 * operation of the MDS that writes: it touches every live ITE, about half of
 * them move (512 bytes each), it is data-parallel over ITBs, and both results
 * go straight back to storage through the write-back codec.  The sequence
 * restated here is mds/xtable.c:95-146 with __itb_add_ite_blob
 * (mds/itb.c:501-532), __itb_add_index and __itb_get_free_index (:215-322),
 * itb_del_ite and __ite_unlink (:567-671) and get_free_itb (:1229-1304):
 *
 *   pom_itb_split_dev      <- the check, then the split, over decoded payloads
 *                             in HBM
 *   pom_itb_split_batch    <- the same over stored records: decoded, split and
 *                             both halves encoded on the GPU
 *   pom_itb_split_headers  <- both ITBs' struct itbh from the old one and the
 *                             result, on the host
 *
 * What stays with the caller: the locks, the COW checks and txg_add_itb; the
 * bitmap delta and the AU request; the water-mark test entries < 1 << adepth,
 * which is the caller's policy; and the retry with depth++ when nothing moved:
 * here moved == 0 is a result, and the caller asks again with a deeper
 * split_depth.
 */
#ifndef POM_SPLIT_H
#define POM_SPLIT_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_check.h"      /* struct pom_check_hdr, the ITB layout, POM_GC_E_TRUNCATED */

#ifdef __cplusplus
extern "C" {
#endif

/* Layout (LP64, the reference's build flags).  struct itbh, include/xtable.h:43-102: */
#define POM_ITBH_STATE_OFF 1u               /* u8 state */
#define POM_ITBH_CONFLICTS_OFF 12u          /* atomic_t conflicts: never maintained by the reference */
#define POM_ITBH_TWIN_OFF 208u              /* u64 twin */
#define POM_ITBH_SPLIT_RLINK_OFF 216u       /* u64 split_rlink */
#define POM_ITB_STATE_DIRTY 1u              /* ITB_STATE_DIRTY */

#define POM_SPLIT_DEPTH_MAX 50u             /* mds/xtable.c:168: the reference asserts at depth 50 */
/* A table the check has a finding for, or that the walk cannot get through
 * within its step budget; beside POM_GC_E_TRUNCATED and distinct from every
 * other code of the library. */
#define POM_SPLIT_E_DAMAGED (-4103)

struct pom_split_result {          /* 48 bytes per ITB */
    int32_t  err;                  /* 0, or the first rule that applies */
    uint32_t moved;
    uint32_t old_len, new_len;     /* uncompressed record lengths, 12168 + 512 * (max_offset + 1), or 12168
                                    * when empty; 0 when nothing is produced */
    int32_t  old_entries, new_entries, old_max_offset, new_max_offset, old_pseudo, new_pseudo;
    uint16_t old_inf, old_itu, new_inf, new_itu;
};

/* The split of ITB O -- decoded payload p (the bytes from &itb->lock), its
 * adepth, its header facts -- at split depth sd, with d = 1 << adepth.
 *
 * The new ITB N starts as get_free_itb leaves a table: 3584 zero bytes of lock
 * region, a zero bitmap, 2048 zero index words; entries, max_offset,
 * pseudo_conflicts, inf and itu 0, len 12168, O's adepth.  Then, one chain at
 * a time, for j in [0, d) -- the reference scans 1 << ITB_DEPTH home slots and
 * its adepth is always 10; for a smaller adepth only the home half is scanned,
 * the one deliberate departure, which changes nothing at adepth 10:
 *   1. the chain of home slot j is walked through `conflict`;
 *   2. at a slot whose ITE e has (e.hash >> 10) & (1 << (sd - 1)) set, in u64,
 *      __itb_add_ite_blob(N, e) adds it to N (the first zero bit nr, the 512
 *      bytes to N.ite[nr], __itb_add_index at e.hash & (d - 1), the overflow
 *      slot from __itb_get_free_index with its inf / itu bookkeeping,
 *      max_offset and len by the <= rule), and itb_del_ite(O, e, offset, j)
 *      deletes it from O (the head swap, __ite_unlink's max_offset-- only
 *      when it equals the entry, the entries == 0 reset);
 *   3. need_rescan is the reference's: set when the head moved, consumed at
 *      the next chain element, and it stays set across a `done` break.
 * The ITE numbers in N, the overflow slots N uses, the stale entry / conflict
 * bytes of freed slots in O and both headers' counters depend on that order;
 * every byte is determined, and the contract is byte equality with that
 * sequence.  O's ITE area and lock region are not touched: moved ITEs stay
 * behind as dead bytes, as in the reference, and O's record shrinks only as
 * far as max_offset does.  For a table the check passes the moved set is
 * exactly the live ITEs with the bit set, N's ITEs are numbered 0 ... moved -
 * 1, and neither record is longer than O's was.
 *
 * Error rules; the first that applies decides:
 *   1. the check's err (pom_check.h rules 1 ... 4)
 *   2. split depth outside 1 ... 50                  -> -EINVAL
 *   3. payload_off[b] or new_off[b] not a multiple of 16 -> -EINVAL; the split
 *      loads and stores nothing of that ITB
 *   4. any finding other than kind 15                -> POM_SPLIT_E_DAMAGED; a
 *      table the check refuses is never walked.  (The walk has a hard budget
 *      of 4 * d chain steps and answers the same when it runs out; a table
 *      the check passes needs at most live + moved + 1.)
 *   5. new_cap[b] < 11904 + 512 * moved              -> LZO_E_OUTPUT_OVERRUN,
 *      `moved` kept; nothing is written to new_payload and the payload is
 *      left as it was
 *   6. moved == 0: err 0, both lengths 0, nothing is written
 * With err != 0 nothing but result[b] is written, and its other fields are
 * zero, except `moved` under rule 5.
 */

/* The split of nitb decoded payloads in device memory; enqueue only, like
 * pom_itb_check_dev, which it runs first into `scratch` (with hdr, without
 * POM_CK_ITBID); it then splits what the check passes.  Payload b is
 * payload_len[b] bytes at payload + payload_off[b] and is modified in place:
 * only its 128 bitmap bytes and its 8192 index bytes may change.  `payload` and
 * `new_payload` are 16-byte aligned, so that the offsets' rule 3 makes every
 * 16-byte load and store legal.  status may be NULL; hdr is required (8-byte
 * aligned).  split_depth is a u8 per ITB, or NULL: hdr[b].depth + 1.  On
 * success new_payload + new_off[b] holds exactly new_len - 264 bytes (the
 * payload of N: lock region, bitmap, index, `moved` ITEs); no byte past that
 * is written, and new_cap[b] = payload_len[b] always suffices.  result is
 * 4-byte aligned.  scratch: pom_itb_split_scratch(nitb) bytes, 8-byte aligned,
 * no initial contents required.  No two ITBs of a call may share payload or
 * new_payload bytes.  Every pointer is device memory.  Returns 0, -EINVAL for
 * a NULL hdr, a payload or new_payload that is not 16-byte aligned or a scratch
 * that is not 8-byte aligned (nothing is queued then), or -1 when a launch
 * failed. */
int pom_itb_split_dev(uint8_t *payload, const uint64_t *payload_off,
                      const uint32_t *payload_len, const int32_t *status,
                      const uint8_t *adepth, const struct pom_check_hdr *hdr,
                      const uint8_t *split_depth, uint32_t nitb,
                      uint8_t *new_payload, const uint64_t *new_off, const uint32_t *new_cap,
                      struct pom_split_result *result, void *scratch, void *stream);
size_t pom_itb_split_scratch(uint32_t nitb);

/* Both ITBs' headers after a split that produced something (r->err == 0 and
 * r->moved > 0), as itb_lzo_compress (mds/itb.c:2904-2945) leaves them in the
 * stored records; plain C on the host.  old_hdr: O's 264-byte struct itbh
 * before the split.  old_z, new_z: the sizes of the two payloads' LZO1X-1
 * streams (POM_SPLIT_NO_STREAM: there is none).  A half whose stream is smaller
 * than its payload (z < len - 264) is stored compressed: compress_algo =
 * COMPR_LZO, zlen = the uncompressed record length, len = 264 + z; otherwise
 * uncompressed: COMPR_NONE, len = the uncompressed record length, zlen = 0.
 *   O's: a copy with depth = sd, entries, max_offset, pseudo_conflicts and itu
 *        from r, and len, zlen and compress_algo by that rule.
 *   N's: a copy of O's with flag = ITB_JUST_SPLIT, state = ITB_STATE_DIRTY,
 *        itbid |= 1 << (sd - 1), r's counters for N (inf too), conflicts = 0,
 *        twin = split_rlink = 0, and its own len, zlen and compress_algo.
 * Every other byte of both is O's (pointers and locks included: they mean
 * nothing in a stored record).  old_out and new_out may each be old_hdr.
 * Returns bit 0 set when O is stored compressed and bit 1 when N is, or
 * -EINVAL for sd outside 1 ... 50, r->err != 0, r->moved == 0 or a length
 * below 264 (nothing is written then). */
#define POM_SPLIT_NO_STREAM 0xFFFFFFFFu
int pom_itb_split_headers(const uint8_t *old_hdr, uint8_t sd, const struct pom_split_result *r,
                          uint32_t old_z, uint32_t new_z, uint8_t *old_out, uint8_t *new_out);

/* The split of n ITB records in host memory: rec[b] is a record as stored,
 * [struct itbh][payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes readable;
 * records are not modified.  Selection, header checks, decode, len_ok and the
 * treatment of COMPR_NONE records are pom_itb_check_batch's.  On the GPU each
 * chunk is decoded, checked, split (pom_itb_split_dev; split_depth: a u8 per
 * record, or NULL: h.depth + 1) and both halves are encoded where they lie;
 * only the compressed payloads, 32 bytes of header facts and the split depth
 * go up, only 48 bytes of result and the two stored payloads come back: no
 * decoded byte crosses unless a half does not compress.  result[b] is the
 * device's; err[b] is -EINVAL for a record the header checks refuse, else
 * result[b].err, else LZO_E_OUTPUT_OVERRUN when a half does not fit.  With
 * err[b] == 0 and result[b].moved > 0, old_out[b] and new_out[b] hold the two
 * records as itb_lzo_compress would store them, [header][LZO1X-1 stream] when
 * the stream is smaller than the payload, else [header][payload], and
 * old_len[b] and new_len[b] their lengths (h.len); otherwise both lengths are
 * 0 and neither buffer is written.  out_cap[b] bounds each of the two buffers:
 * if either record is longer, err[b] = LZO_E_OUTPUT_OVERRUN and neither is
 * written; a capacity equal to the input's uncompressed record length always
 * suffices.  Returns 0, LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path
 * is unusable (always, without a GPU: nothing is written then); after a failed
 * chunk every ITB that was not delivered reads LZO_E_ERROR with a zeroed
 * result, zero lengths and untouched buffers. */
int pom_itb_split_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                        const uint8_t *split_depth, uint8_t *const *old_out, uint8_t *const *new_out,
                        const size_t *out_cap, size_t *old_len, size_t *new_len,
                        struct pom_split_result *result, int *err, int *len_ok);

#ifdef __cplusplus
}
#endif

#endif /* POM_SPLIT_H */
