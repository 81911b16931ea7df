/*
 * pom_sweep.h -- the ITB sweep on the MI355X (liblzo_mi355x.so): delete the
 * ITEs an asynchronous unlink left marked, on the GPU, so that a decoded ITB
 * that has to be swept does not have to come back to host memory.
 *
 * With hmo.conf.async_unlink set, ite_unlink (mds/itb.c:676-695) does not
 * delete an entry whose nlink reached 0: it sets (e->flag & ITE_STATE_MASK) =
 * ITE_UNLINKED.  The unlink thread (async_unlink_local, :2806-2848) later walks
 * every home slot's chain of every listed ITB and removes the marked ITEs
 * (async_unlink_ite, :2690-2800, with __ite_unlink, :567-592).  Beside the
 * split it is the reference's only other writer that touches every chain of an
 * ITB; it reads one flag word per live ITE and rewrites only the bitmap, the
 * index table and five header counters:
 *
 *   pom_itb_sweep_dev     <- the check, then the sweep, over decoded payloads
 *                            in HBM
 *   pom_itb_sweep_batch   <- the same over stored records: decoded, swept and
 *                            encoded on the GPU
 *   pom_itb_sweep_header  <- the ITB's struct itbh from the old one and the
 *                            result, on the host
 *
 * What stays with the caller: the hmo.async_unlink list and the
 * ITB_STATE_COWED skip; the rlock; carrying dc from one ITB to the next -- the
 * caller hands each ITB of a wave its budget, a batch is parallel over ITBs
 * and cannot carry it; the profile counters (prof.itb.async_unlink += dc,
 * cbht.aentry -= removed); and dirtying: the reference does not dirty the ITB
 * here (its FIXME at :2701), so `state` is left as it is.
 */
#ifndef POM_SWEEP_H
#define POM_SWEEP_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_split.h"      /* POM_SPLIT_E_DAMAGED, the POM_ITBH_* offsets, struct pom_check_hdr */

#ifdef __cplusplus
extern "C" {
#endif

/* The state bits of an ITE's flag word (u32 at POM_ITE_FLAG_OFF) are
 * POM_ITE_STATE_MASK (pom_readdir.h: ITE_STATE_MASK, include/ite.h:89) and
 * the state that sweeps is POM_ITE_UNLINKED (pom_lookup.h: ITE_UNLINKED,
 * :85); both arrive through pom_split.h. */
#define POM_SWEEP_NO_BUDGET 0xFFFFFFFFu

struct pom_sweep_result {            /* 32 bytes per ITB */
    int32_t  err;                    /* 0, or the first rule that applies */
    uint32_t removed;                /* __ite_unlink calls */
    uint32_t dc;                     /* the reference's *dc increment: removed + head swaps */
    uint32_t len;                    /* uncompressed record length after the sweep; 0 when nothing is produced */
    int32_t  entries, max_offset, pseudo_conflicts;
    uint16_t itu;
    uint16_t visited;                /* home slots the loop got through: d, or j + 1 when the budget test broke
                                      * it after slot j */
};

/* The sweep of one ITB -- decoded payload p (the bytes from &itb->lock), its
 * adepth, its header facts -- with d = 1 << adepth.  An ITE is marked when
 * (flag & POM_ITE_STATE_MASK) == POM_ITE_UNLINKED, whatever its other 29 flag
 * bits hold.  For offset in [0, d):
 *   1. a FREE home slot is skipped, and the budget test with it;
 *   2. a UNIQUE home slot whose ITE is marked is unlinked (__ite_unlink), dc++;
 *   3. otherwise the chain is walked through `conflict`.  A marked member
 *      behind the head is cut out of the chain (the tail: its predecessor
 *      becomes UNIQUE; a middle one: its predecessor's conflict skips it) and
 *      unlinked, dc++.  A marked head sets needswap, dc++ -- and when a live
 *      member follows, the two slots swap their entries, the walk takes that
 *      slot again and unlinks it there, dc++ once more: the head is counted
 *      twice, so dc == removed + swaps.  When no live member follows, the head
 *      is unlinked last;
 *   4. dc >= budget ends the loop: the reference's test, after each used home
 *      slot, so with budget 0 the first used home slot is still swept.
 * __ite_unlink sets the slot FREE (its entry and conflict bytes stay), takes
 * pseudo_conflicts and itu down for a slot of the overflow half, max_offset
 * down by one only when it equals the deleted entry (so it may stay above the
 * highest live ITE: the check allows that), entries down, max_offset to 0 when
 * entries reaches 0, and clears the bitmap bit.  Every byte is determined,
 * and the contract is byte equality with that sequence.  The ITE area and the
 * lock region are not touched: deleted ITEs stay behind as dead bytes, as in
 * the reference, and the record shrinks only as far as max_offset does.
 *
 * Error rules; the first that applies decides:
 *   1. the check's err (pom_check.h rules 1 ... 4)
 *   2. payload_off[b] not a multiple of 16           -> -EINVAL; the sweep
 *      loads and stores nothing of that ITB
 *   3. any finding other than kind 15                -> POM_SPLIT_E_DAMAGED; a
 *      table the check refuses is never walked.  (The walk has a hard budget
 *      of 4 * d chain steps and answers the same when it runs out; a table
 *      the check passes needs at most live + swaps.)
 *   4. removed == 0: err 0, every other field 0, nothing is written
 * With err != 0 nothing but result[b] is written, and its other fields are
 * zero.
 */

/* The sweep of nitb decoded payloads in device memory; enqueue only, like
 * pom_itb_check_dev, which it runs first into `scratch` (with hdr, without
 * POM_CK_ITBID); it then sweeps what the check passes.  Payload b is
 * payload_len[b] bytes at payload + payload_off[b] and is modified in place:
 * only its 128 bitmap bytes and its 8192 index bytes may change.  `payload` is
 * 16-byte aligned, so that the offsets' rule 2 makes every 16-byte load and
 * store legal.  status may be NULL; hdr is required (8-byte aligned).  budget
 * is a u32 per ITB, or NULL: POM_SWEEP_NO_BUDGET for each.  result is 4-byte
 * aligned.  scratch: pom_itb_sweep_scratch(nitb) bytes, 8-byte aligned, no
 * initial contents required.  No two ITBs of a call may share payload bytes.
 * Every pointer is device memory.  Returns 0, -EINVAL for a NULL hdr, a
 * payload that is not 16-byte aligned or a scratch that is not 8-byte aligned
 * (nothing is queued then), or -1 when a launch failed. */
int pom_itb_sweep_dev(uint8_t *payload, const uint64_t *payload_off,
                      const uint32_t *payload_len, const int32_t *status,
                      const uint8_t *adepth, const struct pom_check_hdr *hdr,
                      const uint32_t *budget, uint32_t nitb,
                      struct pom_sweep_result *result, void *scratch, void *stream);
size_t pom_itb_sweep_scratch(uint32_t nitb);

/* The ITB's header after a sweep that removed something (r->err == 0 and
 * r->removed > 0), as itb_lzo_compress (mds/itb.c:2904-2945) leaves it in the
 * stored record; plain C on the host.  old_hdr: the 264-byte struct itbh
 * before the sweep.  z: the size of the swept payload's LZO1X-1 stream
 * (POM_SPLIT_NO_STREAM: there is none).  The output is a copy with entries,
 * max_offset, pseudo_conflicts and itu from r, and len, zlen and compress_algo
 * by pom_itb_split_headers' not-smaller rule (one function holds it for both).
 * Every other byte is the old header's, `state` included: dirtying is the
 * caller's policy.  out may be old_hdr.  Returns 1 when the record is stored
 * compressed and 0 when not, or -EINVAL for r->err != 0, r->removed == 0 or a
 * length below 264 (nothing is written then). */
int pom_itb_sweep_header(const uint8_t *old_hdr, const struct pom_sweep_result *r, uint32_t z, uint8_t *out);

/* The sweep of n ITB records in host memory: rec[b] is a record as stored,
 * [struct itbh][payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes readable;
 * records are not modified.  Selection, header checks, decode, len_ok and the
 * treatment of COMPR_NONE records are pom_itb_check_batch's.  On the GPU each
 * chunk is decoded, checked, swept (pom_itb_sweep_dev; budget: a u32 per
 * record, or NULL) and encoded where it lies; only the compressed payloads, 32
 * bytes of header facts and the budget go up, only 32 bytes of result and the
 * one stored payload come back: no decoded byte crosses unless the swept
 * payload does not compress.  result[b] is the device's; err[b] is -EINVAL for
 * a record the header checks refuse, else result[b].err, else
 * LZO_E_OUTPUT_OVERRUN when the record does not fit.  With err[b] == 0 and
 * result[b].removed > 0, out[b] holds the record as itb_lzo_compress would
 * store it, [header][LZO1X-1 stream] when the stream is smaller than the
 * payload, else [header][payload], and out_len[b] its length (h.len).  With
 * err[b] == 0 and removed == 0, out_len[b] is 0 and out[b] is untouched: the
 * stored record is still right.  out_cap[b] bounds out[b]: if the record is
 * longer, err[b] = LZO_E_OUTPUT_OVERRUN and nothing is written; a capacity
 * equal to the input's uncompressed record length always suffices.  Returns 0,
 * LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path is unusable (always,
 * without a GPU: nothing is written then); after a failed chunk every ITB that
 * was not delivered reads LZO_E_ERROR with a zeroed result, a zero length and
 * an untouched buffer. */
int pom_itb_sweep_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n,
                        const uint32_t *budget, uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                        struct pom_sweep_result *result, int *err, int *len_ok);

#ifdef __cplusplus
}
#endif

#endif /* POM_SWEEP_H */
