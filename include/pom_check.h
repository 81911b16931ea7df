/*
 * pom_check.h -- the ITB check on the MI355X (liblzo_mi355x.so): decode ITBs,
 * verify that the three views of one ITB agree -- the ITE bitmap, the index
 * table's hash chains and the header's counters -- and return a 48-byte
 * report per ITB, so that no decoded payload byte has to leave the GPU.
 *
 * Each read-only walk trusts a different part of an ITB: the GC scan and the
 * listings the bitmap (mdsl/gc.c:968-993, mds/itb.c:2479-2600), the lookups
 * the index chains (itb_search, mds/itb.c:1769-1814), entries_ok the header's
 * h.entries.  Damage shows only where a walk happens to tread.  The
 * reference's own tool, test/mds/itb_analyzer.c with itb_dump
 * (mds/itb.c:2622-2668), prints a table and does not read LZO records.  The
 * invariants checked here are the ones __itb_get_free_index, __itb_add_index,
 * itb_add_ite, __itb_add_ite_blob, __ite_unlink and itb_del_ite maintain
 * (mds/itb.c:215-322, :330-532, :567-671): a table the reference built
 * reports nothing.
 *
 *   pom_itb_check_dev    <- the check over decoded payloads in HBM
 *   pom_itb_check_batch  <- the same over stored records, decoded on the GPU
 *
 * Repair stays with the caller, and so does h.conflicts, which the reference
 * never maintains.  No ITE content beyond `hash` is examined.
 */
#ifndef POM_CHECK_H
#define POM_CHECK_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_lookup.h"     /* the ITB, index and ITE layout, POM_GC_E_TRUNCATED */

#ifdef __cplusplus
extern "C" {
#endif

/* Layout (LP64, the reference's build flags).  struct itbh, include/xtable.h:43-102: */
#define POM_ITBH_MAX_OFFSET_OFF 8u          /* atomic_t max_offset: the highest ITE ever in use */
#define POM_ITBH_PSEUDO_CONFLICTS_OFF 16u   /* atomic_t pseudo_conflicts */
#define POM_ITBH_INF_OFF 250u               /* u16 inf: index next free */
#define POM_ITBH_ITU_OFF 252u               /* u16 itu: index total used, of the overflow half */
/* struct itb, include/xtable.h:77-102.  sizeof(struct itb) - sizeof(struct itbh)
 * is POM_ITB_ITE_OFF (11904): h.len of a record in memory is POM_ITB_SIZE +
 * 512 * (max_offset + 1). */
#define POM_ITB_SIZE 12168u                 /* sizeof(struct itb) */

#define POM_CK_ITBID 0x1u                   /* flags: turns on kind 15; any other bit is -EINVAL */

/* What the walk needs of struct itbh. */
struct pom_check_hdr {              /* 32 bytes */
    int32_t entries, max_offset, pseudo_conflicts;
    uint32_t ulen;                  /* uncompressed record length: h.zlen (LZO) or h.len (NONE) */
    uint16_t inf, itu;
    uint8_t depth, pad[3];
    uint64_t itbid;
};

struct pom_check_report {           /* 48 bytes per ITB */
    uint32_t findings;              /* bit k set iff kind k occurred */
    uint32_t live;                  /* set bitmap bits below d */
    uint16_t used_home, used_over, reached, longest;
    uint16_t count[16];             /* kinds 0 ... 15: how many slots / ITEs */
};

#define POM_CK_SLOT_MASK_WORDS 32u  /* u64 per ITB: one bit per index slot */
#define POM_CK_ITE_MASK_WORDS 16u   /* u64 per ITB: one bit per ITE */

/* The kinds.  The bit number in `findings` is also the index into count[] for
 * kinds 0 ... 15. */
#define POM_CK_S_OUTSIDE 0
#define POM_CK_S_FLAG 1
#define POM_CK_S_LINK_RANGE 2
#define POM_CK_S_LINK_HOME 3
#define POM_CK_S_LINK_FREE 4
#define POM_CK_S_ENTRY_RANGE 5
#define POM_CK_S_ENTRY_DEAD 6
#define POM_CK_S_SHARED 7
#define POM_CK_S_LEAKED 8
#define POM_CK_S_ISLAND 9
#define POM_CK_S_LOOP 10
#define POM_CK_S_MISFILED 11
#define POM_CK_E_STRAY 12
#define POM_CK_E_DUP 13
#define POM_CK_E_ORPHAN 14
#define POM_CK_E_MISPLACED 15
#define POM_CK_H_ENTRIES 16
#define POM_CK_H_ITU 17
#define POM_CK_H_PSEUDO 18
#define POM_CK_H_MAXOFF 19
#define POM_CK_H_LEN 20
#define POM_CK_H_INF 21
#define POM_CK_KINDS 22

/* Error rules for payload p of n bytes and its adepth; the first that applies
 * decides.  Any err != 0 gives a zeroed report and zeroed masks, except `live`
 * where stated.
 *   1. status[b] != 0              -> that code
 *   2. adepth 0 or above 10        -> -EINVAL
 *   3. n < 11904 (the index table is not all there) -> POM_GC_E_TRUNCATED
 *   4. live = set bitmap bits below d = 1 << adepth.  The highest live ITE ends
 *      past n (11904 + 512 * (nr + 1) > n) -> POM_GC_E_TRUNCATED, `live` kept
 *   5. otherwise err = 0 and the report is filled.
 * Findings are not errors.  No byte at or past n is loaded; of the ITE area
 * only the `hash` word of live ITEs below d is loaded; p may sit at any byte
 * alignment.
 *
 * Vocabulary.  Slots are the 2048 struct itb_index words.  The three slot
 * ranges: the home half [0, d), the overflow half [d, 2d), outside [2d, 2048).
 * A slot is USED when its flag is not FREE.  A used slot LINKS when its flag
 * is CONFLICT or OVERFLOW; its target is `conflict`.  A link is GOOD when
 * d <= conflict < 2d and the target is used.  The `entry` of a FREE slot and
 * the `conflict` of a UNIQUE slot are stale bytes and are never examined.
 * indeg(t): the number of used slots below 2d with a good link to t.
 * REACHED: the least set that contains the used home slots and is closed
 * under good links.  refs(nr): the number of used slots below 2d whose
 * entry == nr.
 *
 *    k  name           holds for
 *    0  S_OUTSIDE      a used slot at or above 2d (nothing else is evaluated for it)
 *    1  S_FLAG         a used slot below 2d with flag OVERFLOW (__itb_add_index never writes it)
 *    2  S_LINK_RANGE   a linking slot below 2d with conflict >= 2d
 *    3  S_LINK_HOME    a linking slot below 2d with conflict < d
 *    4  S_LINK_FREE    a linking slot below 2d with d <= conflict < 2d and the target FREE
 *    5  S_ENTRY_RANGE  a used slot below 2d with entry >= d
 *    6  S_ENTRY_DEAD   a used slot below 2d with entry < d and bitmap bit clear
 *    7  S_SHARED       a used overflow slot with indeg >= 2
 *    8  S_LEAKED       a used overflow slot with indeg == 0
 *    9  S_ISLAND       a used overflow slot with indeg >= 1, not reached
 *   10  S_LOOP         a used home slot from which the good links come back to a slot
 *                      already on the path
 *   11  S_MISFILED     a used slot s with entry < d and a live entry, reached from a used
 *                      home slot h (h == s included) with (ite[entry].hash & (d - 1)) != h
 *   12  E_STRAY        a set bitmap bit at or above d (within the 1024 bits)
 *   13  E_DUP          an ITE below d with refs >= 2, live or not
 *   14  E_ORPHAN       a live ITE below d with refs == 0
 *   15  E_MISPLACED    with POM_CK_ITBID and hdr: a live ITE below d whose
 *                      (hash >> 10) & ((1 << depth) - 1) differs from itbid, in u64, with
 *                      every bit kept for depth >= 64
 *   16  H_ENTRIES      entries != live
 *   17  H_ITU          itu != used_over
 *   18  H_PSEUDO       pseudo_conflicts != used_over
 *   19  H_MAXOFF       live > 0 and max_offset is below the highest live bit (signed compare)
 *   20  H_LEN          live > 0 and ulen != 12168 + 512 * (max_offset + 1) (computed in i64)
 *   21  H_INF          inf > d
 * Kinds 16 ... 21 are evaluated only with hdr non-NULL; they have no count.
 *
 * used_home and used_over count the used slots of the two halves, `reached`
 * the reached slots.  `longest` is the most slots on a path from a used home
 * slot that is not S_LOOP; a path ends at a slot that does not link or whose
 * link is not good; 0 with no such path.  slot_mask bit s (bit s % 64 of word
 * s / 64) is set iff slot s has some kind 0 ... 11, ite_mask bit nr iff ITE nr
 * has some kind 12 ... 15.  Every definition is a property of the table, not
 * of a walk order.
 */

/* The check over nitb decoded payloads in device memory; enqueue only, like
 * pom_gc_scan_dev.  Payload b is payload_len[b] bytes at payload +
 * payload_off[b], at any byte alignment; adepth[b] is its header's adepth.
 * status and hdr may be NULL; hdr is 8-byte aligned, report 4-byte aligned.
 * slot_mask (32 u64 per ITB) and ite_mask (16 u64 per ITB) may each be NULL.
 * Nothing outside report, the masks and err is written.  Every pointer is
 * device memory.  Returns 0, -EINVAL for a flags bit other than POM_CK_ITBID,
 * or -1 when the launch failed. */
int pom_itb_check_dev(const uint8_t *payload, const uint64_t *payload_off,
                      const uint32_t *payload_len, const int32_t *status,
                      const uint8_t *adepth, const struct pom_check_hdr *hdr,
                      uint32_t nitb, uint32_t flags,
                      struct pom_check_report *report, uint64_t *slot_mask, uint64_t *ite_mask,
                      int32_t *err, void *stream);

/* The same for n ITB records in host memory: rec[b] is a record as stored,
 * [struct itbh][payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes readable;
 * records are not modified.  The header checks (a record that fails them gets
 * err[b] = -EINVAL and a zeroed report), the decode (safe semantics, capacity
 * h.zlen - 264; a decoder code becomes err[b]), len_ok and the treatment of
 * COMPR_NONE records are pom_gc_scan_batch's, but a record with h.entries == 0
 * is sent to the GPU like any other: its bitmap and index must be empty too.
 * hdr is filled from each record's header, so kinds 16 ... 21 are evaluated.
 * slot_mask, ite_mask and len_ok may be NULL.  Only the compressed payloads
 * and 32 bytes of header facts per ITB go to the GPU; only err, the 48-byte
 * reports and, when asked for, 384 bytes of masks per ITB come back.  Returns
 * 0, -EINVAL (a flags bit other than POM_CK_ITBID), LZO_E_OUT_OF_MEMORY, or
 * LZO_E_ERROR when the GPU path is unusable (always, without a GPU); then
 * every ITB that was not delivered reads LZO_E_ERROR with a zeroed report. */
int pom_itb_check_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, uint32_t flags,
                        struct pom_check_report *report, uint64_t *slot_mask, uint64_t *ite_mask,
                        int *err, int *len_ok);

#ifdef __cplusplus
}
#endif

#endif /* POM_CHECK_H */
