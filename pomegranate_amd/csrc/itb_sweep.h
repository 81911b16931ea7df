// itb_sweep.h -- the ITB sweep's rules (include/pom_sweep.h), stated once and
// built on itb_split.h's index words and itb_check.h's check.  Two statements
// of async_unlink_ite (mds/itb.c:2690-2800) over an index table, an ITE bitmap
// and the header's counters held in plain arrays (struct itb_sweep_state: in
// LDS in the kernel of itb_sweep.hip, on the stack of itb_sweep_one on the
// CPU, where tests/native/itb_sweep_host.cc runs both):
//   itb_sweep_serial    the reference's loop as it stands
//   the pieces the kernel uses, a chain at a time: itb_sweep_chain_dc (the dry
//   count), itb_sweep_chain (the chain's index edits and its deletes in
//   __ite_unlink order) and itb_sweep_fold (the counters from the ordered
//   deletes).  Chains of different home slots are disjoint in a table the
//   check passes, so their edits are independent; what depends on the loop's
//   order -- max_offset and the budget's stop -- follows from the per-chain
//   counts' prefix sums and the ordered list.
// Of each live ITE only one bit is kept: whether its state is ITE_UNLINKED.
// This header is plain C++17 outside hipcc.
//
// Every walk here is bounded, whatever the table holds: a chain by
// itb_sweep_budget(d) steps, the serial loop by as many in all, and every slot
// or ITE number is range-checked before it is an index.  A bound that is hit
// is POM_SPLIT_E_DAMAGED; after a passing check none can be.
#ifndef POM_ITB_SWEEP_H
#define POM_ITB_SWEEP_H

#include <stddef.h>
#include <stdint.h>

#include "itb_split.h"
#include "pom_sweep.h"

static_assert(sizeof(pom_sweep_result) == 32, "the ABI's result");
static_assert(POM_ITE_FLAG_OFF % 4 == 0, "the flag word is an aligned dword of a 16-byte aligned payload");

constexpr uint32_t kItbSweepBad = 0xFFFFFFFFu;          // a count: the walk met what a passing check rules out
constexpr uint32_t kItbSweepOver = 1u << 15;            // list[]: the freed slot lies in the overflow half; below it the ITE
constexpr uint32_t kItbSweepRemShift = 16;              // a chain's two counts in one word: dc | removed << 16

struct itb_sweep_counts {
    int32_t entries, max_offset, pseudo;
    uint32_t itu;                                       // u16 in struct itbh: wraps as one
};

struct itb_sweep_state {
    uint32_t idx[kItbCheckSlots];
    uint64_t bm[POM_CK_ITE_MASK_WORDS];                 // the ITE bitmap
    uint64_t ub[POM_CK_ITE_MASK_WORDS];                 // per ITE: live and ITE_UNLINKED
    uint16_t list[kItbCheckItes];                       // the deleted ITEs in loop order, | kItbSweepOver
    itb_sweep_counts h;
    uint32_t removed, dc, visited, steps;
    int32_t err;
};

ITB_SCAN_FN uint32_t itb_sweep_budget(uint32_t d)
{
    return 4u * d;
}

// (e->flag & ITE_STATE_MASK) == ITE_UNLINKED
ITB_SCAN_FN bool itb_sweep_marked(uint32_t flag)
{
    return (flag & POM_ITE_STATE_MASK) == POM_ITE_UNLINKED;
}

ITB_SCAN_FN bool itb_sweep_bit(const uint64_t* mask, uint32_t nr)
{
    return (mask[nr >> 6] >> (nr & 63u)) & 1u;
}

// h.len of a table with these counters.
ITB_SCAN_FN uint32_t itb_sweep_len(const itb_sweep_counts& h)
{
    if (h.entries == 0)
        return POM_ITB_SIZE;
    return (uint32_t)((int64_t)POM_ITB_SIZE + (int64_t)POM_ITE_SIZE * ((int64_t)h.max_offset + 1));
}

// What a passing check rules out of a slot on a chain: a free or OVERFLOW
// slot, an entry past the table, a link that leaves the overflow half.
ITB_SCAN_FN bool itb_sweep_slot_ok(uint32_t w, uint32_t d)
{
    const uint32_t flag = itb_split_flag(w), conflict = itb_split_conflict(w);
    if (flag != POM_IDX_UNIQUE && flag != POM_IDX_CONFLICT)
        return false;
    if (itb_split_entry(w) >= d)
        return false;
    return flag == POM_IDX_UNIQUE || (conflict >= d && conflict < 2u * d);
}

// ---------------------------------------------------------------------------
// __ite_unlink's counters (mds/itb.c:567-592) for the delete of ITE `entry`
// from a slot of the overflow half (over) or the home half.
// ---------------------------------------------------------------------------
ITB_SCAN_FN void itb_sweep_unlinked(itb_sweep_counts& h, uint32_t entry, bool over)
{
    if (over) {
        h.pseudo--;
        h.itu = (h.itu - 1u) & 0xFFFFu;
    }
    if (h.max_offset == (int32_t)entry)
        h.max_offset--;
    if (--h.entries == 0)
        h.max_offset = 0;
}

// ---------------------------------------------------------------------------
// The reference's loop as it stands, over T.idx / T.bm / T.h with T.ub as
// (e->flag & ITE_STATE_MASK) == ITE_UNLINKED.  Returns 0 or
// POM_SPLIT_E_DAMAGED; T.removed, T.dc, T.visited and T.steps (one per slot
// examined, the retry after a swap included) are filled.  On an error the
// table is left part swept: the caller works on a copy.
// ---------------------------------------------------------------------------
ITB_SCAN_FN bool itb_sweep_serial_unlink(itb_sweep_state& T, uint32_t d, uint32_t offset)
{
    const uint32_t w = T.idx[offset], entry = itb_split_entry(w);
    if (entry >= d)
        return false;
    T.idx[offset] = itb_split_with_flag(w, POM_IDX_FREE);
    itb_sweep_unlinked(T.h, entry, offset >= d);
    T.bm[entry >> 6] &= ~(1ull << (entry & 63u));
    T.removed++;
    return true;
}

ITB_SCAN_FN int32_t itb_sweep_serial(itb_sweep_state& T, uint32_t d, uint32_t budget)
{
    const uint32_t total = d;
    uint32_t offset = 0;
    T.removed = T.dc = T.steps = 0;
    T.visited = d;
    while (offset < total) {
        uint32_t w = T.idx[offset];
        if (itb_split_flag(w) == POM_IDX_FREE) {
            offset++;
            continue;
        }
        if (++T.steps > itb_sweep_budget(d) || !itb_sweep_slot_ok(w, d))
            return POM_SPLIT_E_DAMAGED;
        if (itb_split_flag(w) == POM_IDX_UNIQUE) {
            if (itb_sweep_bit(T.ub, itb_split_entry(w))) {
                if (!itb_sweep_serial_unlink(T, d, offset))
                    return POM_SPLIT_E_DAMAGED;
                T.dc++;
            }
        } else {
            const uint32_t saved = offset;
            uint32_t prev = offset;
            bool quit = false, needswap = false, first = true;
            do {
                for (;;) {                              // (retry: the slot again after the swap)
                    if (!first && ++T.steps > itb_sweep_budget(d))
                        return POM_SPLIT_E_DAMAGED;
                    first = false;
                    w = T.idx[offset];
                    if (!itb_sweep_slot_ok(w, d))       // (the reference breaks on FREE: no chain of a passing table has one)
                        return POM_SPLIT_E_DAMAGED;
                    if (itb_sweep_bit(T.ub, itb_split_entry(w))) {
                        if (offset == saved) {
                            needswap = true;
                            prev = offset;
                        } else if (itb_split_flag(w) == POM_IDX_UNIQUE) {
                            T.idx[prev] = itb_split_with_flag(T.idx[prev], POM_IDX_UNIQUE);
                            if (!itb_sweep_serial_unlink(T, d, offset))
                                return POM_SPLIT_E_DAMAGED;
                            quit = true;
                        } else {
                            T.idx[prev] = itb_split_with_conflict(T.idx[prev], itb_split_conflict(w));
                            if (!itb_sweep_serial_unlink(T, d, offset))
                                return POM_SPLIT_E_DAMAGED;
                        }
                        T.dc++;
                    } else {
                        if (needswap) {
                            const uint32_t s = T.idx[saved];
                            T.idx[offset] = itb_split_with_entry(w, itb_split_entry(s));
                            T.idx[saved] = itb_split_with_entry(s, itb_split_entry(w));
                            needswap = false;
                            continue;
                        }
                        if (itb_split_flag(w) == POM_IDX_UNIQUE)
                            quit = true;
                        prev = offset;
                    }
                    break;
                }
                offset = itb_split_conflict(w);
            } while (offset < 2u * total && !quit);
            if (needswap) {
                if (itb_split_flag(T.idx[saved]) != POM_IDX_UNIQUE || !itb_sweep_serial_unlink(T, d, saved))
                    return POM_SPLIT_E_DAMAGED;
            }
            offset = saved;
        }
        offset++;
        if (T.dc >= budget) {
            T.visited = offset;
            break;
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// The pieces.  Home slot j's chain, dry: its dc (the marked members, plus one
// when the head is marked and a live member follows) with its marked members
// above kItbSweepRemShift; 0 for a FREE home slot; kItbSweepBad for a chain a
// passing check rules out.
// ---------------------------------------------------------------------------
ITB_SCAN_FN uint32_t itb_sweep_chain_dc(const uint32_t* idx, const uint64_t* ub, uint32_t d, uint32_t j)
{
    uint32_t w = idx[j];
    if (itb_split_flag(w) == POM_IDX_FREE)
        return 0;
    uint32_t marked = 0, offset = j;
    bool head = false, live_behind = false;
    for (uint32_t steps = itb_sweep_budget(d); ; steps--) {
        if (steps == 0 || !itb_sweep_slot_ok(w, d))
            return kItbSweepBad;
        const bool m = itb_sweep_bit(ub, itb_split_entry(w));
        marked += m;
        if (offset == j)
            head = m;
        else if (!m)
            live_behind = true;
        if (itb_split_flag(w) == POM_IDX_UNIQUE)
            break;
        offset = itb_split_conflict(w);
        w = idx[offset];
    }
    if (marked > kItbCheckItes)
        return kItbSweepBad;
    return (marked + (head && live_behind ? 1u : 0u)) | marked << kItbSweepRemShift;
}

// Home slot j's chain, swept: the index edits of the reference's loop, and the
// chain's deletes in __ite_unlink order as list[at], list[at + 1], ... (the ITE
// number, | kItbSweepOver when the freed slot lies in the overflow half).
// Returns what itb_sweep_chain_dc returns.  The bitmap and the counters are
// the caller's: itb_sweep_fold takes them from the list.
ITB_SCAN_FN uint32_t itb_sweep_chain(uint32_t* idx, const uint64_t* ub, uint32_t d, uint32_t j, uint16_t* list,
                                     uint32_t at)
{
    uint32_t w = idx[j];
    if (itb_split_flag(w) == POM_IDX_FREE)
        return 0;
    uint32_t dc = 0, marked = 0, steps = itb_sweep_budget(d);
    // __ite_unlink's part in the index, and the list
    const auto unlink = [&](uint32_t offset) {
        const uint32_t u = idx[offset];
        if (at + marked >= kItbCheckItes)
            return false;
        idx[offset] = itb_split_with_flag(u, POM_IDX_FREE);
        list[at + marked++] = (uint16_t)(itb_split_entry(u) | (offset >= d ? kItbSweepOver : 0u));
        return true;
    };
    if (!itb_sweep_slot_ok(w, d))
        return kItbSweepBad;
    if (itb_split_flag(w) == POM_IDX_UNIQUE) {
        if (itb_sweep_bit(ub, itb_split_entry(w))) {
            if (!unlink(j))
                return kItbSweepBad;
            dc++;
        }
        return dc | marked << kItbSweepRemShift;
    }
    uint32_t offset = j, prev = j;
    bool quit = false, needswap = false;
    do {
        for (;;) {                                      // (retry: the slot again after the swap)
            if (steps-- == 0)
                return kItbSweepBad;
            w = idx[offset];
            if (!itb_sweep_slot_ok(w, d))
                return kItbSweepBad;
            if (itb_sweep_bit(ub, itb_split_entry(w))) {
                if (offset == j) {
                    needswap = true;
                    prev = offset;
                } else {
                    if (itb_split_flag(w) == POM_IDX_UNIQUE) {
                        idx[prev] = itb_split_with_flag(idx[prev], POM_IDX_UNIQUE);
                        quit = true;
                    } else {
                        idx[prev] = itb_split_with_conflict(idx[prev], itb_split_conflict(w));
                    }
                    if (!unlink(offset))
                        return kItbSweepBad;
                }
                dc++;
            } else {
                if (needswap) {
                    const uint32_t s = idx[j];
                    idx[offset] = itb_split_with_entry(w, itb_split_entry(s));
                    idx[j] = itb_split_with_entry(s, itb_split_entry(w));
                    needswap = false;
                    continue;
                }
                if (itb_split_flag(w) == POM_IDX_UNIQUE)
                    quit = true;
                prev = offset;
            }
            break;
        }
        offset = itb_split_conflict(w);
    } while (offset < 2u * d && !quit);
    if (needswap) {
        if (itb_split_flag(idx[j]) != POM_IDX_UNIQUE || !unlink(j))
            return kItbSweepBad;
    }
    return dc | marked << kItbSweepRemShift;
}

// The counters after the deletes list[0 ... n) in loop order: __ite_unlink's
// fold over them (max_offset-- only when it equals the deleted ITE, 0 once
// entries reaches 0).
ITB_SCAN_FN void itb_sweep_fold(itb_sweep_counts& h, const uint16_t* list, uint32_t n)
{
    for (uint32_t k = 0; k < n; k++)
        itb_sweep_unlinked(h, list[k] & (kItbSweepOver - 1u), (list[k] & kItbSweepOver) != 0);
}

// Rule 2.
ITB_SCAN_FN int32_t itb_sweep_precheck(uint64_t payload_off)
{
    return (payload_off & 15u) ? kItbScanEinval : 0;
}

// Dword i (0 ... 7) of the result of a sweep that removed something: the
// kernel stores one a lane.
static_assert(offsetof(pom_sweep_result, removed) == 4 && offsetof(pom_sweep_result, dc) == 8 &&
              offsetof(pom_sweep_result, len) == 12 && offsetof(pom_sweep_result, entries) == 16 &&
              offsetof(pom_sweep_result, pseudo_conflicts) == 24 && offsetof(pom_sweep_result, itu) == 28 &&
              offsetof(pom_sweep_result, visited) == 30, "the result as eight dwords");
ITB_SCAN_FN uint32_t itb_sweep_result_word(const itb_sweep_state& T, uint32_t i)
{
    switch (i) {
    case 0: return 0u;
    case 1: return T.removed;
    case 2: return T.dc;
    case 3: return itb_sweep_len(T.h);
    case 4: return (uint32_t)T.h.entries;
    case 5: return (uint32_t)T.h.max_offset;
    case 6: return (uint32_t)T.h.pseudo;
    default: return (T.h.itu & 0xFFFFu) | (T.visited & 0xFFFFu) << 16;
    }
}

ITB_SCAN_FN void itb_sweep_counts_of(itb_sweep_state& T, const pom_check_hdr& h)
{
    T.h = itb_sweep_counts{h.entries, h.max_offset, h.pseudo_conflicts, h.itu};
    T.removed = T.dc = T.visited = T.steps = 0;
    T.err = 0;
}

#ifndef __HIPCC__
#include <string.h>

// ---------------------------------------------------------------------------
// The whole sweep of one ITB on the CPU (the caller has dealt with status): the
// check, the rules, the sweep -- the serial loop, or (parts) the pieces in the
// kernel's data flow: every chain's dry count, the prefix sums and the
// budget's stop slot, the chains' edits (here from the last chain to the
// first: their order is free), the fold.  p is modified in place (bitmap and
// index only).  steps (may be NULL): the serial loop's.  Returns result->err.
// ---------------------------------------------------------------------------
static inline int32_t itb_sweep_one(uint8_t* p, uint32_t n, uint32_t adepth, const pom_check_hdr& hdr, uint32_t budget,
                                    uint64_t payload_off, bool parts, pom_sweep_result* result, uint32_t* steps)
{
    *result = pom_sweep_result{};
    if (steps)
        *steps = 0;
    pom_check_report rep;
    int32_t err = itb_check_one(p, n, adepth, &hdr, 0, &rep, nullptr, nullptr);
    if (err == 0)
        err = itb_sweep_precheck(payload_off);
    if (err == 0 && (rep.findings & ~(1u << POM_CK_E_MISPLACED)))
        err = POM_SPLIT_E_DAMAGED;
    if (err != 0)
        return result->err = err;

    const uint32_t d = 1u << adepth;
    static thread_local itb_sweep_state T;
    memset(&T, 0, sizeof T);
    itb_sweep_counts_of(T, hdr);
    memcpy(T.idx, p + POM_ITB_INDEX_OFF, sizeof T.idx);
    memcpy(T.bm, p + POM_ITB_BITMAP_OFF, sizeof T.bm);
    for (uint32_t nr = 0; nr < d; nr++)
        if (itb_sweep_bit(T.bm, nr)) {
            uint32_t flag;
            memcpy(&flag, p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr + POM_ITE_FLAG_OFF, 4);
            if (itb_sweep_marked(flag))
                T.ub[nr >> 6] |= 1ull << (nr & 63u);
        }
    if (!parts) {
        err = itb_sweep_serial(T, d, budget);
        if (steps)
            *steps = T.steps;
    } else {
        static thread_local uint32_t count[kItbCheckItes], before[kItbCheckItes];
        uint32_t sum = 0, stop = d;
        for (uint32_t j = 0; j < d && err == 0; j++) {
            count[j] = itb_sweep_chain_dc(T.idx, T.ub, d, j);
            if (count[j] == kItbSweepBad)
                err = POM_SPLIT_E_DAMAGED;
            before[j] = sum;
            sum += count[j];
            if (stop == d && itb_split_flag(T.idx[j]) != POM_IDX_FREE && (sum & 0xFFFFu) >= budget)
                stop = j;
        }
        if (err == 0) {
            const uint32_t last = stop < d ? stop : d - 1u;
            const uint32_t upto = before[last] + count[last];
            T.visited = stop < d ? stop + 1u : d;
            T.dc = upto & 0xFFFFu;
            T.removed = upto >> kItbSweepRemShift;
            for (uint32_t j = last + 1u; j-- > 0 && err == 0 && T.removed != 0;)
                if (itb_sweep_chain(T.idx, T.ub, d, j, T.list, before[j] >> kItbSweepRemShift) != count[j])
                    err = POM_SPLIT_E_DAMAGED;
            if (err == 0 && T.removed != 0) {
                for (uint32_t k = 0; k < T.removed; k++) {
                    const uint32_t e = T.list[k] & (kItbSweepOver - 1u);
                    T.bm[e >> 6] &= ~(1ull << (e & 63u));
                }
                itb_sweep_fold(T.h, T.list, T.removed);
            }
        }
    }
    if (err != 0)
        return result->err = err;
    if (T.removed == 0)
        return 0;
    memcpy(p + POM_ITB_BITMAP_OFF, T.bm, sizeof T.bm);
    memcpy(p + POM_ITB_INDEX_OFF, T.idx, sizeof T.idx);
    for (uint32_t i = 0; i < sizeof *result / 4; i++) {
        const uint32_t w = itb_sweep_result_word(T, i);
        memcpy(reinterpret_cast<uint8_t*>(result) + 4u * i, &w, 4);
    }
    return 0;
}
#endif

#endif
