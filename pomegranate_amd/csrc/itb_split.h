// itb_split.h -- the ITB split's rules (include/pom_split.h), stated once and
// built on itb_find.h's slot layout and itb_check.h's check.  The loop of
// itb_split_local (mds/xtable.c:95-146) runs over both tables' index words,
// bitmaps and counters held in plain arrays (struct itb_split_state: in LDS in
// the kernel of itb_split.hip, on the stack of itb_split_one on the CPU, where
// tests/native/itb_split_host.cc runs it); no ITE byte is looked at while it
// runs: of each live ITE only its home slot and its move bit are kept, 16 bits.
// This header is plain C++17 outside hipcc.
//
// Every walk here is bounded, whatever the table holds: the loop by
// itb_split_budget(d) chain steps, a delete by 2d + 2 slots, a free-slot
// search by d, and every slot or ITE number is range-checked before it is an
// index.  A bound that is hit is POM_SPLIT_E_DAMAGED; after a passing check
// none can be.
#ifndef POM_ITB_SPLIT_H
#define POM_ITB_SPLIT_H

#include <stddef.h>
#include <stdint.h>

#include "itb_check.h"
#include "pom_split.h"

static_assert(sizeof(pom_split_result) == 48, "the ABI's result");
static_assert(POM_ITB_BITMAP_OFF % 16 == 0 && POM_ITB_INDEX_OFF % 16 == 0 && POM_ITB_ITE_OFF % 16 == 0 &&
              POM_ITE_SIZE % 16 == 0, "16-byte loads and stores at a 16-byte aligned payload");
static_assert(POM_ITB_BITMAP_OFF + POM_ITB_BITMAP_BYTES == POM_ITB_INDEX_OFF, "bitmap, then index");

constexpr int32_t kItbSplitOverrun = -5;                // LZO_E_OUTPUT_OVERRUN
constexpr uint32_t kItbSplitMove = 1u << 15;            // info[]: the ITE moves; below it its home slot
constexpr uint32_t kItbSplitHome = (1u << POM_ITB_ADEPTH_MAX) - 1u;
constexpr uint32_t kItbSplitEntryMask = (1u << POM_IDX_ENTRY_BITS) - 1u;
constexpr uint32_t kItbSplitFlagMask = 3u << POM_IDX_FLAG_SHIFT;

// One table's counters as the loop keeps them (h.len follows from them).
struct itb_split_side {
    int32_t entries, max_offset, pseudo;
    uint32_t inf, itu;                                  // u16 in struct itbh: itu wraps as one
};

struct itb_split_state {
    uint32_t oidx[kItbCheckSlots], nidx[kItbCheckSlots];
    uint64_t obm[POM_CK_ITE_MASK_WORDS], nbm[POM_CK_ITE_MASK_WORDS];
    uint16_t info[kItbCheckItes];                       // per ITE of O: home | kItbSplitMove; 0 for a dead one
    uint16_t from[kItbCheckItes];                       // per ITE of N: the ITE of O it is a copy of
    itb_split_side o, n;
    uint32_t moved, steps;
    int32_t err;
};

ITB_SCAN_FN uint32_t itb_split_budget(uint32_t d)
{
    return 4u * d;
}

// (e.hash >> ITB_DEPTH) & (1UL << (depth - 1)), in u64; sd is 1 ... 50.
ITB_SCAN_FN bool itb_split_moves(uint64_t hash, uint32_t sd)
{
    return ((hash >> POM_ITB_ADEPTH_MAX) >> (sd - 1u)) & 1u;
}

ITB_SCAN_FN uint16_t itb_split_info(uint64_t hash, uint32_t d, uint32_t sd)
{
    return (uint16_t)(((uint32_t)hash & (d - 1u)) | (itb_split_moves(hash, sd) ? kItbSplitMove : 0u));
}

// h.len of a table with these counters.
ITB_SCAN_FN uint32_t itb_split_len(const itb_split_side& s)
{
    if (s.entries == 0)
        return POM_ITB_SIZE;
    return (uint32_t)((int64_t)POM_ITB_SIZE + (int64_t)POM_ITE_SIZE * ((int64_t)s.max_offset + 1));
}

ITB_SCAN_FN uint32_t itb_split_flag(uint32_t w) { return w >> POM_IDX_FLAG_SHIFT; }
ITB_SCAN_FN uint32_t itb_split_entry(uint32_t w) { return w & kItbSplitEntryMask; }
ITB_SCAN_FN uint32_t itb_split_conflict(uint32_t w) { return (w >> POM_IDX_ENTRY_BITS) & kItbSplitEntryMask; }
ITB_SCAN_FN uint32_t itb_split_with_flag(uint32_t w, uint32_t f) { return (w & ~kItbSplitFlagMask) | f << POM_IDX_FLAG_SHIFT; }
ITB_SCAN_FN uint32_t itb_split_with_entry(uint32_t w, uint32_t e) { return (w & ~kItbSplitEntryMask) | e; }
ITB_SCAN_FN uint32_t itb_split_with_conflict(uint32_t w, uint32_t c)
{
    return (w & ~(kItbSplitEntryMask << POM_IDX_ENTRY_BITS)) | c << POM_IDX_ENTRY_BITS;
}

// ---------------------------------------------------------------------------
// N: __itb_get_free_index, __itb_add_index, __itb_add_ite_blob
// (mds/itb.c:215-322, :501-532).  false: the table is full (it cannot be: N
// takes at most the d ITEs O has).
// ---------------------------------------------------------------------------
ITB_SCAN_FN uint32_t itb_split_free_index(itb_split_state& T, uint32_t d)
{
    uint32_t nr = T.n.inf;
    if (nr >= d)
        nr = 0;
    for (uint32_t c = d; c; c--) {
        if (itb_split_flag(T.nidx[nr + d]) == POM_IDX_FREE) {
            T.n.inf = nr + 1u;
            T.n.itu = (T.n.itu + 1u) & 0xFFFFu;
            return nr + d;
        }
        if (++nr == d)
            nr = 0;
    }
    return 2u * d;
}

ITB_SCAN_FN bool itb_split_add(itb_split_state& T, uint32_t d, uint32_t old_nr)
{
    uint32_t nr = d;                                    // find_first_zero_bit(bitmap, d)
    for (uint32_t w = 0; 64u * w < d; w++)
        if (~T.nbm[w]) {
            nr = 64u * w + (uint32_t)__builtin_ctzll(~T.nbm[w]);
            break;
        }
    if (nr >= d)
        return false;
    T.nbm[nr >> 6] |= 1ull << (nr & 63u);
    T.from[nr] = (uint16_t)old_nr;
    const uint32_t offset = T.info[old_nr] & kItbSplitHome;
    const uint32_t w = T.nidx[offset];
    if (itb_split_flag(w) == POM_IDX_FREE) {
        T.nidx[offset] = itb_split_with_entry(itb_split_with_flag(w, POM_IDX_UNIQUE), nr);
    } else {
        // UNIQUE: the home slot links to a new tail; CONFLICT: the home slot's
        // word moves behind and the new ITE takes the head.  (OVERFLOW is never
        // written, so N never holds it.)
        const uint32_t f = itb_split_free_index(T, d);
        if (f >= 2u * d)
            return false;
        if (itb_split_flag(w) == POM_IDX_UNIQUE) {
            T.nidx[offset] = itb_split_with_conflict(itb_split_with_flag(w, POM_IDX_CONFLICT), f);
            T.nidx[f] = itb_split_with_entry(itb_split_with_flag(T.nidx[f], POM_IDX_UNIQUE), nr);
        } else {
            T.nidx[f] = w;
            T.nidx[offset] = itb_split_with_conflict(itb_split_with_entry(w, nr), f);
        }
        T.n.pseudo++;
    }
    if (T.n.max_offset <= (int32_t)nr)
        T.n.max_offset = (int32_t)nr;
    T.n.entries++;
    return true;
}

// ---------------------------------------------------------------------------
// O: __ite_unlink and itb_del_ite (mds/itb.c:567-671).
// ---------------------------------------------------------------------------
ITB_SCAN_FN bool itb_split_unlink(itb_split_state& T, uint32_t d, uint32_t offset)
{
    const uint32_t w = T.oidx[offset], entry = itb_split_entry(w);
    if (entry >= d)
        return false;
    T.oidx[offset] = itb_split_with_flag(w, POM_IDX_FREE);
    if (offset >= d) {
        T.o.pseudo--;
        T.o.itu = (T.o.itu - 1u) & 0xFFFFu;
    }
    if (T.o.max_offset == (int32_t)entry)
        T.o.max_offset--;
    if (--T.o.entries == 0)
        T.o.max_offset = 0;
    T.obm[entry >> 6] &= ~(1ull << (entry & 63u));
    return true;
}

// The unlink of the ITE in slot `offset` of home slot pos's chain.
ITB_SCAN_FN bool itb_split_del(itb_split_state& T, uint32_t d, uint32_t offset, uint32_t pos)
{
    const uint32_t total = 2u * d;
    const uint32_t head = T.oidx[pos];
    if (itb_split_flag(head) == POM_IDX_FREE)
        return true;
    if (itb_split_flag(head) == POM_IDX_UNIQUE)
        return offset == pos ? itb_split_unlink(T, d, offset) : true;
    const uint32_t saved = pos;
    uint32_t prev = pos;
    bool quit = false, needswap = false, hit = false;
    pos = offset;
    offset = saved;
    uint32_t budget = total + 2u;
    do {
        for (;;) {                                      // (retry: the slot again after the swap)
            if (budget-- == 0)
                return false;
            const uint32_t w = T.oidx[offset];
            if (itb_split_flag(w) == POM_IDX_FREE)
                return needswap ? itb_split_unlink(T, d, saved) : true;
            if (pos == offset || hit) {
                if (offset == saved) {
                    needswap = true;
                    prev = offset;
                } else {
                    if (itb_split_flag(w) == POM_IDX_UNIQUE)
                        T.oidx[prev] = itb_split_with_flag(T.oidx[prev], POM_IDX_UNIQUE);
                    else
                        T.oidx[prev] = itb_split_with_conflict(T.oidx[prev], itb_split_conflict(w));
                    if (!itb_split_unlink(T, d, offset))
                        return false;
                    quit = true;
                }
                break;
            }
            if (needswap) {
                const uint32_t s = T.oidx[saved];
                T.oidx[offset] = itb_split_with_entry(w, itb_split_entry(s));
                T.oidx[saved] = itb_split_with_entry(s, itb_split_entry(w));
                needswap = false;
                hit = true;
                continue;
            }
            if (itb_split_flag(w) == POM_IDX_UNIQUE)
                quit = true;
            prev = offset;
            break;
        }
        offset = itb_split_conflict(T.oidx[offset]);
    } while (offset < total && !quit);
    return needswap ? itb_split_unlink(T, d, saved) : true;
}

// ---------------------------------------------------------------------------
// The loop (mds/xtable.c:103-146) over T.oidx / T.obm / T.o, filling T.nidx /
// T.nbm / T.from / T.n, which the caller has zeroed.  T.info is filled for
// every ITE below d.  Returns 0 or POM_SPLIT_E_DAMAGED; T.moved and T.steps
// count the ITEs moved and the chain steps taken.
// ---------------------------------------------------------------------------
ITB_SCAN_FN int32_t itb_split_index(itb_split_state& T, uint32_t d)
{
    uint32_t moved = 0, steps = 0;
    bool need_rescan = false;
    for (uint32_t j = 0; j < d; j++) {
        for (;;) {                                      // rescan:
            if (itb_split_flag(T.oidx[j]) == POM_IDX_FREE)
                break;
            uint32_t offset = j;
            bool rescan = false;
            for (;;) {
                if (++steps > itb_split_budget(d))
                    return POM_SPLIT_E_DAMAGED;
                const uint32_t w = T.oidx[offset], flag = itb_split_flag(w), entry = itb_split_entry(w);
                const bool done = flag == POM_IDX_UNIQUE;
                const uint32_t conflict = flag == POM_IDX_CONFLICT ? itb_split_conflict(w) : 0u;
                // what a passing check rules out: a free or OVERFLOW slot on a
                // chain, an entry past the table, a link that leaves the
                // overflow half
                if ((!done && flag != POM_IDX_CONFLICT) || entry >= d ||
                    (flag == POM_IDX_CONFLICT && (conflict < d || conflict >= 2u * d)))
                    return POM_SPLIT_E_DAMAGED;
                if (T.info[entry] & kItbSplitMove) {
                    if (!itb_split_add(T, d, entry) || !itb_split_del(T, d, offset, j))
                        return POM_SPLIT_E_DAMAGED;
                    moved++;
                    if (offset == j)
                        need_rescan = true;
                }
                if (done)
                    break;
                if (need_rescan) {
                    need_rescan = false;
                    rescan = true;
                    break;
                }
                offset = conflict;
            }
            if (!rescan)
                break;
        }
    }
    T.moved = moved;
    T.steps = steps;
    return 0;
}

// Rules 2 and 3; sd: the split depth asked for (hdr.depth + 1 without one).
ITB_SCAN_FN int32_t itb_split_precheck(uint32_t sd, uint64_t payload_off, uint64_t new_off)
{
    if (sd < 1u || sd > POM_SPLIT_DEPTH_MAX)
        return kItbScanEinval;
    return ((payload_off | new_off) & 15u) ? kItbScanEinval : 0;
}

// Dword i (0 ... 11) of the result of a split that produced something: the
// kernel stores one a lane.
static_assert(offsetof(pom_split_result, moved) == 4 && offsetof(pom_split_result, old_len) == 8 &&
              offsetof(pom_split_result, old_entries) == 16 && offsetof(pom_split_result, old_max_offset) == 24 &&
              offsetof(pom_split_result, old_pseudo) == 32 && offsetof(pom_split_result, old_inf) == 40 &&
              offsetof(pom_split_result, new_inf) == 44, "the result as twelve dwords");
ITB_SCAN_FN uint32_t itb_split_result_word(const itb_split_state& T, uint32_t i)
{
    switch (i) {
    case 0: return 0u;
    case 1: return T.moved;
    case 2: return itb_split_len(T.o);
    case 3: return itb_split_len(T.n);
    case 4: return (uint32_t)T.o.entries;
    case 5: return (uint32_t)T.n.entries;
    case 6: return (uint32_t)T.o.max_offset;
    case 7: return (uint32_t)T.n.max_offset;
    case 8: return (uint32_t)T.o.pseudo;
    case 9: return (uint32_t)T.n.pseudo;
    case 10: return (T.o.inf & 0xFFFFu) | (T.o.itu & 0xFFFFu) << 16;
    default: return (T.n.inf & 0xFFFFu) | (T.n.itu & 0xFFFFu) << 16;
    }
}

// O's counters from the header facts, N's as get_free_itb leaves them.
ITB_SCAN_FN void itb_split_sides(itb_split_state& T, const pom_check_hdr& h)
{
    T.o = itb_split_side{h.entries, h.max_offset, h.pseudo_conflicts, h.inf, h.itu};
    T.n = itb_split_side{0, 0, 0, 0u, 0u};
    T.moved = T.steps = 0;
    T.err = 0;
}

#ifndef __HIPCC__
#include <string.h>

// ---------------------------------------------------------------------------
// The whole split of one ITB on the CPU (the caller has dealt with status):
// the check, the rules, the loop, the copies.  p is modified in place (bitmap
// and index only); np gets N's payload.  steps (may be NULL): the chain steps
// the loop took.  Returns result->err.
// ---------------------------------------------------------------------------
static inline int32_t itb_split_one(uint8_t* p, uint32_t n, uint32_t adepth, const pom_check_hdr& hdr, uint32_t sd,
                                    uint64_t payload_off, uint64_t new_off, uint8_t* np, uint32_t new_cap,
                                    pom_split_result* result, uint32_t* steps)
{
    *result = pom_split_result{};
    if (steps)
        *steps = 0;
    pom_check_report rep;
    int32_t err = itb_check_one(p, n, adepth, &hdr, 0, &rep, nullptr, nullptr);
    if (err == 0)
        err = itb_split_precheck(sd, payload_off, new_off);
    if (err == 0 && (rep.findings & ~(1u << POM_CK_E_MISPLACED)))
        err = POM_SPLIT_E_DAMAGED;
    if (err != 0)
        return result->err = err;

    const uint32_t d = 1u << adepth;
    static thread_local itb_split_state T;
    memset(&T, 0, sizeof T);
    itb_split_sides(T, hdr);
    memcpy(T.oidx, p + POM_ITB_INDEX_OFF, sizeof T.oidx);
    memcpy(T.obm, p + POM_ITB_BITMAP_OFF, sizeof T.obm);
    uint32_t moved = 0;
    for (uint32_t nr = 0; nr < d; nr++)
        if ((T.obm[nr >> 6] >> (nr & 63u)) & 1u) {
            T.info[nr] = itb_split_info(itb_scan_ld64(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr + POM_ITE_HASH_OFF), d, sd);
            moved += (T.info[nr] & kItbSplitMove) != 0;
        }
    if (new_cap < POM_ITB_ITE_OFF + POM_ITE_SIZE * moved) {
        result->moved = moved;
        return result->err = kItbSplitOverrun;
    }
    if (moved == 0)
        return 0;
    err = itb_split_index(T, d);
    if (steps)
        *steps = T.steps;
    if (err == 0 && T.moved != moved)
        err = POM_SPLIT_E_DAMAGED;
    if (err != 0)
        return result->err = err;
    memset(np, 0, POM_ITB_BITMAP_OFF);
    memcpy(np + POM_ITB_BITMAP_OFF, T.nbm, sizeof T.nbm);
    memcpy(np + POM_ITB_INDEX_OFF, T.nidx, sizeof T.nidx);
    for (uint32_t k = 0; k < moved; k++)
        memcpy(np + POM_ITB_ITE_OFF + POM_ITE_SIZE * k, p + POM_ITB_ITE_OFF + POM_ITE_SIZE * T.from[k], POM_ITE_SIZE);
    memcpy(p + POM_ITB_BITMAP_OFF, T.obm, sizeof T.obm);
    memcpy(p + POM_ITB_INDEX_OFF, T.oidx, sizeof T.oidx);
    for (uint32_t i = 0; i < sizeof *result / 4; i++) {
        const uint32_t w = itb_split_result_word(T, i);
        memcpy(reinterpret_cast<uint8_t*>(result) + 4u * i, &w, 4);
    }
    return 0;
}
#endif

#endif
