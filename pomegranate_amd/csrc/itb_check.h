// itb_check.h -- the ITB check's rules (include/pom_check.h), stated once and
// built on itb_scan.h's payload checks and loader and itb_find.h's slot
// decode.  The kernel of itb_check.hip combines the pieces below over bitmaps
// in LDS, 64 slots a ballot; itb_check_one walks a payload one slot and one
// bit at a time on the CPU, where tests/native/itb_check_host.cc runs it.
// This header is plain C++17 outside hipcc.
//
// No byte at or past the payload's n is loaded; of the ITE area only the hash
// word of live ITEs below d.  Every payload load is itb_scan_ld64 at a
// multiple of 8 from the payload's start, so p may sit at any byte alignment.
#ifndef POM_ITB_CHECK_H
#define POM_ITB_CHECK_H

#include <stdint.h>

#include "itb_find.h"
#include "pom_check.h"

static_assert(sizeof(pom_check_hdr) == 32 && sizeof(pom_check_report) == 48, "the ABI's two structs");
static_assert(POM_ITB_INDEX_ENTRIES == 64u * POM_CK_SLOT_MASK_WORDS, "a bit per slot");
static_assert(1u << POM_ITB_ADEPTH_MAX == 64u * POM_CK_ITE_MASK_WORDS, "a bit per ITE");
static_assert(2u << POM_ITB_ADEPTH_MAX == POM_ITB_INDEX_ENTRIES, "both halves inside the table");
static_assert(POM_ITB_SIZE == 264u + POM_ITB_ITE_OFF, "struct itbh, then the payload up to the ITEs");

constexpr uint32_t kItbCheckFlags = POM_CK_ITBID;
constexpr uint32_t kItbCheckSlots = POM_ITB_INDEX_ENTRIES;
constexpr uint32_t kItbCheckItes = 1u << POM_ITB_ADEPTH_MAX;
constexpr uint32_t kItbCheckSlotKinds = 12;        // kinds 0 ... 11 are a slot's
constexpr uint32_t kItbCheckCounted = 16;          // kinds 0 ... 15 have a count
// what itb_check_local adds to a slot's kinds 0 ... 6
constexpr uint32_t kItbCheckGood = 1u << 16;       // the slot has a good link
constexpr uint32_t kItbCheckRef = 1u << 17;        // the slot refers to an ITE below d
// what itb_check_walk returns besides the path's length
constexpr uint32_t kItbCheckLooped = 1u << 31;

// ---------------------------------------------------------------------------
// Rules 2 and 3; rule 4 is itb_scan_live's, which also counts `live`.
// ---------------------------------------------------------------------------
ITB_SCAN_FN int32_t itb_check_precheck(uint32_t n, uint32_t adepth)
{
    if (adepth == 0 || adepth > POM_ITB_ADEPTH_MAX)
        return kItbScanEinval;
    return n < POM_ITB_ITE_OFF ? POM_GC_E_TRUNCATED : 0;
}

// ---------------------------------------------------------------------------
// Kinds 0 ... 6 of used slot s, from its own word, whether its link's target
// (read only for d <= conflict < 2d) is used, and whether its entry's bitmap
// bit (read only for entry < d) is set.  A slot outside has kind 0 alone.
// ---------------------------------------------------------------------------
ITB_SCAN_FN bool itb_check_links(const itb_find_slot& v)
{
    return v.flag == POM_IDX_CONFLICT || v.flag == POM_IDX_OVERFLOW;
}

// The slot's link points into the overflow half: its target's flag decides.
ITB_SCAN_FN bool itb_check_link_inside(const itb_find_slot& v, uint32_t s, uint32_t d)
{
    return s < 2u * d && itb_check_links(v) && v.conflict >= d && v.conflict < 2u * d;
}

ITB_SCAN_FN uint32_t itb_check_local(uint32_t s, const itb_find_slot& v, uint32_t d, bool target_used,
                                     bool entry_live)
{
    if (v.flag == POM_IDX_FREE)
        return 0;
    if (s >= 2u * d)
        return 1u << POM_CK_S_OUTSIDE;
    uint32_t k = 0;
    if (v.flag == POM_IDX_OVERFLOW)
        k |= 1u << POM_CK_S_FLAG;
    if (itb_check_links(v)) {
        if (v.conflict >= 2u * d)
            k |= 1u << POM_CK_S_LINK_RANGE;
        else if (v.conflict < d)
            k |= 1u << POM_CK_S_LINK_HOME;
        else
            k |= target_used ? kItbCheckGood : 1u << POM_CK_S_LINK_FREE;
    }
    if (v.entry >= d)
        k |= 1u << POM_CK_S_ENTRY_RANGE;
    else
        k |= kItbCheckRef | (entry_live ? 0u : 1u << POM_CK_S_ENTRY_DEAD);
    return k;
}

// ---------------------------------------------------------------------------
// The path from used home slot h over the good links.  A path goes on only in
// the overflow half, so it holds at most d + 1 distinct slots: one more good
// link is a repeat, and h is S_LOOP.  Every slot on the way is reached, and
// misfiled when its live entry below d hashes to another home slot; both are
// marks that may be set any number of times.  Returns the slots on the path,
// or kItbCheckLooped.
//   T.slot(s)       the decoded slot
//   T.live(nr)      the bitmap bit of an ITE below d
//   T.home(nr)      hash & (d - 1) of a live ITE below d
//   T.reach(s), T.misfile(s)
// ---------------------------------------------------------------------------
template <class Table>
ITB_SCAN_FN uint32_t itb_check_walk(Table& T, uint32_t h, uint32_t d)
{
    uint32_t s = h, len = 0;
    for (;;) {
        const itb_find_slot v = T.slot(s);
        if (++len > d + 1u)
            return kItbCheckLooped;
        T.reach(s);
        if (v.entry < d && T.live(v.entry) && T.home(v.entry) != h)
            T.misfile(s);
        if (!itb_check_link_inside(v, s, d) || T.slot(v.conflict).flag == POM_IDX_FREE)
            return len;
        s = v.conflict;
    }
}

// ---------------------------------------------------------------------------
// Kind 15 for one live ITE, and kinds 16 ... 21.
// ---------------------------------------------------------------------------
ITB_SCAN_FN bool itb_check_misplaced(uint64_t hash, const pom_check_hdr& h)
{
    const uint64_t mask = h.depth >= 64 ? ~0ull : (1ull << h.depth) - 1ull;
    return ((hash >> POM_ITB_ADEPTH_MAX) & mask) != h.itbid;
}

// top: the highest live bit (read only for live > 0).
ITB_SCAN_FN uint32_t itb_check_header(const pom_check_hdr& h, uint32_t d, uint32_t live, uint32_t top,
                                      uint32_t used_over)
{
    uint32_t k = 0;
    if ((int64_t)h.entries != (int64_t)live)
        k |= 1u << POM_CK_H_ENTRIES;
    if ((uint32_t)h.itu != used_over)
        k |= 1u << POM_CK_H_ITU;
    if ((int64_t)h.pseudo_conflicts != (int64_t)used_over)
        k |= 1u << POM_CK_H_PSEUDO;
    if (live > 0 && (int64_t)h.max_offset < (int64_t)top)
        k |= 1u << POM_CK_H_MAXOFF;
    if (live > 0 && (int64_t)h.ulen != (int64_t)POM_ITB_SIZE +
                                           (int64_t)POM_ITE_SIZE * ((int64_t)h.max_offset + 1))
        k |= 1u << POM_CK_H_LEN;
    if ((uint32_t)h.inf > d)
        k |= 1u << POM_CK_H_INF;
    return k;
}

#ifndef __HIPCC__
// ---------------------------------------------------------------------------
// The whole check of one ITB on the CPU, one slot and one bit at a time (the
// caller has dealt with status).  hdr, slot_mask (32 words) and ite_mask (16
// words) may be NULL.  Returns err.
// ---------------------------------------------------------------------------
struct itb_check_cpu_table {
    const uint8_t* p;
    uint32_t d;
    uint8_t reached[kItbCheckSlots], misfiled[kItbCheckSlots];
    itb_find_slot slot(uint32_t s) const { return itb_find_slot_at(p, s); }
    bool live(uint32_t nr) const { return (p[POM_ITB_BITMAP_OFF + nr / 8u] >> (nr % 8u)) & 1u; }
    uint32_t home(uint32_t nr) const
    {
        return (uint32_t)itb_scan_ld64(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr + POM_ITE_HASH_OFF) & (d - 1u);
    }
    void reach(uint32_t s) { reached[s] = 1; }
    void misfile(uint32_t s) { misfiled[s] = 1; }
};

static inline int32_t itb_check_one(const uint8_t* p, uint32_t n, uint32_t adepth, const pom_check_hdr* hdr,
                                    uint32_t flags, pom_check_report* report, uint64_t* slot_mask,
                                    uint64_t* ite_mask)
{
    *report = pom_check_report{};
    if (slot_mask)
        for (uint32_t w = 0; w < POM_CK_SLOT_MASK_WORDS; w++)
            slot_mask[w] = 0;
    if (ite_mask)
        for (uint32_t w = 0; w < POM_CK_ITE_MASK_WORDS; w++)
            ite_mask[w] = 0;
    int32_t err = itb_check_precheck(n, adepth);
    if (err != 0)
        return err;
    uint32_t live = 0;
    err = itb_scan_live(p, n, adepth, &live);
    report->live = live;
    if (err != 0)
        return err;

    const uint32_t d = 1u << adepth;
    static thread_local itb_check_cpu_table T;
    T = itb_check_cpu_table{};
    T.p = p;
    T.d = d;
    uint32_t slot_kinds[kItbCheckSlots] = {}, ite_kinds[kItbCheckItes] = {};
    uint32_t indeg[kItbCheckSlots] = {}, refs[kItbCheckItes] = {};
    uint32_t used_home = 0, used_over = 0, longest = 0, top = 0;

    for (uint32_t s = 0; s < kItbCheckSlots; s++) {
        const itb_find_slot v = T.slot(s);
        if (v.flag == POM_IDX_FREE)
            continue;
        const bool target_used = itb_check_link_inside(v, s, d) && T.slot(v.conflict).flag != POM_IDX_FREE;
        const bool entry_live = s < 2u * d && v.entry < d && T.live(v.entry);
        const uint32_t k = itb_check_local(s, v, d, target_used, entry_live);
        slot_kinds[s] = k & 0xFFFFu;
        if (k & kItbCheckGood)
            indeg[v.conflict]++;
        if (k & kItbCheckRef)
            refs[v.entry]++;
        if (s < d)
            used_home++;
        else if (s < 2u * d)
            used_over++;
    }
    for (uint32_t h = 0; h < d; h++) {
        if (T.slot(h).flag == POM_IDX_FREE)
            continue;
        const uint32_t len = itb_check_walk(T, h, d);
        if (len == kItbCheckLooped)
            slot_kinds[h] |= 1u << POM_CK_S_LOOP;
        else if (len > longest)
            longest = len;
    }
    uint32_t reached = 0;
    for (uint32_t s = 0; s < 2u * d; s++) {
        reached += T.reached[s];
        if (T.misfiled[s])
            slot_kinds[s] |= 1u << POM_CK_S_MISFILED;
        if (s < d || T.slot(s).flag == POM_IDX_FREE)
            continue;
        if (indeg[s] >= 2)
            slot_kinds[s] |= 1u << POM_CK_S_SHARED;
        if (indeg[s] == 0)
            slot_kinds[s] |= 1u << POM_CK_S_LEAKED;
        else if (!T.reached[s])
            slot_kinds[s] |= 1u << POM_CK_S_ISLAND;
    }
    for (uint32_t nr = 0; nr < kItbCheckItes; nr++) {
        const bool bit = (p[POM_ITB_BITMAP_OFF + nr / 8u] >> (nr % 8u)) & 1u;
        if (nr >= d) {
            if (bit)
                ite_kinds[nr] |= 1u << POM_CK_E_STRAY;
            continue;
        }
        if (bit)
            top = nr;
        if (refs[nr] >= 2)
            ite_kinds[nr] |= 1u << POM_CK_E_DUP;
        if (bit && refs[nr] == 0)
            ite_kinds[nr] |= 1u << POM_CK_E_ORPHAN;
        if (bit && hdr && (flags & POM_CK_ITBID) &&
            itb_check_misplaced(itb_scan_ld64(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr + POM_ITE_HASH_OFF), *hdr))
            ite_kinds[nr] |= 1u << POM_CK_E_MISPLACED;
    }

    uint32_t findings = 0;
    for (uint32_t s = 0; s < kItbCheckSlots; s++) {
        if (!slot_kinds[s])
            continue;
        findings |= slot_kinds[s];
        for (uint32_t k = 0; k < kItbCheckSlotKinds; k++)
            report->count[k] += (slot_kinds[s] >> k) & 1u;
        if (slot_mask)
            slot_mask[s / 64u] |= 1ull << (s % 64u);
    }
    for (uint32_t nr = 0; nr < kItbCheckItes; nr++) {
        if (!ite_kinds[nr])
            continue;
        findings |= ite_kinds[nr];
        for (uint32_t k = kItbCheckSlotKinds; k < kItbCheckCounted; k++)
            report->count[k] += (ite_kinds[nr] >> k) & 1u;
        if (ite_mask)
            ite_mask[nr / 64u] |= 1ull << (nr % 64u);
    }
    if (hdr)
        findings |= itb_check_header(*hdr, d, live, top, used_over);
    report->findings = findings;
    report->used_home = (uint16_t)used_home;
    report->used_over = (uint16_t)used_over;
    report->reached = (uint16_t)reached;
    report->longest = (uint16_t)longest;
    return 0;
}
#endif

#endif
