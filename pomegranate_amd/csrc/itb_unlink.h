// itb_unlink.h -- the ITB unlink's rules (include/pom_unlink.h), stated once and
// built on itb_find.h's match and record words, itb_split.h's index words and
// itb_sweep.h's __ite_unlink counters:
//   itb_unlink_ite      ite_unlink's arithmetic (mds/itb.c:676-707) on (flag,
//                       mode, nlink, async) as one pure function
//   itb_unlink_del      itb_del_ite (:602-671) over an index table, an ITE
//                       bitmap and the header's counters held in plain arrays
//   itb_unlink_request  one request against the table as the earlier requests
//                       left it: the walk of itb_search (:1769-1797), then
//                       itb_unlink_apply
//   itb_unlink_list, itb_unlink_member, itb_unlink_apply
//                       the same walk as the kernel takes it: the chain's
//                       members listed a round at a time, each matched on its
//                       own, the lowest that matches is the hit
// Everything a request can change -- the index, the bitmap, the counters, each
// live ITE's flag word and its (mode, nlink) word -- lives in struct
// itb_unlink_state (in LDS in the kernel of itb_unlink.hip, static in
// itb_unlink_one on the CPU, where tests/native/itb_unlink_host.cc runs both
// forms); names, uuids and hashes never change and are read from the payload.
// This header is plain C++17 outside hipcc.
//
// Every walk here is bounded, whatever the table holds: a chain by
// kItbUnlinkSteps slots, and every slot or ITE number is range-checked before
// it is an index.  A bound that is hit is kItbUnlinkBad, POM_SPLIT_E_DAMAGED
// for the ITB; after a passing check none can be.
#ifndef POM_ITB_UNLINK_H
#define POM_ITB_UNLINK_H

#include <stddef.h>
#include <stdint.h>

#include "itb_find.h"
#include "itb_sweep.h"
#include "pom_unlink.h"

static_assert(sizeof(pom_unlink_result) == 32, "the ABI's result");
static_assert(POM_ITE_MODE_OFF % 4 == 0 && POM_ITE_NLINK_OFF == POM_ITE_MODE_OFF + 2, "mode and nlink are one dword");
static_assert(POM_ITE_MODE_OFF / 8 == (POM_ITE_MD_OFF + 8) / 8, "the record's third word holds them in its upper half");

constexpr uint32_t kItbUnlinkFlags = POM_UL_UNLINK | POM_LK_BY_NAME | POM_LK_BY_UUID | POM_LK_ITE_ACTIVE | POM_LK_ITE_SHADOW;
constexpr uint32_t kItbUnlinkSteps = kItbCheckItes + 1u;    // a chain of a passing table has at most d members
constexpr uint32_t kItbUnlinkRefused = 0xFFFFFFFEu;         // a `what`: request rule 9
constexpr uint32_t kItbUnlinkBad = 0xFFFFFFFFu;             // a `what` or a count: what a passing check rules out
constexpr uint32_t kItbUnlinkRound = 64;                    // members a round of the kernel's walk lists
constexpr uint32_t kItbUnlinkMdWord = (POM_ITE_MODE_OFF - POM_ITE_MD_OFF) / 8 + 1;     // the record word with mode and nlink

struct itb_unlink_state {
    uint32_t idx[kItbCheckSlots];
    uint64_t bm[POM_CK_ITE_MASK_WORDS];                 // the ITE bitmap
    uint64_t dirty[POM_CK_ITE_MASK_WORDS];              // per ITE: its flag or nlink differs from the payload's
    uint32_t flag[kItbCheckItes];                       // per live ITE: e->flag
    uint32_t mn[kItbCheckItes];                         // per live ITE: s.mdu.mode | s.mdu.nlink << 16
    itb_sweep_counts h;
    uint32_t removed, changed, hits;
};

// ---------------------------------------------------------------------------
// ite_unlink (mds/itb.c:676-707, and the delta's condition :701-716) on the
// flag word, mode and nlink (u16 each): the flag and nlink it leaves, and
// `what` with POM_UL_DELTA; kItbUnlinkRefused for the flags of rule 9, with
// nothing changed.
// ---------------------------------------------------------------------------
struct itb_unlink_step {
    uint32_t flag, nlink, what;
};

ITB_SCAN_FN itb_unlink_step itb_unlink_ite(uint32_t flag, uint32_t mode, uint32_t nlink, bool async)
{
    itb_unlink_step s{flag, nlink & 0xFFFFu, POM_UL_NONE};
    const bool file = (flag & (POM_ITE_FLAG_NORMAL | POM_ITE_FLAG_SYM)) != 0, ls = (flag & POM_ITE_FLAG_LS) != 0;
    const bool kv = (flag & POM_ITE_FLAG_KV) != 0;
    if (kv && (file || ls)) {
        s.what = kItbUnlinkRefused;
        return s;
    }
    if (file) {
        s.nlink = (s.nlink - 1u) & 0xFFFFu;
        if (mode & POM_UL_MODE_DIR)
            s.nlink = (s.nlink - 1u) & 0xFFFFu;
        if (s.nlink != 0) {
            s.flag = (flag & ~POM_ITE_STATE_MASK) | POM_ITE_SHADOW;
            s.what = POM_UL_SHADOWED;
        } else if (async) {
            s.flag = (flag & ~POM_ITE_STATE_MASK) | POM_ITE_UNLINKED;
            s.what = POM_UL_MARKED;
        } else {
            s.what = POM_UL_DELETED;
        }
    } else if (ls) {
        s.nlink = 0;
        s.what = POM_UL_DELETED;
    } else if (kv) {
        s.what = POM_UL_DELETED;
    }
    if ((flag & POM_ITE_FLAG_SDT) && (kv || s.nlink == 0))
        s.what |= POM_UL_DELTA;
    return s;
}

// ---------------------------------------------------------------------------
// itb_del_ite (mds/itb.c:602-671): `target` is the slot that hit, `home` the
// request's home slot.  false: the walk met what a passing check rules out, a
// trailing needswap among it, or deleted nothing.
// ---------------------------------------------------------------------------
// __ite_unlink (:567-592)
ITB_SCAN_FN bool itb_unlink_free(itb_unlink_state& T, uint32_t d, uint32_t offset)
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

ITB_SCAN_FN bool itb_unlink_del(itb_unlink_state& T, uint32_t d, uint32_t target, uint32_t home)
{
    if (home >= d || target >= 2u * d)
        return false;
    uint32_t w = T.idx[home];
    if (!itb_sweep_slot_ok(w, d))
        return false;
    if (itb_split_flag(w) == POM_IDX_UNIQUE)
        return target == home && itb_unlink_free(T, d, home);
    const uint32_t before = T.removed;
    uint32_t offset = home, prev = home, steps = kItbUnlinkSteps + 1u;     // (the retry takes one more)
    bool quit = false, needswap = false, hit = false;
    do {
        for (;;) {                                      // (retry: the slot again after the swap)
            if (steps-- == 0)
                return false;
            w = T.idx[offset];
            if (!itb_sweep_slot_ok(w, d))               // (the reference breaks on FREE: no chain of a passing table has one)
                return false;
            if (offset == target || hit) {
                if (offset == home) {
                    needswap = true;
                    prev = offset;
                } else {
                    if (itb_split_flag(w) == POM_IDX_UNIQUE)
                        T.idx[prev] = itb_split_with_flag(T.idx[prev], POM_IDX_UNIQUE);
                    else
                        T.idx[prev] = itb_split_with_conflict(T.idx[prev], itb_split_conflict(w));
                    if (!itb_unlink_free(T, d, offset))
                        return false;
                    quit = true;
                }
            } else {
                if (needswap) {
                    const uint32_t s = T.idx[home];
                    T.idx[offset] = itb_split_with_entry(w, itb_split_entry(s));
                    T.idx[home] = itb_split_with_entry(s, itb_split_entry(w));
                    needswap = false;
                    hit = true;
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
    return !needswap && T.removed == before + 1u;
}

// ---------------------------------------------------------------------------
// A request's own checks (rule 4), the match of one chain member (rule 7) and
// the record
// ---------------------------------------------------------------------------
ITB_SCAN_FN bool itb_unlink_req_ok(const pom_lookup_req& q, uint32_t names_len)
{
    return !(q.flag & ~kItbUnlinkFlags) && q.namelen <= kItbFindNameMax && q.column == 0 &&
           (uint64_t)q.name_off + q.namelen <= names_len;
}

// ite_match on ITE `entry` (below d, inside the payload) with its flag as the
// earlier requests left it.
ITB_SCAN_FN bool itb_unlink_member(const itb_unlink_state& T, const uint8_t* p, uint32_t entry, const pom_lookup_req& q,
                                   const uint8_t* names)
{
    const uint8_t* ite = p + POM_ITB_ITE_OFF + POM_ITE_SIZE * entry;
    const uint64_t fn = (itb_scan_ld64(ite + POM_ITE_FLAG_OFF) & ~0xFFFFFFFFull) | T.flag[entry];
    return itb_find_match_fn(ite, fn, q, names);
}

// Word w (0 ... 16) of the record of ITE `entry`: the lookup's without a
// column, with mode and nlink as the earlier requests left them.
ITB_SCAN_FN uint64_t itb_unlink_word(const itb_unlink_state& T, const uint8_t* p, uint32_t entry, uint32_t w)
{
    const uint64_t v = itb_find_word(p, POM_ITB_ITE_OFF + (uint64_t)POM_ITE_SIZE * entry, kItbFindNoColumn, w);
    return w == kItbUnlinkMdWord ? ((v & 0xFFFFFFFFull) | (uint64_t)T.mn[entry] << 32) : v;
}

// ---------------------------------------------------------------------------
// ite_unlink on the ITE that hit in slot `slot` of home slot `home`'s chain.
// Returns `what`, kItbUnlinkRefused (nothing changed) or kItbUnlinkBad.
// ---------------------------------------------------------------------------
ITB_SCAN_FN uint32_t itb_unlink_apply(itb_unlink_state& T, uint32_t d, bool async, uint32_t slot, uint32_t home,
                                      uint32_t entry)
{
    const uint32_t flag = T.flag[entry], mn = T.mn[entry];
    const itb_unlink_step s = itb_unlink_ite(flag, mn & 0xFFFFu, mn >> 16, async);
    if (s.what == kItbUnlinkRefused)
        return s.what;
    if (s.flag != flag || s.nlink != mn >> 16)
        T.dirty[entry >> 6] |= 1ull << (entry & 63u);
    T.flag[entry] = s.flag;
    T.mn[entry] = (mn & 0xFFFFu) | s.nlink << 16;
    if ((s.what & POM_UL_WHAT_MASK) == POM_UL_DELETED && !itb_unlink_del(T, d, slot, home))
        return kItbUnlinkBad;
    if ((s.what & POM_UL_WHAT_MASK) != POM_UL_NONE)
        T.changed++;
    T.hits++;
    return s.what;
}

// ---------------------------------------------------------------------------
// The walk, a round at a time: up to `room` members of the chain from slot
// *offset on, as slot[k] and entry[k]; *offset is where the chain goes on when
// *more is set.  A FREE slot ends the chain, as in the reference.  Returns the
// count, or kItbUnlinkBad for a slot or an ITE a passing check rules out.
// ---------------------------------------------------------------------------
ITB_SCAN_FN uint32_t itb_unlink_list(const uint32_t* idx, uint32_t d, uint32_t n, uint32_t* offset, uint16_t* slot,
                                     uint16_t* entry, uint32_t room, bool* more)
{
    uint32_t k = 0, o = *offset;
    *more = false;
    while (k < room) {
        if (o >= 2u * d)
            return kItbUnlinkBad;
        const uint32_t w = idx[o];
        if (itb_split_flag(w) == POM_IDX_FREE)
            return k;
        if (!itb_sweep_slot_ok(w, d) || !itb_scan_ite_inside(itb_split_entry(w), n))
            return kItbUnlinkBad;
        slot[k] = (uint16_t)o;
        entry[k] = (uint16_t)itb_split_entry(w);
        k++;
        if (itb_split_flag(w) == POM_IDX_UNIQUE)
            return k;
        o = itb_split_conflict(w);
    }
    *offset = o;
    *more = true;
    return k;
}

// ---------------------------------------------------------------------------
// One request (rules 4 ... 10; the caller has dealt with rules 0 and 1) in the
// reference's form, a slot at a time.  Returns err; *what is kItbUnlinkBad
// when the ITB is damaged.  On 0, *nr is the ITE that hit, and rec (when not
// NULL) gets the record's seventeen words as they were before the unlink.
// ---------------------------------------------------------------------------
ITB_SCAN_FN int32_t itb_unlink_request(itb_unlink_state& T, const uint8_t* p, uint32_t n, uint32_t d, bool async,
                                       const pom_lookup_req& q, const uint8_t* names, uint32_t names_len, uint32_t* nr,
                                       uint32_t* depth, uint32_t* what, uint64_t* rec)
{
    *nr = *depth = *what = 0;
    if (!itb_unlink_req_ok(q, names_len))
        return kItbScanEinval;
    const uint32_t home = (uint32_t)q.hash & (d - 1u);
    uint32_t offset = home, dep = 0;
    for (;;) {
        if (offset >= 2u * d || dep == kItbUnlinkSteps) {
            *what = kItbUnlinkBad;
            return POM_SPLIT_E_DAMAGED;
        }
        const uint32_t w = T.idx[offset];
        if (itb_split_flag(w) == POM_IDX_FREE)
            break;
        const uint32_t entry = itb_split_entry(w);
        if (!itb_sweep_slot_ok(w, d) || !itb_scan_ite_inside(entry, n)) {
            *what = kItbUnlinkBad;
            return POM_SPLIT_E_DAMAGED;
        }
        dep++;
        if (itb_unlink_member(T, p, entry, q, names)) {
            *depth = dep;
            uint64_t words[kItbFindRecWords];
            for (uint32_t i = 0; i < kItbFindRecWords; i++)
                words[i] = itb_unlink_word(T, p, entry, i);
            const uint32_t did = itb_unlink_apply(T, d, async, offset, home, entry);
            if (did == kItbUnlinkRefused)
                return kItbScanEinval;
            if (did == kItbUnlinkBad) {
                *what = kItbUnlinkBad;
                return POM_SPLIT_E_DAMAGED;
            }
            *nr = entry;
            *what = did;
            if (rec)
                for (uint32_t i = 0; i < kItbFindRecWords; i++)
                    rec[i] = words[i];
            return 0;
        }
        if (itb_split_flag(w) == POM_IDX_UNIQUE)
            break;
        offset = itb_split_conflict(w);
    }
    *depth = dep;
    return kItbFindEnoent;
}

// Rule 2.
ITB_SCAN_FN int32_t itb_unlink_precheck(uint64_t payload_off)
{
    return (payload_off & 15u) ? kItbScanEinval : 0;
}

// Dword i (0 ... 7) of the result of an ITB whose err is 0: the kernel stores
// one a lane.
static_assert(offsetof(pom_unlink_result, changed) == 4 && offsetof(pom_unlink_result, removed) == 8 &&
              offsetof(pom_unlink_result, len) == 12 && offsetof(pom_unlink_result, entries) == 16 &&
              offsetof(pom_unlink_result, pseudo_conflicts) == 24 && offsetof(pom_unlink_result, itu) == 28 &&
              offsetof(pom_unlink_result, hits) == 30, "the result as eight dwords");
ITB_SCAN_FN uint32_t itb_unlink_result_word(const itb_unlink_state& T, uint32_t i)
{
    const uint32_t hits = (T.hits < 0xFFFFu ? T.hits : 0xFFFFu) << 16;
    if (T.changed == 0)
        return i == 7 ? hits : 0u;
    switch (i) {
    case 0: return 0u;
    case 1: return T.changed;
    case 2: return T.removed;
    case 3: return itb_sweep_len(T.h);
    case 4: return (uint32_t)T.h.entries;
    case 5: return (uint32_t)T.h.max_offset;
    case 6: return (uint32_t)T.h.pseudo;
    default: return (T.h.itu & 0xFFFFu) | hits;
    }
}

ITB_SCAN_FN void itb_unlink_counts_of(itb_unlink_state& T, const pom_check_hdr& h)
{
    T.h = itb_sweep_counts{h.entries, h.max_offset, h.pseudo_conflicts, h.itu};
    T.removed = T.changed = T.hits = 0;
}

#ifndef __HIPCC__
#include <string.h>

// ---------------------------------------------------------------------------
// The unlinks of one ITB on the CPU (the caller has dealt with status): the
// check, the rules, the nreq requests of the group in order -- as
// itb_unlink_request takes them, or (parts) in the kernel's data flow: the
// chain's members listed kItbUnlinkRound a round, each matched on its own, the
// lowest match the hit.  b is the group's number (rule 0).  p is modified in
// place.  out: 136 bytes a request, at any alignment.  Returns result->err.
// ---------------------------------------------------------------------------
static inline void itb_unlink_put_record(uint8_t* out, const uint64_t* words)
{
    for (uint32_t w = 0; w < kItbFindRecWords; w++)
        for (uint32_t j = 0; j < 8; j++)
            out[8u * w + j] = words ? (uint8_t)(words[w] >> (8u * j)) : 0;
}

static inline int32_t itb_unlink_one(uint8_t* p, uint32_t n, uint32_t adepth, const pom_check_hdr& hdr, bool async,
                                     uint64_t payload_off, uint32_t b, const pom_lookup_req* req, uint32_t nreq,
                                     const uint8_t* names, uint32_t names_len, bool parts, int32_t* err, uint32_t* nr,
                                     uint32_t* depth, uint32_t* what, uint8_t* out, pom_unlink_result* result)
{
    *result = pom_unlink_result{};
    pom_check_report rep;
    int32_t e = itb_check_one(p, n, adepth, &hdr, 0, &rep, nullptr, nullptr);
    if (e == 0)
        e = itb_unlink_precheck(payload_off);
    if (e == 0 && (rep.findings & ~(1u << POM_CK_E_MISPLACED)))
        e = POM_SPLIT_E_DAMAGED;

    const uint32_t d = e == 0 ? 1u << adepth : 0u;
    static thread_local itb_unlink_state T;
    if (e == 0) {
        memset(&T, 0, sizeof T);
        itb_unlink_counts_of(T, hdr);
        memcpy(T.idx, p + POM_ITB_INDEX_OFF, sizeof T.idx);
        memcpy(T.bm, p + POM_ITB_BITMAP_OFF, sizeof T.bm);
        for (uint32_t i = 0; i < d; i++)
            if (itb_sweep_bit(T.bm, i)) {
                memcpy(&T.flag[i], p + POM_ITB_ITE_OFF + POM_ITE_SIZE * i + POM_ITE_FLAG_OFF, 4);
                memcpy(&T.mn[i], p + POM_ITB_ITE_OFF + POM_ITE_SIZE * i + POM_ITE_MODE_OFF, 4);
            }
    }
    for (uint32_t r = 0; r < nreq; r++) {
        const pom_lookup_req& q = req[r];
        uint64_t words[kItbFindRecWords];
        uint32_t w = 0;
        nr[r] = depth[r] = what[r] = 0;
        if (q.itb != b) {
            err[r] = kItbScanEinval;
        } else if (e != 0) {
            err[r] = e;
        } else if (!parts) {
            err[r] = itb_unlink_request(T, p, n, d, async, q, names, names_len, &nr[r], &depth[r], &w, words);
        } else if (!itb_unlink_req_ok(q, names_len)) {
            err[r] = kItbScanEinval;
        } else {
            const uint32_t home = (uint32_t)q.hash & (d - 1u);
            uint32_t offset = home, dep = 0;
            uint16_t slot[kItbUnlinkRound], entry[kItbUnlinkRound];
            bool more = true;
            err[r] = kItbFindEnoent;
            while (more && w != kItbUnlinkBad) {
                const uint32_t cnt = itb_unlink_list(T.idx, d, n, &offset, slot, entry, kItbUnlinkRound, &more);
                if (cnt == kItbUnlinkBad || dep + cnt > kItbUnlinkSteps) {
                    w = kItbUnlinkBad;
                    break;
                }
                uint32_t k = cnt;
                for (uint32_t lane = cnt; lane-- > 0;)          // (any order: the lowest match wins)
                    if (itb_unlink_member(T, p, entry[lane], q, names))
                        k = lane;
                if (k == cnt) {
                    dep += cnt;
                    continue;
                }
                dep += k + 1u;
                for (uint32_t i = 0; i < kItbFindRecWords; i++)
                    words[i] = itb_unlink_word(T, p, entry[k], i);
                w = itb_unlink_apply(T, d, async, slot[k], home, entry[k]);
                err[r] = w == kItbUnlinkRefused ? kItbScanEinval : 0;
                nr[r] = err[r] == 0 ? entry[k] : 0;
                more = false;
            }
            depth[r] = dep;
        }
        if (w == kItbUnlinkBad) {
            e = POM_SPLIT_E_DAMAGED;
            break;
        }
        what[r] = err[r] == 0 ? w : 0;
        itb_unlink_put_record(out + POM_LK_REC_SIZE * r, err[r] == 0 ? words : nullptr);
    }
    if (e != 0) {
        for (uint32_t r = 0; r < nreq; r++) {
            err[r] = req[r].itb != b ? kItbScanEinval : e;
            nr[r] = depth[r] = what[r] = 0;
            itb_unlink_put_record(out + POM_LK_REC_SIZE * r, nullptr);
        }
        return result->err = e;
    }
    if (T.changed != 0) {
        if (T.removed != 0) {
            memcpy(p + POM_ITB_BITMAP_OFF, T.bm, sizeof T.bm);
            memcpy(p + POM_ITB_INDEX_OFF, T.idx, sizeof T.idx);
        }
        for (uint32_t i = 0; i < d; i++)
            if (itb_sweep_bit(T.dirty, i)) {
                const uint16_t nlink = (uint16_t)(T.mn[i] >> 16);
                memcpy(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * i + POM_ITE_FLAG_OFF, &T.flag[i], 4);
                memcpy(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * i + POM_ITE_NLINK_OFF, &nlink, 2);
            }
    }
    for (uint32_t i = 0; i < sizeof *result / 4; i++) {
        const uint32_t v = itb_unlink_result_word(T, i);
        memcpy(reinterpret_cast<uint8_t*>(result) + 4u * i, &v, 4);
    }
    return 0;
}
#endif

#endif
