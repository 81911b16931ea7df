// itb_find.h -- the lookup's walk over one decoded ITB payload (the
// INDEX_LOOKUP branch of itb_search, mds/itb.c:1769-1814, with ite_match,
// :1119-1148), stated once and built on itb_scan.h's payload checks and its
// alignment-safe loader.  The kernel of itb_find.hip runs itb_find_one with
// one lane per request and copies the records out with the wave
// (itb_find_granule); tests/native/itb_find_host.cc runs both on the CPU.
// This header is plain C++17 outside hipcc.
//
// The rules for one request are include/pom_lookup.h's.  No byte at or past
// the payload's n is loaded and none outside [0, names_len) of the name blob;
// p and the blob may sit at any byte alignment: every payload load is
// itb_scan_ld64 at a multiple of 8 from the payload's start (one load when p
// is 8-byte aligned, else byte by byte), index slots included.
#ifndef POM_ITB_FIND_H
#define POM_ITB_FIND_H

#include <stdint.h>

#include "itb_scan.h"
#include "pom_lookup.h"

static_assert(sizeof(pom_lookup_req) == 32, "the request as four u64");
static_assert(POM_ITB_INDEX_OFF % 8 == 0 && POM_ITB_INDEX_SIZE == 4, "two slots a load");
static_assert(POM_ITB_INDEX_OFF + POM_ITB_INDEX_SIZE * POM_ITB_INDEX_ENTRIES == POM_ITB_ITE_OFF, "index, then ITEs");
static_assert(POM_ITE_HASH_OFF % 8 == 0 && POM_ITE_MD_OFF % 8 == 0 && POM_MDU_SIZE % 8 == 0, "ld64 fields");
static_assert(POM_LK_REC_SIZE == 8 + POM_MDU_SIZE + POM_COLUMN_SIZE, "uuid, MDU, column");
static_assert(POM_ITE_COLUMN_OFF + POM_COLUMN_SIZE * POM_ITE_COLUMNS <= POM_ITE_SIZE, "columns inside the ITE");
static_assert(POM_ITE_NAME_OFF + POM_ITE_NAME_MAX <= POM_ITE_SIZE, "s.name inside the ITE");

constexpr int32_t kItbFindEnoent = POM_LK_E_NOENT;
constexpr uint32_t kItbFindFlags = POM_LK_BY_NAME | POM_LK_BY_UUID | POM_LK_LOOKUP | POM_LK_COLUMN |
                                   POM_LK_ITE_ACTIVE | POM_LK_ITE_SHADOW;
constexpr uint32_t kItbFindNameMax = 255;                   // hi->namelen is a u8
constexpr uint32_t kItbFindRecWords = POM_LK_REC_SIZE / 8;  // 17
constexpr uint32_t kItbFindNoColumn = POM_ITE_COLUMNS;      // a record whose column stays zero
constexpr uint64_t kItbFindNoIte = ~0ull;                   // a record of zeros

// ---------------------------------------------------------------------------
// The index table
// ---------------------------------------------------------------------------
struct itb_find_slot {
    uint32_t entry, conflict, flag;
};

// Slot `offset` (below 2048) of a payload that holds the whole table.
ITB_SCAN_FN itb_find_slot itb_find_slot_at(const uint8_t* p, uint32_t offset)
{
    const uint64_t w = itb_scan_ld64(p + POM_ITB_INDEX_OFF + 8u * (offset >> 1));
    const uint32_t v = (uint32_t)(w >> (32u * (offset & 1u)));
    constexpr uint32_t mask = (1u << POM_IDX_ENTRY_BITS) - 1u;
    return itb_find_slot{v & mask, (v >> POM_IDX_ENTRY_BITS) & mask, v >> POM_IDX_FLAG_SHIFT};
}

// ---------------------------------------------------------------------------
// The request's own checks (rule 4) and the match (rule 7)
// ---------------------------------------------------------------------------
ITB_SCAN_FN bool itb_find_req_ok(const pom_lookup_req& q, uint32_t names_len)
{
    return !(q.flag & ~kItbFindFlags) && q.namelen <= kItbFindNameMax &&
           !((q.flag & POM_LK_COLUMN) && q.column >= POM_ITE_COLUMNS) &&
           (uint64_t)q.name_off + q.namelen <= names_len;
}

// The low k (1 ... 8) bytes of eight, from a blob at any alignment; only those
// k bytes are loaded unless all eight are asked for.
ITB_SCAN_FN uint64_t itb_find_name_bytes(const uint8_t* s, uint32_t k)
{
    if (k == 8)
        return itb_scan_ld64(s);
    uint64_t v = 0;
    for (uint32_t i = 0; i < k; i++)
        v |= (uint64_t)s[i] << (8 * i);
    return v;
}

// memcmp(e->s.name, hi->name, hi->namelen) == 0, eight bytes a step; the ITE's
// side is whole words of s.name (namelen <= 255 keeps them inside it).
ITB_SCAN_FN bool itb_find_name_eq(const uint8_t* ite, const uint8_t* name, uint32_t namelen)
{
    for (uint32_t i = 0; i < namelen; i += 8) {
        const uint32_t k = namelen - i < 8u ? namelen - i : 8u;
        const uint64_t keep = k >= 8u ? ~0ull : (1ull << (8u * k)) - 1ull;
        if ((itb_scan_ld64(ite + POM_ITE_NAME_OFF + i) & keep) != itb_find_name_bytes(name + i, k))
            return false;
    }
    return true;
}

// ite_match (mds/itb.c:1119-1148) on an ITE that lies inside the payload, with
// its flag and namelen words given as fn (a writer keeps the flags its earlier
// requests changed outside the payload: itb_unlink.h).
ITB_SCAN_FN bool itb_find_match_fn(const uint8_t* ite, uint64_t fn, const pom_lookup_req& q, const uint8_t* names)
{
    const uint32_t state = (uint32_t)fn & POM_ITE_STATE_MASK;
    if ((q.flag & POM_LK_ITE_SHADOW) && state != POM_ITE_SHADOW && state != POM_ITE_UNLINKED)
        return false;
    if ((q.flag & POM_LK_ITE_ACTIVE) && state != 0)                 // ITE_ACTIVE
        return false;
    if (state == POM_ITE_UNLINKED && !(q.flag & POM_LK_ITE_SHADOW))
        return false;
    if (q.flag & POM_LK_BY_UUID)
        return itb_scan_ld64(ite + POM_ITE_UUID_OFF) == q.uuid && itb_scan_ld64(ite + POM_ITE_HASH_OFF) == q.hash;
    if (q.flag & POM_LK_BY_NAME)
        return (uint32_t)(fn >> 32) == q.namelen && itb_find_name_eq(ite, names + q.name_off, q.namelen);
    return false;
}

ITB_SCAN_FN bool itb_find_match(const uint8_t* ite, const pom_lookup_req& q, const uint8_t* names)
{
    return itb_find_match_fn(ite, itb_scan_ld64(ite + POM_ITE_FLAG_OFF), q, names);     // flag, namelen
}

// ---------------------------------------------------------------------------
// The chain walk (rules 5, 6 and 8) from index slot `offset`, with the match
// as a parameter: match(ite) on an ITE that lies inside the payload.  The
// payload holds the whole index table.  Returns err; on 0, *nr is the ITE
// that hit.  itb_kvget.h walks with its own match.
// ---------------------------------------------------------------------------
template <class Match>
ITB_SCAN_FN int32_t itb_find_walk(const uint8_t* p, uint32_t n, uint32_t offset, const Match& match, uint32_t* nr,
                                  uint32_t* depth)
{
    uint32_t d = 0;
    int32_t err = kItbFindEnoent;
    while (offset < POM_ITB_INDEX_ENTRIES) {
        const itb_find_slot s = itb_find_slot_at(p, offset);
        if (s.flag == POM_IDX_FREE)
            break;
        if (d == POM_ITB_INDEX_ENTRIES) {
            err = POM_LK_E_LOOP;
            break;
        }
        d++;
        if (!itb_scan_ite_inside(s.entry, n)) {
            err = POM_GC_E_TRUNCATED;
            break;
        }
        if (match(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * s.entry)) {
            *nr = s.entry;
            err = 0;
            break;
        }
        if (s.flag == POM_IDX_UNIQUE)
            break;
        offset = s.conflict;
    }
    *depth = d;
    return err;
}

// (a member function: ITB_SCAN_FN without the CPU build's `static`)
#ifdef __HIPCC__
#define ITB_FIND_MEMBER __device__ __forceinline__
#else
#define ITB_FIND_MEMBER inline
#endif

struct itb_find_lookup_match {
    const pom_lookup_req& q;
    const uint8_t* names;
    ITB_FIND_MEMBER bool operator()(const uint8_t* ite) const { return itb_find_match(ite, q, names); }
};

// ---------------------------------------------------------------------------
// The whole walk for one request (rules 2 ... 8; the caller has dealt with
// req.itb and status).  Returns err; on 0, *nr is the ITE that hit.
// ---------------------------------------------------------------------------
ITB_SCAN_FN int32_t itb_find_one(const uint8_t* p, uint32_t n, uint32_t adepth, const pom_lookup_req& q,
                                 const uint8_t* names, uint32_t names_len, uint32_t* nr, uint32_t* depth)
{
    *nr = *depth = 0;
    if (adepth == 0 || adepth > POM_ITB_ADEPTH_MAX)
        return kItbScanEinval;
    if (n < POM_ITB_ITE_OFF)
        return POM_GC_E_TRUNCATED;
    if (!itb_find_req_ok(q, names_len))
        return kItbScanEinval;
    return itb_find_walk(p, n, (uint32_t)q.hash & ((1u << adepth) - 1u), itb_find_lookup_match{q, names}, nr, depth);
}

// ---------------------------------------------------------------------------
// The record: seventeen little-endian u64
// ---------------------------------------------------------------------------
// Word w of the record built from the ITE at payload + ite_off
// (kItbFindNoIte: a request that did not end in 0, all zeros) with column
// `col` (kItbFindNoColumn: zeros).
ITB_SCAN_FN uint64_t itb_find_word(const uint8_t* payload, uint64_t ite_off, uint32_t col, uint32_t w)
{
    if (ite_off == kItbFindNoIte)
        return 0;
    const uint8_t* ite = payload + ite_off;
    if (w == 0)
        return itb_scan_ld64(ite + POM_ITE_UUID_OFF);
    if (w <= POM_MDU_SIZE / 8)
        return itb_scan_ld64(ite + POM_ITE_MD_OFF + 8u * (w - 1u));
    if (col >= POM_ITE_COLUMNS)
        return 0;
    return itb_scan_ld64(ite + POM_ITE_COLUMN_OFF + POM_COLUMN_SIZE * col + 8u * (w - 1u - POM_MDU_SIZE / 8));
}

ITB_SCAN_FN uint32_t itb_find_column_of(const pom_lookup_req& q)
{
    return (q.flag & POM_LK_COLUMN) ? q.column : kItbFindNoColumn;
}

// One lane writing its own record, byte by byte (out at any alignment).
ITB_SCAN_FN void itb_find_record_bytes(uint8_t* out, const uint8_t* payload, uint64_t ite_off, uint32_t col)
{
    for (uint32_t w = 0; w < kItbFindRecWords; w++) {
        const uint64_t v = itb_find_word(payload, ite_off, col, w);
        for (uint32_t j = 0; j < 8; j++)
            out[8u * w + j] = (uint8_t)(v >> (8u * j));
    }
}

// The wave's copy of its cnt (1 ... 64) consecutive records into a 16-byte
// aligned span: record k is built from the ITE at payload + ite_off[k] and
// col[k].  Granule g is the span's bytes [16g, 16g + 16), two words of one
// record or the last word of one and the first of the next (136 = 8 * 17); a
// lane stores it at once.  The span's last granule is half a granule when cnt
// is odd.  Mem: st16(byte offset, lo, hi), st8(byte offset, v).
ITB_SCAN_FN uint32_t itb_find_granules(uint32_t cnt)
{
    return (cnt * kItbFindRecWords + 1u) >> 1;
}

template <class Mem>
ITB_SCAN_FN void itb_find_granule(const Mem& mem, const uint8_t* payload, const uint64_t* ite_off,
                                  const uint32_t* col, uint32_t cnt, uint32_t g)
{
    const uint32_t w0 = 2u * g, k0 = w0 / kItbFindRecWords, w1 = w0 + 1u, k1 = w1 / kItbFindRecWords;
    const uint64_t lo = itb_find_word(payload, ite_off[k0], col[k0], w0 - k0 * kItbFindRecWords);
    if (k1 >= cnt) {
        mem.st8(16u * g, lo);
        return;
    }
    mem.st16(16u * g, lo, itb_find_word(payload, ite_off[k1], col[k1], w1 - k1 * kItbFindRecWords));
}

#endif
