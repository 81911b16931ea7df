// itb_dents.h -- the directory listing's walk over one decoded ITB payload
// (the FS branch of itb_readdir, mds/itb.c:2536-2589), stated once and built
// on itb_scan.h's bitmap walk.  The kernels of itb_dents.hip walk a payload
// with one wave, 64 bitmap bits a round; itb_dents_one below walks it bit by
// bit.  Both only combine the functions of this header, which is plain C++17
// outside hipcc, where tests/native/itb_dents_host.cc runs it on the CPU --
// the wave's copy plan (itb_dents_granule) included, lane by lane.
//
// The rules for one ITB are include/pom_readdir.h's: itb_scan.h's checks and
// live count first, then
//   a live ITE is emitted iff (flag & 7) == ITE_ACTIVE and !(flag & ITE_FLAG_KV)
//   an emitted ITE with namelen > 256 -> POM_RD_E_NAME and no record at all
//   each emitted nr, ascending, yields [u64 uuid][u16 mode][u16 namelen][u32 0][name]
// No byte at or past n is loaded, and none outside a live ITE except the
// bitmap; p may sit at any byte alignment (every load is itb_scan_ld64 at a
// multiple of 8 from the payload's start: one load when p is 8-byte aligned,
// else byte by byte).
#ifndef POM_ITB_DENTS_H
#define POM_ITB_DENTS_H

#include <stdint.h>

#include "itb_scan.h"
#include "pom_readdir.h"

static_assert(POM_ITE_FLAG_OFF % 8 == 0 && POM_ITE_NAMELEN_OFF == POM_ITE_FLAG_OFF + 4, "one load: flag, namelen");
static_assert(POM_ITE_UUID_OFF % 8 == 0 && POM_ITE_NAME_OFF % 8 == 0 && POM_ITB_ITE_OFF % 8 == 0, "ld64 fields");
static_assert(POM_DENT_HDR == 16 && POM_DENT_MODE_OFF == 8 && POM_DENT_NAMELEN_OFF == 10, "the header as two u64");
static_assert(POM_ITE_NAME_MAX <= 0xFFFFu, "namelen fits the record's u16");

// Sixteen little-endian bytes: byte j is byte j of lo, byte 8 + j byte j of hi.
struct itb_dents_u128 {
    uint64_t lo, hi;
};

constexpr uint32_t kItbDentsRecMax = POM_DENT_HDR + POM_ITE_NAME_MAX;       // 272
// One ITB's records: at most 278,528 bytes.
constexpr uint32_t kItbDentsItbMax = (1u << POM_ITB_ADEPTH_MAX) * kItbDentsRecMax;

ITB_SCAN_FN const uint8_t* itb_dents_ite(const uint8_t* p, uint32_t nr)
{
    return p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr;
}

// flag (low half) and namelen (high half) of ITE nr, which must be inside.
ITB_SCAN_FN uint64_t itb_dents_flag_namelen(const uint8_t* p, uint32_t nr)
{
    return itb_scan_ld64(itb_dents_ite(p, nr) + POM_ITE_FLAG_OFF);
}

// The emit test of mds/itb.c:2569-2574 (ITE_ACTIVE is state 0).
ITB_SCAN_FN bool itb_dents_emits(uint64_t flag_namelen)
{
    const uint32_t flag = (uint32_t)flag_namelen;
    return (flag & POM_ITE_STATE_MASK) == 0 && !(flag & POM_ITE_FLAG_KV);
}

ITB_SCAN_FN uint32_t itb_dents_namelen(uint64_t flag_namelen)
{
    return (uint32_t)(flag_namelen >> 32);
}

// The name-length rule: longer names are POM_RD_E_NAME.
ITB_SCAN_FN bool itb_dents_name_ok(uint32_t namelen)
{
    return namelen <= POM_ITE_NAME_MAX;
}

// The record header of ITE nr (mds/itb.c:2577-2579 in its zeroed buffer).
ITB_SCAN_FN itb_dents_u128 itb_dents_header(const uint8_t* p, uint32_t nr, uint32_t namelen)
{
    const uint8_t* ite = itb_dents_ite(p, nr);
    const uint64_t uuid = itb_scan_ld64(ite + POM_ITE_UUID_OFF);
    const uint64_t w = itb_scan_ld64(ite + (POM_ITE_MODE_OFF & ~7u));
    const uint64_t mode = (w >> (8u * (POM_ITE_MODE_OFF & 7u))) & 0xFFFFu;
    return itb_dents_u128{uuid, mode | (uint64_t)namelen << 8u * (POM_DENT_NAMELEN_OFF - 8u)};
}

ITB_SCAN_FN uint32_t itb_dents_header_namelen(const itb_dents_u128& h)
{
    return (uint32_t)(h.hi >> 8u * (POM_DENT_NAMELEN_OFF - 8u)) & 0xFFFFu;
}

// ---------------------------------------------------------------------------
// Pieces of a record's byte stream, sixteen bytes at a time
// ---------------------------------------------------------------------------
ITB_SCAN_FN uint64_t itb_dents_low_bytes(uint32_t k)        // the low k of eight bytes set
{
    return k >= 8u ? ~0ull : (1ull << (8u * k)) - 1ull;
}

// v with only its bytes [from, to) kept; 0 <= from, to <= 16.
ITB_SCAN_FN itb_dents_u128 itb_dents_keep(itb_dents_u128 v, uint32_t from, uint32_t to)
{
    if (to <= from)
        return itb_dents_u128{0, 0};
    const uint64_t lo = itb_dents_low_bytes(to) & ~itb_dents_low_bytes(from);
    const uint64_t hi = itb_dents_low_bytes(to > 8u ? to - 8u : 0u) & ~itb_dents_low_bytes(from > 8u ? from - 8u : 0u);
    return itb_dents_u128{v.lo & lo, v.hi & hi};
}

// Byte j of the result is byte o + j of v, 0 where v has none; -16 < o < 16.
ITB_SCAN_FN itb_dents_u128 itb_dents_shift(itb_dents_u128 v, int32_t o)
{
    if (o == 0)
        return v;
    const uint32_t s = 8u * (uint32_t)(o > 0 ? o : -o);     // 8 ... 120
    if (o > 0)
        return s >= 64u ? itb_dents_u128{v.hi >> (s - 64u), 0}
                        : itb_dents_u128{v.lo >> s | v.hi << (64u - s), v.hi >> s};
    return s >= 64u ? itb_dents_u128{0, v.lo << (s - 64u)}
                    : itb_dents_u128{v.lo << s, v.hi << s | v.lo >> (64u - s)};
}

// Byte j of the result is name byte q + j of ITE nr where 0 <= q + j < namelen,
// else 0; q >= -15, namelen <= 256.  Three aligned words of the ITE cover any
// sixteen such bytes: they start at or behind ITE byte 88 and end before its
// byte 384, inside the ITE whatever namelen is.
ITB_SCAN_FN itb_dents_u128 itb_dents_name16(const uint8_t* p, uint32_t nr, int32_t q, uint32_t namelen)
{
    const int32_t from = q < 0 ? -q : 0;
    const int32_t to = (int32_t)namelen - q < 16 ? (int32_t)namelen - q : 16;
    if (to <= from)
        return itb_dents_u128{0, 0};
    const uint32_t a = (uint32_t)((int32_t)POM_ITE_NAME_OFF + q);       // within the ITE: 89 ... 359
    const uint8_t* base = itb_dents_ite(p, nr) + (a & ~7u);
    const uint32_t s = 8u * (a & 7u);
    const uint64_t w0 = itb_scan_ld64(base), w1 = itb_scan_ld64(base + 8), w2 = itb_scan_ld64(base + 16);
    const itb_dents_u128 v = s == 0 ? itb_dents_u128{w0, w1}
                                    : itb_dents_u128{w0 >> s | w1 << (64u - s), w1 >> s | w2 << (64u - s)};
    return itb_dents_keep(v, (uint32_t)from, (uint32_t)to);
}

// Sixteen bytes of a record's stream (header, then name) from its byte o on:
// byte j of the result is stream byte o + j, 0 where the record has none.
// -16 < o < 16 + namelen.
ITB_SCAN_FN itb_dents_u128 itb_dents_piece(const itb_dents_u128& hdr, const uint8_t* p, uint32_t nr, int32_t o)
{
    const itb_dents_u128 h = o < (int32_t)POM_DENT_HDR ? itb_dents_shift(hdr, o) : itb_dents_u128{0, 0};
    const itb_dents_u128 n = itb_dents_name16(p, nr, o - (int32_t)POM_DENT_HDR, itb_dents_header_namelen(hdr));
    return itb_dents_u128{h.lo | n.lo, h.hi | n.hi};
}

// ---------------------------------------------------------------------------
// The wave's copy plan for one round of 64 bitmap bits
// ---------------------------------------------------------------------------
// The round's emitted ITEs, compacted in bit order: record k starts at byte
// start[k] of the round's span (start[0] == 0, each record is at least 16
// bytes), is ITE nr[k] and has the header hdr[k].  The span goes to the
// addresses dst ... dst + span; addresses at or past `end` (the output's cap,
// at most dst + span) are not written.
struct itb_dents_round {
    const uint32_t* start;
    const uint32_t* nr;
    const itb_dents_u128* hdr;
    uint32_t cnt, span;
    const uint8_t* p;
    uint64_t dst, end;
};

// The span is cut at the destination's multiples of 16: granule 0 holds dst.
ITB_SCAN_FN uint32_t itb_dents_granules(const itb_dents_round& R)
{
    return (uint32_t)((R.dst + R.span - (R.dst & ~15ull) + 15u) >> 4);
}

// Granule g of the round: a lane finds the one or two records that reach into
// it (records are at least as long as a granule), assembles the sixteen bytes
// from their headers and names and stores them at once; the granules at the
// span's head and tail, and the one the cap cuts, go out byte by byte.
// Mem: st16(address, u128) to a 16-byte aligned address, st1(address, byte).
template <class Mem>
ITB_SCAN_FN void itb_dents_granule(const Mem& mem, const itb_dents_round& R, uint32_t g)
{
    const uint64_t addr = (R.dst & ~15ull) + 16ull * g;
    const int32_t s0 = (int32_t)(int64_t)(addr - R.dst);            // -15 ... span - 1
    const uint32_t s = s0 < 0 ? 0u : (uint32_t)s0;
    uint32_t k = 0;                                                  // the last record that starts at or before s
    for (uint32_t step = 32; step; step >>= 1) {
        const uint32_t t = k + step;
        if (t < R.cnt && R.start[t] <= s)
            k = t;
    }
    itb_dents_u128 v = itb_dents_piece(R.hdr[k], R.p, R.nr[k], s0 - (int32_t)R.start[k]);
    if (k + 1 < R.cnt && (int32_t)R.start[k + 1] < s0 + 16) {
        const itb_dents_u128 u = itb_dents_piece(R.hdr[k + 1], R.p, R.nr[k + 1], s0 - (int32_t)R.start[k + 1]);
        v.lo |= u.lo;
        v.hi |= u.hi;
    }
    if (s0 >= 0 && addr + 16u <= R.end) {
        mem.st16(addr, v);
        return;
    }
    for (uint32_t j = 0; j < 16; j++) {
        const uint64_t a = addr + j;
        if (a >= R.dst && a < R.end)
            mem.st1(a, (uint8_t)((j < 8 ? v.lo >> 8u * j : v.hi >> 8u * (j - 8u)) & 0xFFu));
    }
}

// ---------------------------------------------------------------------------
// The whole walk, one bit at a time: records to out[0, cap) (the byte count
// goes on past cap).  Returns the ITB's err.
// ---------------------------------------------------------------------------
ITB_SCAN_FN int32_t itb_dents_one(const uint8_t* p, uint32_t n, uint32_t adepth, uint8_t* out, uint64_t cap,
                                  uint32_t* live, uint32_t* dnum, uint32_t* bytes)
{
    *live = *dnum = *bytes = 0;
    int32_t err = itb_scan_precheck(n, adepth);
    if (err == 0)
        err = itb_scan_live(p, n, adepth, live);
    if (err != 0)
        return err;
    const uint32_t rounds = itb_scan_rounds(adepth);
    // all or nothing: the names are checked before a byte is written
    for (uint32_t r = 0; r < rounds; r++)
        for (uint64_t w = itb_scan_word(p, r, adepth); w; w &= w - 1) {
            const uint64_t fn = itb_dents_flag_namelen(p, 64u * r + (uint32_t)__builtin_ctzll(w));
            if (itb_dents_emits(fn) && !itb_dents_name_ok(itb_dents_namelen(fn)))
                return POM_RD_E_NAME;
        }
    uint32_t k = 0;
    uint64_t at = 0;
    for (uint32_t r = 0; r < rounds; r++)
        for (uint64_t w = itb_scan_word(p, r, adepth); w; w &= w - 1) {
            const uint32_t nr = 64u * r + (uint32_t)__builtin_ctzll(w);
            const uint64_t fn = itb_dents_flag_namelen(p, nr);
            if (!itb_dents_emits(fn))
                continue;
            const uint32_t namelen = itb_dents_namelen(fn);
            const itb_dents_u128 h = itb_dents_header(p, nr, namelen);
            const uint8_t* name = itb_dents_ite(p, nr) + POM_ITE_NAME_OFF;
            for (uint32_t j = 0; j < POM_DENT_HDR + namelen; j++, at++)
                if (at < cap)
                    out[at] = j < 8                ? (uint8_t)(h.lo >> 8u * j)
                              : j < POM_DENT_HDR ? (uint8_t)(h.hi >> 8u * (j - 8u))
                                                 : name[j - POM_DENT_HDR];
            k++;
        }
    *dnum = k;
    *bytes = (uint32_t)at;
    return 0;
}

#endif
