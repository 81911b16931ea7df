// itb_kvget.h -- the key/value point get over one decoded ITB payload (the
// INDEX_KV branches of ite_match, mds/itb.c:1095-1116, and of the lookup's
// copy, :1808-1810 with __data_column_hook :1650-1661, and the reply of
// mds/cbht.c:929-977), stated once: the rules and the plan by which a wave
// copies its packed, variable-length records.  Built on itb_scan.h's payload
// checks and loader and on itb_find.h's index table and chain walk.  The
// kernels of itb_kvget.hip only combine the functions of this header, which is
// plain C++17 outside hipcc, where tests/native/itb_kvget_host.cc runs it on
// the CPU.
//
// The rules for one request are include/pom_kvget.h's.  No byte at or past the
// payload's n is loaded and none outside [0, keys_len) of the key blob; p, the
// blob and out may sit at any byte alignment: every payload load is
// itb_scan_ld64 at a multiple of 8 from the payload's start.
#ifndef POM_ITB_KVGET_H
#define POM_ITB_KVGET_H

#include <stdint.h>

#include "itb_find.h"
#include "pom_kvget.h"

static_assert(sizeof(pom_kvget_req) == 32 && alignof(pom_kvget_req) == 8, "the request as four u64");
static_assert(POM_KV_FLAGS_OFF == POM_ITE_MD_OFF && POM_KV_FLAGS_OFF % 8 == 0, "the record starts at an ITE word");
static_assert(POM_KV_KEY_OFF % 8 == 0 && POM_KV_KLEN_OFF % 8 == 0 && POM_KV_VALUE_OFF == POM_KV_KLEN_OFF + 4,
              "klen and v.value[0 ... 3] share a word");
static_assert(POM_KV_VALUE_OFF + POM_KV_VALUE_MAX <= POM_ITE_COLUMN_OFF, "v.value in front of the columns");
static_assert(POM_KV_VALUE_OFF - POM_KV_FLAGS_OFF == POM_KV_HEADER_LEN, "KV_HEADER_LEN");
static_assert(POM_KG_REC_MAX == POM_KV_HEADER_LEN + POM_KV_VALUE_MAX + POM_COLUMN_SIZE, "header, value, column");
static_assert(POM_KG_LEASE_OFF % 8 == 0 && POM_KG_LEASE_OFF == POM_ITE_MD_OFF + POM_MDU_DTIME_OFF, "mdu.dtime");
static_assert(POM_ITE_COLUMN_OFF % 8 == 0 && POM_COLUMN_SIZE % 8 == 0, "ld64 columns");
// every source piece of a record is longer than a granule: a granule holds bytes of at most two pieces
static_assert(POM_KV_HEADER_LEN > 16 && POM_COLUMN_SIZE > 16, "a granule meets at most two pieces");

constexpr uint32_t kItbKvgetFlags = POM_KG_LOOKUP | POM_KG_COLUMN | POM_KG_KV;
constexpr uint32_t kItbKvgetNoColumn = 0;       // a piece offset no column has
constexpr uint32_t kItbKvgetWave = 64;          // requests whose records one wave copies

// ---------------------------------------------------------------------------
// The request's own checks (rule 4) and the match (rule 6)
// ---------------------------------------------------------------------------
ITB_SCAN_FN bool itb_kvget_is_str(const pom_kvget_req& q)
{
    return (q.kvflag & POM_KV_STR) != 0;
}

ITB_SCAN_FN bool itb_kvget_req_ok(const pom_kvget_req& q, uint32_t keys_len)
{
    return !(q.flag & ~kItbKvgetFlags) && !(q.kvflag & ~POM_KG_KVFLAG_MASK) &&
           !((q.flag & POM_KG_COLUMN) && (q.kvflag & POM_KG_MAX_COLUMN) >= POM_ITE_COLUMNS) &&
           !(itb_kvget_is_str(q) && q.sklen <= POM_KV_VALUE_MAX && (uint64_t)q.skey_off + q.sklen > keys_len);
}

// memcmp(hi->data, e->v.value, sklen) == 0 for sklen <= 320.  The ITE's side
// is whole aligned words: v.value starts in the upper half of klen's word,
// then eight bytes a step; the blob's side is read as itb_find_name_bytes
// reads names.
ITB_SCAN_FN bool itb_kvget_skey_eq(const uint8_t* ite, const uint8_t* skey, uint32_t sklen)
{
    if (sklen == 0)
        return true;
    const uint32_t k0 = sklen < 4u ? sklen : 4u;
    const uint64_t head = itb_scan_ld64(ite + POM_KV_KLEN_OFF) >> 32;
    if ((head & ((1ull << (8u * k0)) - 1ull)) != itb_find_name_bytes(skey, k0))
        return false;
    for (uint32_t i = 4; i < sklen; i += 8) {
        const uint32_t k = sklen - i < 8u ? sklen - i : 8u;
        const uint64_t keep = k >= 8u ? ~0ull : (1ull << (8u * k)) - 1ull;
        if ((itb_scan_ld64(ite + POM_KV_VALUE_OFF + i) & keep) != itb_find_name_bytes(skey + i, k))
            return false;
    }
    return true;
}

// ite_match's INDEX_KV branch on an ITE that lies inside the payload.
struct itb_kvget_match {
    const pom_kvget_req& q;
    const uint8_t* keys;
    ITB_FIND_MEMBER bool operator()(const uint8_t* ite) const
    {
        if (itb_scan_ld64(ite + POM_KV_KEY_OFF) != q.key)
            return false;
        if (!itb_kvget_is_str(q))
            return true;
        if (q.sklen > POM_KV_VALUE_MAX || (uint32_t)itb_scan_ld64(ite + POM_KV_KLEN_OFF) != q.sklen)
            return false;
        return itb_kvget_skey_eq(ite, keys + q.skey_off, q.sklen);
    }
};

// ---------------------------------------------------------------------------
// The whole get for one request (rules 2 ... 7; the caller has dealt with
// req.itb and status).  Returns err; on 0, *nr is the ITE that hit, *len the
// record's length and *lease the ITE's bytes 80 ... 87.
// ---------------------------------------------------------------------------
ITB_SCAN_FN uint32_t itb_kvget_column_bytes(const pom_kvget_req& q)
{
    return (q.flag & POM_KG_COLUMN) ? POM_COLUMN_SIZE : 0u;
}

ITB_SCAN_FN int32_t itb_kvget_one(const uint8_t* p, uint32_t n, uint32_t adepth, const pom_kvget_req& q,
                                  const uint8_t* keys, uint32_t keys_len, uint32_t* nr, uint32_t* depth,
                                  uint32_t* len, uint64_t* lease)
{
    *nr = *depth = *len = 0;
    *lease = 0;
    if (adepth == 0 || adepth > POM_ITB_ADEPTH_MAX)
        return kItbScanEinval;
    if (n < POM_ITB_ITE_OFF)
        return POM_GC_E_TRUNCATED;
    if (!itb_kvget_req_ok(q, keys_len))
        return kItbScanEinval;
    uint32_t hit = 0;
    const int32_t err =
        itb_find_walk(p, n, (uint32_t)q.key & ((1u << adepth) - 1u), itb_kvget_match{q, keys}, &hit, depth);
    if (err != 0)
        return err;
    const uint8_t* ite = p + POM_ITB_ITE_OFF + POM_ITE_SIZE * hit;
    const uint64_t fl = itb_scan_ld64(ite + POM_KV_FLAGS_OFF);      // v.flags, v.len
    if (!((uint32_t)fl & (POM_KV_NORMAL | POM_KV_STR)))
        return kItbScanEinval;
    const uint32_t vlen = (uint32_t)(fl >> 32);
    if (vlen > POM_KV_VALUE_MAX)
        return POM_KG_E_VALUE;
    *nr = hit;
    *len = POM_KV_HEADER_LEN + vlen + itb_kvget_column_bytes(q);
    *lease = itb_scan_ld64(ite + POM_KG_LEASE_OFF);
    return 0;
}

// ---------------------------------------------------------------------------
// The record's sources: two pieces of the hit's ITE
// ---------------------------------------------------------------------------
// Where a request's record comes from: kv bytes from ITE byte 24, then 24
// bytes from ITE byte col_off when the request asked for a column.  A request
// that did not end in 0 has len 0 and no piece.
struct itb_kvget_src {
    uint64_t ite_off;       // the ITE's byte offset from `payload`
    uint32_t kv;            // KV_HEADER_LEN + v.len, or 0
    uint32_t col_off;       // ITE byte of the column, or kItbKvgetNoColumn
};

ITB_SCAN_FN itb_kvget_src itb_kvget_src_of(const pom_kvget_req& q, uint64_t payload_off, uint32_t nr, uint32_t len)
{
    if (len == 0)
        return itb_kvget_src{0, 0, kItbKvgetNoColumn};
    const uint32_t cb = itb_kvget_column_bytes(q);
    return itb_kvget_src{payload_off + POM_ITB_ITE_OFF + (uint64_t)POM_ITE_SIZE * nr, len - cb,
                         cb ? POM_ITE_COLUMN_OFF + POM_COLUMN_SIZE * (q.kvflag & POM_KG_MAX_COLUMN)
                            : kItbKvgetNoColumn};
}

// One lane writing its own record byte by byte to out + start ..., below cap.
// Mem: st1(byte offset of out, value).
template <class Mem>
ITB_SCAN_FN void itb_kvget_record_bytes(const Mem& mem, uint64_t start, uint64_t cap, const uint8_t* payload,
                                        const itb_kvget_src& s)
{
    const uint8_t* ite = payload + s.ite_off;
    for (uint32_t i = 0; i < s.kv && i < POM_KV_HEADER_LEN + POM_KV_VALUE_MAX; i += 8) {
        const uint64_t v = itb_scan_ld64(ite + POM_KV_FLAGS_OFF + i);
        for (uint32_t j = 0; j < 8 && i + j < s.kv; j++)
            if (start + i + j < cap)
                mem.st1(start + i + j, (uint8_t)(v >> (8u * j)));
    }
    if (s.col_off == kItbKvgetNoColumn)
        return;
    for (uint32_t i = 0; i < POM_COLUMN_SIZE; i += 8) {
        const uint64_t v = itb_scan_ld64(ite + s.col_off + i);
        for (uint32_t j = 0; j < 8; j++)
            if (start + s.kv + i + j < cap)
                mem.st1(start + s.kv + i + j, (uint8_t)(v >> (8u * j)));
    }
}

// ---------------------------------------------------------------------------
// The wave's copy of its cnt (1 ... 64) consecutive records
// ---------------------------------------------------------------------------
// The records are the bytes [lo, hi) of out; rel[k] = record k's start - lo
// (rel[cnt] is not needed: a record's end is its pieces' end).  The span is
// cut into granules of 16 bytes at 16-byte aligned ADDRESSES: with mis = out's
// address mod 16, granule g covers the addresses mis + offset in
// [a0 + 16g, a0 + 16g + 16), a0 = (mis + lo) & ~15.
struct itb_kvget_piece {
    uint64_t ite_off;       // the ITE's byte offset from `payload`
    uint32_t at;            // the ITE byte asked for
    uint32_t left;          // bytes of the piece from there on
};

// The record that holds byte x (below hi - lo) of the span: the last whose
// start is at or before x.  A zero-length record shares its start with the
// record behind it (or with the span's end), so it never owns a byte.
ITB_SCAN_FN uint32_t itb_kvget_owner(const uint32_t* rel, uint32_t cnt, uint32_t x)
{
    uint32_t k = 0;
    for (uint32_t step = kItbKvgetWave / 2; step; step >>= 1)
        if (k + step < cnt && rel[k + step] <= x)
            k += step;
    return k;
}

ITB_SCAN_FN itb_kvget_piece itb_kvget_locate(const uint32_t* rel, const itb_kvget_src* src, uint32_t cnt, uint32_t x)
{
    const uint32_t k = itb_kvget_owner(rel, cnt, x);
    const uint32_t o = x - rel[k];
    const itb_kvget_src s = src[k];
    if (o < s.kv)
        return itb_kvget_piece{s.ite_off, POM_KV_FLAGS_OFF + o, s.kv - o};
    if (s.col_off == kItbKvgetNoColumn || o - s.kv >= POM_COLUMN_SIZE)
        return itb_kvget_piece{s.ite_off, 0, 0};
    return itb_kvget_piece{s.ite_off, s.col_off + (o - s.kv), POM_COLUMN_SIZE - (o - s.kv)};
}

struct itb_kvget_u128 {
    uint64_t lo, hi;
};

// take (1 ... 16) bytes from ITE byte p.at on into the low bytes of 128 bits,
// the rest zero: up to three aligned words of the ITE, each holding a byte
// that was asked for (so none leaves the ITE, which is a multiple of 8 from
// the payload's start).
ITB_SCAN_FN itb_kvget_u128 itb_kvget_gather(const uint8_t* payload, const itb_kvget_piece& p, uint32_t take)
{
    const uint32_t r = p.at & 7u, sh = 8u * r;
    const uint8_t* a = payload + p.ite_off + (p.at - r);
    const uint64_t w0 = itb_scan_ld64(a);
    const uint64_t w1 = r + take > 8u ? itb_scan_ld64(a + 8) : 0;
    const uint64_t w2 = r + take > 16u ? itb_scan_ld64(a + 16) : 0;
    itb_kvget_u128 v;
    v.lo = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0;
    v.hi = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1;
    if (take < 8u) {
        v.lo &= (1ull << (8u * take)) - 1ull;
        v.hi = 0;
    } else if (take < 16u) {
        v.hi &= take == 8u ? 0ull : (1ull << (8u * (take - 8u))) - 1ull;
    }
    return v;
}

// v's bytes moved up by `by` (0 ... 15) bytes.
ITB_SCAN_FN itb_kvget_u128 itb_kvget_shl(itb_kvget_u128 v, uint32_t by)
{
    const uint32_t sh = 8u * (by & 7u);
    if (by >= 8u)
        return itb_kvget_u128{0, v.lo << sh};
    return itb_kvget_u128{v.lo << sh, sh ? (v.hi << sh) | (v.lo >> (64u - sh)) : v.hi};
}

ITB_SCAN_FN uint32_t itb_kvget_granules(uint32_t mis, uint64_t lo, uint64_t hi)
{
    if (hi <= lo)
        return 0;
    const uint64_t a0 = (mis + lo) & ~15ull;
    return (uint32_t)((mis + hi - a0 + 15u) >> 4);
}

// Granule g of the wave's span, written below cap.  Mem: st16(byte offset of
// out -- a 16-byte aligned address --, lo, hi) and st1(byte offset, value).
// Byte stores appear only in the span's first and last granule and where the
// cap cuts.
template <class Mem>
ITB_SCAN_FN void itb_kvget_granule(const Mem& mem, const uint8_t* payload, const uint32_t* rel,
                                   const itb_kvget_src* src, uint32_t cnt, uint32_t mis, uint64_t lo, uint64_t hi,
                                   uint64_t cap, uint32_t g)
{
    const uint64_t end = hi < cap ? hi : cap;
    const uint64_t ga = ((mis + lo) & ~15ull) + 16ull * g;          // the granule's address, mis-relative
    const uint64_t a = ga > mis + lo ? ga : mis + lo;
    const uint64_t b = ga + 16u < mis + end ? ga + 16u : mis + end;
    if (a >= b)
        return;
    const uint32_t want = (uint32_t)(b - a);                        // 1 ... 16
    const uint32_t x = (uint32_t)(a - mis - lo);
    const itb_kvget_piece p0 = itb_kvget_locate(rel, src, cnt, x);
    const uint32_t n0 = p0.left < want ? p0.left : want;
    if (n0 == 0)                                                    // (a table that names no source for x)
        return;
    itb_kvget_u128 v = itb_kvget_gather(payload, p0, n0);
    if (n0 < want) {
        // (the next piece is longer than a granule: it holds all the rest)
        const itb_kvget_piece p1 = itb_kvget_locate(rel, src, cnt, x + n0);
        if (p1.left < want - n0)
            return;
        const itb_kvget_u128 u = itb_kvget_shl(itb_kvget_gather(payload, p1, want - n0), n0);
        v.lo |= u.lo;
        v.hi |= u.hi;
    }
    if (want == 16u) {
        mem.st16(a - mis, v.lo, v.hi);
        return;
    }
    for (uint32_t i = 0; i < want; i++)
        mem.st1(a - mis + i, (uint8_t)((i < 8u ? v.lo >> (8u * i) : v.hi >> (8u * (i - 8u)))));
}

#endif
