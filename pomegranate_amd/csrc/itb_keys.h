// itb_keys.h -- the key/value table listing's walk over one decoded ITB
// payload (the INDEX_KV branch of itb_readdir, mds/itb.c:2472-2534, with
// __readdir_filter, :2422-2458), stated once and built on itb_scan.h's bitmap
// walk.  The kernels of itb_keys.hip walk a payload with one wave, 64 bitmap
// bits a round; itb_keys_one below walks it bit by bit.  Both only combine
// the functions of this header, which is plain C++17 outside hipcc, where
// tests/native/itb_keys_host.cc runs it on the CPU -- the wave's copy plan
// (itb_keys_granule) included, lane by lane.
//
// The rules for one ITB are include/pom_kvlist.h's: itb_scan.h's checks and
// live count first, then for every live ITE
//   kind     NORMAL if v.flags & 0x8000, else STR if v.flags & 0x4000, else NAME
//   key      NORMAL: "%ld" of v.key; STR: v.klen bytes of v.value; NAME: namelen bytes of s.name
//   errors   STR with klen > 320 -> POM_KV_E_KEY, NAME with namelen > 256 -> POM_RD_E_NAME (KEY wins)
//   filter   op 2, 3: NORMAL and STR entries only where the needle occurs in the value
//   record   [u32 keylen][key]
// No byte at or past n is loaded, and none outside a live ITE except the
// bitmap; p may sit at any byte alignment (every load is itb_scan_ld64 at a
// multiple of 8 from the payload's start).  The search reads ITE bytes 40 ...
// 367 at the most.
#ifndef POM_ITB_KEYS_H
#define POM_ITB_KEYS_H

#include <stdint.h>

#include "itb_dents.h"
#include "itb_scan.h"
#include "pom_kvlist.h"

static_assert(POM_KV_FLAGS_OFF % 8 == 0 && POM_KV_KEY_OFF % 8 == 0 && POM_KV_KLEN_OFF % 8 == 0, "ld64 fields");
static_assert(POM_KV_VALUE_OFF == POM_KV_KLEN_OFF + 4, "the value starts four bytes into an aligned word");
static_assert(POM_KV_VALUE_OFF + POM_KV_VALUE_MAX == 364 && POM_KV_VALUE_OFF + POM_KV_VALUE_MAX <= POM_ITE_COLUMN_OFF,
              "the value ends before the columns");
static_assert(POM_KV_FLAGS_OFF + POM_KV_HEADER_LEN == POM_KV_VALUE_OFF && POM_KV_FLAGS_OFF + POM_KV_SIZE == 368, "struct kv");

enum : uint32_t { kItbKeysNormal = 0, kItbKeysStr = 1, kItbKeysName = 2 };

constexpr uint32_t kItbKeysValueEnd = POM_KV_VALUE_OFF + POM_KV_VALUE_MAX;      // ITE byte 364
constexpr uint32_t kItbKeysRecMax = 4u + POM_KV_VALUE_MAX;                       // 324
// One ITB's records: at most 331,776 bytes.
constexpr uint32_t kItbKeysItbMax = (1u << POM_ITB_ADEPTH_MAX) * kItbKeysRecMax;
constexpr uint32_t kItbKeysHeadMax = 4u + POM_KV_TEXT_MAX;                       // 24: a NORMAL record

// The kind test of mds/itb.c:2485-2494.
ITB_SCAN_FN uint32_t itb_keys_kind(uint32_t vflags)
{
    return vflags & POM_KV_NORMAL ? kItbKeysNormal : vflags & POM_KV_STR ? kItbKeysStr : kItbKeysName;
}

// ---------------------------------------------------------------------------
// "%ld": the decimal text of a key, without a 64-bit divide by a variable
// ---------------------------------------------------------------------------
// |key| as u64 (INT64_MIN included).
ITB_SCAN_FN uint64_t itb_keys_magnitude(uint64_t key)
{
    return (int64_t)key < 0 ? 0ull - key : key;
}

// Decimal digits of mag: 1 ... 20.
ITB_SCAN_FN uint32_t itb_keys_digits(uint64_t mag)
{
    uint32_t d = 1;
    uint64_t t = 10;                                // 10^d; 10^19 is the last power that fits
    while (d < 20u && mag >= t) {
        d++;
        if (d < 20u)
            t *= 10u;
    }
    return d;
}

// The length of the text: digits and the sign.
ITB_SCAN_FN uint32_t itb_keys_text_len(uint64_t key)
{
    return itb_keys_digits(itb_keys_magnitude(key)) + ((int64_t)key < 0 ? 1u : 0u);
}

// The first bytes of a record's stream, those that do not come from the ITE:
// byte j of the stream is byte j of w0, w1, w2 (little-endian, 24 bytes), for
// j < len.  STR and NAME records: the length word; NORMAL: that and the text.
struct itb_keys_head {
    uint64_t w0, w1, w2;
    uint32_t len;
};

// One more byte in front of the 20 text bytes held in {a0, a1, a2's low half}.
ITB_SCAN_FN void itb_keys_push_front(uint64_t& a0, uint64_t& a1, uint64_t& a2, uint32_t c)
{
    a2 = a2 << 8 | a1 >> 56;
    a1 = a1 << 8 | a0 >> 56;
    a0 = a0 << 8 | c;
}

ITB_SCAN_FN itb_keys_head itb_keys_head_normal(uint64_t key)
{
    const uint64_t mag = itb_keys_magnitude(key);
    const uint32_t nd = itb_keys_digits(mag);
    // three parts of at most nine digits: divides by constants only
    const uint64_t q1 = mag / 1000000000ull;
    const uint32_t q2 = (uint32_t)(q1 / 1000000000ull);
    const uint32_t r0 = (uint32_t)(mag - q1 * 1000000000ull), r1 = (uint32_t)(q1 - (uint64_t)q2 * 1000000000ull);
    uint64_t a0 = 0, a1 = 0, a2 = 0;
    uint32_t cur = r0;
    for (uint32_t i = 0; i < 20u; i++) {            // least significant digit first, each in front of the last
        if (i >= nd)
            break;
        if (i == 9u)
            cur = r1;
        if (i == 18u)
            cur = q2;
        const uint32_t next = cur / 10u;
        itb_keys_push_front(a0, a1, a2, '0' + (cur - 10u * next));
        cur = next;
    }
    uint32_t len = nd;
    if ((int64_t)key < 0) {
        itb_keys_push_front(a0, a1, a2, '-');
        len++;
    }
    // the length word in front of the text
    return itb_keys_head{a0 << 32 | len, a1 << 32 | a0 >> 32, a2 << 32 | a1 >> 32, 4u + len};
}

ITB_SCAN_FN itb_keys_head itb_keys_head_len(uint32_t keylen)
{
    return itb_keys_head{keylen, 0, 0, 4u};
}

ITB_SCAN_FN uint8_t itb_keys_head_byte(const itb_keys_head& h, uint32_t j)      // j < 24
{
    return (uint8_t)((j < 8u ? h.w0 >> 8u * j : j < 16u ? h.w1 >> 8u * (j - 8u) : h.w2 >> 8u * (j - 16u)) & 0xFFu);
}

// ---------------------------------------------------------------------------
// One live entry
// ---------------------------------------------------------------------------
// kind; keylen (0 when bad); bad: 0, POM_KV_E_KEY or POM_RD_E_NAME; klen as
// stored (STR); the stream's head; the ITE byte the key's bytes start at
// (STR, NAME; NORMAL has none: memlen 0).
struct itb_keys_entry {
    uint32_t kind, keylen, klen, memoff, memlen;
    int32_t bad;
    itb_keys_head head;
};

// ITE nr must be inside the payload.  kWithHead: also the record's head
// (the count kernel needs lengths alone).
template <bool kWithHead>
ITB_SCAN_FN itb_keys_entry itb_keys_load(const uint8_t* p, uint32_t nr)
{
    const uint8_t* ite = itb_dents_ite(p, nr);
    itb_keys_entry e{};
    e.kind = itb_keys_kind((uint32_t)itb_scan_ld64(ite + POM_KV_FLAGS_OFF));
    if (e.kind == kItbKeysNormal) {
        const uint64_t key = itb_scan_ld64(ite + POM_KV_KEY_OFF);
        e.keylen = itb_keys_text_len(key);
        if (kWithHead)
            e.head = itb_keys_head_normal(key);
    } else if (e.kind == kItbKeysStr) {
        e.klen = (uint32_t)itb_scan_ld64(ite + POM_KV_KLEN_OFF);
        e.bad = e.klen > POM_KV_VALUE_MAX ? POM_KV_E_KEY : 0;
        e.keylen = e.memlen = e.bad ? 0u : e.klen;
        e.memoff = POM_KV_VALUE_OFF;
    } else {
        const uint32_t namelen = itb_dents_namelen(itb_dents_flag_namelen(p, nr));
        e.bad = itb_dents_name_ok(namelen) ? 0 : POM_RD_E_NAME;
        e.keylen = e.memlen = e.bad ? 0u : namelen;
        e.memoff = POM_ITE_NAME_OFF;
    }
    if (kWithHead && e.kind != kItbKeysNormal)
        e.head = itb_keys_head_len(e.keylen);
    return e;
}

// ---------------------------------------------------------------------------
// The filter: the needle in the value
// ---------------------------------------------------------------------------
// The needle's effective length: its bytes up to the first zero byte.
ITB_SCAN_FN uint32_t itb_keys_needle_len(const uint8_t* needle, uint32_t needle_len)
{
    uint32_t m = 0;
    while (m < needle_len && needle[m] != 0)
        m++;
    return m;
}

// The failure table of the linear search: fail[i] = the length of the longest
// proper prefix of needle[0, i] that is also its suffix.  k falls with every
// step of the inner loop and rises by one a step of the outer: 2m steps.
ITB_SCAN_FN void itb_keys_failure(const uint8_t* needle, uint32_t m, uint8_t* fail)
{
    uint32_t k = 0;
    if (m)
        fail[0] = 0;
    for (uint32_t i = 1; i < m; i++) {
        while (k > 0 && needle[i] != needle[k])
            k = fail[k - 1];
        if (needle[i] == needle[k])
            k++;
        fail[i] = (uint8_t)k;
    }
}

// ITE bytes through aligned 8-byte words, the last word kept.
struct itb_keys_cursor {
    const uint8_t* ite;
    uint32_t wi;
    uint64_t w;
};

ITB_SCAN_FN uint32_t itb_keys_byte(itb_keys_cursor& c, uint32_t i)             // ITE byte i
{
    if ((i >> 3) != c.wi) {
        c.wi = i >> 3;
        c.w = itb_scan_ld64(c.ite + 8u * c.wi);
    }
    return (uint32_t)(c.w >> 8u * (i & 7u)) & 0xFFu;
}

// Where the haystack starts: ITE byte 44 for NORMAL, 44 + klen for STR
// (klen <= 320, so at most 364: empty).
ITB_SCAN_FN uint32_t itb_keys_hay_start(const itb_keys_entry& e)
{
    return POM_KV_VALUE_OFF + (e.kind == kItbKeysStr ? e.klen : 0u);
}

// strstr(ITE bytes from `from` to the first zero byte or to byte 364, needle[0, m)) != NULL;
// needle[0, m) holds no zero byte, fail is its failure table (kLinear only).
// kLinear: one pass over the value, at most 320 + 320 steps.  Else the plain
// search with a first-byte skip: at most (321 - m) * m byte compares.
template <bool kLinear>
ITB_SCAN_FN bool itb_keys_match(const uint8_t* ite, uint32_t from, const uint8_t* needle, uint32_t m,
                                const uint8_t* fail)
{
    if (m == 0)
        return true;
    itb_keys_cursor c{ite, ~0u, 0};
    if (kLinear) {
        const uint32_t n0 = needle[0];
        uint32_t k = 0;
        for (uint32_t i = from; i < kItbKeysValueEnd; i++) {
            const uint32_t b = itb_keys_byte(c, i);
            if (b == 0)
                return false;
            if (k == 0 && b != n0)                  // most bytes: no look at the tables
                continue;
            while (k > 0 && b != needle[k])         // k falls with every step, and rises by one a byte
                k = fail[k - 1];
            if (b == needle[k])
                k++;
            if (k == m)
                return true;
        }
        return false;
    }
    itb_keys_cursor d{ite, ~0u, 0};
    const uint32_t n0 = needle[0];
    for (uint32_t i = from; i + m <= kItbKeysValueEnd; i++) {
        const uint32_t b = itb_keys_byte(c, i);
        if (b == 0)
            return false;
        if (b != n0)
            continue;
        uint32_t j = 1;                             // a zero byte of the value equals no needle byte
        while (j < m && itb_keys_byte(d, i + j) == needle[j])
            j++;
        if (j == m)
            return true;
    }
    return false;
}

// The filter of mds/itb.c:2510-2530 for an entry that is not bad.
template <bool kLinear>
ITB_SCAN_FN bool itb_keys_emits(const uint8_t* p, uint32_t nr, const itb_keys_entry& e, uint32_t op,
                                const uint8_t* needle, uint32_t m, const uint8_t* fail)
{
    if (op < POM_KV_OP_GREP || e.kind == kItbKeysName)
        return true;
    return itb_keys_match<kLinear>(itb_dents_ite(p, nr), itb_keys_hay_start(e), needle, m, fail);
}

// ---------------------------------------------------------------------------
// Pieces of a record's byte stream, sixteen bytes at a time
// ---------------------------------------------------------------------------
// Byte j of the result is byte o + j of the head, 0 where it has none; o > -16.
ITB_SCAN_FN itb_dents_u128 itb_keys_head16(const itb_keys_head& h, int32_t o)
{
    itb_dents_u128 v{0, 0};
    if (o < 16)
        v = itb_dents_shift(itb_dents_u128{h.w0, h.w1}, o);
    if (o > 0 && o < (int32_t)kItbKeysHeadMax) {
        const itb_dents_u128 u = itb_dents_shift(itb_dents_u128{h.w2, 0}, o - 16);
        v.lo |= u.lo;
        v.hi |= u.hi;
    }
    return v;
}

// Byte j of the result is value byte q + j of ITE nr where 0 <= q + j < klen,
// else 0; klen <= 320.  Three aligned words of the ITE cover any sixteen such
// bytes: they start at or behind ITE byte 24 and end before its byte 384.
ITB_SCAN_FN itb_dents_u128 itb_keys_value16(const uint8_t* p, uint32_t nr, int32_t q, uint32_t klen)
{
    const int32_t from = q < 0 ? -q : 0;
    const int32_t to = (int32_t)klen - q < 16 ? (int32_t)klen - q : 16;
    if (to <= from)
        return itb_dents_u128{0, 0};
    const uint32_t a = (uint32_t)((int32_t)POM_KV_VALUE_OFF + q);       // within the ITE: 29 ... 363
    const uint8_t* base = itb_dents_ite(p, nr) + (a & ~7u);
    const uint32_t s = 8u * (a & 7u);
    const uint64_t w0 = itb_scan_ld64(base), w1 = itb_scan_ld64(base + 8), w2 = itb_scan_ld64(base + 16);
    const itb_dents_u128 v = s == 0 ? itb_dents_u128{w0, w1}
                                    : itb_dents_u128{w0 >> s | w1 << (64u - s), w1 >> s | w2 << (64u - s)};
    return itb_dents_keep(v, (uint32_t)from, (uint32_t)to);
}

// What the copy plan keeps of a record besides its head: where its key bytes
// come from.  meta = memlen | name << 16.
ITB_SCAN_FN uint32_t itb_keys_meta(const itb_keys_entry& e)
{
    return e.memlen | (e.kind == kItbKeysName ? 1u << 16 : 0u);
}

// Sixteen bytes of a record's stream (head, then key bytes from the ITE) from
// its byte o on; o > -16.
ITB_SCAN_FN itb_dents_u128 itb_keys_piece(const itb_keys_head& h, uint32_t meta, const uint8_t* p, uint32_t nr, int32_t o)
{
    itb_dents_u128 v = itb_keys_head16(h, o);
    const uint32_t memlen = meta & 0xFFFFu;
    if (memlen) {
        const int32_t q = o - (int32_t)h.len;
        const itb_dents_u128 u = meta >> 16 ? itb_dents_name16(p, nr, q, memlen) : itb_keys_value16(p, nr, q, memlen);
        v.lo |= u.lo;
        v.hi |= u.hi;
    }
    return v;
}

// ---------------------------------------------------------------------------
// The wave's copy plan for one round of 64 bitmap bits
// ---------------------------------------------------------------------------
// The round's emitted entries, compacted in bit order: record k starts at byte
// start[k] of the round's span (start[0] == 0, each record is at least 4
// bytes), is ITE nr[k], has the head {w0[k], w1[k], w2[k]} of hlen[k] bytes
// and the key bytes meta[k] names.  The span goes to the addresses dst ...
// dst + span; addresses at or past `end` (the output's cap, at most dst +
// span) are not written.
struct itb_keys_round {
    const uint64_t *w0, *w1, *w2;
    const uint32_t *start, *nr, *meta;
    const uint8_t* hlen;
    uint32_t cnt, span;
    const uint8_t* p;
    uint64_t dst, end;
};

ITB_SCAN_FN uint32_t itb_keys_granules(const itb_keys_round& R)
{
    return (uint32_t)((R.dst + R.span - (R.dst & ~15ull) + 15u) >> 4);
}

// Granule g of the round (the span cut at the destination's multiples of 16;
// granule 0 holds dst): a lane finds the records that reach into it -- the one
// that holds its first byte and at most four that start inside, records being
// at least 4 bytes -- assembles the sixteen bytes and stores them at once; the
// granules at the span's head and tail, and the one the cap cuts, go out byte
// by byte.  Mem: st16(address, u128) to a 16-byte aligned address,
// st1(address, byte).
template <class Mem>
ITB_SCAN_FN void itb_keys_granule(const Mem& mem, const itb_keys_round& R, uint32_t g)
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
    itb_dents_u128 v{0, 0};
    for (uint32_t i = 0; i < 5u; i++) {
        const uint32_t t = k + i;
        if (t >= R.cnt || (i && (int32_t)R.start[t] >= s0 + 16))
            break;
        const itb_keys_head h{R.w0[t], R.w1[t], R.w2[t], R.hlen[t]};
        const itb_dents_u128 u = itb_keys_piece(h, R.meta[t], R.p, R.nr[t], s0 - (int32_t)R.start[t]);
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
// goes on past cap; out may be NULL with cap 0), the emit mask to mask[0, 16)
// unless NULL.  needle[0, needle_len) as the caller gave it.  Returns the
// ITB's err.
// ---------------------------------------------------------------------------
template <bool kLinear>
ITB_SCAN_FN int32_t itb_keys_one(const uint8_t* p, uint32_t n, uint32_t adepth, uint32_t op, const uint8_t* needle,
                                 uint32_t needle_len, uint8_t* out, uint64_t cap, uint32_t* live, uint32_t* dnum,
                                 uint32_t* bytes, uint32_t* keybytes, uint64_t* mask)
{
    *live = *dnum = *bytes = *keybytes = 0;
    if (mask)
        for (uint32_t r = 0; r < POM_KV_MASK_WORDS; r++)
            mask[r] = 0;
    int32_t err = itb_scan_precheck(n, adepth);
    if (err == 0)
        err = itb_scan_live(p, n, adepth, live);
    if (err != 0)
        return err;
    const uint32_t rounds = itb_scan_rounds(adepth);
    // all or nothing: the keys are checked before a byte is written
    uint32_t kb = 0;
    for (uint32_t r = 0; r < rounds; r++)
        for (uint64_t w = itb_scan_word(p, r, adepth); w; w &= w - 1) {
            const itb_keys_entry e = itb_keys_load<false>(p, 64u * r + (uint32_t)__builtin_ctzll(w));
            if (e.bad == POM_KV_E_KEY)
                return e.bad;
            if (e.bad)
                err = e.bad;
            kb += e.keylen;
        }
    if (err != 0)
        return err;
    uint8_t fail[POM_KV_NEEDLE_MAX + 1];
    const uint32_t m = itb_keys_needle_len(needle, needle_len);
    if (kLinear && op >= POM_KV_OP_GREP)
        itb_keys_failure(needle, m, fail);
    uint32_t k = 0;
    uint64_t at = 0;
    for (uint32_t r = 0; r < rounds; r++)
        for (uint64_t w = itb_scan_word(p, r, adepth); w; w &= w - 1) {
            const uint32_t lane = (uint32_t)__builtin_ctzll(w), nr = 64u * r + lane;
            const itb_keys_entry e = itb_keys_load<true>(p, nr);
            if (!itb_keys_emits<kLinear>(p, nr, e, op, needle, m, fail))
                continue;
            if (mask)
                mask[r] |= 1ull << lane;
            const uint8_t* ite = itb_dents_ite(p, nr);
            for (uint32_t j = 0; j < e.head.len + e.memlen; j++, at++)
                if (at < cap)
                    out[at] = j < e.head.len ? itb_keys_head_byte(e.head, j) : ite[e.memoff + j - e.head.len];
            k++;
        }
    *dnum = k;
    *bytes = (uint32_t)at;
    *keybytes = kb;
    return 0;
}

#endif
