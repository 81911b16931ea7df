// lzo1x_grammar.h -- the LZO1X instruction grammar of the speculative decoders
// (lzo1x_decode_fast.hip, lzo1x_decode_win.hip, lzo1x_decode_lat.hip), stated
// once.  The stream (lib/minilzo.c:3308-3699) is a
// state machine over instruction starts (pos, state): one step turns a start
// into at most two ops -- A, a literal run or a match, and B, a match's 1-3
// trailing literals -- and the next start.  Two forms of that step:
//
//   lzo1x_decode_word     branch-free, from the instruction's first four bytes;
//                         it says when the instruction needs the other form
//   lzo1x_decode_general  every instruction: length extensions of any length,
//                         bytes fetched one at a time by the caller's reader
//
// The exact decoder (dec_run in lzo1x_kernels.hip) writes as it parses and does
// not come through here.  The header is plain C++17 outside hipcc, where
// tests/native/grammar_host.cc runs both forms against each other on the CPU.
#ifndef POM_LZO1X_GRAMMAR_H
#define POM_LZO1X_GRAMMAR_H

#include <stdint.h>

#ifdef __HIPCC__
#define LZO1X_FN __device__ __forceinline__
#else
#define LZO1X_FN static inline
#endif

// parse states (instruction starts)
constexpr uint32_t ST_A = 0;   // top: t < 16 is a literal run
constexpr uint32_t ST_B = 1;   // after a literal run: t < 16 is a 3-byte M1 (dist > 0x800)
constexpr uint32_t ST_C = 2;   // after trailing literals: t < 16 is a 2-byte M1
constexpr uint32_t ST_F = 3;   // first byte of the stream (lib/minilzo.c:3357)

constexpr uint32_t kLzoLit = 0x80000000u;        // op source: literal bytes at an input position

// One instruction from (pos, st): up to two ops and the next start.  `eof` is
// the EOF marker (lib/minilzo.c:3580) as read; `bad` is a refusal: a read at
// or past the end z of the input, an instruction or its literals ending past
// z, an EOF marker that does not end at z, a 32-bit wrap, a capped zero run.
// The other fields of a bad instruction mean nothing, nor does the source of
// an op of length 0.
struct Lzo1xIns {
    uint32_t pos, st;       // next instruction start
    uint32_t aL, aS;        // op A: length, source (literal: kLzoLit | input pos; match: distance)
    uint32_t bL, bS;        // op B: trailing literals (bL == 0: none)
    bool eof, bad;
};

// Bits [off, off + n) of w.  UBFE: the bit-field-extract instruction, for
// per-lane use; else a shift and a mask, which stay on the scalar unit when
// w is wave-uniform (and are the host's form).
template <bool UBFE>
LZO1X_FN uint32_t lzo1x_bits(uint32_t w, uint32_t off, uint32_t n)
{
#ifdef __HIPCC__
    if (UBFE)
        return __builtin_amdgcn_ubfe(w, off, n);
#endif
    return (w >> off) & ((1u << n) - 1u);
}

// Branch-free form: every field of an instruction without a length extension,
// or with one of a single non-zero byte, lies in its first 4 bytes, the word
// lo (byte 0 = the byte at pos; bytes at or past z are 0).  A pure function of
// (lo, pos, st, z): bit-field extracts and selects, so lanes decoding
// different instruction kinds do not diverge.  `general`: the extension's
// first byte is 0 and the result is void -- take lzo1x_decode_general.  (So
// must a caller whose word does not hold 4 bytes of the input from pos.)
template <bool UBFE>
LZO1X_FN Lzo1xIns lzo1x_decode_word(uint32_t lo, uint32_t pos, uint32_t st, uint32_t z, bool& general)
{
    const uint32_t t = lo & 0xFFu, b1 = lzo1x_bits<UBFE>(lo, 8, 8);
    const bool flit = st == ST_F && t > 17;                        // :3357-3365
    const uint32_t se = st == ST_F ? ST_A : st;
    const bool lit = !flit && se == ST_A && t < 16;                // :3367-3414
    const bool m1 = !flit && !lit && t < 16;
    const bool m2 = !flit && t >= 64;
    const bool m3 = !flit && t >= 32 && t < 64;
    const bool m4 = !flit && t >= 16 && t < 32;
    const bool ext = (lit && t == 0) || (m3 && (t & 31) == 0) || (m4 && (t & 7) == 0);
    general = ext && b1 == 0;                                      // 255-chunk extension
    const uint32_t e = ext ? 1u : 0u;
    const uint32_t o16 = lzo1x_bits<UBFE>(lo, 8u + 8u * e, 16);    // bytes 1+e, 2+e
    const uint32_t dd4 = ((t & 8u) << 11) + (o16 >> 2);
    const uint32_t used = (m1 || m2) ? 2u : 3u + e;                // match instruction bytes
    const uint32_t tl = lzo1x_bits<UBFE>(lo, 8u * (used - 2u), 2); // match_done, :3650
    const uint32_t nlit = flit ? t - 17 : (ext ? 15u + b1 : t) + 3u;
    const uint32_t L = m1 ? (se == ST_B ? 3u : 2u)
                     : m2 ? (t >> 5) + 1u
                     : m3 ? (ext ? 31u + b1 : (t & 31u)) + 2u
                          : (ext ? 7u + b1 : (t & 7u)) + 2u;
    const uint32_t d = m1 ? (se == ST_B ? 0x801u : 1u) + (t >> 2) + (b1 << 2)
                     : m2 ? 1u + ((t >> 2) & 7u) + (b1 << 3)
                     : m3 ? 1u + (o16 >> 2) : dd4 + 0x4000u;
    const bool eof = m4 && dd4 == 0;                               // :3580
    const bool islit = flit || lit;
    const uint32_t hdr = flit ? 1u : 1u + e;                       // literal-run header bytes
    Lzo1xIns r;
    r.eof = eof;
    r.aL = eof ? 0u : islit ? nlit : L;
    r.aS = islit ? kLzoLit | (pos + hdr) : d;
    r.bL = (islit || eof) ? 0u : tl;
    r.bS = kLzoLit | (pos + used);
    // the instruction (header, then literals) ends at r.pos
    r.pos = islit ? pos + hdr + nlit : pos + used + (eof ? 0u : tl);
    r.st = islit ? (flit && nlit < 4 ? ST_C : ST_B) : (tl && !eof ? ST_C : ST_A);
    r.bad = eof ? r.pos != z : r.pos > z;
    return r;
}

// Zero-run policy of the general form: a length extension is refused once
// `limit` zero bytes have been read and the run has not ended.  Every node or
// lane that starts inside a long run would scan the rest of it, so the
// decoders that parse speculatively give a guess up early; the exact decoder
// takes the block and decodes it in linear time.
//   kLzoZerosAny      the op-set decoder: no cap (its u32 length wraps like
//                     the sum it replaces; the wrap is a refusal below)
//   kLzoZerosWinSpec  the windowed decoder's speculative lanes: 64 zeros pass
//   kLzoZerosWinTrue  its true path scans each run once, but from 2^24 zeros
//                     on refuses: the reference keeps a 64-bit length
//                     (lib/minilzo.c:3805), and from 16,843,009 zeros on, 255
//                     per zero passes 2^32 -- a u32 sum would wrap to a small,
//                     valid-looking length
//   kLzoZerosLat      the latency decoder: 63 zeros pass (a length past ~16 K)
// bulk(p, z): zero bytes at p that the decoder can tell at once (0: none);
// only the windowed decoder's true path has such a scan.
constexpr uint32_t kLzoZerosAny = 0xFFFFFFFFu;
constexpr uint32_t kLzoZerosWinSpec = 65;
constexpr uint32_t kLzoZerosWinTrue = 1u << 24;
constexpr uint32_t kLzoZerosLat = 64;
struct Lzo1xZeroRun {
    uint32_t limit;
    constexpr uint32_t bulk(uint32_t, uint32_t) const { return 0u; }
};

// General form.  rd(p) is the input byte at p (0 at or past z); zr the
// zero-run policy.
template <class Rd, class Zr>
LZO1X_FN Lzo1xIns lzo1x_decode_general(Rd rd, Zr zr, uint32_t pos, uint32_t st, uint32_t z)
{
    Lzo1xIns r;
    r.aL = r.bL = r.aS = r.bS = 0;
    r.eof = false;
    r.st = ST_A;
    bool capped = false;
    // (p ends one past the extension's last byte; zeros that run into z end
    // on a read at z, which is a refusal)
    auto ext = [&](uint32_t& p, uint32_t base) -> uint32_t {
        uint32_t n = 0;     // zero bytes
        while (p < z) {
            if (n >= zr.limit) {
                capped = true;
                break;
            }
            const uint32_t k = zr.bulk(p, z);
            if (k) {
                n += k;
                p += k;
                continue;
            }
            if (rd(p) != 0)
                break;
            n++;
            p++;
        }
        const uint32_t v = 255u * n + base + rd(p);
        p++;
        return v;
    };
    uint32_t t = rd(pos);
    uint32_t end;           // one past the last header byte read
    if (st == ST_F && t > 17) {                           // :3357-3365
        const uint32_t n = t - 17;
        end = pos + 1;
        r.aL = n;
        r.aS = kLzoLit | end;
        r.pos = end + n;
        r.st = n < 4 ? ST_C : ST_B;
    } else if (t < 16 && (st == ST_A || st == ST_F)) {    // literal run, :3367-3414
        end = pos + 1;
        if (t == 0)
            t = ext(end, 15);
        r.aL = t + 3;
        r.aS = kLzoLit | end;
        r.pos = end + t + 3;
        r.st = ST_B;
    } else {
        uint32_t L, d;
        if (t < 16) {                                     // M1 forms, :3416-3443 / :3600-3612
            d = (st == ST_B ? 0x801u : 1u) + (t >> 2) + (rd(pos + 1) << 2);
            L = st == ST_B ? 3u : 2u;
            end = pos + 2;
        } else if (t >= 64) {                             // M2
            d = 1 + ((t >> 2) & 7) + (rd(pos + 1) << 3);
            L = (t >> 5) + 1;
            end = pos + 2;
        } else {                                          // M3, M4 / EOF
            const bool m3 = t >= 32;
            L = t & (m3 ? 31u : 7u);
            end = pos + 1;
            if (L == 0)
                L = ext(end, m3 ? 31u : 7u);
            L += 2;
            const uint32_t dd = (m3 ? 0u : (t & 8) << 11) + ((rd(end) | (rd(end + 1) << 8)) >> 2);
            end += 2;
            r.eof = !m3 && dd == 0;                       // :3580
            d = m3 ? 1 + dd : dd + 0x4000;
        }
        r.pos = end;
        if (!r.eof) {
            r.aL = L;
            r.aS = d;
            const uint32_t tl = rd(end - 2) & 3;          // match_done, :3650-3653
            if (tl) {
                r.bL = tl;
                r.bS = kLzoLit | end;
                r.pos = end + tl;
                r.st = ST_C;
            }
        }
    }
    // every byte read lies below `end`: reads or literals past the input
    // (INPUT_OVERRUN), a wrapped length, a capped run, or an EOF marker not
    // at the end (INPUT_NOT_CONSUMED)
    r.bad = end > z || r.pos > z || r.pos < end || capped || (r.eof && r.pos != z);
    return r;
}

#endif
