// itb_scan.h -- the garbage collector's walk over one decoded ITB payload
// (mdsl/gc.c:968-993 with __add_to_brtree, mdsl/gc.c:788-802), stated once.
// The kernels of itb_scan.hip walk a payload with one wave, 64 bitmap bits a
// round; itb_scan_one below walks it bit by bit.  Both only combine the
// functions of this header, which is plain C++17 outside hipcc, where
// tests/native/itb_scan_host.cc runs it on the CPU.
//
// The rules for one ITB (payload p of n bytes, adepth, column 0 ... 5):
//   adepth 0 or above 10            -> -EINVAL (the bitmap has 1024 bits; the
//                                      reference would read the index as bitmap)
//   n < 3712 (bitmap incomplete)    -> POM_GC_E_TRUNCATED, live = 0
//   live = set bits below 1 << adepth; bits at or above it are ignored
//   a live bit nr whose ITE ends past n (11904 + 512 * (nr + 1) > n)
//                                   -> POM_GC_E_TRUNCATED and no range at all
//                                      (ITEs ascend with nr: the highest live
//                                      bit decides)
//   each live nr, ascending, with column.len > 0 emits
//                                      {offset, offset + len + 1}, u64, wrapping
// No byte at or past n is loaded; p may sit at any byte alignment.
#ifndef POM_ITB_SCAN_H
#define POM_ITB_SCAN_H

#include <stdint.h>

#include "pom_gc.h"

#ifdef __HIPCC__
#define ITB_SCAN_FN __device__ __forceinline__
#else
#define ITB_SCAN_FN static inline
#endif

constexpr int32_t kItbScanEinval = -22;           // -EINVAL
constexpr uint32_t kItbScanRounds = POM_ITB_BITMAP_BYTES / 8;

// Eight little-endian bytes at p: one load when p is 8-byte aligned (every
// field read here sits at a multiple of 8 from the payload's start), else
// byte by byte.
ITB_SCAN_FN uint64_t itb_scan_ld64(const uint8_t* p)
{
    uint64_t v = 0;
    if (((uintptr_t)p & 7u) == 0) {
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8);
        return v;
    }
    for (uint32_t i = 0; i < 8; i++)
        v |= (uint64_t)p[i] << (8 * i);
    return v;
}

// 0 when the bitmap can be walked, else the ITB's error.
ITB_SCAN_FN int32_t itb_scan_precheck(uint32_t n, uint32_t adepth)
{
    if (adepth == 0 || adepth > POM_ITB_ADEPTH_MAX)
        return kItbScanEinval;
    return n < POM_ITB_BITMAP_OFF + POM_ITB_BITMAP_BYTES ? POM_GC_E_TRUNCATED : 0;
}

// Rounds of 64 bits that hold a bit below 1 << adepth.
ITB_SCAN_FN uint32_t itb_scan_rounds(uint32_t adepth)
{
    return ((1u << adepth) + 63u) >> 6;
}

// Round r's bitmap word, bits 64r ... 64r + 63 (find_next_bit's little-endian
// unsigned long, lib/bitmap.c:163), with the bits at or above 1 << adepth cleared.
ITB_SCAN_FN uint64_t itb_scan_word(const uint8_t* p, uint32_t r, uint32_t adepth)
{
    const uint32_t limit = 1u << adepth;
    const uint32_t below = limit > 64u * r ? limit - 64u * r : 0u;
    const uint64_t keep = below >= 64u ? ~0ull : (1ull << below) - 1ull;
    return itb_scan_ld64(p + POM_ITB_BITMAP_OFF + 8u * r) & keep;
}

// Highest set bit of a non-zero word of round r, as a bit number.
ITB_SCAN_FN uint32_t itb_scan_top(uint64_t w, uint32_t r)
{
    return 64u * r + 63u - (uint32_t)__builtin_clzll(w);
}

// ITE nr lies wholly inside a payload of n bytes.
ITB_SCAN_FN bool itb_scan_ite_inside(uint32_t nr, uint32_t n)
{
    return POM_ITB_ITE_OFF + POM_ITE_SIZE * (nr + 1u) <= n;
}

ITB_SCAN_FN const uint8_t* itb_scan_column(const uint8_t* p, uint32_t nr, uint32_t column)
{
    return p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr + POM_ITE_COLUMN_OFF + POM_COLUMN_SIZE * column;
}

// __add_to_brtree's test (mdsl/gc.c:792) on ITE nr, which must be inside.
ITB_SCAN_FN bool itb_scan_has_range(const uint8_t* p, uint32_t nr, uint32_t column)
{
    return itb_scan_ld64(itb_scan_column(p, nr, column) + POM_COLUMN_LEN_OFF) != 0;
}

// The node it builds (mdsl/gc.c:795-796).
ITB_SCAN_FN pom_gc_range itb_scan_range(const uint8_t* p, uint32_t nr, uint32_t column)
{
    const uint8_t* c = itb_scan_column(p, nr, column);
    const uint64_t len = itb_scan_ld64(c + POM_COLUMN_LEN_OFF);
    const uint64_t off = itb_scan_ld64(c + POM_COLUMN_OFFSET_OFF);
    return pom_gc_range{off, off + len + 1u};
}

// The live count and, when the highest live ITE ends past n, TRUNCATED.
// precheck must have passed.
ITB_SCAN_FN int32_t itb_scan_live(const uint8_t* p, uint32_t n, uint32_t adepth, uint32_t* live)
{
    uint32_t cnt = 0, top = 0;
    const uint32_t rounds = itb_scan_rounds(adepth);
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t w = itb_scan_word(p, r, adepth);
        cnt += (uint32_t)__builtin_popcountll(w);
        if (w)
            top = itb_scan_top(w, r);
    }
    *live = cnt;
    return cnt && !itb_scan_ite_inside(top, n) ? POM_GC_E_TRUNCATED : 0;
}

// The whole walk, one bit at a time: up to cap ranges to out (the count goes
// on past cap).  Returns the ITB's err.
ITB_SCAN_FN int32_t itb_scan_one(const uint8_t* p, uint32_t n, uint32_t adepth, uint32_t column,
                                 pom_gc_range* out, uint64_t cap, uint32_t* live, uint32_t* nranges)
{
    *live = *nranges = 0;
    int32_t err = itb_scan_precheck(n, adepth);
    if (err == 0)
        err = itb_scan_live(p, n, adepth, live);
    if (err != 0)
        return err;
    uint32_t k = 0;
    const uint32_t rounds = itb_scan_rounds(adepth);
    for (uint32_t r = 0; r < rounds; r++)
        for (uint64_t w = itb_scan_word(p, r, adepth); w; w &= w - 1) {
            const uint32_t nr = 64u * r + (uint32_t)__builtin_ctzll(w);
            if (!itb_scan_has_range(p, nr, column))
                continue;
            if (k < cap)
                out[k] = itb_scan_range(p, nr, column);
            k++;
        }
    *nranges = k;
    return 0;
}

#endif
