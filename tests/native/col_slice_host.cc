// col_slice_host.cc -- pomegranate_amd/csrc/col_slice.h on the CPU (never part
// of the product library).
//   libcol_slice_host.so  col_slice_decide_host(), col_slice_want_ok_host():
//                         the header's decision and length bound
//                         (tests/test_col_slice.py compares them with its
//                         restatement of api/api.c:6447-6460);
//                         col_slice_copy_host(): one slice through the copy
//                         plan, every tile and lane, over checked memory
//   col_slice_check       (-DCOL_SLICE_CHECK) the plan against a byte loop
//                         over source offsets, destination alignments and
//                         lengths, and the decision against 128-bit
//                         arithmetic.  Every column and every destination is
//                         a heap block of exactly its length, so a sanitizer
//                         build sees any access outside.
// The plan works on addresses; here they are virtual (a column at any residue
// mod 16 although malloc aligns its blocks), and CheckedMem maps them to the
// blocks and holds every access against the rules of col_slice.h.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "col_slice.h"

namespace {

struct CheckedMem {
    const uint8_t* col;         // a block of exactly col_len bytes
    uint64_t col_va, col_len;
    uint8_t* dst;               // a block of exactly dst_len bytes
    uint64_t dst_va, dst_len;
    uint8_t* times;             // stores per destination byte
    mutable int bad_load = 0, bad_store = 0;

    bool in_col(uint64_t a) const { return a >= col_va && a < col_va + col_len; }
    // an aligned dword may be loaded when it overlaps the column
    bool dword_ok(uint64_t a) const { return a + 4 > col_va && a < col_va + col_len; }
    // the bytes outside the column read as 0xEE: one that reaches the output shows
    uint8_t byte(uint64_t a) const { return in_col(a) ? col[a - col_va] : 0xEE; }
    uint32_t dword(uint64_t a) const
    {
        return byte(a) | (uint32_t)byte(a + 1) << 8 | (uint32_t)byte(a + 2) << 16 | (uint32_t)byte(a + 3) << 24;
    }
    col_slice_u128 ld16(uint64_t a) const
    {
        bad_load += (a & 15) != 0;
        for (uint32_t k = 0; k < 4; k++)
            bad_load += !dword_ok(a + 4 * k);
        return col_slice_u128{{dword(a), dword(a + 4), dword(a + 8), dword(a + 12)}};
    }
    uint32_t ld4(uint64_t a) const
    {
        bad_load += (a & 3) != 0 || !dword_ok(a);
        return dword(a);
    }
    uint8_t ld1(uint64_t a) const
    {
        bad_load += !in_col(a);
        return byte(a);
    }
    void st1(uint64_t a, uint8_t b) const
    {
        if (a < dst_va || a >= dst_va + dst_len) {
            bad_store++;
            return;
        }
        dst[a - dst_va] = b;
        times[a - dst_va]++;
    }
    void st16(uint64_t a, const col_slice_u128& v) const
    {
        bad_store += (a & 15) != 0;
        for (uint32_t i = 0; i < 16; i++)
            st1(a + i, (uint8_t)(v.w[i / 4] >> (8 * (i % 4))));
    }
};

// The whole slice as the kernel's workgroups run it.  0, or what went wrong:
// 1 a load outside the rules, 2 a store outside the slice, 3 a byte stored
// twice or not at all.
int run_plan(const uint8_t* col, uint64_t col_va, uint64_t col_len, uint64_t offset, uint32_t len, uint8_t* dst,
             uint64_t dst_va)
{
    std::vector<uint8_t> times(len + 1, 0);
    CheckedMem m{col, col_va, col_len, dst, dst_va, len, times.data()};
    const col_slice_plan P = col_slice_plan_make(dst_va, col_va + offset, len, col_va, col_va + col_len);
    const uint32_t tiles = col_slice_tiles(P);
    for (uint32_t t = tiles; t-- > 0;)                  // any order: the tiles are independent
        for (uint32_t lane = 0; lane < kColSliceTileLanes; lane++)
            col_slice_tile_lane(m, P, t, lane);
    if (m.bad_load)
        return 1;
    if (m.bad_store)
        return 2;
    for (uint32_t i = 0; i < len; i++)
        if (times[i] != 1)
            return 3;
    return 0;
}

}  // namespace

extern "C" int32_t col_slice_decide_host(int col_ok, int hdr_ok, int32_t status, uint64_t produced, uint64_t want,
                                         uint64_t offset, uint64_t size, uint64_t* out_len)
{
    return col_slice_decide(col_ok, hdr_ok, status, produced, want, offset, size, out_len);
}

extern "C" int col_slice_want_ok_host(uint64_t want, uint64_t zlen)
{
    return col_slice_want_ok(want, zlen);
}

// The column is col_len bytes at virtual address col_va, the slice's len bytes
// go to dst, which stands at virtual address dst_va.
extern "C" int col_slice_copy_host(const uint8_t* col, uint64_t col_va, uint64_t col_len, uint64_t offset,
                                   uint32_t len, uint8_t* dst, uint64_t dst_va)
{
    if (offset > col_len || len > col_len - offset)
        return -1;
    return run_plan(col, col_va, col_len, offset, len, dst, dst_va);
}

#ifdef COL_SLICE_CHECK
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int failures = 0;

void check_copy(uint32_t col_res, uint32_t offset, uint32_t len, uint32_t behind, uint32_t dst_res)
{
    const uint64_t col_len = (uint64_t)offset + len + behind;
    uint8_t* col = static_cast<uint8_t*>(malloc(col_len + (col_len == 0)));
    uint8_t* dst = static_cast<uint8_t*>(malloc(len + (len == 0)));
    for (uint64_t i = 0; i < col_len; i++)
        col[i] = (uint8_t)rnd();
    memset(dst, 0xA5, len);
    const int rc = run_plan(col, 0x100000 + col_res, col_len, offset, len, dst, 0x900000 + dst_res);
    bool same = true;
    for (uint32_t i = 0; i < len; i++)
        same &= dst[i] == col[offset + i];
    if (rc != 0 || !same) {
        failures++;
        fprintf(stderr, "copy: column at %u mod 16, offset %u, len %u, %u bytes behind, destination at %u mod 16: "
                        "rc %d, bytes %s\n", col_res, offset, len, behind, dst_res, rc, same ? "equal" : "differ");
    }
    free(col);
    free(dst);
}

// api/api.c:6447-6460 behind the decode's checks, with offset + size in 128 bits
int32_t naive_decide(int col_ok, int hdr_ok, int32_t status, uint64_t produced, uint64_t want, uint64_t offset,
                     uint64_t size, uint64_t* n)
{
    *n = 0;
    if (!col_ok)
        return -22;
    if (!hdr_ok)
        return -1;
    if (status)
        return status;
    if (produced != want)
        return -1;
    if (offset > want)
        return -22;
    const unsigned __int128 end = (unsigned __int128)offset + size;
    *n = end > want ? want - offset : size;
    return 0;
}

void check_decide(int col_ok, int hdr_ok, int32_t status, uint64_t produced, uint64_t want, uint64_t offset,
                  uint64_t size)
{
    uint64_t got = 77, exp = 0;
    const int32_t e = col_slice_decide(col_ok, hdr_ok, status, produced, want, offset, size, &got);
    const int32_t w = naive_decide(col_ok, hdr_ok, status, produced, want, offset, size, &exp);
    if (e != w || got != exp) {
        failures++;
        fprintf(stderr, "decide: col_ok %d hdr_ok %d status %d produced %llu want %llu offset %llu size %llu: "
                        "err %d/%d len %llu/%llu\n", col_ok, hdr_ok, status, (unsigned long long)produced,
                (unsigned long long)want, (unsigned long long)offset, (unsigned long long)size, e, w,
                (unsigned long long)got, (unsigned long long)exp);
    }
}

}  // namespace

int main()
{
    const uint32_t T = kColSliceTileBytes;
    // the sweep: source offsets 0-17, destination alignments 0-15, the lengths
    // around a granule, two granules and a tile; the column at several
    // residues, ending with the slice or a few bytes behind it
    for (uint32_t offset = 0; offset <= 17; offset++)
        for (uint32_t dst_res = 0; dst_res < 16; dst_res++)
            for (uint32_t len : {0u, 1u, 15u, 16u, 17u, 31u, 33u, T - 1, T, T + 1})
                for (uint32_t col_res : {0u, 1u, 7u, 12u})
                    for (uint32_t behind : {0u, 3u})
                        check_copy(col_res, offset, len, behind, dst_res);
    // several tiles, a head and a tail, every residue pair
    for (uint32_t col_res = 0; col_res < 16; col_res++)
        for (uint32_t dst_res = 0; dst_res < 16; dst_res++)
            check_copy(col_res, 5, 2 * T + 1, col_res % 3, dst_res);
    for (uint32_t t = 0; t < 2000; t++)
        check_copy((uint32_t)(rnd() % 16), (uint32_t)(rnd() % 300), (uint32_t)(rnd() % (3 * T)),
                   (uint32_t)(rnd() % 40), (uint32_t)(rnd() % 16));
    // the decision: every rule, and the edges of the clamp
    const uint64_t M = ~0ull;
    for (uint64_t want : {(uint64_t)0, (uint64_t)1, (uint64_t)4096, (uint64_t)0xFFFFFFF0ull})
        for (uint64_t offset : {(uint64_t)0, (uint64_t)1, want - 1, want, want + 1, M})
            for (uint64_t size : {(uint64_t)0, (uint64_t)1, want, want + 1, M - 1, M})
                for (int32_t status : {0, -4, -8})
                    for (uint64_t produced : {want, want + 1, want - 1})
                        for (int flags = 0; flags < 4; flags++)
                            check_decide(flags & 1, flags >> 1, status, produced, want, offset, size);
    // the length bound: 255 bytes out per byte in, no more
    for (uint64_t z : {(uint64_t)0, (uint64_t)1, (uint64_t)4, (uint64_t)1000, (uint64_t)16843000})
        if (!col_slice_want_ok(255 * z, z) || col_slice_want_ok(255 * z + 1, z) ||
            (z && !col_slice_want_ok(255 * z - 1, z)) || col_slice_want_ok(0xFFFFFFF1ull, M)) {
            failures++;
            fprintf(stderr, "want_ok: z = %llu\n", (unsigned long long)z);
        }
    if (failures) {
        fprintf(stderr, "col_slice_check: %d FAILED\n", failures);
        return 1;
    }
    printf("col_slice_check: ok\n");
    return 0;
}
#endif
