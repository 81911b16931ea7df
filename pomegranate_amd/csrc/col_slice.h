// col_slice.h -- a column read by offset and size (api/api.c:6447-6460 behind
// the decode of :6427-6446), stated once: the decision for one request, and
// the copy plan the kernel of col_slice.hip runs.  The decision part is also
// plain C (column_codec.c decides the requests of columns that never reach the
// GPU with it); the plan part is C++17 outside hipcc, where
// tests/native/col_slice_host.cc runs it on the CPU over checked memory.
//
// The rules for one request r on column c = req[r].col, W = want[c] the
// recorded length, in this order, the first that applies deciding:
//   1  c >= ncol                               -> -EINVAL
//   2  the column is shorter than its header   -> LZO_E_ERROR
//   3  a decoder code other than 0             -> that code
//   4  a produced length other than W          -> LZO_E_ERROR
//   5  offset > W                              -> -EINVAL (offset == W: an empty read)
//   6  otherwise err = 0, out_len = min(size, W - offset)
// With err != 0, out_len = 0 and nothing is copied.
//
// The copy of len bytes from source address src to destination address dst:
//   head   the bytes up to the first 16-byte-aligned destination address
//          (at most 15, fewer when len is), stored one byte a lane
//   body   whole 16-byte granules at aligned destination addresses, one a
//          lane, 256 a tile; granule g's bytes lie shift = (src + head) & 15
//          bytes into the aligned source granule at q = src + head - shift +
//          16g, so they are the 32 bytes at q and q + 16 shifted down by
//          shift bytes (q + 16 is not loaded when shift is 0)
//   tail   the up to 15 bytes behind the last granule, one byte a lane
// A source granule is loaded whole when it lies inside the column's range
// rounded out to aligned dwords, else dword by dword, each only where it
// overlaps the range (the argument of win_load in lzo1x_kernels.hip: an
// aligned dword that overlaps an allocation never leaves its page).
#ifndef POM_COL_SLICE_H
#define POM_COL_SLICE_H

#include <stdint.h>

#ifdef __HIPCC__
#define COL_SLICE_FN __device__ __forceinline__
#else
#define COL_SLICE_FN static inline
#endif

#define COL_SLICE_EINVAL (-22)                    /* -EINVAL */
#define COL_SLICE_E_ERROR (-1)                    /* LZO_E_ERROR */
#define COL_SLICE_WANT_MAX 0xFFFFFFF0ull          /* the batch ABI's 32-bit capacity */

/* The decision.  col_ok: c < ncol (the other arguments are not looked at
 * without it); hdr_ok: the column holds its 8-byte header; status, produced:
 * the decoder's code and length.  Returns err; *out_len as the rules say. */
COL_SLICE_FN int32_t col_slice_decide(int col_ok, int hdr_ok, int32_t status, uint64_t produced,
                                      uint64_t want, uint64_t offset, uint64_t size, uint64_t *out_len)
{
    *out_len = 0;
    if (!col_ok)
        return COL_SLICE_EINVAL;
    if (!hdr_ok)
        return COL_SLICE_E_ERROR;
    if (status != 0)
        return status;
    if (produced != want)
        return COL_SLICE_E_ERROR;
    if (offset > want)
        return COL_SLICE_EINVAL;
    /* offset <= want: no offset + size, which wraps for size = UINT64_MAX */
    *out_len = size < want - offset ? size : want - offset;
    return 0;
}

/* A header length the GPU path stages room for: it fits the 32-bit capacity,
 * and zlen stream bytes can yield it.  A literal yields one byte per input
 * byte; the densest match is a token, k zero extension bytes, the final
 * length byte and two offset bytes: at most 288 + 255k bytes from k + 4. */
COL_SLICE_FN int col_slice_want_ok(uint64_t want, uint64_t zlen)
{
    return want <= COL_SLICE_WANT_MAX && want / 255u + (want % 255u != 0) <= zlen;
}

#ifdef __cplusplus

constexpr uint32_t kColSliceTileLanes = 256;
constexpr uint32_t kColSliceTileBytes = 16 * kColSliceTileLanes;

struct col_slice_u128 {
    uint32_t w[4];
};

struct col_slice_plan {
    uint64_t dst, src;      // addresses of the slice's first byte
    uint64_t lo4, hi4;      // the column's range rounded out to aligned dwords
    uint32_t head, tail;    // bytes stored narrow before and behind the granules
    uint32_t ngran;         // whole granules between them
    uint32_t shift;         // bytes from an aligned source granule to the destination's
};

// col_lo, col_hi: the addresses of the column's first byte and of the byte
// behind its last; [src, src + len) lies inside.
COL_SLICE_FN col_slice_plan col_slice_plan_make(uint64_t dst, uint64_t src, uint32_t len, uint64_t col_lo,
                                                uint64_t col_hi)
{
    col_slice_plan P;
    P.dst = dst;
    P.src = src;
    P.lo4 = col_lo & ~(uint64_t)3;
    P.hi4 = (col_hi + 3u) & ~(uint64_t)3;
    const uint32_t to_aligned = (uint32_t)(16u - (dst & 15u)) & 15u;
    P.head = len < to_aligned ? len : to_aligned;
    P.ngran = (len - P.head) >> 4;
    P.tail = (len - P.head) & 15u;
    P.shift = (uint32_t)((src + P.head) & 15u);
    return P;
}

// Tiles of a slice: one when there is no whole granule but a head or a tail.
COL_SLICE_FN uint32_t col_slice_tiles(const col_slice_plan& P)
{
    const uint32_t t = (P.ngran + kColSliceTileLanes - 1) / kColSliceTileLanes;
    return t ? t : (P.head | P.tail) != 0;
}

// {hi, lo} shifted down by bits (0, 8, 16 or 24): v_alignbit_b32.
COL_SLICE_FN uint32_t col_slice_funnel(uint32_t lo, uint32_t hi, uint32_t bits)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_alignbit(hi, lo, bits);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
#endif
}

// The aligned 16 bytes at q: one load inside [lo4, hi4), else the dwords
// inside it (the others read as 0 and are never part of a granule).
// Mem: ld16(addr), ld4(addr), ld1(addr), st16(addr, v), st1(addr, byte).
template <class Mem>
COL_SLICE_FN col_slice_u128 col_slice_load16(const Mem& m, uint64_t q, uint64_t lo4, uint64_t hi4)
{
    if (q >= lo4 && q + 16u <= hi4)
        return m.ld16(q);
    col_slice_u128 v;
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t a = q + 4u * k;
        v.w[k] = a >= lo4 && a < hi4 ? m.ld4(a) : 0u;
    }
    return v;
}

// a then b as eight dwords, shifted down by WS dwords and `bits` bits.
template <int WS>
COL_SLICE_FN col_slice_u128 col_slice_merge(const col_slice_u128& a, const col_slice_u128& b, uint32_t bits)
{
    const uint32_t w[8] = {a.w[0], a.w[1], a.w[2], a.w[3], b.w[0], b.w[1], b.w[2], b.w[3]};
    col_slice_u128 v;
    for (int k = 0; k < 4; k++)
        v.w[k] = col_slice_funnel(w[k + WS], w[k + WS + 1], bits);
    return v;
}

// Granule g of the body.  shift is the same for every granule of a slice, so
// the switch is uniform over the workgroup.
template <class Mem>
COL_SLICE_FN col_slice_u128 col_slice_granule(const Mem& m, const col_slice_plan& P, uint32_t g)
{
    const uint64_t q = P.src + P.head - P.shift + 16ull * g;
    const col_slice_u128 a = col_slice_load16(m, q, P.lo4, P.hi4);
    if (P.shift == 0)
        return a;
    const col_slice_u128 b = col_slice_load16(m, q + 16u, P.lo4, P.hi4);
    const uint32_t bits = 8u * (P.shift & 3u);
    switch (P.shift >> 2) {
    case 0:
        return col_slice_merge<0>(a, b, bits);
    case 1:
        return col_slice_merge<1>(a, b, bits);
    case 2:
        return col_slice_merge<2>(a, b, bits);
    default:
        return col_slice_merge<3>(a, b, bits);
    }
}

// What lane `lane` of the workgroup that owns tile `tile` does: its granule,
// and in the first and last tile a head or tail byte.
template <class Mem>
COL_SLICE_FN void col_slice_tile_lane(const Mem& m, const col_slice_plan& P, uint32_t tile, uint32_t lane)
{
    const uint32_t g = tile * kColSliceTileLanes + lane;
    if (g < P.ngran)
        m.st16(P.dst + P.head + 16ull * g, col_slice_granule(m, P, g));
    if (tile == 0 && lane < P.head)
        m.st1(P.dst + lane, m.ld1(P.src + lane));
    if (tile + 1 == col_slice_tiles(P) && lane < P.tail) {
        const uint64_t o = P.head + 16ull * P.ngran + lane;
        m.st1(P.dst + o, m.ld1(P.src + o));
    }
}

#endif /* __cplusplus */

#endif
