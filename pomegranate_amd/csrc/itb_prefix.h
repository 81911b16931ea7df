// itb_prefix.h -- what the ITB walks (itb_scan.hip, itb_dents.hip) share
// besides their rules: the exclusive prefix over the per-ITB counts, between
// the count and the emit launch, and the ballot rank.  Device code only; in
// the anonymous namespace, so each .hip file gets its own copy.
#ifndef POM_ITB_PREFIX_H
#define POM_ITB_PREFIX_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzo1x_wave.h"

namespace {

constexpr uint32_t kPrefixThreads = 1024;

// Lanes below this one whose bit is set in m.
__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// first[0 .. n] = the exclusive prefix of counts[0 .. n), u64.  One workgroup
// over tiles of kPrefixThreads counts, the running total carried from tile to
// tile.  A tile's sum must fit u32: the callers bound their counts.
__global__ __launch_bounds__(kPrefixThreads) void itb_prefix_kernel(
    const uint32_t* __restrict__ counts, uint32_t n, uint64_t* __restrict__ first)
{
    __shared__ uint32_t wsum[kPrefixThreads / 64];
    const uint32_t t = threadIdx.x, lane = lane_id(), w = t / 64;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n; base += kPrefixThreads) {
        const uint32_t i = base + t;
        const uint32_t v = i < n ? counts[i] : 0u;
        const uint32_t incl = wave_incl_scan(v);
        if (lane == 63)
            wsum[w] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
        for (uint32_t k = 0; k < kPrefixThreads / 64; k++) {
            const uint32_t s = wsum[k];
            before += k < w ? s : 0u;
            tile += s;
        }
        if (i < n)
            first[i] = carry + before + (incl - v);
        carry += tile;
        __syncthreads();
    }
    if (t == 0)
        first[n] = carry;
}

}  // namespace

#endif
