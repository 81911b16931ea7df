// gc_merge.hip -- the garbage collector's range tree on gfx950 (include/pom_gc.h
// pom_gc_merge_dev; the rules are gc_merge.h's): the live ranges sorted by low,
// merged by a running maximum, the merged map and its sums written out.
// Stream-ordered launches whose number follows from n alone; no workgroup
// waits for another, no atomic touches global memory:
//   gc_prep_kernel           key = low (or the dropped key), payload = high
//   per radix pass, 8 of them:
//     gc_hist_kernel         table[digit][tile]
//     scan (sum, u32)        table -> each digit's and tile's base, in place
//     gc_scatter_kernel      keys and payloads to base + rank, stable
//   scan (max, u64)          runmax
//   scan (sum, u32)          the heads before every element (the heads on the fly)
//   gc_emit_kernel           out[k].low by the head, out[k].high by the last; per-tile sums
//   gc_stat_kernel           one workgroup over the per-tile sums: stat
// A scan is gc_scan_reduce_kernel (per tile), gc_scan_agg_kernel (one
// workgroup over the tile aggregates, a loop with a carry) and
// gc_scan_down_kernel (per tile); a scan of one tile is its downsweep alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gc_merge.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kWave = 64;
static_assert(kGcRound == kWave, "a round is one wave's keys");
constexpr uint32_t kSortWaves = kGcSortThreads / kWave;
constexpr uint32_t kSortRounds = kGcSortTile / kGcSortThreads;      // rounds of 64 keys a wave
constexpr uint32_t kStatThreads = 1024;
static_assert(kGcSortTile % kGcSortThreads == 0 && kGcAggThreads % kWave == 0, "whole waves");

// ---------------------------------------------------------------------------
// The scan primitive
// ---------------------------------------------------------------------------
struct SumOp {
    using T = uint32_t;
    static __device__ __forceinline__ T identity() { return 0u; }
    static __device__ __forceinline__ T combine(T a, T b) { return a + b; }
    static __device__ __forceinline__ T wave_incl(T v) { return wave_incl_scan(v); }
};

struct MaxOp {
    using T = uint64_t;
    static __device__ __forceinline__ T identity() { return 0ull; }
    static __device__ __forceinline__ T combine(T a, T b) { return gc_merge_max(a, b); }
    static __device__ __forceinline__ T wave_incl(T v)
    {
        const uint32_t lane = lane_id();
        for (uint32_t d = 1; d < kWave; d <<= 1) {
            const T up = __shfl_up(v, d);
            if (lane >= d)
                v = gc_merge_max(v, up);
        }
        return v;
    }
};

// Over the workgroup's threads in thread order: *excl = everything before
// this thread's v; returns the workgroup's total.  lds: one T per wave.
template <class Op, uint32_t kThreads>
__device__ __forceinline__ typename Op::T block_scan(typename Op::T v, typename Op::T* lds, typename Op::T* excl)
{
    using T = typename Op::T;
    const uint32_t lane = lane_id(), w = threadIdx.x / kWave;
    const T incl = Op::wave_incl(v);
    T before = __shfl_up(incl, 1);
    if (lane == 0)
        before = Op::identity();
    if (lane == kWave - 1)
        lds[w] = incl;
    __syncthreads();
    T wave_before = Op::identity(), total = Op::identity();
    for (uint32_t k = 0; k < kThreads / kWave; k++) {
        const T s = lds[k];
        if (k < w)
            wave_before = Op::combine(wave_before, s);
        total = Op::combine(total, s);
    }
    __syncthreads();
    *excl = Op::combine(wave_before, before);
    return total;
}

// The scans' inputs: element i of n.
struct TableIn {
    using Op = SumOp;
    static constexpr bool kExclusive = true;
    const uint32_t* table;
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return table[i]; }
};

struct HighIn {
    using Op = MaxOp;
    static constexpr bool kExclusive = false;
    const uint64_t *key, *val;
    __device__ __forceinline__ uint64_t load(uint32_t i) const { return gc_merge_high(key[i], val[i]); }
};

struct HeadIn {
    using Op = SumOp;
    static constexpr bool kExclusive = true;
    const uint64_t *key, *runmax;
    __device__ __forceinline__ uint32_t load(uint32_t i) const
    {
        return gc_merge_head(i, key[i], i ? runmax[i - 1] : 0ull) ? 1u : 0u;
    }
};

// A thread's kGcScanItems consecutive elements of tile blockIdx.x, identity past n.
template <class In>
__device__ __forceinline__ typename In::Op::T scan_load(const In& in, uint32_t n, typename In::Op::T (&v)[kGcScanItems])
{
    using Op = typename In::Op;
    const uint32_t i0 = blockIdx.x * kGcScanTile + threadIdx.x * kGcScanItems;
    typename Op::T sum = Op::identity();
#pragma unroll
    for (uint32_t j = 0; j < kGcScanItems; j++) {
        v[j] = i0 + j < n ? in.load(i0 + j) : Op::identity();
        sum = Op::combine(sum, v[j]);
    }
    return sum;
}

template <class In>
__global__ __launch_bounds__(kGcScanThreads) void gc_scan_reduce_kernel(In in, uint32_t n, typename In::Op::T* agg)
{
    using Op = typename In::Op;
    __shared__ typename Op::T lds[kGcScanThreads / kWave];
    typename Op::T v[kGcScanItems], excl;
    const typename Op::T mine = scan_load(in, n, v);
    const typename Op::T total = block_scan<Op, kGcScanThreads>(mine, lds, &excl);
    if (threadIdx.x == 0)
        agg[blockIdx.x] = total;
}

// agg[0 .. ntiles) -> its exclusive scan, agg[ntiles] = the total.  One
// workgroup over passes of kGcAggThreads aggregates, the carry from pass to pass.
template <class Op>
__global__ __launch_bounds__(kGcAggThreads) void gc_scan_agg_kernel(typename Op::T* agg, uint32_t ntiles)
{
    using T = typename Op::T;
    __shared__ T lds[kGcAggThreads / kWave];
    T carry = Op::identity();
    for (uint32_t base = 0; base < ntiles; base += kGcAggThreads) {
        const uint32_t i = base + threadIdx.x;
        const T v = i < ntiles ? agg[i] : Op::identity();
        T excl;
        const T total = block_scan<Op, kGcAggThreads>(v, lds, &excl);
        if (i < ntiles)
            agg[i] = Op::combine(carry, excl);
        carry = Op::combine(carry, total);
    }
    if (threadIdx.x == 0)
        agg[ntiles] = carry;
}

// agg: the tiles' exclusive scan, or NULL for a scan of one tile.  out may be
// the input's own array: a thread reads its elements before it writes them.
template <class In>
__global__ __launch_bounds__(kGcScanThreads) void gc_scan_down_kernel(In in, uint32_t n, const typename In::Op::T* agg,
                                                                      typename In::Op::T* out)
{
    using Op = typename In::Op;
    using T = typename Op::T;
    __shared__ T lds[kGcScanThreads / kWave];
    T v[kGcScanItems], excl;
    const T mine = scan_load(in, n, v);
    block_scan<Op, kGcScanThreads>(mine, lds, &excl);
    T run = agg ? Op::combine(agg[blockIdx.x], excl) : excl;
    const uint32_t i0 = blockIdx.x * kGcScanTile + threadIdx.x * kGcScanItems;
#pragma unroll
    for (uint32_t j = 0; j < kGcScanItems; j++) {
        const T incl = Op::combine(run, v[j]);
        if (i0 + j < n)
            out[i0 + j] = In::kExclusive ? run : incl;
        run = incl;
    }
}

template <class In>
void launch_scan(const In& in, uint32_t n, typename In::Op::T* agg, typename In::Op::T* out, hipStream_t s)
{
    const uint32_t tiles = gc_merge_tiles(n, kGcScanTile);
    if (tiles > 1) {
        hipLaunchKernelGGL(gc_scan_reduce_kernel<In>, dim3(tiles), dim3(kGcScanThreads), 0, s, in, n, agg);
        hipLaunchKernelGGL(gc_scan_agg_kernel<typename In::Op>, dim3(1), dim3(kGcAggThreads), 0, s, agg, tiles);
    }
    hipLaunchKernelGGL(gc_scan_down_kernel<In>, dim3(tiles), dim3(kGcScanThreads), 0, s, in, n,
                       tiles > 1 ? agg : nullptr, out);
}

// ---------------------------------------------------------------------------
// The sort
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gc_prep_kernel(const pom_gc_range* __restrict__ in, uint32_t n,
                                                      uint64_t* __restrict__ key, uint64_t* __restrict__ val)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const uint64_t low = in[i].low, high = in[i].high;
        key[i] = gc_merge_key(low, high);
        val[i] = high;
    }
}

// Lanes below this one whose bit is set in m (itb_prefix.h has the same line,
// and with it a kernel this file has no use for).
__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The lanes of the wave that are live and hold digit d.
__device__ __forceinline__ uint64_t wave_peers(uint32_t d, bool live)
{
    uint64_t peers = wave_ballot(live);
#pragma unroll
    for (uint32_t b = 0; b < kGcRadixBits; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = wave_ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// Wave w owns keys [w, w + 1) * kGcSortTile / kSortWaves of the tile, 64 a
// round, so that tile order is (wave, round, lane).  hist[w][d] = its keys of
// digit d: one lane per digit and round adds the round's count, and only this
// wave touches hist[w].
__device__ __forceinline__ void tile_histogram(const uint64_t* __restrict__ key, uint32_t n, uint32_t pass,
                                               uint32_t (&hist)[kSortWaves][kGcRadix])
{
    const uint32_t lane = lane_id(), w = threadIdx.x / kWave;
    for (uint32_t x = threadIdx.x; x < kSortWaves * kGcRadix; x += kGcSortThreads)
        (&hist[0][0])[x] = 0;
    __syncthreads();
    const uint32_t e0 = blockIdx.x * kGcSortTile + w * (kGcSortTile / kSortWaves) + lane;
#pragma unroll 4
    for (uint32_t r = 0; r < kSortRounds; r++) {
        const uint32_t e = e0 + r * kWave;
        const bool live = e < n;
        const uint32_t d = gc_merge_digit(live ? key[e] : 0ull, pass);
        const uint64_t peers = wave_peers(d, live);
        if (live && lanes_below(peers) == 0)
            lds_store(&hist[w][d], lds_load(&hist[w][d]) + (uint32_t)__popcll(peers));
    }
    __syncthreads();
}

// table[d * ntiles + tile]: digit-major, so that its exclusive scan is each
// digit's and tile's first place in the pass's output.
__global__ __launch_bounds__(kGcSortThreads) void gc_hist_kernel(const uint64_t* __restrict__ key, uint32_t n,
                                                                 uint32_t pass, uint32_t* __restrict__ table)
{
    __shared__ uint32_t hist[kSortWaves][kGcRadix];
    tile_histogram(key, n, pass, hist);
    const uint32_t d = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kSortWaves; w++)
        sum += hist[w][d];
    table[d * gridDim.x + blockIdx.x] = sum;
}

__global__ __launch_bounds__(kGcSortThreads) void gc_scatter_kernel(
    const uint64_t* __restrict__ key, const uint64_t* __restrict__ val, uint32_t n, uint32_t pass,
    const uint32_t* __restrict__ base, uint64_t* __restrict__ key_out, uint64_t* __restrict__ val_out)
{
    __shared__ uint32_t hist[kSortWaves][kGcRadix];
    tile_histogram(key, n, pass, hist);
    // hist[w][d] becomes the place of wave w's first key of digit d
    {
        const uint32_t d = threadIdx.x;
        uint32_t at = base[d * gridDim.x + blockIdx.x];
        for (uint32_t w = 0; w < kSortWaves; w++) {
            const uint32_t c = hist[w][d];
            hist[w][d] = at;
            at += c;
        }
    }
    __syncthreads();
    const uint32_t lane = lane_id(), w = threadIdx.x / kWave;
    const uint32_t e0 = blockIdx.x * kGcSortTile + w * (kGcSortTile / kSortWaves) + lane;
#pragma unroll 2
    for (uint32_t r = 0; r < kSortRounds; r++) {
        const uint32_t e = e0 + r * kWave;
        const bool live = e < n;
        const uint64_t k = live ? key[e] : 0ull;
        const uint64_t v = live ? val[e] : 0ull;
        const uint32_t d = gc_merge_digit(k, pass);
        const uint64_t peers = wave_peers(d, live);
        const uint32_t before = lanes_below(peers);
        const uint32_t at = lds_load(&hist[w][d]);
        if (live) {
            const uint32_t to = gc_merge_slot(at, before, (uint32_t)__popcll(peers));
            if (to < n) {                       // (always, when the table is this pass's)
                key_out[to] = k;
                val_out[to] = v;
            }
            if (before == 0)
                lds_store(&hist[w][d], at + (uint32_t)__popcll(peers));
        }
    }
}

// ---------------------------------------------------------------------------
// Emit and stat
// ---------------------------------------------------------------------------
struct gc_part {
    uint64_t sum;           // the extents' high - low, as far as this tile's heads and lasts give it
    uint32_t heads, kept;
};

__global__ __launch_bounds__(kGcScanThreads) void gc_emit_kernel(
    const uint64_t* __restrict__ key, const uint64_t* __restrict__ runmax, const uint32_t* __restrict__ kidx,
    uint32_t n, pom_gc_range* __restrict__ out, uint64_t out_cap, gc_part* __restrict__ part)
{
    __shared__ uint64_t lsum[kGcScanThreads / kWave];
    __shared__ uint32_t lheads[kGcScanThreads / kWave], lkept[kGcScanThreads / kWave];
    uint64_t sum = 0;
    uint32_t heads = 0, kept = 0;
    for (uint32_t r = 0; r < kGcScanItems; r++) {
        const uint32_t i = blockIdx.x * kGcScanTile + r * kGcScanThreads + threadIdx.x;
        if (i >= n)
            continue;
        const uint64_t ki = key[i], mi = runmax[i];
        const bool head = gc_merge_head(i, ki, i ? runmax[i - 1] : 0ull);
        const bool last = gc_merge_last(i, n, ki, i + 1u < n ? key[i + 1] : 0ull, mi);
        const uint32_t x = gc_merge_extent(kidx[i], head);
        kept += gc_merge_key_kept(ki);
        if (head) {
            heads++;
            sum -= ki;
            if (x < out_cap)
                out[x].low = ki;
        }
        if (last) {
            sum += mi;
            if (x < out_cap)
                out[x].high = mi;
        }
    }
    // the workgroup's sums, wave by wave
    for (uint32_t d = kWave / 2; d; d >>= 1) {
        sum += __shfl_down(sum, d);
        heads += __shfl_down(heads, d);
        kept += __shfl_down(kept, d);
    }
    const uint32_t w = threadIdx.x / kWave;
    if (lane_id() == 0) {
        lsum[w] = sum;
        lheads[w] = heads;
        lkept[w] = kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        gc_part p{0, 0, 0};
        for (uint32_t k = 0; k < kGcScanThreads / kWave; k++) {
            p.sum += lsum[k];
            p.heads += lheads[k];
            p.kept += lkept[k];
        }
        part[blockIdx.x] = p;
    }
}

// One workgroup over the tiles' sums.  stat may sit at any 8-byte alignment.
__global__ __launch_bounds__(kStatThreads) void gc_stat_kernel(const gc_part* __restrict__ part, uint32_t tiles,
                                                               const uint64_t* __restrict__ runmax, uint32_t n,
                                                               pom_gc_stat* __restrict__ stat)
{
    __shared__ uint64_t lsum[kStatThreads / kWave], lheads[kStatThreads / kWave], lkept[kStatThreads / kWave];
    uint64_t sum = 0, heads = 0, kept = 0;
    for (uint32_t t = threadIdx.x; t < tiles; t += kStatThreads) {
        sum += part[t].sum;
        heads += part[t].heads;
        kept += part[t].kept;
    }
    for (uint32_t d = kWave / 2; d; d >>= 1) {
        sum += __shfl_down(sum, d);
        heads += __shfl_down(heads, d);
        kept += __shfl_down(kept, d);
    }
    const uint32_t w = threadIdx.x / kWave;
    if (lane_id() == 0) {
        lsum[w] = sum;
        lheads[w] = heads;
        lkept[w] = kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = heads = kept = 0;
        for (uint32_t k = 0; k < kStatThreads / kWave; k++) {
            sum += lsum[k];
            heads += lheads[k];
            kept += lkept[k];
        }
        stat->valid = sum;
        stat->max = n ? runmax[n - 1] : 0ull;
        stat->nout = heads;
        stat->nin = n;
        stat->nwrapped = n - kept;
    }
}

}  // namespace

extern "C" size_t pom_gc_merge_scratch(uint32_t n)
{
    return n > kGcMergeMaxN ? 0 : gc_merge_scratch_layout(n).total;
}

extern "C" int pom_gc_merge_dev(const struct pom_gc_range* in, uint32_t n, void* scratch, size_t scratch_bytes,
                                struct pom_gc_range* out, uint64_t out_cap, struct pom_gc_stat* stat, void* stream)
{
    if (n > kGcMergeMaxN || ((uintptr_t)scratch & 7u) != 0)
        return -1;
    const gc_merge_layout L = gc_merge_scratch_layout(n);
    if (scratch_bytes < L.total)
        return -1;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* base = static_cast<uint8_t*>(scratch);
    uint64_t* key[2] = {reinterpret_cast<uint64_t*>(base + L.o_key[0]), reinterpret_cast<uint64_t*>(base + L.o_key[1])};
    uint64_t* val[2] = {reinterpret_cast<uint64_t*>(base + L.o_val[0]), reinterpret_cast<uint64_t*>(base + L.o_val[1])};
    uint32_t* table = reinterpret_cast<uint32_t*>(base + L.o_table);
    uint64_t* agg = reinterpret_cast<uint64_t*>(base + L.o_agg);
    gc_part* part = reinterpret_cast<gc_part*>(base + L.o_part);
    if (n) {
        hipLaunchKernelGGL(gc_prep_kernel, dim3(gc_merge_tiles(n, 256)), dim3(256), 0, s, in, n, key[0], val[0]);
        for (uint32_t pass = 0; pass < kGcPasses; pass++) {
            const uint32_t a = pass & 1u, b = a ^ 1u;
            hipLaunchKernelGGL(gc_hist_kernel, dim3(L.sort_tiles), dim3(kGcSortThreads), 0, s, key[a], n, pass, table);
            launch_scan(TableIn{table}, L.table_len, reinterpret_cast<uint32_t*>(agg), table, s);
            hipLaunchKernelGGL(gc_scatter_kernel, dim3(L.sort_tiles), dim3(kGcSortThreads), 0, s, key[a], val[a], n,
                               pass, table, key[b], val[b]);
        }
        uint64_t* runmax = key[1];
        uint32_t* kidx = reinterpret_cast<uint32_t*>(val[1]);
        launch_scan(HighIn{key[0], val[0]}, n, agg, runmax, s);
        launch_scan(HeadIn{key[0], runmax}, n, reinterpret_cast<uint32_t*>(agg), kidx, s);
        hipLaunchKernelGGL(gc_emit_kernel, dim3(L.range_tiles), dim3(kGcScanThreads), 0, s, key[0], runmax, kidx, n, out,
                           out_cap, part);
    }
    hipLaunchKernelGGL(gc_stat_kernel, dim3(1), dim3(kStatThreads), 0, s, part, L.range_tiles, key[1], n, stat);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
