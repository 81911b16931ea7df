// itb_sweep.hip -- the ITB sweep on gfx950 (include/pom_sweep.h; the rules are
// itb_sweep.h's).  It runs behind the check (itb_check.hip), whose err and
// report it reads.  One workgroup of 256 lanes per ITB, one launch:
//   load    the bitmap and index table (8320 bytes) go to LDS with 16-byte
//           loads; then one live ITE a lane: its flag word is the only ITE
//           byte the rules need, kept as one bit a wave ballot collects (per
//           ITE, not per slot, so that it stays right when a head swap moves
//           two entries).
//   count   one home slot a lane: itb_sweep_chain_dc, dry.  The chains' dc and
//           marked counts ride one workgroup prefix sum as a packed word; the
//           budget's stop slot is the lowest used home slot whose inclusive dc
//           reaches the budget (an LDS atomicMin), and `removed` is the
//           marked prefix there: rule 4 is decided before anything is edited.
//   edit    one chain a lane, up to the stop slot: itb_sweep_chain edits the
//           index in LDS -- chains of a table the check passes are disjoint --
//           and puts its deletes at the chain's prefix offset of the list, so
//           the list is in the loop's order; the lane clears its ITEs' bitmap
//           bits with LDS atomicAnd.
//   fold    lane 0: itb_sweep_fold over the list, at most d LDS reads.
//   store   all lanes: the bitmap and index in place, 16-byte vector stores;
//           the result's eight dwords, a lane each.
// An ITB that ends in an error, or with nothing removed, stores its result and
// nothing else: all stores come behind the last rule.
//
// LDS: the index table of 8 KiB, two bitmaps of 128 B, the list of 2 KiB and
// the counters: 10.6 KiB a workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_sweep.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kSweepThreads = 256;
constexpr uint32_t kSweepWaves = kSweepThreads / 64;
// then a grid stride: a workgroup takes ITB b, b + 4096, ... in the same LDS
// (tests/test_gpu_itb_sweep.py test_dev_many_itbs_reuse_the_workgroup quotes the 4096)
constexpr uint32_t kSweepGridMax = 4096;
constexpr uint32_t kHeadGranules = (POM_ITB_BITMAP_BYTES + POM_ITB_INDEX_SIZE * POM_ITB_INDEX_ENTRIES) / 16;  // 520
constexpr uint32_t kBitmapGranules = POM_ITB_BITMAP_BYTES / 16;                                              // 8
constexpr uint32_t kRounds = kItbCheckItes / kSweepThreads;     // home slots a lane: j = 256 r + tid
static_assert(kRounds == 4, "the count and edit phases keep four chains' counts in registers");

// A workgroup reuses this for every ITB it takes and rewrites only what the
// next ITB reads: T.ub's words below d / 64 and T.list[k] for k < removed.
// What lies beyond is stale, and safe only because every entry is checked
// against d and every k against removed before it is an index.
struct alignas(16) SweepLds {
    itb_sweep_state T;              // idx and bm lie at multiples of 16
    uint32_t wsum[kSweepWaves];     // the waves' totals of one scan round
    uint32_t stop;                  // the budget's stop slot; d: none
    uint32_t upto;                  // the packed inclusive prefix at the last slot swept
    uint32_t bad;                   // a chain walk met what a passing check rules out
};
static_assert(offsetof(itb_sweep_state, idx) % 16 == 0 && offsetof(itb_sweep_state, bm) % 16 == 0, "16-byte LDS accesses");

// Granule g of the bitmap and index in LDS.
__device__ __forceinline__ uint4* head_granule(uint64_t* bm, uint32_t* idx, uint32_t g)
{
    return g < kBitmapGranules ? reinterpret_cast<uint4*>(bm) + g : reinterpret_cast<uint4*>(idx) + (g - kBitmapGranules);
}

__global__ __launch_bounds__(kSweepThreads) void itb_sweep_kernel(
    uint8_t* payload, const uint64_t* __restrict__ payload_off, const uint8_t* __restrict__ adepth,
    const pom_check_hdr* __restrict__ hdr, const uint32_t* __restrict__ budget, uint32_t nitb,
    const uint32_t* __restrict__ ck_report, const int32_t* __restrict__ ck_err, uint32_t* __restrict__ result)
{
    __shared__ SweepLds S;
    itb_sweep_state& T = S.T;
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (uint32_t b = blockIdx.x; b < nitb; b += gridDim.x) {
        // ---- rules 1 ... 3: everything here is uniform over the workgroup
        int32_t e = ck_err[b];
        const uint64_t poff = payload_off[b];
        if (e == 0)
            e = itb_sweep_precheck(poff);
        if (e == 0 && (ck_report[12u * b] & ~(1u << POM_CK_E_MISPLACED)))
            e = POM_SPLIT_E_DAMAGED;
        uint32_t removed = 0;
        if (e == 0) {
            // (the check has passed adepth, and the highest live ITE lies inside the payload)
            uint8_t* p = payload + poff;
            const uint32_t d = 1u << adepth[b];
            const uint32_t limit = budget ? budget[b] : POM_SWEEP_NO_BUDGET;

            // ---- load
            for (uint32_t g = tid; g < kHeadGranules; g += kSweepThreads)
                *head_granule(T.bm, T.idx, g) = *reinterpret_cast<const uint4*>(p + POM_ITB_BITMAP_OFF + 16u * g);
            if (tid == 0) {
                itb_sweep_counts_of(T, hdr[b]);
                S.stop = d;
                S.upto = 0;
                S.bad = 0;
            }
            __syncthreads();
            for (uint32_t nr = tid; nr < ((d + 63u) & ~63u); nr += kSweepThreads) {
                bool marked = false;
                if (nr < d && itb_sweep_bit(T.bm, nr))
                    marked = itb_sweep_marked(*reinterpret_cast<const uint32_t*>(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr +
                                                                                 POM_ITE_FLAG_OFF));
                const uint64_t m = wave_ballot(marked);
                if (lane == 0)
                    T.ub[nr >> 6] = m;
            }
            __syncthreads();

            // ---- count: the chains' packed counts and their exclusive prefix, four home slots a lane
            uint32_t count[kRounds] = {0, 0, 0, 0}, before[kRounds] = {0, 0, 0, 0};
            uint32_t carry = 0;
#pragma unroll
            for (uint32_t r = 0; r < kRounds; r++) {
                if (r * kSweepThreads >= d)                         // (uniform)
                    break;
                const uint32_t j = r * kSweepThreads + tid;
                uint32_t c = 0;
                bool used = false;
                if (j < d) {
                    used = itb_split_flag(T.idx[j]) != POM_IDX_FREE;
                    c = itb_sweep_chain_dc(T.idx, T.ub, d, j);
                    if (c == kItbSweepBad) {
                        S.bad = 1;
                        c = 0;
                    }
                }
                uint32_t incl = wave_incl_scan(c);
                if (lane == 63)
                    S.wsum[wave] = incl;
                __syncthreads();
                uint32_t total = 0;
                for (uint32_t w = 0; w < kSweepWaves; w++) {
                    if (w == wave)
                        incl += carry + total;
                    total += S.wsum[w];
                }
                carry += total;
                count[r] = c;
                before[r] = incl - c;
                if (used && (incl & 0xFFFFu) >= limit)
                    atomicMin(&S.stop, j);
                __syncthreads();                                    // the next round rewrites wsum
            }
            const uint32_t stop = S.stop;
            const uint32_t last = stop < d ? stop : d - 1u;
#pragma unroll
            for (uint32_t r = 0; r < kRounds; r++)
                if (r * kSweepThreads + tid == last)
                    S.upto = before[r] + count[r];
            __syncthreads();
            const uint32_t upto = S.upto;
            removed = upto >> kItbSweepRemShift;
            if (S.bad)
                e = POM_SPLIT_E_DAMAGED;

            // ---- rule 4, then the edit phase
            if (e == 0 && removed != 0) {
#pragma unroll
                for (uint32_t r = 0; r < kRounds; r++) {
                    const uint32_t j = r * kSweepThreads + tid, mine = count[r] >> kItbSweepRemShift;
                    if (j <= last && mine != 0) {
                        const uint32_t at = before[r] >> kItbSweepRemShift;
                        if (itb_sweep_chain(T.idx, T.ub, d, j, T.list, at) != count[r])
                            S.bad = 1;
                        else
                            for (uint32_t k = 0; k < mine; k++) {
                                const uint32_t nr = T.list[at + k] & (kItbSweepOver - 1u);
                                atomicAnd(reinterpret_cast<uint32_t*>(T.bm) + (nr >> 5), ~(1u << (nr & 31u)));
                            }
                    }
                }
                __syncthreads();
                if (S.bad)
                    e = POM_SPLIT_E_DAMAGED;
                if (e == 0) {
                    // ---- fold
                    if (tid == 0) {
                        T.removed = removed;
                        T.dc = upto & 0xFFFFu;
                        T.visited = stop < d ? stop + 1u : d;
                        itb_sweep_fold(T.h, T.list, removed);
                    }
                    // ---- store: the bitmap and index in place
                    for (uint32_t g = tid; g < kHeadGranules; g += kSweepThreads)
                        *reinterpret_cast<uint4*>(p + POM_ITB_BITMAP_OFF + 16u * g) = *head_granule(T.bm, T.idx, g);
                    __syncthreads();
                }
            }
        }
        // ---- the result: eight dwords, a lane each
        if (tid < 8) {
            uint32_t v;
            if (e == 0 && removed != 0)
                v = itb_sweep_result_word(T, tid);
            else
                v = tid == 0 ? (uint32_t)e : 0u;
            result[8u * b + tid] = v;
        }
        __syncthreads();                                // the next ITB reuses the LDS
    }
}

// The encoder's source lengths of a chunk's nitb payloads, from the results: 0
// where nothing is produced.
__global__ __launch_bounds__(kSweepThreads) void itb_sweep_lens_kernel(const uint32_t* __restrict__ result,
                                                                       uint32_t nitb, uint32_t* __restrict__ len)
{
    const uint32_t b = blockIdx.x * kSweepThreads + threadIdx.x;
    if (b >= nitb)
        return;
    const bool produced = result[8u * b] == 0u && result[8u * b + 1u] != 0u;
    len[b] = produced ? result[8u * b + 3u] - (POM_ITB_SIZE - POM_ITB_ITE_OFF) : 0u;
}

}  // namespace

extern "C" int lzo_mi355x_launch_itb_sweep_lens(const struct pom_sweep_result* result, uint32_t nitb, uint32_t* len,
                                                hipStream_t stream)
{
    if (nitb == 0)
        return 0;
    hipLaunchKernelGGL(itb_sweep_lens_kernel, dim3((nitb + kSweepThreads - 1) / kSweepThreads), dim3(kSweepThreads), 0,
                       stream, reinterpret_cast<const uint32_t*>(result), nitb, len);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzo_mi355x_launch_itb_sweep(uint8_t* payload, const uint64_t* payload_off, const uint8_t* adepth,
                                           const struct pom_check_hdr* hdr, const uint32_t* budget, uint32_t nitb,
                                           const struct pom_check_report* ck_report, const int32_t* ck_err,
                                           struct pom_sweep_result* result, hipStream_t stream)
{
    if (nitb == 0)
        return 0;
    const uint32_t grid = nitb < kSweepGridMax ? nitb : kSweepGridMax;
    hipLaunchKernelGGL(itb_sweep_kernel, dim3(grid), dim3(kSweepThreads), 0, stream, payload, payload_off, adepth, hdr,
                       budget, nitb, reinterpret_cast<const uint32_t*>(ck_report), ck_err,
                       reinterpret_cast<uint32_t*>(result));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
