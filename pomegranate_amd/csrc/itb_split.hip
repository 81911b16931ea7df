// itb_split.hip -- the ITB split on gfx950 (include/pom_split.h; the rules are
// itb_split.h's).  It runs behind the check (itb_check.hip), whose err and
// report it reads.  One workgroup of 256 lanes per ITB, one launch:
//   load    O's bitmap and index table (8320 bytes) go to LDS with 16-byte
//           loads, N's bitmap and index are cleared there; then one live ITE a
//           lane: its hash word is the only ITE byte the rules need, kept as
//           16 bits (home slot, move bit).  `moved` is the sum of the waves'
//           ballots, so rule 5 is decided before anything is written.
//   index   itb_split_index on lane 0, over both tables in LDS.  The order of
//           the reference's loop decides N's ITE numbers, its overflow slots
//           and O's stale bytes, so the loop is run as it stands, not split
//           over lanes; it makes LDS accesses only.
//   copy    all lanes: N's zero lock region, its bitmap and index from LDS,
//           every moved ITE (32 lanes an ITE, 16 bytes a lane, four granules
//           in flight a lane), O's bitmap and index in place, the result's
//           twelve dwords.  Every store is a vector store.
// An ITB that ends in an error, or with nothing moved, stores its result and
// nothing else: all stores come behind the last rule.
//
// LDS: two index tables of 8 KiB, two bitmaps of 128 B, 2 KiB of ITE facts and
// 2 KiB of the new -> old ITE map, the counters: 20.6 KiB a workgroup, 7
// workgroups a CU of the 160 KiB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_split.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kSplitThreads = 256;
// then a grid stride: a workgroup takes ITB b, b + 4096, ... in the same LDS
// (tests/test_gpu_itb_split.py test_dev_many_itbs_reuse_the_workgroup quotes the 4096)
constexpr uint32_t kSplitGridMax = 4096;
constexpr uint32_t kHeadGranules = (POM_ITB_BITMAP_BYTES + POM_ITB_INDEX_SIZE * POM_ITB_INDEX_ENTRIES) / 16;  // 520
constexpr uint32_t kBitmapGranules = POM_ITB_BITMAP_BYTES / 16;                                              // 8
constexpr uint32_t kLockGranules = POM_ITB_BITMAP_OFF / 16;                                                  // 224
constexpr uint32_t kIteGranules = POM_ITE_SIZE / 16;                                                         // 32
constexpr uint32_t kInFlight = 4;
static_assert(kInFlight == 4, "the ITE copy names its four granules");

// A workgroup reuses this for every ITB it takes and rewrites only what the next
// ITB reads: T.info[nr] for nr < d and T.from[k] for k < moved.  What lies
// beyond is stale, and safe only because every entry is checked against d and
// every k against moved before it is an index.
struct alignas(16) SplitLds {
    itb_split_state T;              // oidx, nidx, obm and nbm lie at multiples of 16
    uint32_t want;                  // live ITEs with the move bit
};
static_assert(offsetof(itb_split_state, nidx) % 16 == 0 && offsetof(itb_split_state, obm) % 16 == 0 &&
              offsetof(itb_split_state, nbm) % 16 == 0, "16-byte LDS accesses");

// Granule g of a table's bitmap and index in LDS.
__device__ __forceinline__ uint4* head_granule(uint64_t* bm, uint32_t* idx, uint32_t g)
{
    return g < kBitmapGranules ? reinterpret_cast<uint4*>(bm) + g : reinterpret_cast<uint4*>(idx) + (g - kBitmapGranules);
}

__global__ __launch_bounds__(kSplitThreads) void itb_split_kernel(
    uint8_t* payload, const uint64_t* __restrict__ payload_off, const uint8_t* __restrict__ adepth,
    const pom_check_hdr* __restrict__ hdr, const uint8_t* __restrict__ split_depth, uint32_t nitb,
    uint8_t* new_payload, const uint64_t* __restrict__ new_off, const uint32_t* __restrict__ new_cap,
    const uint32_t* __restrict__ ck_report, const int32_t* __restrict__ ck_err, uint32_t* __restrict__ result)
{
    __shared__ SplitLds S;
    itb_split_state& T = S.T;
    const uint32_t tid = threadIdx.x, lane = lane_id();
    for (uint32_t b = blockIdx.x; b < nitb; b += gridDim.x) {
        // ---- rules 1 ... 4: everything here is uniform over the workgroup
        int32_t e = ck_err[b];
        const uint32_t sd = split_depth ? split_depth[b] : (uint32_t)hdr[b].depth + 1u;
        const uint64_t poff = payload_off[b], noff = new_off[b];
        if (e == 0)
            e = itb_split_precheck(sd, poff, noff);
        if (e == 0 && (ck_report[12u * b] & ~(1u << POM_CK_E_MISPLACED)))
            e = POM_SPLIT_E_DAMAGED;
        uint32_t moved = 0;
        if (e == 0) {
            // (the check has passed adepth, and the highest live ITE lies inside the payload)
            uint8_t* p = payload + poff;
            uint8_t* np = new_payload + noff;
            const uint32_t d = 1u << adepth[b];

            // ---- load
            for (uint32_t g = tid; g < kHeadGranules; g += kSplitThreads) {
                *head_granule(T.obm, T.oidx, g) = *reinterpret_cast<const uint4*>(p + POM_ITB_BITMAP_OFF + 16u * g);
                *head_granule(T.nbm, T.nidx, g) = make_uint4(0, 0, 0, 0);
            }
            if (tid == 0) {
                itb_split_sides(T, hdr[b]);
                S.want = 0;
            }
            __syncthreads();
            for (uint32_t nr = tid; nr < ((d + 63u) & ~63u); nr += kSplitThreads) {
                uint16_t info = 0;
                if (nr < d && ((T.obm[nr >> 6] >> (nr & 63u)) & 1u))
                    info = itb_split_info(*reinterpret_cast<const uint64_t*>(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr +
                                                                             POM_ITE_HASH_OFF), d, sd);
                if (nr < d)
                    T.info[nr] = info;
                const uint64_t m = wave_ballot(info & kItbSplitMove);
                if (lane == 0 && m)
                    atomicAdd(&S.want, (uint32_t)__popcll(m));
            }
            __syncthreads();
            moved = S.want;

            // ---- rules 5 and 6, then the index phase
            if (new_cap[b] < POM_ITB_ITE_OFF + POM_ITE_SIZE * moved)
                e = kItbSplitOverrun;
            if (e == 0 && moved != 0) {
                if (tid == 0) {
                    int32_t ie = itb_split_index(T, d);
                    if (ie == 0 && T.moved != moved)
                        ie = POM_SPLIT_E_DAMAGED;
                    T.err = ie;
                }
                __syncthreads();
                e = T.err;
                if (e == 0) {
                    // ---- copy: N, then O's bitmap and index in place
                    for (uint32_t g = tid; g < kLockGranules; g += kSplitThreads)
                        *reinterpret_cast<uint4*>(np + 16u * g) = make_uint4(0, 0, 0, 0);
                    for (uint32_t g = tid; g < kHeadGranules; g += kSplitThreads) {
                        *reinterpret_cast<uint4*>(np + POM_ITB_BITMAP_OFF + 16u * g) = *head_granule(T.nbm, T.nidx, g);
                        *reinterpret_cast<uint4*>(p + POM_ITB_BITMAP_OFF + 16u * g) = *head_granule(T.obm, T.oidx, g);
                    }
                    const uint32_t total = moved * kIteGranules;
                    const auto ite_granule = [&](uint32_t g) {
                        return *reinterpret_cast<const uint4*>(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * T.from[g / kIteGranules] +
                                                               16u * (g % kIteGranules));
                    };
                    uint32_t g = tid;
                    for (; g + (kInFlight - 1u) * kSplitThreads < total; g += kInFlight * kSplitThreads) {
                        const uint4 v0 = ite_granule(g), v1 = ite_granule(g + kSplitThreads);
                        const uint4 v2 = ite_granule(g + 2u * kSplitThreads), v3 = ite_granule(g + 3u * kSplitThreads);
                        *reinterpret_cast<uint4*>(np + POM_ITB_ITE_OFF + 16u * g) = v0;
                        *reinterpret_cast<uint4*>(np + POM_ITB_ITE_OFF + 16u * (g + kSplitThreads)) = v1;
                        *reinterpret_cast<uint4*>(np + POM_ITB_ITE_OFF + 16u * (g + 2u * kSplitThreads)) = v2;
                        *reinterpret_cast<uint4*>(np + POM_ITB_ITE_OFF + 16u * (g + 3u * kSplitThreads)) = v3;
                    }
                    for (; g < total; g += kSplitThreads)
                        *reinterpret_cast<uint4*>(np + POM_ITB_ITE_OFF + 16u * g) = ite_granule(g);
                }
            }
        }
        // ---- the result: twelve dwords, a lane each
        if (tid < 12) {
            uint32_t v;
            if (e == 0 && moved != 0)
                v = itb_split_result_word(T, tid);
            else
                v = tid == 0 ? (uint32_t)e : tid == 1 && e == kItbSplitOverrun ? moved : 0u;
            result[12u * b + tid] = v;
        }
        __syncthreads();                                // the next ITB reuses the LDS
    }
}

// The encoder's source lengths of a chunk's 2 * nitb halves, from the results:
// half 0 the old payloads, half 1 the new ones; 0 where nothing is produced.
__global__ __launch_bounds__(kSplitThreads) void itb_split_lens_kernel(const uint32_t* __restrict__ result,
                                                                       uint32_t nitb, uint32_t* __restrict__ len)
{
    const uint32_t b = blockIdx.x * kSplitThreads + threadIdx.x;
    if (b >= nitb)
        return;
    const bool produced = result[12u * b] == 0u && result[12u * b + 1u] != 0u;
    len[b] = produced ? result[12u * b + 2u] - (POM_ITB_SIZE - POM_ITB_ITE_OFF) : 0u;
    len[nitb + b] = produced ? result[12u * b + 3u] - (POM_ITB_SIZE - POM_ITB_ITE_OFF) : 0u;
}

}  // namespace

extern "C" int lzo_mi355x_launch_itb_split_lens(const struct pom_split_result* result, uint32_t nitb, uint32_t* len,
                                                hipStream_t stream)
{
    if (nitb == 0)
        return 0;
    hipLaunchKernelGGL(itb_split_lens_kernel, dim3((nitb + kSplitThreads - 1) / kSplitThreads), dim3(kSplitThreads), 0,
                       stream, reinterpret_cast<const uint32_t*>(result), nitb, len);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzo_mi355x_launch_itb_split(uint8_t* payload, const uint64_t* payload_off, const uint8_t* adepth,
                                           const struct pom_check_hdr* hdr, const uint8_t* split_depth, uint32_t nitb,
                                           uint8_t* new_payload, const uint64_t* new_off, const uint32_t* new_cap,
                                           const struct pom_check_report* ck_report, const int32_t* ck_err,
                                           struct pom_split_result* result, hipStream_t stream)
{
    if (nitb == 0)
        return 0;
    const uint32_t grid = nitb < kSplitGridMax ? nitb : kSplitGridMax;
    hipLaunchKernelGGL(itb_split_kernel, dim3(grid), dim3(kSplitThreads), 0, stream, payload, payload_off, adepth, hdr,
                       split_depth, nitb, new_payload, new_off, new_cap, reinterpret_cast<const uint32_t*>(ck_report),
                       ck_err, reinterpret_cast<uint32_t*>(result));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
