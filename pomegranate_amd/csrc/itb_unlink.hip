// itb_unlink.hip -- the ITB unlink on gfx950 (include/pom_unlink.h; the rules
// are itb_unlink.h's).  It runs behind the check (itb_check.hip), whose err and
// report it reads.  One workgroup of 256 lanes per ITB, one launch:
//   load    the bitmap and index table (8320 bytes) go to LDS with 16-byte
//           loads; then one live ITE a lane: its flag word and its (mode,
//           nlink) word, the only ITE bytes a request can change, into two LDS
//           tables.  Everything a request changes stays in LDS until the end,
//           so no request has to see another's global store.
//   apply   wave 0 alone, the ITB's requests in the caller's order.  Per
//           request lane 0 walks the chain in LDS and lists up to 64 members
//           (itb_unlink_list); lane k matches member k (itb_unlink_member: the
//           state from LDS; uuid, hash, namelen and name from the payload), so
//           a chain costs one dependent memory round trip a round, not one a
//           member; the ballot's lowest lane is the hit.  Lanes 0 ... 16 store
//           the record, eight bytes each, with mode and nlink from LDS; lane
//           0 applies ite_unlink and itb_del_ite to LDS (itb_unlink_apply).
//   store   all lanes, behind the last rule: the bitmap and index in place
//           with 16-byte vector stores when a delete happened, the flag and
//           nlink of the ITEs a request changed, the result's eight dwords.
// An ITB that ends in an error stores its result, its requests' codes and zero
// records, and nothing else.
//
// LDS: the index table of 8 KiB, the two ITE tables of 4 KiB each, two bitmaps
// of 128 B, a round's member list and the counters: 16.5 KiB a workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_unlink.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kUnlinkThreads = 256;
// then a grid stride: a workgroup takes ITB b, b + 4096, ... in the same LDS
// (tests/test_gpu_unlink.py test_dev_many_itbs_reuse_the_workgroup quotes the 4096)
constexpr uint32_t kUnlinkGridMax = 4096;
constexpr uint32_t kHeadGranules = (POM_ITB_BITMAP_BYTES + POM_ITB_INDEX_SIZE * POM_ITB_INDEX_ENTRIES) / 16;  // 520
constexpr uint32_t kBitmapGranules = POM_ITB_BITMAP_BYTES / 16;                                              // 8
static_assert(kItbUnlinkRound == 64, "a round is one wave's lanes");

// A workgroup reuses this for every ITB it takes and rewrites only what the
// next ITB reads: T.flag and T.mn of its live ITEs, T.dirty's 16 words.  What
// lies beyond is stale, and safe only because every entry is checked against
// d and is live (the check) before it is an index.
struct alignas(16) UnlinkLds {
    itb_unlink_state T;                 // idx and bm lie at multiples of 16
    uint16_t mslot[kItbUnlinkRound];    // a round's members: their slots
    uint16_t ment[kItbUnlinkRound];     // and ITEs
    uint32_t cnt, more;                 // lane 0's answers to its wave
    uint32_t bad;                       // a walk met what a passing check rules out
};
static_assert(offsetof(itb_unlink_state, idx) % 16 == 0 && offsetof(itb_unlink_state, bm) % 16 == 0, "16-byte LDS accesses");

// Granule g of the bitmap and index in LDS.
__device__ __forceinline__ uint4* head_granule(uint64_t* bm, uint32_t* idx, uint32_t g)
{
    return g < kBitmapGranules ? reinterpret_cast<uint4*>(bm) + g : reinterpret_cast<uint4*>(idx) + (g - kBitmapGranules);
}

// The wave's LDS writes before, its LDS reads behind (one wave's DS
// operations execute in order; this keeps the compiler from moving them).
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void store_word(uint8_t* out, uint32_t r, uint32_t w, uint64_t v)
{
    *reinterpret_cast<uint2*>(out + (uint64_t)POM_LK_REC_SIZE * r + 8u * w) = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(kUnlinkThreads) void itb_unlink_kernel(
    uint8_t* payload, const uint64_t* __restrict__ payload_off, const uint32_t* __restrict__ payload_len,
    const uint8_t* __restrict__ adepth, const pom_check_hdr* __restrict__ hdr, uint32_t nitb, uint32_t async,
    const pom_lookup_req* __restrict__ req, const uint32_t* __restrict__ req_first, uint32_t nreq,
    const uint8_t* __restrict__ names, uint32_t names_len, const uint32_t* __restrict__ ck_report,
    const int32_t* __restrict__ ck_err, int32_t* __restrict__ err, uint32_t* __restrict__ nr, uint32_t* __restrict__ depth, uint32_t* __restrict__ what,
    uint8_t* __restrict__ out, uint32_t* __restrict__ result)
{
    __shared__ UnlinkLds S;
    itb_unlink_state& T = S.T;
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (uint32_t b = blockIdx.x; b < nitb; b += gridDim.x) {
        // ---- ITB rules 1 ... 3: everything here is uniform over the workgroup
        int32_t e = ck_err[b];
        const uint64_t poff = payload_off[b];
        if (e == 0)
            e = itb_unlink_precheck(poff);
        if (e == 0 && (ck_report[12u * b] & ~(1u << POM_CK_E_MISPLACED)))
            e = POM_SPLIT_E_DAMAGED;
        // (a group that reaches past nreq is cut there: nothing outside the result arrays is written)
        const uint32_t r0 = req_first[b] < nreq ? req_first[b] : nreq;
        const uint32_t r1 = req_first[b + 1u] < nreq ? req_first[b + 1u] : nreq;
        // (the check has passed adepth, and the highest live ITE lies inside the payload)
        uint8_t* p = payload + poff;
        const uint32_t d = e == 0 ? 1u << adepth[b] : 0u, n = payload_len[b];

        // ---- load
        if (tid == 0)
            S.bad = 0;
        if (e == 0) {
            for (uint32_t g = tid; g < kHeadGranules; g += kUnlinkThreads)
                *head_granule(T.bm, T.idx, g) = *reinterpret_cast<const uint4*>(p + POM_ITB_BITMAP_OFF + 16u * g);
            if (tid == 0)
                itb_unlink_counts_of(T, hdr[b]);
            if (tid < POM_CK_ITE_MASK_WORDS)
                T.dirty[tid] = 0;
        }
        __syncthreads();
        if (e == 0) {
            for (uint32_t i = tid; i < d; i += kUnlinkThreads)
                if (itb_sweep_bit(T.bm, i)) {
                    const uint8_t* ite = p + POM_ITB_ITE_OFF + POM_ITE_SIZE * i;
                    T.flag[i] = *reinterpret_cast<const uint32_t*>(ite + POM_ITE_FLAG_OFF);
                    T.mn[i] = *reinterpret_cast<const uint32_t*>(ite + POM_ITE_MODE_OFF);
                }
        }
        __syncthreads();

        // ---- apply: wave 0, the requests in order
        if (e == 0 && wave == 0) {
            bool bad = false;
            for (uint32_t r = r0; r < r1 && !bad; r++) {
                const pom_lookup_req q = req[r];                    // (one address for the wave)
                const uint32_t home = (uint32_t)q.hash & (d - 1u);
                int32_t re = kItbFindEnoent;
                uint32_t slot = 0, entry = 0, dep = 0, did = 0;
                bool have = false;
                if (q.itb != b || !itb_unlink_req_ok(q, names_len)) {
                    re = kItbScanEinval;
                } else {
                    uint32_t offset = home;                         // (lane 0's: where the chain goes on)
                    for (;;) {
                        if (lane == 0) {
                            bool more;
                            S.cnt = itb_unlink_list(T.idx, d, n, &offset, S.mslot, S.ment, kItbUnlinkRound, &more);
                            S.more = more;
                        }
                        wave_lds_fence();
                        const uint32_t cnt = __builtin_amdgcn_readfirstlane(S.cnt);
                        const uint32_t more = __builtin_amdgcn_readfirstlane(S.more);
                        if (cnt == kItbUnlinkBad || dep + cnt > kItbUnlinkSteps) {
                            bad = true;
                            break;
                        }
                        const bool m = lane < cnt && itb_unlink_member(T, p, S.ment[lane < cnt ? lane : 0u], q, names);
                        const uint64_t mask = wave_ballot(m);
                        if (mask != 0) {
                            const uint32_t k = (uint32_t)__builtin_ctzll(mask);
                            slot = S.mslot[k];
                            entry = S.ment[k];
                            dep += k + 1u;
                            have = true;
                        } else {
                            dep += cnt;
                        }
                        wave_lds_fence();                           // the next round rewrites the list
                        if (have || !more)
                            break;
                    }
                }
                if (bad)
                    break;
                if (have) {
                    // (pure, so every lane decides rule 9 for itself)
                    const uint32_t mn = T.mn[entry];
                    if (itb_unlink_ite(T.flag[entry], mn & 0xFFFFu, mn >> 16, async != 0).what == kItbUnlinkRefused) {
                        re = kItbScanEinval;
                    } else {
                        re = 0;
                        if (lane < kItbFindRecWords)
                            store_word(out, r, lane, itb_unlink_word(T, p, entry, lane));
                        wave_lds_fence();                           // the record's reads before the unlink's writes
                        if (lane == 0)
                            S.cnt = itb_unlink_apply(T, d, async != 0, slot, home, entry);
                        wave_lds_fence();
                        did = __builtin_amdgcn_readfirstlane(S.cnt);
                        if (did == kItbUnlinkBad) {
                            bad = true;
                            break;
                        }
                    }
                }
                if (re != 0 && lane < kItbFindRecWords)
                    store_word(out, r, lane, 0);
                if (lane == 0) {
                    err[r] = re;
                    nr[r] = re == 0 ? entry : 0u;
                    depth[r] = dep;
                    what[r] = re == 0 ? did : 0u;
                }
                wave_lds_fence();
            }
            if (bad && lane == 0)
                S.bad = 1;
        }
        __syncthreads();
        if (S.bad)
            e = POM_SPLIT_E_DAMAGED;

        if (e != 0) {
            // ---- every request of the ITB reads its code
            for (uint32_t r = r0 + tid; r < r1; r += kUnlinkThreads) {
                err[r] = req[r].itb != b ? kItbScanEinval : e;
                nr[r] = depth[r] = what[r] = 0;
                for (uint32_t w = 0; w < kItbFindRecWords; w++)
                    store_word(out, r, w, 0);
            }
        } else if (T.changed != 0) {
            // ---- store: the bitmap and index in place, the ITEs a request changed
            if (T.removed != 0)
                for (uint32_t g = tid; g < kHeadGranules; g += kUnlinkThreads)
                    *reinterpret_cast<uint4*>(p + POM_ITB_BITMAP_OFF + 16u * g) = *head_granule(T.bm, T.idx, g);
            for (uint32_t i = tid; i < d; i += kUnlinkThreads)
                if (itb_sweep_bit(T.dirty, i)) {
                    uint8_t* ite = p + POM_ITB_ITE_OFF + POM_ITE_SIZE * i;
                    *reinterpret_cast<uint32_t*>(ite + POM_ITE_FLAG_OFF) = T.flag[i];
                    *reinterpret_cast<uint16_t*>(ite + POM_ITE_NLINK_OFF) = (uint16_t)(T.mn[i] >> 16);
                }
        }
        // ---- the result: eight dwords, a lane each
        if (tid < 8)
            result[8u * b + tid] = e != 0 ? (tid == 0 ? (uint32_t)e : 0u) : itb_unlink_result_word(T, tid);
        __syncthreads();                                // the next ITB reuses the LDS
    }
}

// The encoder's source lengths of a chunk's nitb payloads, from the results: 0
// where nothing is produced.
__global__ __launch_bounds__(kUnlinkThreads) void itb_unlink_lens_kernel(const uint32_t* __restrict__ result,
                                                                         uint32_t nitb, uint32_t* __restrict__ len)
{
    const uint32_t b = blockIdx.x * kUnlinkThreads + threadIdx.x;
    if (b >= nitb)
        return;
    const bool produced = result[8u * b] == 0u && result[8u * b + 1u] != 0u &&
                          result[8u * b + 3u] >= POM_ITB_SIZE - POM_ITB_ITE_OFF;
    len[b] = produced ? result[8u * b + 3u] - (POM_ITB_SIZE - POM_ITB_ITE_OFF) : 0u;
}

}  // namespace

extern "C" int lzo_mi355x_launch_itb_unlink_lens(const struct pom_unlink_result* result, uint32_t nitb, uint32_t* len,
                                                 hipStream_t stream)
{
    if (nitb == 0)
        return 0;
    hipLaunchKernelGGL(itb_unlink_lens_kernel, dim3((nitb + kUnlinkThreads - 1) / kUnlinkThreads), dim3(kUnlinkThreads), 0,
                       stream, reinterpret_cast<const uint32_t*>(result), nitb, len);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzo_mi355x_launch_itb_unlink(uint8_t* payload, const uint64_t* payload_off, const uint32_t* payload_len,
                                            const uint8_t* adepth, const struct pom_check_hdr* hdr, uint32_t nitb,
                                            int async_unlink, const struct pom_lookup_req* req,
                                            const uint32_t* req_first, uint32_t nreq, const uint8_t* names,
                                            uint32_t names_len,
                                            const struct pom_check_report* ck_report, const int32_t* ck_err,
                                            int32_t* err, uint32_t* nr, uint32_t* depth, uint32_t* what, uint8_t* out,
                                            struct pom_unlink_result* result, hipStream_t stream)
{
    if (nitb == 0)
        return 0;
    const uint32_t grid = nitb < kUnlinkGridMax ? nitb : kUnlinkGridMax;
    hipLaunchKernelGGL(itb_unlink_kernel, dim3(grid), dim3(kUnlinkThreads), 0, stream, payload, payload_off, payload_len,
                       adepth, hdr, nitb, async_unlink != 0 ? 1u : 0u, req, req_first, nreq, names, names_len,
                       reinterpret_cast<const uint32_t*>(ck_report), ck_err, err, nr, depth, what, out,
                       reinterpret_cast<uint32_t*>(result));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
