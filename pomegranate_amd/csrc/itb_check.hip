// itb_check.hip -- the ITB check on gfx950 (include/pom_check.h; the rules are
// itb_check.h's).  One workgroup of 256 lanes per ITB, one launch:
//   stage   the 128-byte bitmap and the 8 KiB index table go to LDS through
//           itb_scan_ld64, a u64 a lane a step; after that the only global
//           loads are one hash word per live ITE below d.
//   A       slots: wave w takes slots 64 * (4r + w) + lane in round r.  Kinds
//           0 ... 6 and `used` are ballots, so a wave's 64 slots are one u64
//           of a per-kind bitmap that lane 0 stores whole: no atomics.  indeg
//           and refs scatter by target, so they are two bitmaps each, "seen
//           once" and "seen twice": atomicOr on the first, and on the second
//           when the old value already had the bit.  Whatever the order of the
//           lanes, `once` ends as indeg >= 1 and `twice` as indeg >= 2.
//           ITEs: one live ITE a lane; hash & (d - 1) goes to LDS as a u16, so
//           that pass B never leaves LDS; kind 15 is a ballot.
//   B       one used home slot a lane walks its chain in LDS (itb_check_walk,
//           bounded by d + 1 slots).  Reached and misfiled marks are atomicOr
//           without a result, S_LOOP is a ballot, `longest` an atomicMax.
//   C       word-wise: kinds 7 ... 9 from used / once / twice / reached, 12
//           ... 14 from the bitmap and refs; every count is a popcount of a
//           kind's bitmap, added up with an LDS atomicAdd (integer, so the
//           order does not matter).  Twelve lanes store the report's twelve
//           dwords; the masks are stored by the lanes that OR them together.
// Because every finding is a bit of a bitmap, nothing is counted twice when
// two chains share a slot or a walk goes round a cycle, and the result does
// not depend on how lanes are scheduled.
//
// LDS: 8 KiB of table, 2 KiB of hash bits, 17 slot bitmaps of 256 B, the
// staged bitmap and 3 ITE bitmaps of 128 B, the counters: 14.8 KiB a
// workgroup.  Of the 160 KiB a CU has that allows 10 workgroups; the kernel's
// 70 VGPRs allow 7 waves a SIMD, 7 workgroups of 4 waves a CU, so registers,
// not LDS, bound occupancy.
// Banks: pass A reads the table as consecutive dwords (conflict-free), a
// ballot's u64 is stored by one lane; the scattered atomicOr of indeg / refs
// and pass B's chain hops hit banks at random, as any pointer chase does --
// in a table the MDS built most home slots are UNIQUE and never hop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_check.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kCheckThreads = 256;
constexpr uint32_t kCheckWaves = kCheckThreads / kWave;
// then a grid stride: a workgroup takes ITB b, b + 4096, ... in the same LDS
// (tests/test_gpu_check.py test_dev_many_itbs_reuse_the_workgroup quotes the 4096)
constexpr uint32_t kCheckGridMax = 4096;
constexpr uint32_t kSlotWords = POM_CK_SLOT_MASK_WORDS, kIteWords = POM_CK_ITE_MASK_WORDS;

// slot bitmaps beyond kinds 0 ... 11
enum { SB_USED = kItbCheckSlotKinds, SB_ONCE, SB_TWICE, SB_REACHED, SB_MASK, SB_N };
// ITE bitmaps: kind 15, and refs seen once and twice (kinds 12 ... 14 follow from them in pass C)
enum { IB_MISPLACED, IB_ONCE, IB_TWICE, IB_N };
// counters: kinds 0 ... 15, then
enum { CT_USED_HOME = kItbCheckCounted, CT_USED_OVER, CT_REACHED, CT_LONGEST, CT_N };

struct CheckLds {
    uint64_t index[kItbCheckSlots / 2];             // two slots a word, as in the payload
    uint64_t bitmap[kIteWords];
    uint64_t sb[SB_N][kSlotWords];
    uint64_t ib[IB_N][kIteWords];
    uint32_t ct[CT_N];
    uint16_t home[kItbCheckItes];                   // hash & (d - 1) of a live ITE below d
};

__device__ __forceinline__ void lds_or(uint64_t* w, uint64_t bit)
{
    atomicOr(reinterpret_cast<unsigned long long*>(w), (unsigned long long)bit);
}

__device__ __forceinline__ uint64_t lds_or_old(uint64_t* w, uint64_t bit)
{
    return atomicOr(reinterpret_cast<unsigned long long*>(w), (unsigned long long)bit);
}

// itb_check_walk's table over LDS.
struct LdsTable {
    CheckLds& S;
    __device__ __forceinline__ itb_find_slot slot(uint32_t s) const
    {
        const uint32_t v = (uint32_t)(S.index[s >> 1] >> (32u * (s & 1u)));
        constexpr uint32_t mask = (1u << POM_IDX_ENTRY_BITS) - 1u;
        return itb_find_slot{v & mask, (v >> POM_IDX_ENTRY_BITS) & mask, v >> POM_IDX_FLAG_SHIFT};
    }
    __device__ __forceinline__ bool live(uint32_t nr) const { return (S.bitmap[nr >> 6] >> (nr & 63u)) & 1u; }
    __device__ __forceinline__ uint32_t home(uint32_t nr) const { return S.home[nr]; }
    __device__ __forceinline__ void reach(uint32_t s) { lds_or(&S.sb[SB_REACHED][s >> 6], 1ull << (s & 63u)); }
    __device__ __forceinline__ void misfile(uint32_t s)
    {
        lds_or(&S.sb[POM_CK_S_MISFILED][s >> 6], 1ull << (s & 63u));
    }
};

// The bits of word w (64 a word) that lie in [lo, hi).
__device__ __forceinline__ uint64_t span_bits(uint32_t w, uint32_t lo, uint32_t hi)
{
    const uint32_t base = 64u * w;
    const uint32_t a = lo > base ? lo - base : 0u, b = hi > base ? hi - base : 0u;
    const uint64_t below_b = b >= 64u ? ~0ull : (1ull << b) - 1ull;
    const uint64_t below_a = a >= 64u ? ~0ull : (1ull << a) - 1ull;
    return below_b & ~below_a;
}

__global__ __launch_bounds__(kCheckThreads) void itb_check_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint32_t* __restrict__ payload_len, const int32_t* __restrict__ status,
    const uint8_t* __restrict__ adepth, const pom_check_hdr* __restrict__ hdr, uint32_t nitb, uint32_t flags,
    uint32_t* __restrict__ report, uint64_t* __restrict__ slot_mask, uint64_t* __restrict__ ite_mask,
    int32_t* __restrict__ err)
{
    __shared__ CheckLds S;
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    LdsTable T{S};
    for (uint32_t b = blockIdx.x; b < nitb; b += gridDim.x) {
        // ---- the error rules: everything here is uniform over the workgroup
        int32_t e = status ? status[b] : 0;
        const uint8_t* p = payload + payload_off[b];
        const uint32_t n = payload_len[b], ad = adepth[b];
        if (e == 0)
            e = itb_check_precheck(n, ad);
        uint32_t live = 0, top = 0;
        if (e == 0) {
            if (tid < kIteWords)
                S.bitmap[tid] = itb_scan_ld64(p + POM_ITB_BITMAP_OFF + 8u * tid);
            __syncthreads();
            const uint32_t rounds = itb_scan_rounds(ad);
            for (uint32_t r = 0; r < rounds; r++) {
                const uint64_t w = S.bitmap[r] & span_bits(r, 0, 1u << ad);
                live += (uint32_t)__popcll(w);
                if (w)
                    top = itb_scan_top(w, r);
            }
            if (live && !itb_scan_ite_inside(top, n))
                e = POM_GC_E_TRUNCATED;
        }
        if (e != 0) {
            if (tid < 12)
                report[12u * b + tid] = tid == 1 ? live : 0u;
            if (slot_mask && tid < kSlotWords)
                slot_mask[kSlotWords * b + tid] = 0;
            if (ite_mask && tid < kIteWords)
                ite_mask[kIteWords * b + tid] = 0;
            if (tid == 0)
                err[b] = e;
            __syncthreads();                        // the next ITB restages the bitmap
            continue;
        }
        const uint32_t d = 1u << ad;

        // ---- stage the index table, clear the bitmaps and counters
        for (uint32_t i = tid; i < kItbCheckSlots / 2; i += kCheckThreads)
            S.index[i] = itb_scan_ld64(p + POM_ITB_INDEX_OFF + 8u * i);
        for (uint32_t i = tid; i < SB_N * kSlotWords; i += kCheckThreads)
            (&S.sb[0][0])[i] = 0;
        if (tid < IB_N * kIteWords)
            (&S.ib[0][0])[tid] = 0;
        if (tid < CT_N)
            S.ct[tid] = 0;
        __syncthreads();

        // ---- pass A, slots
        for (uint32_t w = wave; w < kSlotWords; w += kCheckWaves) {
            const uint32_t s = 64u * w + lane;
            const itb_find_slot v = T.slot(s);
            const bool target_used = itb_check_link_inside(v, s, d) && T.slot(v.conflict).flag != POM_IDX_FREE;
            const bool entry_live = s < 2u * d && v.entry < d && T.live(v.entry);
            const uint32_t k = itb_check_local(s, v, d, target_used, entry_live);
            const uint64_t used = wave_ballot(v.flag != POM_IDX_FREE);
            if (used == 0)
                continue;                           // (wave-uniform)
            if (lane == 0)
                S.sb[SB_USED][w] = used;
            for (uint32_t kind = 0; kind <= POM_CK_S_ENTRY_DEAD; kind++) {
                const uint64_t m = wave_ballot((k >> kind) & 1u);
                if (lane == 0 && m)
                    S.sb[kind][w] = m;
            }
            if (k & kItbCheckGood) {
                const uint64_t bit = 1ull << (v.conflict & 63u);
                if (lds_or_old(&S.sb[SB_ONCE][v.conflict >> 6], bit) & bit)
                    lds_or(&S.sb[SB_TWICE][v.conflict >> 6], bit);
            }
            if (k & kItbCheckRef) {
                const uint64_t bit = 1ull << (v.entry & 63u);
                if (lds_or_old(&S.ib[IB_ONCE][v.entry >> 6], bit) & bit)
                    lds_or(&S.ib[IB_TWICE][v.entry >> 6], bit);
            }
        }
        // ---- pass A, ITEs: the one global load per live ITE
        const bool by_itbid = hdr && (flags & POM_CK_ITBID);
        for (uint32_t w = wave; 64u * w < d; w += kCheckWaves) {
            const uint32_t nr = 64u * w + lane;
            const bool is_live = nr < d && T.live(nr);
            bool misplaced = false;
            if (is_live) {
                const uint64_t hash = itb_scan_ld64(p + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr + POM_ITE_HASH_OFF);
                S.home[nr] = (uint16_t)((uint32_t)hash & (d - 1u));
                misplaced = by_itbid && itb_check_misplaced(hash, hdr[b]);
            }
            const uint64_t m = wave_ballot(misplaced);
            if (lane == 0 && m)
                S.ib[IB_MISPLACED][w] = m;
        }
        __syncthreads();

        // ---- pass B: one used home slot a lane
        for (uint32_t w = wave; 64u * w < d; w += kCheckWaves) {
            const uint32_t h = 64u * w + lane;
            bool looped = false;
            if (h < d && ((S.sb[SB_USED][w] >> lane) & 1u)) {
                const uint32_t len = itb_check_walk(T, h, d);
                looped = len == kItbCheckLooped;
                if (!looped)
                    atomicMax(&S.ct[CT_LONGEST], len);
            }
            const uint64_t m = wave_ballot(looped);
            if (lane == 0 && m)
                S.sb[POM_CK_S_LOOP][w] = m;
        }
        __syncthreads();

        // ---- pass C: a word a lane.  Slot words first, then the ITE words.
        if (tid < kSlotWords) {
            const uint32_t w = tid;
            const uint64_t used = S.sb[SB_USED][w], over = used & span_bits(w, d, 2u * d);
            const uint64_t once = S.sb[SB_ONCE][w], twice = S.sb[SB_TWICE][w], reached = S.sb[SB_REACHED][w];
            S.sb[POM_CK_S_SHARED][w] = over & twice;
            S.sb[POM_CK_S_LEAKED][w] = over & ~once;
            S.sb[POM_CK_S_ISLAND][w] = over & once & ~reached;
            uint64_t any = 0;
            for (uint32_t kind = 0; kind < kItbCheckSlotKinds; kind++) {
                const uint64_t m = S.sb[kind][w];
                any |= m;
                if (m)
                    atomicAdd(&S.ct[kind], (uint32_t)__popcll(m));
            }
            S.sb[SB_MASK][w] = any;
            atomicAdd(&S.ct[CT_USED_HOME], (uint32_t)__popcll(used & span_bits(w, 0, d)));
            atomicAdd(&S.ct[CT_USED_OVER], (uint32_t)__popcll(over));
            atomicAdd(&S.ct[CT_REACHED], (uint32_t)__popcll(reached));
            if (slot_mask)
                slot_mask[kSlotWords * b + w] = any;
        } else if (tid >= kWave && tid < kWave + kIteWords) {
            const uint32_t w = tid - kWave;
            const uint64_t bits = S.bitmap[w], below = span_bits(w, 0, d);
            const uint64_t once = S.ib[IB_ONCE][w], twice = S.ib[IB_TWICE][w];
            const uint64_t kinds[4] = {bits & ~below, twice & below, bits & below & ~once,
                                       S.ib[IB_MISPLACED][w]};
            uint64_t any = 0;
            for (uint32_t i = 0; i < 4; i++) {
                any |= kinds[i];
                if (kinds[i])
                    atomicAdd(&S.ct[kItbCheckSlotKinds + i], (uint32_t)__popcll(kinds[i]));
            }
            if (ite_mask)
                ite_mask[kIteWords * b + w] = any;
        }
        __syncthreads();

        // ---- the report: twelve dwords, a lane each
        if (tid < 12) {
            uint32_t findings = 0;
            for (uint32_t kind = 0; kind < kItbCheckCounted; kind++)
                findings |= (S.ct[kind] != 0 ? 1u : 0u) << kind;
            if (hdr)
                findings |= itb_check_header(hdr[b], d, live, top, S.ct[CT_USED_OVER]);
            uint32_t v;
            if (tid == 0)
                v = findings;
            else if (tid == 1)
                v = live;
            else if (tid == 2)
                v = S.ct[CT_USED_HOME] | S.ct[CT_USED_OVER] << 16;
            else if (tid == 3)
                v = S.ct[CT_REACHED] | S.ct[CT_LONGEST] << 16;
            else
                v = S.ct[2u * (tid - 4u)] | S.ct[2u * (tid - 4u) + 1u] << 16;
            report[12u * b + tid] = v;
        }
        if (tid == 0)
            err[b] = 0;
        __syncthreads();                            // the next ITB reuses the LDS
    }
}

}  // namespace

extern "C" int lzo_mi355x_launch_itb_check(const uint8_t* payload, const uint64_t* payload_off,
                                           const uint32_t* payload_len, const int32_t* status,
                                           const uint8_t* adepth, const struct pom_check_hdr* hdr, uint32_t nitb,
                                           uint32_t flags, struct pom_check_report* report, uint64_t* slot_mask,
                                           uint64_t* ite_mask, int32_t* err, hipStream_t stream)
{
    if (nitb == 0)
        return 0;
    const uint32_t grid = nitb < kCheckGridMax ? nitb : kCheckGridMax;
    hipLaunchKernelGGL(itb_check_kernel, dim3(grid), dim3(kCheckThreads), 0, stream, payload, payload_off,
                       payload_len, status, adepth, hdr, nitb, flags, reinterpret_cast<uint32_t*>(report),
                       slot_mask, ite_mask, err);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
