// itb_dents.hip -- the directory listing's ITB walk on gfx950
// (include/pom_readdir.h; the rules and the copy plan are itb_dents.h's).  One
// wave per ITB: in round r lane l owns bitmap bit 64r + l.  Three
// stream-ordered launches, no host round trip between them:
//   itb_dents_count_kernel  live[b], dnum[b], bytes[b], err[b]
//   itb_prefix_kernel       first[0 .. nitb] = exclusive prefix of bytes (u64; itb_prefix.h)
//   itb_dents_emit_kernel   the records, packed, at out + first[b]
// An emit round is a variable-length, byte-packed compaction: a ballot of the
// emitting lanes, a wave exclusive scan of their 16 + namelen, and the round's
// records compacted in bit order into a small LDS table {start, ITE, header}
// of the wave's own.  Then the wave copies the round's span (up to 17,408
// bytes) together: a lane takes one destination-aligned 16-byte granule a
// step, finds the one or two records that reach into it by a binary search
// over the table's starts, assembles the bytes from the headers (LDS) and the
// names (three aligned 8-byte loads inside the ITE) and issues one dwordx4
// store; only the span's head and tail, and what the cap cuts, are byte
// stores.  A payload that is not 8-byte aligned takes the same plan with its
// words loaded byte by byte (itb_scan_ld64).  No scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_dents.h"
#include "itb_prefix.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kDentsThreads = 256;             // 4 waves: 4 ITBs per workgroup
constexpr uint32_t kDentsWaves = kDentsThreads / kWave;
constexpr uint32_t kDentsGridMax = 2048;            // then a grid stride
// a prefix tile's sum fits u32: at most 278,528 bytes an ITB
static_assert((uint64_t)kPrefixThreads * kItbDentsItbMax <= 0xFFFFFFFFull, "prefix tile");

// One wave's table of a round's records (itb_dents_round).
struct DentsTable {
    itb_dents_u128 hdr[kWave];
    uint32_t start[kWave];
    uint32_t nr[kWave];
};

// The wave's LDS writes before, its LDS reads behind (one wave's DS
// operations execute in order; this keeps the compiler from moving them).
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stores by address: every address is formed from the kernel's `out`
// argument, so the stores are global ones, not flat.
struct GlobalOut {
    uint8_t* out;
    __device__ __forceinline__ uint8_t* at(uint64_t a) const { return out + (a - (uint64_t)(uintptr_t)out); }
    __device__ __forceinline__ void st16(uint64_t a, const itb_dents_u128& v) const
    {
        *reinterpret_cast<uint4*>(at(a)) =
            make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
    }
    __device__ __forceinline__ void st1(uint64_t a, uint8_t b) const { *at(a) = b; }
};

__global__ __launch_bounds__(kDentsThreads) void itb_dents_count_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint32_t* __restrict__ payload_len, const int32_t* __restrict__ status,
    const uint8_t* __restrict__ adepth, uint32_t nitb, uint32_t* __restrict__ live,
    uint32_t* __restrict__ dnum, uint32_t* __restrict__ bytes, int32_t* __restrict__ err)
{
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kDentsWaves + threadIdx.x / kWave);
    for (uint32_t b = wave; b < nitb; b += gridDim.x * kDentsWaves) {
        int32_t e = status ? status[b] : 0;
        uint32_t nl = 0, nd = 0, nb = 0;
        if (e == 0) {
            const uint8_t* p = payload + payload_off[b];
            const uint32_t n = payload_len[b], ad = adepth[b];
            e = itb_scan_precheck(n, ad);
            if (e == 0 && (e = itb_scan_live(p, n, ad, &nl)) == 0) {
                const uint32_t rounds = itb_scan_rounds(ad);
                uint32_t mine = 0;                  // this lane's record bytes over the rounds
                bool bad = false;
                for (uint32_t r = 0; r < rounds; r++) {
                    const uint64_t w = itb_scan_word(p, r, ad);
                    bool emits = false;
                    if ((w >> lane) & 1u) {
                        const uint64_t fn = itb_dents_flag_namelen(p, 64u * r + lane);
                        emits = itb_dents_emits(fn);
                        if (emits) {
                            const uint32_t namelen = itb_dents_namelen(fn);
                            bad |= !itb_dents_name_ok(namelen);
                            mine += itb_dents_name_ok(namelen) ? POM_DENT_HDR + namelen : 0u;
                        }
                    }
                    nd += (uint32_t)__popcll(wave_ballot(emits));
                }
                nb = lane_read(wave_incl_scan(mine), kWave - 1);        // at most kItbDentsItbMax
                if (wave_ballot(bad) != 0) {
                    e = POM_RD_E_NAME;
                    nd = nb = 0;
                }
            }
        }
        if (lane == 0) {
            live[b] = nl;
            dnum[b] = nd;
            bytes[b] = nb;
            err[b] = e;
        }
    }
}

// kPerLane: the alternative the wave-cooperative copy is measured against
// (debug key dents_copy=1) -- every emitting lane stores its own record byte
// by byte, 64 ways divergent, up to 272 steps.
template <bool kPerLane>
__global__ __launch_bounds__(kDentsThreads) void itb_dents_emit_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint8_t* __restrict__ adepth, uint32_t nitb, const uint32_t* __restrict__ dnum,
    const int32_t* __restrict__ err, const uint64_t* __restrict__ first, uint8_t* __restrict__ out,
    uint64_t out_cap)
{
    __shared__ DentsTable tables[kDentsWaves];
    const uint32_t lane = lane_id();
    const uint32_t wave_in_group = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t wave = blockIdx.x * kDentsWaves + wave_in_group;
    DentsTable& T = tables[wave_in_group];
    const GlobalOut mem{out};
    const uint64_t cap_end = (uint64_t)(uintptr_t)out + out_cap;
    for (uint32_t b = wave; b < nitb; b += gridDim.x * kDentsWaves) {
        // the count kernel passed this payload's checks and its names when it left err 0
        if (err[b] != 0 || dnum[b] == 0)
            continue;
        const uint8_t* p = payload + payload_off[b];
        const uint32_t ad = adepth[b];
        uint64_t at = first[b];
        const uint32_t rounds = itb_scan_rounds(ad);
        for (uint32_t r = 0; r < rounds && at < out_cap; r++) {
            const uint64_t w = itb_scan_word(p, r, ad);
            const uint32_t nr = 64u * r + lane;
            bool emits = false;
            uint32_t len = 0;
            itb_dents_u128 h{0, 0};
            if ((w >> lane) & 1u) {
                const uint64_t fn = itb_dents_flag_namelen(p, nr);
                emits = itb_dents_emits(fn);
                if (emits) {
                    h = itb_dents_header(p, nr, itb_dents_namelen(fn));
                    len = POM_DENT_HDR + itb_dents_namelen(fn);
                }
            }
            const uint64_t m = wave_ballot(emits);
            if (m == 0)
                continue;
            const uint32_t incl = wave_incl_scan(len);
            const uint32_t span = lane_read(incl, kWave - 1);           // at most 64 * 272
            if (kPerLane) {
                const uint64_t mine = (uint64_t)(uintptr_t)out + at + (incl - len);
                for (uint32_t j = 0; j < len && mine + j < cap_end; j++)
                    mem.st1(mine + j, j < 8u                  ? (uint8_t)(h.lo >> 8u * j)
                                      : j < POM_DENT_HDR ? (uint8_t)(h.hi >> 8u * (j - 8u))
                                                         : itb_dents_ite(p, nr)[POM_ITE_NAME_OFF + j - POM_DENT_HDR]);
                at += span;
                continue;
            }
            if (emits) {
                const uint32_t k = lanes_below(m);
                T.hdr[k] = h;
                T.start[k] = incl - len;
                T.nr[k] = nr;
            }
            wave_lds_fence();
            const uint64_t dst = (uint64_t)(uintptr_t)out + at;
            const itb_dents_round R{T.start, T.nr, T.hdr, (uint32_t)__popcll(m), span, p, dst,
                                    dst + span < cap_end ? dst + span : cap_end};
            const uint32_t granules = itb_dents_granules(R);
            for (uint32_t g = lane; g < granules; g += kWave)
                itb_dents_granule(mem, R, g);
            wave_lds_fence();                       // the next round rewrites the table
            at += span;
        }
    }
}

}  // namespace

extern "C" int lzo_mi355x_launch_readdir(const uint8_t* payload, const uint64_t* payload_off,
                                         const uint32_t* payload_len, const int32_t* status,
                                         const uint8_t* adepth, uint32_t nitb, uint32_t* live,
                                         uint32_t* dnum, uint32_t* bytes, uint64_t* first, uint8_t* out,
                                         uint64_t out_cap, int32_t* err, hipStream_t stream)
{
    const uint32_t need = (nitb + kDentsWaves - 1) / kDentsWaves;
    const uint32_t grid = need < kDentsGridMax ? need : kDentsGridMax;
    if (nitb)
        hipLaunchKernelGGL(itb_dents_count_kernel, dim3(grid), dim3(kDentsThreads), 0, stream, payload,
                           payload_off, payload_len, status, adepth, nitb, live, dnum, bytes, err);
    hipLaunchKernelGGL(itb_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, stream, bytes, nitb, first);
    // debug key dents_copy=1: the per-lane byte copy (measurements)
    if (nitb && out_cap)
        hipLaunchKernelGGL(pom_dbg_int("dents_copy", 0) == 1 ? itb_dents_emit_kernel<true> : itb_dents_emit_kernel<false>,
                           dim3(grid), dim3(kDentsThreads), 0, stream, payload, payload_off, adepth, nitb, dnum,
                           err, first, out, out_cap);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
