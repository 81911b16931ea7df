// itb_find.hip -- the lookup's ITB walk on gfx950 (include/pom_lookup.h; the
// rules and the record's copy plan are itb_find.h's).  One lane per request,
// one launch:
//   walk   lane l of a wave runs itb_find_one for request 64 * wave + l: a
//          chain of dependent 4-byte gathers from the index table with one
//          ITE's flag word (and its uuid and hash, or its name eight bytes a
//          step) compared per hop.  The lanes of a wave follow unrelated
//          chains, so a hop is 64 scattered loads whichever way the work is
//          cut; what hides their latency is the number of waves in flight.
//          err, nr and depth go out as three coalesced dword stores.
//   copy   the wave's 64 records are 8,704 consecutive bytes of `out`.  Each
//          lane leaves {ITE offset, column} in a small LDS table of the
//          wave's own; then a lane takes one 16-byte granule a step -- two
//          words of one record, or the last word of one and the first of the
//          next -- loads them from the ITEs and issues one dwordx4 store, 1 KiB
//          per wave instruction, where `out` is 16-byte aligned.  Otherwise
//          every lane stores its own record byte by byte.
// No atomics, no scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_find.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kFindThreads = 256;              // 4 waves: 256 requests per workgroup
constexpr uint32_t kFindWaves = kFindThreads / kWave;
constexpr uint32_t kFindGridMax = 2048;             // about what is resident at 7 waves a SIMD; then a grid stride

// One wave's table of its records' sources (itb_find_granule).
struct FindTable {
    uint64_t ite_off[kWave];
    uint32_t col[kWave];
};

// The wave's LDS writes before, its LDS reads behind (one wave's DS
// operations execute in order; this keeps the compiler from moving them).
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stores at byte offsets of the wave's span, which is 16-byte aligned.
struct SpanOut {
    uint8_t* span;
    __device__ __forceinline__ void st16(uint32_t o, uint64_t lo, uint64_t hi) const
    {
        *reinterpret_cast<uint4*>(span + o) =
            make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    __device__ __forceinline__ void st8(uint32_t o, uint64_t v) const
    {
        *reinterpret_cast<uint2*>(span + o) = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
};

// kPerLane: the alternative the wave-cooperative copy is measured against
// (debug key find_copy=1) and the path of an `out` that is not 16-byte
// aligned -- every lane stores its own 136 bytes, byte by byte.
template <bool kPerLane>
__global__ __launch_bounds__(kFindThreads) void itb_find_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint32_t* __restrict__ payload_len, const int32_t* __restrict__ status,
    const uint8_t* __restrict__ adepth, uint32_t nitb, const pom_lookup_req* __restrict__ req, uint32_t nreq,
    const uint8_t* __restrict__ names, uint32_t names_len, int32_t* __restrict__ err, uint32_t* __restrict__ nr,
    uint32_t* __restrict__ depth, uint8_t* __restrict__ out)
{
    __shared__ FindTable tables[kFindWaves];
    const uint32_t lane = lane_id();
    const uint32_t wave_in_group = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    FindTable& T = tables[wave_in_group];
    const uint32_t nwaves = (uint32_t)(((uint64_t)nreq + kWave - 1) / kWave);
    for (uint32_t wv = blockIdx.x * kFindWaves + wave_in_group; wv < nwaves; wv += gridDim.x * kFindWaves) {
        const uint32_t r0 = wv * kWave;                                 // wave-uniform
        const uint32_t cnt = nreq - r0 < kWave ? nreq - r0 : kWave;
        const uint32_t r = r0 + lane;
        uint64_t ite_off = kItbFindNoIte;
        uint32_t col = kItbFindNoColumn;
        if (lane < cnt) {
            const pom_lookup_req q = req[r];
            int32_t e = kItbScanEinval;
            uint32_t hit = 0, d = 0;
            if (q.itb < nitb) {
                e = status ? status[q.itb] : 0;
                if (e == 0) {
                    const uint64_t off = payload_off[q.itb];
                    e = itb_find_one(payload + off, payload_len[q.itb], adepth[q.itb], q, names, names_len, &hit, &d);
                    if (e == 0) {
                        ite_off = off + POM_ITB_ITE_OFF + (uint64_t)POM_ITE_SIZE * hit;
                        col = itb_find_column_of(q);
                    }
                }
            }
            err[r] = e;
            nr[r] = hit;
            depth[r] = d;
        }
        uint8_t* span = out + (uint64_t)POM_LK_REC_SIZE * r0;
        if (kPerLane) {
            if (lane < cnt)
                itb_find_record_bytes(span + POM_LK_REC_SIZE * lane, payload, ite_off, col);
            continue;
        }
        T.ite_off[lane] = ite_off;
        T.col[lane] = col;
        wave_lds_fence();
        const SpanOut mem{span};
        const uint32_t granules = itb_find_granules(cnt);
        for (uint32_t g = lane; g < granules; g += kWave)
            itb_find_granule(mem, payload, T.ite_off, T.col, cnt, g);
        wave_lds_fence();                           // the next round rewrites the table
    }
}

}  // namespace

extern "C" int lzo_mi355x_launch_lookup(const uint8_t* payload, const uint64_t* payload_off,
                                        const uint32_t* payload_len, const int32_t* status,
                                        const uint8_t* adepth, uint32_t nitb, const struct pom_lookup_req* req,
                                        uint32_t nreq, const uint8_t* names, uint32_t names_len, int32_t* err,
                                        uint32_t* nr, uint32_t* depth, uint8_t* out, hipStream_t stream)
{
    if (nreq == 0)
        return 0;
    const uint32_t need = (uint32_t)(((uint64_t)nreq + kFindThreads - 1) / kFindThreads);
    const uint32_t grid = need < kFindGridMax ? need : kFindGridMax;
    // 64 records are 8,704 bytes, a multiple of 16: every wave's span is aligned when out is.
    // debug key find_copy=1: the per-lane byte copy on aligned outputs too (measurements)
    const bool per_lane = ((uintptr_t)out & 15u) != 0 || pom_dbg_int("find_copy", 0) == 1;
    hipLaunchKernelGGL(per_lane ? itb_find_kernel<true> : itb_find_kernel<false>, dim3(grid), dim3(kFindThreads), 0,
                       stream, payload, payload_off, payload_len, status, adepth, nitb, req, nreq, names, names_len,
                       err, nr, depth, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
