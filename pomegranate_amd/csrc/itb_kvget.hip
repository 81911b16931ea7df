// itb_kvget.hip -- the key/value point get's ITB walk on gfx950
// (include/pom_kvget.h; the rules and the records' copy plan are
// itb_kvget.h's).  Three launches on the call's stream:
//   find    one lane per request, as itb_find_kernel: lane l of a wave runs
//           itb_kvget_one for request 64 * wave + l -- a chain of dependent
//           4-byte gathers from the index table with one ITE's v.key (and, for
//           a string get, klen and the key bytes as whole words of the ITE)
//           compared per hop.  err, nr, depth, len and lease go out as five
//           coalesced stores.
//   prefix  itb_prefix_kernel over len: first[r] = where record r starts.
//   emit    a wave owns 64 consecutive requests, that is the bytes
//           [first[r0], first[r0 + cnt]) of `out`, at most 23,296.  Each lane
//           leaves its record's start and sources {ITE offset, kv bytes, column
//           offset} in an LDS table of the wave's own; then a lane takes one
//           16-byte granule of the destination a step, at 16-byte aligned
//           addresses whatever out's own alignment: it finds the record that
//           holds the granule's first byte by binary search over the starts,
//           assembles the granule from aligned 8-byte loads of at most two
//           source pieces and issues one dwordx4 store.  Byte stores appear
//           only in a span's first and last granule and where out_cap cuts.
//           The alternative, every lane storing its own record byte by byte,
//           is behind the debug key kvget_copy=1.
// No atomics, no scratch memory, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_kvget.h"
#include "itb_prefix.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kWave = kItbKvgetWave;
constexpr uint32_t kGetThreads = 256;               // 4 waves: 256 requests per workgroup
constexpr uint32_t kGetWaves = kGetThreads / kWave;
constexpr uint32_t kGetGridMax = 2048;              // as itb_find_kernel; then a grid stride
constexpr uint32_t kSpanMax = kWave * POM_KG_REC_MAX;               // 23,296 bytes
constexpr uint32_t kSpanGranules = kSpanMax / 16 + 1;               // a misaligned span meets one more

// a prefix tile's sum fits u32 (itb_prefix.h): 1,024 records are at most 372,736 bytes
static_assert((uint64_t)kPrefixThreads * POM_KG_REC_MAX == 372736 && (uint64_t)kPrefixThreads * POM_KG_REC_MAX < (1ull << 32),
              "a tile of lengths sums in u32");
static_assert(kSpanMax == 23296 && kSpanMax % 16 == 0, "a wave's span");

__global__ __launch_bounds__(kGetThreads) void itb_kvget_find_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint32_t* __restrict__ payload_len, const int32_t* __restrict__ status,
    const uint8_t* __restrict__ adepth, uint32_t nitb, const pom_kvget_req* __restrict__ req, uint32_t nreq,
    const uint8_t* __restrict__ keys, uint32_t keys_len, int32_t* __restrict__ err, uint32_t* __restrict__ nr,
    uint32_t* __restrict__ depth, uint32_t* __restrict__ len, uint64_t* __restrict__ lease)
{
    const uint32_t stride = gridDim.x * kGetThreads;
    const uint32_t rounds = (uint32_t)(((uint64_t)nreq + stride - 1) / stride);
    for (uint32_t k = 0; k < rounds; k++) {
        const uint64_t r64 = (uint64_t)k * stride + blockIdx.x * kGetThreads + threadIdx.x;
        if (r64 >= nreq)
            return;
        const uint32_t r = (uint32_t)r64;
        const pom_kvget_req q = req[r];
        int32_t e = kItbScanEinval;
        uint32_t hit = 0, d = 0, ln = 0;
        uint64_t ls = 0;
        if (q.itb < nitb) {
            e = status ? status[q.itb] : 0;
            if (e == 0)
                e = itb_kvget_one(payload + payload_off[q.itb], payload_len[q.itb], adepth[q.itb], q, keys, keys_len,
                                  &hit, &d, &ln, &ls);
        }
        err[r] = e;
        nr[r] = hit;
        depth[r] = d;
        len[r] = ln;
        lease[r] = ls;
    }
}

// One wave's table of its records' starts and sources (itb_kvget_granule).
struct GetTable {
    itb_kvget_src src[kWave];
    uint32_t rel[kWave];
};

// The wave's LDS writes before, its LDS reads behind (one wave's DS
// operations execute in order; this keeps the compiler from moving them).
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stores at byte offsets of out; st16's address is 16-byte aligned.
struct OutMem {
    uint8_t* out;
    __device__ __forceinline__ void st16(uint64_t o, uint64_t lo, uint64_t hi) const
    {
        *reinterpret_cast<uint4*>(out + o) =
            make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    __device__ __forceinline__ void st1(uint64_t o, uint8_t v) const { out[o] = v; }
};

// kPerLane: the alternative the granule copy is measured against (debug key
// kvget_copy=1) -- every lane stores its own record, byte by byte.
template <bool kPerLane>
__global__ __launch_bounds__(kGetThreads) void itb_kvget_emit_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off, uint32_t nitb,
    const pom_kvget_req* __restrict__ req, uint32_t nreq, const uint32_t* __restrict__ nr,
    const uint32_t* __restrict__ len, const uint64_t* __restrict__ first, uint8_t* __restrict__ out, uint64_t out_cap)
{
    __shared__ GetTable tables[kGetWaves];
    const uint32_t lane = lane_id();
    const uint32_t wave_in_group = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    GetTable& T = tables[wave_in_group];
    const OutMem mem{out};
    const uint32_t mis = (uint32_t)((uintptr_t)out & 15u);
    const uint32_t nwaves = (uint32_t)(((uint64_t)nreq + kWave - 1) / kWave);
    const uint32_t step = gridDim.x * kGetWaves;
    const uint32_t rounds = (nwaves + step - 1) / step;
    for (uint32_t k = 0; k < rounds; k++) {
        const uint32_t wv = k * step + blockIdx.x * kGetWaves + wave_in_group;      // wave-uniform
        if (wv >= nwaves)
            return;
        const uint32_t r0 = wv * kWave;
        const uint32_t cnt = nreq - r0 < kWave ? nreq - r0 : kWave;
        const uint64_t lo = first[r0], hi = first[r0 + cnt];
        // (a span the cap leaves nothing of, or longer than 64 records can be: nothing to do)
        if (lo >= hi || lo >= out_cap || hi - lo > kSpanMax)
            continue;
        itb_kvget_src s = itb_kvget_src{0, 0, kItbKvgetNoColumn};
        uint64_t start = hi;
        if (lane < cnt) {
            const pom_kvget_req q = req[r0 + lane];
            const uint32_t ln = len[r0 + lane];
            start = first[r0 + lane];
            if (ln != 0 && ln <= POM_KG_REC_MAX && ln >= POM_KV_HEADER_LEN + itb_kvget_column_bytes(q) &&
                q.itb < nitb && start >= lo && start + ln <= hi)
                s = itb_kvget_src_of(q, payload_off[q.itb], nr[r0 + lane], ln);
        }
        if (kPerLane) {
            itb_kvget_record_bytes(mem, start, out_cap, payload, s);
            continue;
        }
        T.src[lane] = s;
        T.rel[lane] = (uint32_t)(start - lo);
        wave_lds_fence();
        const uint32_t granules = itb_kvget_granules(mis, lo, hi);
        for (uint32_t g = lane; g < granules && g < kSpanGranules; g += kWave)
            itb_kvget_granule(mem, payload, T.rel, T.src, cnt, mis, lo, hi, out_cap, g);
        wave_lds_fence();                           // the next round rewrites the table
    }
}

}  // namespace

extern "C" int lzo_mi355x_launch_kvget(const uint8_t* payload, const uint64_t* payload_off,
                                       const uint32_t* payload_len, const int32_t* status, const uint8_t* adepth,
                                       uint32_t nitb, const struct pom_kvget_req* req, uint32_t nreq,
                                       const uint8_t* keys, uint32_t keys_len, int32_t* err, uint32_t* nr,
                                       uint32_t* depth, uint32_t* len, uint64_t* lease, uint64_t* first, uint8_t* out,
                                       uint64_t out_cap, hipStream_t stream)
{
    const uint32_t need = (uint32_t)(((uint64_t)nreq + kGetThreads - 1) / kGetThreads);
    const uint32_t grid = need < kGetGridMax ? need : kGetGridMax;
    if (nreq != 0)
        hipLaunchKernelGGL(itb_kvget_find_kernel, dim3(grid), dim3(kGetThreads), 0, stream, payload, payload_off,
                           payload_len, status, adepth, nitb, req, nreq, keys, keys_len, err, nr, depth, len, lease);
    hipLaunchKernelGGL(itb_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, stream, len, nreq, first);
    if (nreq != 0 && out_cap != 0) {
        // debug key kvget_copy=1: the per-lane byte copy (measurements)
        const bool per_lane = pom_dbg_int("kvget_copy", 0) == 1;
        hipLaunchKernelGGL(per_lane ? itb_kvget_emit_kernel<true> : itb_kvget_emit_kernel<false>, dim3(grid),
                           dim3(kGetThreads), 0, stream, payload, payload_off, nitb, req, nreq, nr, len, first, out,
                           out_cap);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
