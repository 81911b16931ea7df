// itb_scan.hip -- the garbage collector's ITB walk on gfx950 (include/pom_gc.h;
// the rules are itb_scan.h's).  One wave per ITB: in round r lane l owns bitmap
// bit 64r + l; the round's word is wave-uniform, the lanes whose bit is live
// load their ITE's column, and a ballot with mbcnt compacts them in bit order.
// Three stream-ordered launches, no host round trip between them:
//   itb_scan_count_kernel   live[b], nranges[b], err[b]
//   itb_prefix_kernel       first[0 .. nitb] = exclusive prefix of nranges (u64; itb_prefix.h)
//   itb_scan_emit_kernel    ranges[first[b] + k], one 16-byte store each
// The emit kernel reads each live ITE's 16 bytes a second time; beside the
// decode that fills the payloads this is noise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_prefix.h"
#include "itb_scan.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kScanThreads = 256;              // 4 waves: 4 ITBs per workgroup
constexpr uint32_t kScanWaves = kScanThreads / kWave;
constexpr uint32_t kScanGridMax = 2048;             // then a grid stride
// a prefix tile's sum fits u32: at most 1024 ranges an ITB
static_assert((uint64_t)kPrefixThreads << POM_ITB_ADEPTH_MAX <= 0xFFFFFFFFull, "prefix tile");

__global__ __launch_bounds__(kScanThreads) void itb_scan_count_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint32_t* __restrict__ payload_len, const int32_t* __restrict__ status,
    const uint8_t* __restrict__ adepth, uint32_t nitb, uint32_t column, uint32_t* __restrict__ live,
    uint32_t* __restrict__ nranges, int32_t* __restrict__ err)
{
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kScanWaves + threadIdx.x / kWave);
    for (uint32_t b = wave; b < nitb; b += gridDim.x * kScanWaves) {
        int32_t e = status ? status[b] : 0;
        uint32_t nl = 0, nr = 0;
        if (e == 0) {
            const uint8_t* p = payload + payload_off[b];
            const uint32_t n = payload_len[b], ad = adepth[b];
            e = itb_scan_precheck(n, ad);
            if (e == 0 && (e = itb_scan_live(p, n, ad, &nl)) == 0) {
                const uint32_t rounds = itb_scan_rounds(ad);
                for (uint32_t r = 0; r < rounds; r++) {
                    const uint64_t w = itb_scan_word(p, r, ad);
                    const bool has = ((w >> lane) & 1u) && itb_scan_has_range(p, 64u * r + lane, column);
                    nr += (uint32_t)__popcll(wave_ballot(has));
                }
            }
        }
        if (lane == 0) {
            live[b] = nl;
            nranges[b] = nr;
            err[b] = e;
        }
    }
}

__global__ __launch_bounds__(kScanThreads) void itb_scan_emit_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint8_t* __restrict__ adepth, uint32_t nitb, uint32_t column,
    const uint32_t* __restrict__ nranges, const int32_t* __restrict__ err,
    const uint64_t* __restrict__ first, pom_gc_range* __restrict__ ranges, uint64_t ranges_cap)
{
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kScanWaves + threadIdx.x / kWave);
    const bool wide = ((uintptr_t)ranges & 15u) == 0;
    for (uint32_t b = wave; b < nitb; b += gridDim.x * kScanWaves) {
        // the count kernel passed this payload's checks when it left err 0
        if (err[b] != 0 || nranges[b] == 0)
            continue;
        const uint8_t* p = payload + payload_off[b];
        const uint32_t ad = adepth[b];
        uint64_t at = first[b];
        if (at >= ranges_cap)
            continue;
        const uint32_t rounds = itb_scan_rounds(ad);
        for (uint32_t r = 0; r < rounds; r++) {
            const uint64_t w = itb_scan_word(p, r, ad);
            const uint32_t nr = 64u * r + lane;
            pom_gc_range g{0, 0};
            bool has = false;
            if ((w >> lane) & 1u) {
                has = itb_scan_has_range(p, nr, column);
                g = itb_scan_range(p, nr, column);
            }
            const uint64_t m = wave_ballot(has);
            const uint64_t idx = at + lanes_below(m);
            if (has && idx < ranges_cap) {
                if (wide) {
                    *reinterpret_cast<ulonglong2*>(ranges + idx) = make_ulonglong2(g.low, g.high);
                } else {
                    ranges[idx].low = g.low;
                    ranges[idx].high = g.high;
                }
            }
            at += (uint32_t)__popcll(m);
        }
    }
}

}  // namespace

extern "C" int lzo_mi355x_launch_gc_scan(const uint8_t* payload, const uint64_t* payload_off,
                                         const uint32_t* payload_len, const int32_t* status,
                                         const uint8_t* adepth, uint32_t nitb, uint32_t column,
                                         uint32_t* live, uint32_t* nranges, uint64_t* first,
                                         struct pom_gc_range* ranges, uint64_t ranges_cap, int32_t* err,
                                         hipStream_t stream)
{
    if (column >= POM_ITE_COLUMNS)
        return -1;
    const uint32_t need = (nitb + kScanWaves - 1) / kScanWaves;
    const uint32_t grid = need < kScanGridMax ? need : kScanGridMax;
    if (nitb)
        hipLaunchKernelGGL(itb_scan_count_kernel, dim3(grid), dim3(kScanThreads), 0, stream, payload,
                           payload_off, payload_len, status, adepth, nitb, column, live, nranges, err);
    hipLaunchKernelGGL(itb_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, stream, nranges, nitb, first);
    if (nitb && ranges_cap)
        hipLaunchKernelGGL(itb_scan_emit_kernel, dim3(grid), dim3(kScanThreads), 0, stream, payload,
                           payload_off, adepth, nitb, column, nranges, err, first, ranges, ranges_cap);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
