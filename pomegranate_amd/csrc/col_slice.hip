// col_slice.hip -- column reads by offset and size on gfx950
// (include/pom_column.h pom_col_slice_dev; the rules and the copy plan are
// col_slice.h's).  Requests lie along blockIdx.y, and kSliceGroups workgroups
// along blockIdx.x stride over one request's tiles of 4 KiB, so a request of
// a whole 16 MiB column is not one workgroup's and no size is needed on the
// host.  Every workgroup of a request decides it again from the same few
// scalars; the first one's lane 0 writes out_len and err.  A lane stores one
// aligned 16-byte granule made of two aligned source granules; only the up
// to 15 bytes before and behind the granules are stored as bytes.  No LDS,
// no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "col_slice.h"
#include "lzo_mi355x_kernels.h"
#include "pom_column.h"

namespace {

// Workgroups per request.  A workgroup with no tile still reads its request's
// scalars: 1,726 reads of 4 KiB take 45 us with 16, 21 us with 4 (2: 13 us),
// 448 reads of 128 KiB 20 us with 16, 23 us with 4 (2: 31 us).
constexpr uint32_t kSliceGroups = 4;
constexpr uint32_t kSliceGridYMax = 4096;           // then a grid stride over the requests

// Global memory by address: every address is formed from a kernel argument
// (the columns' arena for loads, the output for stores), so the accesses are
// global ones, not flat.
struct GlobalMem {
    const uint8_t* data;
    uint8_t* out;
    __device__ __forceinline__ const uint8_t* src(uint64_t a) const { return data + (a - (uint64_t)(uintptr_t)data); }
    __device__ __forceinline__ uint8_t* dst(uint64_t a) const { return out + (a - (uint64_t)(uintptr_t)out); }
    __device__ __forceinline__ col_slice_u128 ld16(uint64_t a) const
    {
        uint4 v = *reinterpret_cast<const uint4*>(src(a));
        // all four dwords count as used: left alone, hipcc narrows the load to the
        // dword pairs each shift's merge reads (three overlapping dwordx2 loads)
        asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
        return col_slice_u128{{v.x, v.y, v.z, v.w}};
    }
    __device__ __forceinline__ uint32_t ld4(uint64_t a) const { return *reinterpret_cast<const uint32_t*>(src(a)); }
    __device__ __forceinline__ uint8_t ld1(uint64_t a) const { return *src(a); }
    __device__ __forceinline__ void st16(uint64_t a, const col_slice_u128& v) const
    {
        *reinterpret_cast<uint4*>(dst(a)) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    }
    __device__ __forceinline__ void st1(uint64_t a, uint8_t b) const { *dst(a) = b; }
};

__global__ __launch_bounds__(kColSliceTileLanes) void col_slice_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ data_off,
    const uint32_t* __restrict__ data_len, const int32_t* __restrict__ status,
    const uint64_t* __restrict__ want, uint32_t ncol, const pom_col_req* __restrict__ req, uint32_t nreq,
    uint8_t* __restrict__ out, const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out_len,
    int32_t* __restrict__ err)
{
    const GlobalMem mem{data, out};
    for (uint32_t r = blockIdx.y; r < nreq; r += gridDim.y) {
        const uint32_t c = req[r].col;
        const uint64_t offset = req[r].offset, size = req[r].size;
        const bool col_ok = c < ncol;
        const int32_t st = col_ok && status ? status[c] : 0;
        const uint32_t produced = col_ok ? data_len[c] : 0u;
        uint64_t n = 0;
        const int32_t e = col_slice_decide(col_ok, 1, st, produced, col_ok ? want[c] : 0u, offset, size, &n);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            out_len[r] = (uint32_t)n;               // n <= want == produced, a u32
            err[r] = e;
        }
        if (n == 0)
            continue;
        const uint64_t col = (uint64_t)(uintptr_t)data + data_off[c];
        const col_slice_plan P = col_slice_plan_make((uint64_t)(uintptr_t)out + out_off[r], col + offset,
                                                     (uint32_t)n, col, col + produced);
        const uint32_t tiles = col_slice_tiles(P);
        for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x)
            col_slice_tile_lane(mem, P, t, threadIdx.x);
    }
}

}  // namespace

extern "C" int lzo_mi355x_launch_col_slice(const uint8_t* data, const uint64_t* data_off,
                                           const uint32_t* data_len, const int32_t* status,
                                           const uint64_t* want, uint32_t ncol, const struct pom_col_req* req,
                                           uint32_t nreq, uint8_t* out, const uint64_t* out_off,
                                           uint32_t* out_len, int32_t* err, hipStream_t stream)
{
    if (nreq == 0)
        return 0;
    const uint32_t gy = nreq < kSliceGridYMax ? nreq : kSliceGridYMax;
    // debug key slice_groups: the workgroups per request (measurements)
    const long g = pom_dbg_int("slice_groups", kSliceGroups);
    const uint32_t gx = g >= 1 && g <= 256 ? (uint32_t)g : kSliceGroups;
    hipLaunchKernelGGL(col_slice_kernel, dim3(gx, gy), dim3(kColSliceTileLanes), 0, stream, data,
                       data_off, data_len, status, want, ncol, req, nreq, out, out_off, out_len, err);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
