// lzo1x_wave.h -- wave-level helpers shared by the gfx950 kernels (device
// code only; one wave is 64 lanes).  Everything is in the anonymous namespace
// and force-inlined: each .hip file gets its own copy.
#ifndef POM_LZO1X_WAVE_H
#define POM_LZO1X_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __ballot(p); }
// Lane masks straight from a v_cmp (a ballot of a compound bool costs a
// v_cndmask and a v_cmp more): active lanes with a == b, a < b, a >= b.
__device__ __forceinline__ uint64_t mask_eq(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 32); }
__device__ __forceinline__ uint64_t mask_lt(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 36); }
__device__ __forceinline__ uint64_t mask_ge(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 35); }

// Inclusive prefix sum over the wave: DPP row shifts inside each 16-lane row,
// then the row totals via readlane (no LDS round trip).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    const uint32_t r0 = lane_read(v, 15), r1 = lane_read(v, 31), r2 = lane_read(v, 47);
    const uint32_t row = lane_id() >> 4;
    v += (row >= 1 ? r0 : 0u) + (row >= 2 ? r1 : 0u) + (row >= 3 ? r2 : 0u);
    return v;
}

// Hand-off words between the waves of a workgroup (LDS, workgroup scope).
__device__ __forceinline__ uint32_t lds_load(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store(uint32_t* p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// An aligned dword in global memory: loads through this type are global_load
// (vmcnt only), not flat_load.
typedef __attribute__((address_space(1))) const uint32_t gdword;

}  // namespace

#endif
