// itb_keys.hip -- the key/value table listing's ITB walk on gfx950
// (include/pom_kvlist.h; the rules and the copy plan are itb_keys.h's).  One
// wave per ITB: in round r lane l owns bitmap bit 64r + l.  Three
// stream-ordered launches, no host round trip between them:
//   itb_keys_count_kernel  live[b], dnum[b], bytes[b], keybytes[b], err[b], mask[16b ... 16b + 15]
//   itb_prefix_kernel      first[0 .. nitb] = exclusive prefix of bytes (u64; itb_prefix.h)
//   itb_keys_emit_kernel   the records, packed, at out + first[b]
// The count kernel is the only one that searches: a workgroup puts the needle
// into LDS once, finds its effective length and (linear form) its failure
// table there, and every lane runs the search over its own entry's value,
// read as aligned 8-byte words of the ITE.  The ballot of the lanes that emit
// is the round's mask word.  The emit kernel reads the mask: a wave exclusive
// scan of the emitting lanes' 4 + keylen, the round's records compacted in
// bit order into a small LDS table of the wave's own {start, ITE, head, key
// bytes' origin}, and the wave copies the round's span (up to 20,736 bytes)
// together: a lane takes one destination-aligned 16-byte granule a step,
// finds the up to five records that reach into it, assembles the bytes from
// the heads (LDS: length words and decimal texts) and the keys (three aligned
// 8-byte loads inside the ITE) and issues one dwordx4 store; only the span's
// head and tail, and what the cap cuts, are byte stores.  No scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itb_keys.h"
#include "itb_prefix.h"
#include "lzo1x_wave.h"
#include "lzo_mi355x_kernels.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kKeysThreads = 256;              // 4 waves: 4 ITBs per workgroup
constexpr uint32_t kKeysWaves = kKeysThreads / kWave;
constexpr uint32_t kKeysGridMax = 2048;             // then a grid stride
// a prefix tile's sum fits u32: at most 331,776 bytes an ITB
static_assert((uint64_t)kPrefixThreads * kItbKeysItbMax <= 0xFFFFFFFFull, "prefix tile");
static_assert(POM_KV_NEEDLE_MAX < kKeysThreads, "one thread a needle byte");
static_assert(POM_KV_MASK_WORDS == kItbScanRounds && POM_KV_MASK_WORDS <= kWave, "a lane a mask word");

// One wave's table of a round's records (itb_keys_round).
struct KeysTable {
    uint64_t w0[kWave], w1[kWave], w2[kWave];
    uint32_t start[kWave], nr[kWave], meta[kWave];
    uint8_t hlen[kWave];
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

// kLinear: the failure-table search; else the plain one (debug key
// keys_search=1, measurements).
template <bool kLinear>
__global__ __launch_bounds__(kKeysThreads) void itb_keys_count_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint32_t* __restrict__ payload_len, const int32_t* __restrict__ status,
    const uint8_t* __restrict__ adepth, uint32_t nitb, uint32_t op, const uint8_t* __restrict__ needle,
    uint32_t needle_len, uint32_t* __restrict__ live, uint32_t* __restrict__ dnum, uint32_t* __restrict__ bytes,
    uint32_t* __restrict__ keybytes, uint64_t* __restrict__ mask, int32_t* __restrict__ err)
{
    __shared__ uint8_t s_needle[POM_KV_NEEDLE_MAX + 1];
    __shared__ uint8_t s_fail[POM_KV_NEEDLE_MAX + 1];
    __shared__ uint32_t s_m;
    uint32_t m = 0;
    if (op >= POM_KV_OP_GREP) {                     // (uniform: every thread takes the barriers)
        if (threadIdx.x < needle_len)
            s_needle[threadIdx.x] = needle[threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t len = itb_keys_needle_len(s_needle, needle_len);
            if (kLinear)
                itb_keys_failure(s_needle, len, s_fail);
            s_m = len;
        }
        __syncthreads();
        m = s_m;
    }
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kKeysWaves + threadIdx.x / kWave);
    for (uint32_t b = wave; b < nitb; b += gridDim.x * kKeysWaves) {
        int32_t e = status ? status[b] : 0;
        uint32_t nl = 0, nd = 0, nb = 0, nk = 0;
        uint64_t mymask = 0;                        // lane r: round r's emit mask
        if (e == 0) {
            const uint8_t* p = payload + payload_off[b];
            const uint32_t n = payload_len[b], ad = adepth[b];
            e = itb_scan_precheck(n, ad);
            if (e == 0 && (e = itb_scan_live(p, n, ad, &nl)) == 0) {
                const uint32_t rounds = itb_scan_rounds(ad);
                uint32_t mine = 0, keys = 0;        // this lane's record and key bytes over the rounds
                bool bad_key = false, bad_name = false;
                for (uint32_t r = 0; r < rounds; r++) {
                    const uint64_t w = itb_scan_word(p, r, ad);
                    bool emits = false;
                    if ((w >> lane) & 1u) {
                        const uint32_t nr = 64u * r + lane;
                        const itb_keys_entry k = itb_keys_load<false>(p, nr);
                        bad_key |= k.bad == POM_KV_E_KEY;
                        bad_name |= k.bad == POM_RD_E_NAME;
                        if (k.bad == 0) {
                            keys += k.keylen;
                            emits = itb_keys_emits<kLinear>(p, nr, k, op, s_needle, m, s_fail);
                            mine += emits ? 4u + k.keylen : 0u;
                        }
                    }
                    const uint64_t mm = wave_ballot(emits);
                    nd += (uint32_t)__popcll(mm);
                    if (lane == r)
                        mymask = mm;
                }
                nb = lane_read(wave_incl_scan(mine), kWave - 1);        // at most kItbKeysItbMax
                nk = lane_read(wave_incl_scan(keys), kWave - 1);
                if (wave_ballot(bad_key) != 0)
                    e = POM_KV_E_KEY;
                else if (wave_ballot(bad_name) != 0)
                    e = POM_RD_E_NAME;
                if (e != 0)
                    nd = nb = nk = 0;
            }
        }
        if (lane < POM_KV_MASK_WORDS)
            mask[(uint64_t)POM_KV_MASK_WORDS * b + lane] = e == 0 ? mymask : 0ull;
        if (lane == 0) {
            live[b] = nl;
            dnum[b] = nd;
            bytes[b] = nb;
            keybytes[b] = nk;
            err[b] = e;
        }
    }
}

// kPerLane: the alternative the wave-cooperative copy is measured against
// (debug key keys_copy=1) -- every emitting lane stores its own record byte
// by byte, 64 ways divergent, up to 324 steps.
template <bool kPerLane>
__global__ __launch_bounds__(kKeysThreads) void itb_keys_emit_kernel(
    const uint8_t* __restrict__ payload, const uint64_t* __restrict__ payload_off,
    const uint8_t* __restrict__ adepth, uint32_t nitb, const uint32_t* __restrict__ dnum,
    const int32_t* __restrict__ err, const uint64_t* __restrict__ mask, const uint64_t* __restrict__ first,
    uint8_t* __restrict__ out, uint64_t out_cap)
{
    __shared__ KeysTable tables[kKeysWaves];
    const uint32_t lane = lane_id();
    const uint32_t wave_in_group = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t wave = blockIdx.x * kKeysWaves + wave_in_group;
    KeysTable& T = tables[wave_in_group];
    const GlobalOut mem{out};
    const uint64_t cap_end = (uint64_t)(uintptr_t)out + out_cap;
    for (uint32_t b = wave; b < nitb; b += gridDim.x * kKeysWaves) {
        // the count kernel passed this payload's checks and its keys when it left err 0
        if (err[b] != 0 || dnum[b] == 0)
            continue;
        const uint8_t* p = payload + payload_off[b];
        const uint32_t ad = adepth[b];
        uint64_t at = first[b];
        const uint32_t rounds = itb_scan_rounds(ad);
        for (uint32_t r = 0; r < rounds && at < out_cap; r++) {
            // the count kernel's ballot; never a bit that is not live
            const uint64_t m = mask[(uint64_t)POM_KV_MASK_WORDS * b + r] & itb_scan_word(p, r, ad);
            if (m == 0)
                continue;
            const uint32_t nr = 64u * r + lane;
            const bool emits = (m >> lane) & 1u;
            itb_keys_entry k{};
            uint32_t len = 0;
            if (emits) {
                k = itb_keys_load<true>(p, nr);
                len = k.head.len + k.memlen;
            }
            const uint32_t incl = wave_incl_scan(len);
            const uint32_t span = lane_read(incl, kWave - 1);           // at most 64 * 324
            if (kPerLane) {
                const uint64_t mine = (uint64_t)(uintptr_t)out + at + (incl - len);
                for (uint32_t j = 0; j < len && mine + j < cap_end; j++)
                    mem.st1(mine + j, j < k.head.len ? itb_keys_head_byte(k.head, j)
                                                     : itb_dents_ite(p, nr)[k.memoff + j - k.head.len]);
                at += span;
                continue;
            }
            if (emits) {
                const uint32_t i = lanes_below(m);
                T.w0[i] = k.head.w0;
                T.w1[i] = k.head.w1;
                T.w2[i] = k.head.w2;
                T.hlen[i] = (uint8_t)k.head.len;
                T.start[i] = incl - len;
                T.nr[i] = nr;
                T.meta[i] = itb_keys_meta(k);
            }
            wave_lds_fence();
            const uint64_t dst = (uint64_t)(uintptr_t)out + at;
            const itb_keys_round R{T.w0, T.w1, T.w2, T.start, T.nr, T.meta, T.hlen, (uint32_t)__popcll(m), span, p,
                                   dst, dst + span < cap_end ? dst + span : cap_end};
            const uint32_t granules = itb_keys_granules(R);
            for (uint32_t g = lane; g < granules; g += kWave)
                itb_keys_granule(mem, R, g);
            wave_lds_fence();                       // the next round rewrites the table
            at += span;
        }
    }
}

}  // namespace

extern "C" int lzo_mi355x_launch_kvlist(const uint8_t* payload, const uint64_t* payload_off,
                                        const uint32_t* payload_len, const int32_t* status,
                                        const uint8_t* adepth, uint32_t nitb, uint32_t op, const uint8_t* needle,
                                        uint32_t needle_len, uint32_t* live, uint32_t* dnum, uint32_t* bytes,
                                        uint32_t* keybytes, uint64_t* mask, uint64_t* first, uint8_t* out,
                                        uint64_t out_cap, int32_t* err, hipStream_t stream)
{
    if (op > POM_KV_OP_GREP_CNT || needle_len > POM_KV_NEEDLE_MAX)
        return -1;
    const uint32_t need = (nitb + kKeysWaves - 1) / kKeysWaves;
    const uint32_t grid = need < kKeysGridMax ? need : kKeysGridMax;
    // no mask asked for: the count kernel's ballots live in memory of the call's own, in stream order
    void* own = nullptr;
    if (!mask && nitb) {
        if (hipMallocAsync(&own, sizeof(uint64_t) * POM_KV_MASK_WORDS * nitb, stream) != hipSuccess)
            return -1;
        mask = static_cast<uint64_t*>(own);
    }
    // debug key keys_search=1: the plain search (measurements)
    if (nitb)
        hipLaunchKernelGGL(pom_dbg_int("keys_search", 0) == 1 ? itb_keys_count_kernel<false> : itb_keys_count_kernel<true>,
                           dim3(grid), dim3(kKeysThreads), 0, stream, payload, payload_off, payload_len, status,
                           adepth, nitb, op, needle, needle_len, live, dnum, bytes, keybytes, mask, err);
    hipLaunchKernelGGL(itb_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, stream, bytes, nitb, first);
    // debug key keys_copy=1: the per-lane byte copy (measurements)
    if (nitb && out_cap)
        hipLaunchKernelGGL(pom_dbg_int("keys_copy", 0) == 1 ? itb_keys_emit_kernel<true> : itb_keys_emit_kernel<false>,
                           dim3(grid), dim3(kKeysThreads), 0, stream, payload, payload_off, adepth, nitb, dnum,
                           err, mask, first, out, out_cap);
    int rc = hipGetLastError() == hipSuccess ? 0 : -1;
    if (own && hipFreeAsync(own, stream) != hipSuccess)
        rc = -1;
    return rc;
}
