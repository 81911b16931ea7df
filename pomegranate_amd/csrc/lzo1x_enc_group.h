// lzo1x_enc_group.h -- index arithmetic of the grouped global-dictionary
// encoder (lzo1x_encode_fast.hip, enc_group_body) and the rule that selects
// it, stated once as plain C++ for the device, the launcher and
// tests/native/enc_group_host.cc on the CPU.
//
// The scratch holds one dictionary region per block in flight ("regions",
// the grid of the one-wave kernel).  The grouped kernel runs them `group` to
// a workgroup: parse wave w of workgroup g owns region group * g + w, and the
// workgroup's `emitters` emit waves (waves group .. group + emitters - 1)
// share its token queues, emit wave e serving the parse slots
// [e * group / emitters, (e + 1) * group / emitters).  The last workgroup may
// be partly filled: a parse wave whose region is not below `regions` is idle
// (it takes no block and reports exit at once).
#ifndef POM_LZO1X_ENC_GROUP_H
#define POM_LZO1X_ENC_GROUP_H

#include <stdint.h>

#ifdef __HIPCC__
#define ENC_GROUP_FN __host__ __device__ __forceinline__
#else
#define ENC_GROUP_FN static inline
#endif

/* Workgroups that cover `regions` regions. */
ENC_GROUP_FN uint32_t enc_group_workgroups(uint32_t regions, uint32_t group)
{
    return regions / group + (regions % group ? 1u : 0u);
}

/* The region of parse wave `wave` (< group) of workgroup `wg`. */
ENC_GROUP_FN uint32_t enc_group_region(uint32_t wg, uint32_t wave, uint32_t group)
{
    return group * wg + wave;
}

/* Does that parse wave have no region? */
ENC_GROUP_FN int enc_group_idle(uint32_t wg, uint32_t wave, uint32_t group, uint32_t regions)
{
    return enc_group_region(wg, wave, group) >= regions;
}

/* The parse slots [first, first + count) that emit wave `e` (< emitters) serves. */
ENC_GROUP_FN uint32_t enc_group_emit_first(uint32_t e, uint32_t group, uint32_t emitters)
{
    return e * group / emitters;
}
ENC_GROUP_FN uint32_t enc_group_emit_count(uint32_t e, uint32_t group, uint32_t emitters)
{
    return (e + 1) * group / emitters - e * group / emitters;
}

/* The selection rule: the grouped kernel runs a batch of `regions` regions
 * only if it has a whole group and its workgroups reach every CU -- the
 * one-wave kernel spreads `regions` workgroups over min(regions, cus) CUs, the
 * grouped one ceil(regions / group) over as many, so with fewer than `cus`
 * workgroups it would leave CUs idle that the one-wave kernel uses (a lone
 * block, a small batch: those stay with the one-wave kernel). */
ENC_GROUP_FN int enc_group_use(uint32_t regions, uint32_t group, uint32_t cus)
{
    return regions >= group && enc_group_workgroups(regions, group) >= cus;
}

#endif
