/* gc_fold.h -- the host half of pom_gc_stat_batch (include/pom_gc.h): the
 * chunks' merged maps and the caller's seed folded into one map by the rule of
 * the range tree.  Plain C, neither HIP nor threads, so that
 * tests/native/gc_merge_host.cc runs it on the CPU.  Internal to
 * liblzo_mi355x.so. */
#ifndef POM_GC_FOLD_H
#define POM_GC_FOLD_H 1

#include <stddef.h>
#include <stdint.h>

#include "pom_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0 when seed[0, nseed) is ascending and disjoint with gaps of at least 1 and
 * every extent has high > low, else -EINVAL. */
int pom_gc_seed_check(const struct pom_gc_range *seed, size_t nseed);

/* maps[k][0, counts[k]) for k < nmaps and seed[0, nseed), in any order among
 * themselves, merged: sorted by low, a range starts a new extent if and only
 * if its low is strictly greater than the largest high so far.  A range with
 * high <= low takes no part.  The first merged_cap extents go to merged; stat
 * gets valid, max and nout of the whole map, and nin = nwrapped = 0 (the
 * caller's business).  Returns 0, POM_GC_E_NOSPACE (nout > merged_cap),
 * -EINVAL (pom_gc_seed_check) or LZO_E_OUT_OF_MEMORY. */
int pom_gc_fold(const struct pom_gc_range *const *maps, const size_t *counts, size_t nmaps,
                const struct pom_gc_range *seed, size_t nseed,
                struct pom_gc_range *merged, size_t merged_cap, struct pom_gc_stat *stat);

#ifdef __cplusplus
}
#endif

#endif
