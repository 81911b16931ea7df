/* gc_fold.c -- gc_fold.h: the fold of the chunks' merged maps and the seed. */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "gc_fold.h"

#define FOLD_E_OUT_OF_MEMORY (-3)   /* LZO_E_OUT_OF_MEMORY (minilzo.h) */

int pom_gc_seed_check(const struct pom_gc_range *seed, size_t nseed)
{
    for (size_t i = 0; i < nseed; i++) {
        if (seed[i].high <= seed[i].low)
            return -EINVAL;
        if (i && seed[i].low <= seed[i - 1].high)
            return -EINVAL;
    }
    return 0;
}

static int by_low(const void *a, const void *b)
{
    const struct pom_gc_range *x = a, *y = b;
    return x->low < y->low ? -1 : x->low > y->low;
}

int pom_gc_fold(const struct pom_gc_range *const *maps, const size_t *counts, size_t nmaps,
                const struct pom_gc_range *seed, size_t nseed,
                struct pom_gc_range *merged, size_t merged_cap, struct pom_gc_stat *stat)
{
    memset(stat, 0, sizeof(*stat));
    if (pom_gc_seed_check(seed, nseed) != 0)
        return -EINVAL;
    size_t total = nseed;
    for (size_t k = 0; k < nmaps; k++)
        total += counts[k];
    struct pom_gc_range *all = malloc((total + 1) * sizeof(*all));
    if (!all)
        return FOLD_E_OUT_OF_MEMORY;
    size_t n = 0;
    for (size_t k = 0; k <= nmaps; k++) {
        const struct pom_gc_range *from = k < nmaps ? maps[k] : seed;
        const size_t cnt = k < nmaps ? counts[k] : nseed;
        for (size_t i = 0; i < cnt; i++)
            if (from[i].high > from[i].low)
                all[n++] = from[i];
    }
    qsort(all, n, sizeof(*all), by_low);
    uint64_t nout = 0, valid = 0, low = 0, high = 0;
    for (size_t i = 0; i <= n; i++) {
        if (i < n && nout && all[i].low <= high) {
            if (all[i].high > high)
                high = all[i].high;
            continue;
        }
        if (nout) {                             /* the extent before this one is complete */
            valid += high - low;
            if (nout <= merged_cap) {
                merged[nout - 1].low = low;
                merged[nout - 1].high = high;
            }
        }
        if (i < n) {
            nout++;
            low = all[i].low;
            high = all[i].high;
        }
    }
    free(all);
    stat->valid = valid;
    stat->max = nout ? high : 0;
    stat->nout = nout;
    return nout > merged_cap ? POM_GC_E_NOSPACE : 0;
}
