/*
 * gc_stat.c -- the MDSL garbage collector's data stat (include/pom_gc.h
 * pom_gc_stat_batch): mdsl_gc_data_stat's tree (mdsl/gc.c:1020-1113) for a
 * batch of ITB records.  The records are selected and their per-ITB results
 * put together exactly as the scan's (pom_walk_begin, pom_walk_finish of
 * gc_scan.c); the chunks -- the scan's, with the merge of each chunk's ranges
 * behind its walk (gc_merge.hip) -- go through the host batches' pipeline
 * (host_records.c, gs_ops); the chunks' merged maps and the caller's seed are
 * folded here (gc_fold.c).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "gc_fold.h"
#include "host_requests.h"
#include "lzo_mi355x.h"
#include "lzo_mi355x_kernels.h"
#include "minilzo.h"
#include "pom_gc.h"

int pom_gc_stat_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int column,
                      const struct pom_gc_range *seed, size_t nseed,
                      struct pom_gc_range *merged, size_t merged_cap, struct pom_gc_stat *stat,
                      uint32_t *live, int *err, int *len_ok, int *entries_ok)
{
    if (lzo_mi355x_device_count() <= 0)
        return LZO_E_ERROR;
    if (column < 0 || column >= (int)POM_ITE_COLUMNS || pom_gc_seed_check(seed, nseed) != 0)
        return -EINVAL;
    memset(stat, 0, sizeof(*stat));
    size_t *first = malloc((n + 1) * sizeof(*first));
    if (!first)
        return LZO_E_OUT_OF_MEMORY;
    /* the scan's outputs without its ranges: nothing is placed, nothing runs out of room */
    const struct pom_walk_out O = {.out = NULL, .out_cap = 0, .unit = sizeof(struct pom_gc_range), .first = first,
                                   .live = live, .err = err, .len_ok = len_ok, .entries_ok = entries_ok,
                                   .count_only = 1};
    struct pom_walk_batch W;
    struct pom_gc_stat_sink M = {NULL, 0, 0};
    int rc = pom_walk_begin(&W, rec, rec_len, n, &O);
    if (rc == LZO_E_OK) {
        W.G.column = column;
        rc = pom_gc_stat_chunked(W.src, W.slen, W.m, &W.G, &M);
    }
    int frc = 0;
    if (rc == LZO_E_OK) {
        /* the order the chunks were delivered in does not reach the result: the fold sorts */
        size_t nmaps = 0, k = 0;
        for (const struct pom_walk_buf *b = M.maps; b; b = b->next)
            nmaps++;
        const struct pom_gc_range **maps = malloc((nmaps + 1) * sizeof(*maps));
        size_t *counts = malloc((nmaps + 1) * sizeof(*counts));
        if (maps && counts) {
            for (const struct pom_walk_buf *b = M.maps; b; b = b->next, k++) {
                maps[k] = (const struct pom_gc_range *)b->bytes;
                counts[k] = (size_t)b->pad;
            }
            frc = pom_gc_fold(maps, counts, nmaps, seed, nseed, merged, merged_cap, stat);
            stat->nin = M.nin;
            stat->nwrapped = M.nwrapped;
        } else {
            frc = LZO_E_OUT_OF_MEMORY;
        }
        free(maps);
        free(counts);
    }
    pom_walk_bufs_free(&M.maps);
    rc = pom_walk_finish(&W, rc, &O);
    free(first);
    return rc != LZO_E_OK ? rc : frc;
}
