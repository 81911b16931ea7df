/*
 * pom_gc.h -- the MDSL garbage collector's data pass on the MI355X
 * (liblzo_mi355x.so): decode ITBs, walk their live column ranges, merge them
 * as the collector's range tree does, and return the merged map with its sums,
 * so that neither a decoded payload byte nor a per-file range has to leave the
 * GPU.
 *
 * Per ITB, mdsl_gc_data_round (mdsl/gc.c:815-1013) reads the record, decodes
 * it (itb_lzo_decompress, mdsl/gc.c:945-955) and walks the ITE bitmap
 * (mdsl/gc.c:968-993), handing each live ITE to __add_to_brtree
 * (mdsl/gc.c:788-802), which adds [offset, offset + len + 1) of one column to
 * a merging range tree when len > 0 (brt_add, lib/brtree.c:44-108).
 * mdsl_gc_data_stat (mdsl/gc.c:1020-1113) then walks the tree in order
 * (brt_loop_on_ranges) and folds it into gds->valid and gds->max
 * (gc_data_stat_cb, mdsl/gc.c:746-753).  These entry points batch all of it:
 *
 *   pom_gc_scan_dev    <- the bitmap walk and __add_to_brtree's range
 *                         mdsl/gc.c:968-993, :788-802 (payloads in HBM)
 *   pom_gc_scan_batch  <- the decode switch and the walk of one round
 *                         mdsl/gc.c:945-993 (records in host memory)
 *   pom_gc_merge_dev   <- brt_add, brt_loop_on_ranges and gc_data_stat_cb
 *                         over ranges in HBM
 *   pom_gc_stat_batch  <- all of the above for records in host memory, with
 *                         the extents of earlier rounds
 *
 * The file walk, hole detection (__is_hole), the range lookup, and gds->total
 * with gds->hole = total - valid, which need the data file, stay with the
 * caller (compose pom_itb_read_batch with pom_gc_stat_batch).
 */
#ifndef POM_GC_H
#define POM_GC_H 1

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Layout (LP64, the reference's build flags).  struct itbh, include/xtable.h:43-75: */
#define POM_ITBH_ADEPTH_OFF 3u      /* u8 adepth: the bitmap has 1 << adepth bits in use */
#define POM_ITBH_ENTRIES_OFF 4u     /* atomic_t entries: live ITEs */
/* Payload offsets, relative to &itb->lock (include/xtable.h:77-102): */
#define POM_ITB_BITMAP_OFF 3584u    /* u8 bitmap[128]: bit nr = bit nr % 8 of byte nr / 8 */
#define POM_ITB_BITMAP_BYTES 128u
#define POM_ITB_INDEX_OFF 3712u     /* struct itb_index index[] */
#define POM_ITB_ITE_OFF 11904u      /* struct ite ite[] */
#define POM_ITB_ADEPTH_MAX 10u      /* 1024 bitmap bits (ITB_DEPTH, include/xtable.h:136) */
/* struct ite, include/ite.h:60-114: */
#define POM_ITE_SIZE 512u
#define POM_ITE_COLUMN_OFF 368u     /* struct column column[6] */
#define POM_ITE_COLUMNS 6u
/* struct column, include/mds_api.h:232-237: */
#define POM_COLUMN_SIZE 24u
#define POM_COLUMN_ITBID_OFF 0u     /* u64 stored_itbid */
#define POM_COLUMN_LEN_OFF 8u       /* u64 len */
#define POM_COLUMN_OFFSET_OFF 16u   /* u64 offset */

/* The node __add_to_brtree builds (mdsl/gc.c:795-796): [offset, offset + len + 1),
 * in u64 arithmetic, wrapping as the C does. */
struct pom_gc_range {
    uint64_t low, high;
};

/* Per-ITB codes besides 0, -EINVAL (adepth 0 or above 10, a bad header) and
 * the decoder's LZO_E_* codes.  TRUNCATED: the payload ends inside the bitmap
 * or before the end of a live ITE; the ITB then yields no range (the
 * reference would read stale bytes of its full-size buffer there). */
#define POM_GC_E_TRUNCATED (-4097)
#define POM_GC_E_NOSPACE (-4098)

/* The walk of mdsl/gc.c:968-993 with __add_to_brtree (mdsl/gc.c:788-802) over
 * nitb decoded payloads in device memory; enqueue only, like
 * lzo_mi355x_decompress_dev.  Payload b is payload_len[b] bytes at payload +
 * payload_off[b], at any byte alignment; no byte outside it is read.
 * adepth[b] is its header's adepth, column 0 ... 5 the column asked for.
 * status may be NULL; a block with status[b] != 0 (its decoder's code) gets
 * err[b] = status[b] and live[b] = nranges[b] = 0.  Otherwise live[b] = the
 * set bitmap bits below 1 << adepth[b] (0 when err[b] says the bitmap is not
 * all there), nranges[b] = those whose column has len > 0, err[b] = 0,
 * -EINVAL or POM_GC_E_TRUNCATED (then nranges[b] = 0).  first has nitb + 1
 * entries: first[b] = the index of block b's first range, first[nitb] = the
 * total.  Block b's ranges, in bit order, go to ranges[first[b] ...] where
 * the index is below ranges_cap; nothing is written at or past ranges_cap
 * (ranges may be NULL when it is 0).  Every pointer is device memory.
 * Returns 0, or -1 when a launch failed or column is out of range. */
int pom_gc_scan_dev(const uint8_t *payload, const uint64_t *payload_off,
                    const uint32_t *payload_len, const int32_t *status,
                    const uint8_t *adepth, uint32_t nitb, int column,
                    uint32_t *live, uint32_t *nranges, uint64_t *first,
                    struct pom_gc_range *ranges, uint64_t ranges_cap, int32_t *err,
                    void *stream);

/* mdsl/gc.c:945-993 for n ITB records in host memory: rec[b] is a record as
 * stored, [struct itbh][payload], COMPR_NONE or COMPR_LZO, rec_len[b] bytes
 * readable; records are not modified.  Per ITB:
 *   err[b] = -EINVAL, no ranges: rec_len below the header size, h.len < 264,
 *     h.len > rec_len[b], a compress_algo other than NONE and LZO (the
 *     reference's default: case, mdsl/gc.c:956-960), an LZO record whose
 *     h.zlen - 264 is outside 1 ... POM_ITB_PAYLOAD_MAX, adepth 0 or above 10.
 *   A COMPR_LZO record is decoded on the GPU with lzo1x_decompress_safe
 *     semantics and capacity h.zlen - 264; a non-zero decoder code becomes
 *     err[b], no ranges (the reference aborts its round on it,
 *     mdsl/gc.c:950-954).  len_ok[b]: the decode produced exactly zlen - 264
 *     bytes (only logged by the reference, mdsl/gc.c:772-777); the walk runs
 *     over what was produced.  A COMPR_NONE record is walked as stored
 *     (len_ok[b] = 1).
 *   live[b] as pom_gc_scan_dev; entries_ok[b]: err[b] == 0 and live[b] ==
 *     h.entries (the reference's warning, mdsl/gc.c:989-993).
 * len_ok and entries_ok may be NULL.  Ranges come out in ITB order, then bit
 * order: first[b] (n + 1 entries) = the index of ITB b's first range,
 * first[n] = the total.  When the total exceeds ranges_cap the call returns
 * POM_GC_E_NOSPACE with first[], live[] and err[] complete and only
 * ranges[0, ranges_cap) written: size the buffer by first[n] and call again.
 * Only the compressed payloads go to the GPU and only the counts and ranges
 * come back.  Returns 0, POM_GC_E_NOSPACE, -EINVAL (column outside 0 ... 5),
 * LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path is unusable. */
int pom_gc_scan_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int column,
                      struct pom_gc_range *ranges, size_t ranges_cap, size_t *first,
                      uint32_t *live, int *err, int *len_ok, int *entries_ok);

/* What the tree computes, whatever the order of insertion: sort the ranges by
 * low; a range starts a new extent if and only if its low is strictly greater
 * than the largest high seen so far (touching ranges merge: the tree's compare
 * returns 0 for them); an extent is [first low, largest high); the walk
 * delivers the extents in ascending order.  A range with high <= low (a wrap
 * of offset + len + 1; the tree's comparator is inconsistent on such a node)
 * is not merged, only counted.
 *   valid     the sum of high - low over the extents (gds->valid), mod 2^64
 *   max       the last extent's high (gds->max), 0 with none
 *   nout      the extents
 *   nin       the ranges that came in
 *   nwrapped  those of them with high <= low */
struct pom_gc_stat {
    uint64_t valid, max, nout, nin, nwrapped;
};

/* The most ranges one pom_gc_merge_dev call takes. */
#define POM_GC_MERGE_MAX (1u << 30)

/* Bytes of device scratch pom_gc_merge_dev needs for n ranges (0 for n above
 * POM_GC_MERGE_MAX). */
size_t pom_gc_merge_scratch(uint32_t n);

/* brt_add, brt_loop_on_ranges and gc_data_stat_cb over n ranges in device
 * memory: a radix sort by low, a running maximum of high, the extents' heads,
 * the merged map; enqueue only, and the number of launches follows from n.
 * in is not modified and may sit at any 8-byte alignment, as may out, stat and
 * scratch; in may be the ranges of a pom_gc_scan_dev queued before on the same
 * stream.  Extent k goes to out[k] for k < out_cap, ascending; stat is always
 * written in full (with n == 0 in is not touched).  Nothing is written outside
 * stat, scratch[0, scratch_bytes) and out[0, min(nout, out_cap)).  Every
 * pointer is device memory.  Returns 0, or -1 when a launch failed, scratch
 * has fewer than pom_gc_merge_scratch(n) bytes or is not 8-byte aligned, or n
 * is above POM_GC_MERGE_MAX. */
int pom_gc_merge_dev(const struct pom_gc_range *in, uint32_t n,
                     void *scratch, size_t scratch_bytes,
                     struct pom_gc_range *out, uint64_t out_cap,
                     struct pom_gc_stat *stat, void *stream);

/* mdsl_gc_data_stat's tree for n ITB records in host memory and one column:
 * per ITB exactly pom_gc_scan_batch's live, err, len_ok and entries_ok; the
 * ranges of every ITB with err[b] == 0 are merged on the GPU, chunk by chunk,
 * and only each chunk's merged map comes back.  The chunks' maps and seed --
 * nseed extents of earlier rounds (mdsl_gc_data_stat runs redo_round into one
 * tree), ascending and disjoint with gaps of at least 1, may be NULL when
 * nseed is 0 -- are folded on the host with the same rule, so the result does
 * not depend on how the batch was cut.  merged gets the first merged_cap
 * extents; stat describes the whole folded map, with nin and nwrapped the
 * ITBs' ranges (the seed's are not counted): gds->valid = stat->valid,
 * gds->max = stat->max.  Returns 0; POM_GC_E_NOSPACE when stat->nout exceeds
 * merged_cap (everything else complete, only merged[0, merged_cap) written);
 * -EINVAL (column outside 0 ... 5, a seed that is not ascending and disjoint);
 * LZO_E_OUT_OF_MEMORY; LZO_E_ERROR when the GPU path is unusable (nothing is
 * computed then). */
int pom_gc_stat_batch(const uint8_t *const *rec, const size_t *rec_len, size_t n, int column,
                      const struct pom_gc_range *seed, size_t nseed,
                      struct pom_gc_range *merged, size_t merged_cap, struct pom_gc_stat *stat,
                      uint32_t *live, int *err, int *len_ok, int *entries_ok);

#ifdef __cplusplus
}
#endif

#endif /* POM_GC_H */
