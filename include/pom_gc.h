/*
 * pom_gc.h -- the MDSL garbage collector's data scan on the MI355X
 * (liblzo_mi355x.so): decode ITBs and return the live column ranges, so that
 * no decoded payload byte has to leave the GPU.
 *
 * Per ITB, mdsl_gc_data_round (mdsl/gc.c:815-1013) reads the record, decodes
 * it (itb_lzo_decompress, mdsl/gc.c:945-955) and walks the ITE bitmap
 * (mdsl/gc.c:968-993), handing each live ITE to __add_to_brtree
 * (mdsl/gc.c:788-802), which keeps [offset, offset + len + 1) of one column
 * when len > 0.  These entry points batch the decode and the walk:
 *
 *   pom_gc_scan_dev    <- the bitmap walk and __add_to_brtree's range
 *                         mdsl/gc.c:968-993, :788-802 (payloads in HBM)
 *   pom_gc_scan_batch  <- the decode switch and the walk of one round
 *                         mdsl/gc.c:945-993 (records in host memory)
 *
 * The file walk, hole detection, the range lookup and the tree itself stay
 * with the caller (compose pom_itb_read_batch with pom_gc_scan_batch).
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

#ifdef __cplusplus
}
#endif

#endif /* POM_GC_H */
