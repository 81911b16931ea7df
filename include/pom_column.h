/*
 * pom_column.h -- the client column-data codec of api/api.c on the MI355X
 * LZO1X batch path (liblzo_mi355x.so).
 *
 * Column data written with SCD_LZO is [size_t original length][LZO1X-1
 * stream] (LP64: an 8-byte length), sent raw when that is not smaller than
 * the data:
 *   pom_col_zip_batch   <- hvfs_fwrite SCD_LZO     api/api.c:6509-6541
 *   pom_col_zipv        <- hvfs_fwritev SCD_LZO    api/api.c:6652-6689
 *   pom_col_unzip_batch <- the read side           api/api.c:6427-6446
 *   pom_col_read_batch  <- the read side with its region copy
 *                                                  api/api.c:6427-6460
 *   pom_col_slice_dev   <- the region copy alone   api/api.c:6447-6460
 *
 * Three reference defects are not reproduced:
 *   - the zip buffer is len + 8 bytes (api/api.c:6512), which LZO1X-1 output
 *     can overrun on incompressible data (up to len + len/16 + 67): here the
 *     output never exceeds the caller's capacity;
 *   - hvfs_fwritev compresses each iovec into its own stream and
 *     concatenates them, which the read side (one lzo1x_decompress call)
 *     cannot decode (INPUT_NOT_CONSUMED after the first stream).  Here
 *     pom_col_zipv writes the iovecs as one stream, which that same read side
 *     decodes, and pom_col_unzip_batch also reads the reference writer's
 *     layout (consecutive streams until the input is used up), so columns the
 *     reference already wrote stay readable;
 *   - at api/api.c:6441-6446 a decode that returns LZO_E_OK with olen !=
 *     olen_cmp jumps to fallback: with err == 0, and the read then reports
 *     `size` bytes although it wrote none.  Here that column is LZO_E_ERROR,
 *     in pom_col_read_batch as in pom_col_unzip_batch.
 */
#ifndef POM_COLUMN_H
#define POM_COLUMN_H 1

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POM_COL_HDR 8u              /* sizeof(size_t) on LP64 */

/* Capacity that always holds the zipped form of len bytes. */
size_t pom_col_zip_bound(size_t len);

/* n columns.  zip_len[b] = bytes written to zip[b]; compressed[b] = 1 for
 * [len][LZO1X], 0 when the column goes raw (nothing is written then, as the
 * reference falls back to the caller's buffer).  Returns 0, or an LZO_E_*
 * code when the GPU path is unusable. */
int pom_col_zip_batch(const uint8_t *const *data, const size_t *len, size_t n,
                      uint8_t *const *zip, const size_t *zip_cap, size_t *zip_len,
                      int *compressed);

/* The iovec form: the iovecs are one column of sum(iov_len) bytes. */
int pom_col_zipv(const uint8_t *const *iov_base, const size_t *iov_len, size_t iovcnt,
                 uint8_t *zip, size_t zip_cap, size_t *zip_len, int *compressed);

/* n zipped columns -> out[b] (capacity out_cap[b]).  err[b] = 0 when the
 * stream (or the reference fwritev layout's consecutive streams) decodes to
 * exactly its recorded length, else the decoder's LZO_E_* code, or
 * LZO_E_ERROR for a length mismatch or a column shorter than its header.
 * out_len[b] = bytes produced. */
int pom_col_unzip_batch(const uint8_t *const *zip, const size_t *zip_len, size_t n,
                        uint8_t *const *out, const size_t *out_cap, size_t *out_len, int *err);

/* One read: size bytes from byte offset of decoded column col. */
struct pom_col_req { uint64_t offset, size; uint32_t col, pad; };   /* pad: 0 */

/* api/api.c:6427-6460 for ncol zipped columns and nreq reads of them.  Several
 * requests may name one column; it is decoded once.  A column no request names
 * is not sent to the GPU.  out[r] has room for req[r].size bytes.
 *
 * Per request, c = req[r].col and W = the length column c records; the first
 * rule that applies decides:
 *   1  c >= ncol                                   err = -EINVAL
 *   2  column c is shorter than its 8-byte header  err = LZO_E_ERROR
 *   3  the decoder's code is not 0                 err = that code
 *   4  the decode produced another length than W   err = LZO_E_ERROR
 *   5  offset > W                                  err = -EINVAL (api/api.c:6449-6454;
 *                                                  offset == W is a valid empty read)
 *   6  otherwise err = 0, out_len = min(size, W - offset); size = UINT64_MAX
 *      is legal
 * With err != 0, out_len = 0 and no byte of out[r] is written; no byte is
 * ever written past out[r] + out_len[r].
 *
 * The decode has lzo1x_decompress_safe semantics with capacity W, so a stream
 * that yields more than W reports LZO_E_OUTPUT_OVERRUN (pom_col_unzip_batch
 * called with a larger capacity reports LZO_E_ERROR there).  W sizes device
 * memory and comes from an unchecked header: W > 0xFFFFFFF0 (the batch ABI's
 * 32-bit capacity) and W > 255 * (zip_len - 8) (more than the stream's bytes
 * can yield: a match turns k + 4 bytes into at most 288 + 255k) are
 * LZO_E_ERROR under rule 3 before anything is allocated.  The reference
 * hvfs_fwritev layout is read as pom_col_unzip_batch reads it.
 *
 * Returns 0, LZO_E_OUT_OF_MEMORY, or LZO_E_ERROR when the GPU path is
 * unusable (without a GPU: always). */
int pom_col_read_batch(const uint8_t *const *zip, const size_t *zip_len, size_t ncol,
                       const struct pom_col_req *req, size_t nreq,
                       uint8_t *const *out, size_t *out_len, int *err);

/* The region copy alone over decoded columns in HBM; enqueue only.  Column c
 * is data_len[c] bytes (the produced length, e.g. lzo_mi355x_decompress_dev's
 * out_len) at data + data_off[c], status[c] its decoder code (status NULL: all
 * 0) and want[c] its recorded length; request r lands at out + out_off[r].
 * Rules 1 and 3 to 6 above give out_len[r] and err[r].  data_off and out_off
 * may have any alignment; no byte outside a column is loaded except within an
 * aligned dword that overlaps it, and no byte outside [out_off[r], out_off[r]
 * + out_len[r]) is written.  Returns 0, or -1 when the launch failed. */
int pom_col_slice_dev(const uint8_t *data, const uint64_t *data_off, const uint32_t *data_len,
                      const int32_t *status, const uint64_t *want, uint32_t ncol,
                      const struct pom_col_req *req, uint32_t nreq,
                      uint8_t *out, const uint64_t *out_off,
                      uint32_t *out_len, int32_t *err, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* POM_COLUMN_H */
