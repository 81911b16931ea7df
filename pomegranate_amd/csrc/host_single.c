/* host_single.c -- the minilzo.h call surface of liblzo_mi355x.so (lzo_init,
 * lzo1x_1_compress, lzo1x_decompress, lzo1x_decompress_safe; reference
 * lib/minilzo.c) on top of the HIP kernels.  Every codec call runs on the
 * GPU; there is no CPU codec in this library.  A call made without a usable
 * GPU returns LZO_E_ERROR and says why on stderr once.
 *
 * The entry points code one block per call, synchronously.  Calls that arrive
 * together from several threads on the same GPU (the MDS commit threads,
 * mds/txg.c:1010-1011, and the service threads that load ITBs,
 * mds/itb.c:2964) are combined by the queue of single_queue.h into groups of
 * one kind, each run here as one launch.  Debug key sc_combine=0 turns
 * combining off (every call its own launch).
 * Staging of a group of k calls (pom_layout_single):
 *   [0, o_src)      header arrays: src_off u64[k], dst_off u64[k], src_len[k],
 *                   dst_cap[k], out_len[k], status[k], pre-scan length[k] and
 *                   status[k], the decoder's fallback list (count + k ids)
 *   [o_src, o_dst)  the inputs, 256-byte aligned
 *   [o_dst, htotal) host only: the outputs (each: worst case, the caller's
 *                   capacity or a guess)
 * The kernels write the output and its length/status straight into the pinned
 * host staging (hipHostMalloc, mapped into the device's address space), so
 * nothing is copied back; the caller reads it only after the stream
 * synchronisation, which is what makes the kernels' writes visible to the
 * host.  One H2D copy ([0, o_dst)), one kernel, one synchronisation: the
 * windowed decoder refuses few valid streams, so the exact decoder runs only
 * when a status says a block was handed over.
 */
#include <pthread.h>
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "host_pipeline.h"
#include "lzo_mi355x.h"
#include "minilzo.h"
#include "single_queue.h"

/* Per device: the queue, and the staging of its groups.  The leader flag
 * gives one group at a time per device, so one slot serves every thread
 * (per-thread slots each grew to the groups their thread happened to lead,
 * and every regrowth is a hipMalloc / hipHostMalloc). */
struct sc_dev {
    struct sc_queue q;
    int ready;                  /* the slot's stream is created */
    struct slot slot;
};

static struct sc_dev sc_d[kMaxDev];
static __thread uint64_t sc_last_group[kMaxDev];   /* per device: group of this thread's last single call */
static pthread_once_t sc_once = PTHREAD_ONCE_INIT;

static void sc_init(void)
{
    for (int d = 0; d < kMaxDev; d++)
        sc_queue_init(&sc_d[d].q);
}

/* The group's slot; without combining (D == NULL) the calling thread's own. */
static struct slot *sc_slot(struct sc_dev *D)
{
    if (!D)
        return pom_single_slot();
    if (!D->ready) {
        if (hipStreamCreateWithFlags(&D->slot.stream, hipStreamNonBlocking) != hipSuccess)
            return NULL;
        D->ready = 1;
    }
    return &D->slot;
}

/* One launch for the k calls g[0..k) (all of one kind): fills each call's rc
 * and produced length and copies its output.  The queue's run callback. */
static void sc_run_group(struct sc_req **g, int k, void *ctx)
{
    const enum sc_kind kind = g[0]->kind;
    const int trace = pom_dbg_int("sc_trace", 0) == 1;
    const double t0 = trace ? pom_now_ms() : 0.0;
    size_t z[kScGroup], room[kScGroup], o_src[kScGroup], o_out[kScGroup];
    for (int i = 0; i < k; i++) {
        g[i]->rc = LZO_E_ERROR;
        z[i] = g[i]->src_len;
        room[i] = g[i]->room;
    }
    struct slot *t = sc_slot(ctx);
    if (!t)
        return;
    struct single_layout L;
    pom_layout_single(&L, (size_t)k, z, room, o_src, o_out);
    if (pom_slot_reserve(t, L.dtotal, L.htotal) != 0)
        return;
    uint8_t *h = t->hmem, *d = t->dmem;
    hipStream_t s = t->stream;
    /* the host side's arrays: filled here, and out_len and status written by the kernels */
    uint64_t *so = (uint64_t *)(h + L.o_srcoff), *dof = (uint64_t *)(h + L.o_dstoff);
    uint32_t *sl = (uint32_t *)(h + L.o_srclen), *dc = (uint32_t *)(h + L.o_dstcap);
    uint32_t *olen = (uint32_t *)(h + L.o_outlen);
    int32_t *ost = (int32_t *)(h + L.o_status);
    const uint32_t *plen = (const uint32_t *)(h + L.o_plen);
    /* the device side's, as the kernels read them */
    const uint64_t *d_so = (const uint64_t *)(d + L.o_srcoff), *d_dof = (const uint64_t *)(d + L.o_dstoff);
    const uint32_t *d_sl = (const uint32_t *)(d + L.o_srclen), *d_dc = (const uint32_t *)(d + L.o_dstcap);
    uint32_t *d_fb = (uint32_t *)(d + L.o_fb);
    memset(h, 0, L.o_src);
    for (int i = 0; i < k; i++) {
        so[i] = o_src[i];
        dof[i] = o_out[i];
        sl[i] = (uint32_t)z[i];
        dc[i] = (uint32_t)room[i];
        ost[i] = -1;
        if (z[i])
            memcpy(h + o_src[i], g[i]->src, z[i]);
    }
    if (hipMemcpyAsync(d, h, L.o_dst, hipMemcpyHostToDevice, s) != hipSuccess)
        return;
    int rc;
    if (kind == SC_COMPRESS) {
        /* no scratch: the LDS-dictionary encoder, faster for a few blocks; the
         * general encoder's pass only for a block over 16 MiB */
        int big = 0;
        for (int i = 0; i < k; i++)
            big |= z[i] > LZO_MI355X_FAST_MAX_N;
        rc = lzo_mi355x_launch_compress_fast(d, d_so, d_sl, h, d_dof, d_dc, olen, ost, (uint32_t)k, NULL, 0, s);
        if (rc == 0 && big)
            rc = lzo_mi355x_launch_compress(d, d_so, d_sl, h, d_dof, d_dc, olen, ost, (uint32_t)k, 1, s);
    } else {
        /* SC_UNCHECKED: decoded into the room; the unchecked decoder never
         * reports an output overrun (lib/minilzo.c:3676-3680), so
         * OUTPUT_OVERRUN here means the stream is longer than the room.
         * The latency decoder where the group is its kind (pom_lat_decode),
         * else the windowed one, which never reads its output back (host
         * memory); the fallback list lives in the header (zeroed by the H2D
         * copy). */
        const int lat = pom_lat_decode(d, so, sl, h, dof, dc, (uint32_t)k, olen, ost, d_fb, d_fb + 1, s);
        rc = lat < 0   ? -1
             : lat > 0 ? 0
                       : lzo_mi355x_launch_decompress_win(d, d_so, d_sl, h, d_dof, d_dc, olen, ost, d_fb,
                                                          d_fb + 1, (uint32_t)k, s);
    }
    if (rc != 0 || hipStreamSynchronize(s) != hipSuccess)
        return;
    if (kind != SC_COMPRESS) {
        int handed = 0;
        for (int i = 0; i < k; i++)
            handed |= ost[i] == LZO_MI355X_DEC_PENDING;
        if (handed &&
            (lzo_mi355x_launch_decompress_exact(d, d_so, d_sl, h, d_dof, d_dc, olen, ost, d_fb, d_fb + 1,
                                                (uint32_t)k, (uint32_t)k, kind == SC_UNCHECKED, s) != 0 ||
             hipStreamSynchronize(s) != hipSuccess))
            return;
    }
    int over = 0;
    for (int i = 0; i < k; i++)
        over |= kind == SC_UNCHECKED && ost[i] == LZO_E_OUTPUT_OVERRUN;
    if (over) {
        /* rare: the decoded lengths (inputs still on the GPU); a call whose
         * stream is longer than its room retries with that much room */
        if (lzo_mi355x_launch_decoded_length(d, d_so, d_sl, (uint32_t *)(d + L.o_plen),
                                             (int32_t *)(d + L.o_pstatus), (uint32_t)k, NULL, 0xFFFFFFFFu,
                                             s) != 0 ||
            hipMemcpyAsync(h + L.pre_off, d + L.pre_off, L.pre_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return;
    }
    for (int i = 0; i < k; i++) {
        struct sc_req *r = g[i];
        if (over && ost[i] == LZO_E_OUTPUT_OVERRUN && plen[i] > r->room) {
            r->produced = plen[i];
            r->rc = 1;
            continue;
        }
        const size_t n = olen[i] < r->room ? olen[i] : r->room;
        if (n)
            memcpy(r->dst, h + o_out[i], n);
        r->produced = olen[i];
        r->rc = ost[i];
    }
    if (trace)
        fprintf(stderr, "pom single-call group: kind %d, %d calls, %.3f ms\n", (int)kind, k, pom_now_ms() - t0);
}

static int single_call(enum sc_kind kind, const uint8_t *src, size_t src_len, uint8_t *dst,
                       size_t room, size_t *produced)
{
    int dev = 0;
    if (src_len > 0xFFFFFFF0u || room > 0xFFFFFFF0u || lzo_mi355x_device_count() <= 0 ||
        hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev)
        return LZO_E_ERROR;
    struct sc_req r = {kind, src, src_len, dst, room, 0, LZO_E_ERROR, 0, 0, NULL};
    if (pom_dbg_int("sc_combine", 1) == 0) {
        struct sc_req *g = &r;
        sc_run_group(&g, 1, NULL);
    } else {
        pthread_once(&sc_once, sc_init);
        sc_queue_call(&sc_d[dev].q, &r, &sc_last_group[dev], sc_run_group, &sc_d[dev]);
    }
    *produced = r.produced;
    return r.rc;
}

/* lib/minilzo.c:3159-3207.  The output is the reference's with a zero-filled
 * wrkmem (SURVEY.md finding 3), so wrkmem is not read. */
int lzo1x_1_compress(const lzo_bytep src, lzo_uint src_len, lzo_bytep dst, lzo_uintp dst_len,
                     lzo_voidp wrkmem)
{
    (void)wrkmem;
    size_t n = 0;
    const int rc = single_call(SC_COMPRESS, src, src_len, dst,
                               lzo_mi355x_worst_compress(src_len), &n);
    if (rc != LZO_E_ERROR)
        *dst_len = n;
    return rc;
}

/* lib/minilzo.c:3703-4190: *dst_len is the capacity in, the produced length out. */
int lzo1x_decompress_safe(const lzo_bytep src, lzo_uint src_len, lzo_bytep dst,
                          lzo_uintp dst_len, lzo_voidp wrkmem)
{
    (void)wrkmem;
    size_t n = 0;
    const int rc = single_call(SC_SAFE, src, src_len, dst, *dst_len, &n);
    if (rc != LZO_E_ERROR)
        *dst_len = n;
    return rc;
}

/* GPU pre-scan of one host-resident stream: decoded length and status.  A
 * group of one call with no room, on the calling thread's own slot. */
int lzo_mi355x_decoded_length(const uint8_t *src, unsigned long src_len, unsigned long *dst_len)
{
    struct slot *t = pom_single_slot();
    if (!t || src_len > 0xFFFFFFF0u)
        return LZO_E_ERROR;
    struct single_layout L;
    const size_t z = src_len, room = 0;
    size_t o_src, o_out;
    pom_layout_single(&L, 1, &z, &room, &o_src, &o_out);
    if (pom_slot_reserve(t, L.dtotal, L.htotal) != 0)
        return LZO_E_ERROR;
    uint8_t *h = t->hmem, *d = t->dmem;
    hipStream_t s = t->stream;
    memset(h, 0, L.o_src);
    *(uint64_t *)(h + L.o_srcoff) = o_src;
    *(uint32_t *)(h + L.o_srclen) = (uint32_t)src_len;
    if (src_len)
        memcpy(h + o_src, src, src_len);
    if (hipMemcpyAsync(d, h, o_src + src_len, hipMemcpyHostToDevice, s) != hipSuccess ||
        lzo_mi355x_launch_decoded_length(d, (const uint64_t *)(d + L.o_srcoff), (const uint32_t *)(d + L.o_srclen),
                                         (uint32_t *)(d + L.o_plen), (int32_t *)(d + L.o_pstatus), 1, NULL,
                                         0xFFFFFFFFu, s) != 0 ||
        hipMemcpyAsync(h + L.pre_off, d + L.pre_off, L.pre_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return LZO_E_ERROR;
    *dst_len = *(const uint32_t *)(h + L.o_plen);
    return *(const int32_t *)(h + L.o_pstatus);
}

/* The unchecked decoder (lib/minilzo.c:3308-3699) that mds/itb.c:2964,
 * mdsl/gc.c:770 and api/api.c:6438 call.  It never learns the destination
 * size (mds/itb.c:2951-2964 passes an uninitialised *out_len): the GPU
 * decodes into a guessed room (16x the input, at least 256 KiB) and the
 * output comes back with its length in one round trip; only a block that
 * decodes to more than that takes a length pre-scan and a second decode. */
int lzo1x_decompress(const lzo_bytep src, lzo_uint src_len, lzo_bytep dst, lzo_uintp dst_len,
                     lzo_voidp wrkmem)
{
    (void)wrkmem;
    size_t room = (size_t)src_len * 16;
    if (room < ((size_t)256 << 10))
        room = (size_t)256 << 10;
    if (room > 0xFFFFFFF0u)
        room = 0xFFFFFFF0u;
    size_t n = 0;
    int rc = single_call(SC_UNCHECKED, src, src_len, dst, room, &n);
    if (rc == 1)                                   /* longer than the guess */
        rc = single_call(SC_UNCHECKED, src, src_len, dst, n, &n);
    if (rc != LZO_E_ERROR)
        *dst_len = n;
    return rc;
}

/* ------------------------------------------------------------------------ */
/* The rest of the liblzo2 surface                                          */
/* ------------------------------------------------------------------------ */

/* lib/minilzo.c:2567-2598: a zero version or a type-size mismatch is
 * LZO_E_ERROR; additionally the GPU must be usable. */
int __lzo_init_v2(unsigned v, int s1, int s2, int s3, int s4, int s5, int s6, int s7, int s8,
                  int s9)
{
    if (v == 0)
        return LZO_E_ERROR;
    int ok = (s1 == -1 || s1 == (int)sizeof(short)) && (s2 == -1 || s2 == (int)sizeof(int)) &&
             (s3 == -1 || s3 == (int)sizeof(long)) &&
             (s4 == -1 || s4 == (int)sizeof(lzo_uint32)) &&
             (s5 == -1 || s5 == (int)sizeof(lzo_uint)) &&
             (s6 == -1 || s6 == (int)lzo_sizeof_dict_t) &&
             (s7 == -1 || s7 == (int)sizeof(char *)) &&
             (s8 == -1 || s8 == (int)sizeof(lzo_voidp)) &&
             (s9 == -1 || s9 == (int)sizeof(lzo_callback_t));
    if (!ok)
        return LZO_E_ERROR;
    return lzo_mi355x_device_count() > 0 ? LZO_E_OK : LZO_E_ERROR;
}

unsigned lzo_version(void) { return LZO_VERSION; }
const char *lzo_version_string(void) { return LZO_VERSION_STRING; }
const char *lzo_version_date(void) { return LZO_VERSION_DATE; }
lzo_charp _lzo_version_string(void) { return (lzo_charp)LZO_VERSION_STRING; }
lzo_charp _lzo_version_date(void) { return (lzo_charp)LZO_VERSION_DATE; }
/* lib/minilzo.c:2306-2314 (minilzo builds return LZO_VERSION_STRING) */
lzo_bytep lzo_copyright(void) { return (lzo_bytep)LZO_VERSION_STRING; }

/* Host utilities of the reference's minilzo.c (lib/minilzo.c:2355-2500). */
int lzo_memcmp(const lzo_voidp a, const lzo_voidp b, lzo_uint len) { return memcmp(a, b, len); }
lzo_voidp lzo_memcpy(lzo_voidp dst, const lzo_voidp src, lzo_uint len) { return memcpy(dst, src, len); }
lzo_voidp lzo_memmove(lzo_voidp dst, const lzo_voidp src, lzo_uint len) { return memmove(dst, src, len); }
lzo_voidp lzo_memset(lzo_voidp buf, int c, lzo_uint len) { return memset(buf, c, len); }

lzo_uint32 lzo_adler32(lzo_uint32 c, const lzo_bytep buf, lzo_uint len)
{
    if (buf == NULL)
        return 1;
    uint32_t lo = c & 0xffffu, hi = (c >> 16) & 0xffffu;
    const unsigned char *p = buf;
    while (len > 0) {
        /* 5552 bytes keep both sums below 2^32 before the reduction */
        lzo_uint k = len < 5552 ? len : 5552;
        len -= k;
        for (lzo_uint i = 0; i < k; i++) {
            lo += p[i];
            hi += lo;
        }
        p += k;
        lo %= 65521u;
        hi %= 65521u;
    }
    return (hi << 16) | lo;
}

int _lzo_config_check(void)
{
    union {
        unsigned long a[2];
        unsigned char b[2 * sizeof(unsigned long)];
    } u;
    u.a[0] = u.a[1] = 0;
    u.b[0] = 128;
    lzo_uint v;
    memcpy(&v, u.b, sizeof v);
    return v == 128 ? LZO_E_OK : LZO_E_ERROR;       /* little-endian, as the codec assumes */
}

lzo_uintptr_t __lzo_ptr_linear(const lzo_voidp ptr) { return (lzo_uintptr_t)ptr; }

unsigned __lzo_align_gap(const lzo_voidp p, lzo_uint size)
{
    const lzo_uintptr_t a = (lzo_uintptr_t)p;
    return size ? (unsigned)(((a + size - 1) / size) * size - a) : 0u;
}
