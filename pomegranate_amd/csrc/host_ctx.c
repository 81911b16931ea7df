/* host_ctx.c -- what every host-side call of liblzo_mi355x.so runs on: the
 * GPU probe, the per-thread, per-device streams and staging, and the
 * per-device scratch of the latency decoder with the one routine that uses it.
 *
 * Threading: callers are MDS commit/service threads, the MDSL
 * GC thread and client threads.  Each host thread gets, on each GPU it uses,
 * kSlots HIP streams with their own device/pinned staging (grown on demand up
 * to one chunk, freed at thread exit), so concurrent calls never share device
 * state.  A host batch spreads over the GPUs on one helper thread per GPU
 * (batch_split.c), which use the calling thread's per-GPU resources. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "host_pipeline.h"
#include "lzo_mi355x.h"

/* ------------------------------------------------------------------------ */
/* GPU availability (checked once per process)                              */
/* ------------------------------------------------------------------------ */
static pthread_once_t gpu_once = PTHREAD_ONCE_INIT;
static int gpu_count;

static void gpu_probe(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fprintf(stderr, "liblzo_mi355x: no usable GPU (hipGetDeviceCount=%d); "
                        "the MI355X LZO1X codec has no CPU fallback\n", n);
        n = 0;
    }
    gpu_count = n;
}

int lzo_mi355x_device_count(void)
{
    pthread_once(&gpu_once, gpu_probe);
    return gpu_count;
}

/* ------------------------------------------------------------------------ */
/* Per-thread, per-device streams and staging                               */
/* ------------------------------------------------------------------------ */
struct tctx {
    struct dctx dev[kMaxDev];
};

static pthread_key_t tkey;
static pthread_once_t tkey_once = PTHREAD_ONCE_INIT;

static void tctx_free(void *p)
{
    struct tctx *t = p;
    if (!t)
        return;
    for (int d = 0; d < kMaxDev; d++) {
        struct dctx *c = &t->dev[d];
        if (!c->ready)
            continue;
        hipSetDevice(d);
        for (int k = 0; k < kSlots; k++) {
            if (c->s[k].dmem)
                hipFree(c->s[k].dmem);
            if (c->s[k].hmem)
                hipHostFree(c->s[k].hmem);
            hipStreamDestroy(c->s[k].stream);
        }
    }
    free(t);
}

static void tkey_make(void)
{
    pthread_key_create(&tkey, tctx_free);
}

struct tctx *pom_tctx_get(void)
{
    if (lzo_mi355x_device_count() <= 0)
        return NULL;
    pthread_once(&tkey_once, tkey_make);
    struct tctx *t = pthread_getspecific(tkey);
    if (!t) {
        t = calloc(1, sizeof(*t));
        if (!t)
            return NULL;
        pthread_setspecific(tkey, t);
    }
    return t;
}

struct dctx *pom_dctx_get(struct tctx *t, int device)
{
    if (device < 0 || device >= kMaxDev)
        return NULL;
    struct dctx *c = &t->dev[device];
    if (!c->ready) {
        for (int k = 0; k < kSlots; k++)
            if (hipStreamCreateWithFlags(&c->s[k].stream, hipStreamNonBlocking) != hipSuccess) {
                while (k-- > 0)
                    hipStreamDestroy(c->s[k].stream);
                return NULL;
            }
        c->ready = 1;
    }
    return c;
}

int pom_slot_reserve(struct slot *t, size_t dbytes, size_t hbytes)
{
    /* growth: +25%, or doubling up to 64 MiB (combined single calls grow
     * their groups step by step; each regrowth is a hipMalloc/hipHostMalloc).
     * The device side grows in 2 MiB steps: a lone 536 KB lzo1x_1_compress,
     * whose device staging holds only its input, took 5,260-5,272 us on a
     * 1 MiB allocation against 5,240-5,244 on a 2 MiB one (and 607 against
     * 600 us for 64 KiB; profiles/host_split/ab.log, g2) -- presumably the
     * larger allocation's larger page fragments. */
    const size_t kDoubleMax = (size_t)64 << 20;
    if (dbytes > t->dcap) {
        const size_t old = t->dcap;
        if (t->dmem)
            hipFree(t->dmem);
        t->dmem = NULL;
        t->dcap = 0;
        size_t want = POM_ALIGN_UP(dbytes + dbytes / 4, 2 << 20);
        if (want < 2 * old && 2 * old <= kDoubleMax)
            want = 2 * old;
        if (hipMalloc((void **)&t->dmem, want) != hipSuccess)
            return -1;
        t->dcap = want;
    }
    if (hbytes > t->hcap) {
        const size_t old = t->hcap;
        if (t->hmem)
            hipHostFree(t->hmem);
        t->hmem = NULL;
        t->hcap = 0;
        size_t want = POM_ALIGN_UP(hbytes + hbytes / 4, 1 << 20);
        if (want < 2 * old && 2 * old <= kDoubleMax)
            want = 2 * old;
        if (hipHostMalloc((void **)&t->hmem, want, hipHostMallocDefault) != hipSuccess)
            return -1;
        t->hcap = want;
    }
    return 0;
}

struct slot *pom_single_slot(void)
{
    struct tctx *t = pom_tctx_get();
    int dev = 0;
    if (!t || hipGetDevice(&dev) != hipSuccess)
        return NULL;
    struct dctx *c = pom_dctx_get(t, dev);
    return c ? &c->s[0] : NULL;
}

/* ------------------------------------------------------------------------ */
/* The latency decoder                                                      */
/* ------------------------------------------------------------------------ */
/* Its scratch: ONE buffer per device, shared by every thread's host-batch
 * chunks and combined single-call groups (per-thread, per-slot buffers of up
 * to 1 GiB each pinned GBs of HBM).  A user holds the mutex while it launches,
 * waits (on the GPU, through the event) for the previous use's kernels, and
 * records its own.  Groups needing more than kLatMaxScratch (from ~1 MB of
 * compressed input) take the windowed decoder. */
static const size_t kLatMaxScratch = (size_t)256 << 20;
struct lat_scratch {
    pthread_mutex_t mu;
    void *buf;
    size_t cap;
    hipEvent_t done;            /* the last use's kernels (created with the buffer) */
};
static struct lat_scratch lat_s[kMaxDev];
static pthread_once_t lat_once = PTHREAD_ONCE_INIT;

static void lat_init(void)
{
    for (int d = 0; d < kMaxDev; d++)
        pthread_mutex_init(&lat_s[d].mu, NULL);
}

/* The device's scratch, at least `bytes`, locked, with stream s ordered
 * after its last use; NULL (unlocked) if the device or memory is missing. */
static struct lat_scratch *lat_acquire(size_t bytes, hipStream_t s)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev || bytes > kLatMaxScratch)
        return NULL;
    pthread_once(&lat_once, lat_init);
    struct lat_scratch *L = &lat_s[dev];
    pthread_mutex_lock(&L->mu);
    if (!L->done && hipEventCreateWithFlags(&L->done, hipEventDisableTiming) != hipSuccess) {
        L->done = NULL;
        pthread_mutex_unlock(&L->mu);
        return NULL;
    }
    if (L->cap < bytes) {
        hipEventSynchronize(L->done);           /* (a never-recorded event is complete) */
        if (L->buf)
            hipFree(L->buf);
        L->buf = NULL;
        L->cap = 0;
        size_t want = POM_ALIGN_UP(bytes + bytes / 4, (size_t)1 << 20);
        want = want < kLatMaxScratch ? want : kLatMaxScratch;
        if (hipMalloc(&L->buf, want) != hipSuccess) {
            L->buf = NULL;
            pthread_mutex_unlock(&L->mu);
            return NULL;
        }
        L->cap = want;
    }
    if (hipStreamWaitEvent(s, L->done, 0) != hipSuccess) {
        pthread_mutex_unlock(&L->mu);
        return NULL;
    }
    return L;
}

static void lat_release(struct lat_scratch *L, hipStream_t s)
{
    hipEventRecord(L->done, s);
    pthread_mutex_unlock(&L->mu);
}

/* A decode whose compressed block is at least this long takes the latency
 * decoder (the whole GPU on one block, 0.11-0.14 ms from 32 KiB up to 536 KB,
 * where the windowed decoder's one workgroup takes 0.14-2.2 ms); shorter ones
 * (equal at 12 KB) the caller's other decoders.  Debug keys: sc_lat_min sets
 * the threshold (bytes of compressed input), sc_lat=0 turns it off. */
static int use_lat_decoder(size_t z)
{
    const long min_z = pom_dbg_int("sc_lat", 1) == 0 ? 0x7FFFFFFFL : pom_dbg_int("sc_lat_min", 2048L);
    return z >= (size_t)(min_z > 0 ? min_z : 2048L);
}

/* (Separate pipelines on four streams were measured first: they did not
 * overlap -- three 64 KiB blocks 0.38 ms against 0.19 for one.) */
int pom_lat_decode(const uint8_t *src, const uint64_t *src_off, const uint32_t *z, uint8_t *dst,
                   const uint64_t *dst_off, const uint32_t *cap, uint32_t nb, uint32_t *out_len,
                   int32_t *status, uint32_t *fb, uint32_t *ids, hipStream_t s)
{
    if (nb == 0 || nb > kLatGroup)
        return 0;
    for (uint32_t i = 0; i < nb; i++)
        if (!use_lat_decoder(z[i]))
            return 0;
    const size_t need = lzo_mi355x_decompress_lat_scratch_n(src_off, z, cap, nb);
    if (need == 0 || need > kLatMaxScratch)
        return 0;                               /* out of its range */
    struct lat_scratch *LS = lat_acquire(need, s);
    if (!LS)
        return 0;
    const int rc = lzo_mi355x_launch_decompress_lat_n(src, src_off, z, dst, dst_off, cap, nb, out_len, status,
                                                      fb, ids, 0, LS->buf, LS->cap, s);
    lat_release(LS, s);
    return rc == 0 ? 1 : -1;
}
