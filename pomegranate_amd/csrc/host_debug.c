/* host_debug.c -- debug and experiment switches: ONE environment variable,
 * POM_LZO_DEBUG, a comma-separated list of key=value (INTEGRATION.md section
 * 6).  No product path needs it; an unset key takes its default.  Keys, by the
 * file that reads them:
 *   lzo_host.c             decoder=fast|win (device batches), host_timing=1,
 *                          slots=N, chunk_mb=N, dec_small_first=0, ooo=0,
 *                          enc_lds_max=N, fail_chunk=K (tests: a device's K-th
 *                          chunk delivery fails)
 *   host_ctx.c             sc_lat=0, sc_lat_min=BYTES
 *   host_single.c          sc_combine=0, sc_trace=1
 *   lzo1x_encode_fast.hip  enc_waves=1|2, enc_group=41|81|82|84, enc_grid=N
 *   itb_codec.c            append_worker=0, abuf_prealloc=0, fail_remap=1
 *   the record kernels     dents_copy, keys_search, keys_copy, find_copy,
 *                          kvget_copy, slice_groups (A/B switches of their launchers)
 * The variable is read once, at the first use, into a private copy;
 * lzo_mi355x_debug_reload() reads it again (tests change it between calls).
 * So the hot paths never call getenv.  Each (re)load publishes a new,
 * immutable copy through one atomic pointer, so a lookup on any thread reads
 * either the old or the new string whole, never one being rewritten; the
 * replaced copies are not freed (a reload is a test-time event and a lookup
 * may still be reading one). */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "host_debug.h"
#include "lzo_mi355x.h"

static pthread_mutex_t dbg_mu = PTHREAD_MUTEX_INITIALIZER;
static const char *dbg_cur;

static void dbg_load(int always)
{
    pthread_mutex_lock(&dbg_mu);
    if (always || !dbg_cur) {
        const char *e = getenv("POM_LZO_DEBUG");
        char *copy = strdup(e ? e : "");
        if (copy)
            __atomic_store_n(&dbg_cur, copy, __ATOMIC_RELEASE);
    }
    pthread_mutex_unlock(&dbg_mu);
}

void lzo_mi355x_debug_reload(void)
{
    dbg_load(1);
}

const char *pom_dbg_str(const char *key, char *buf, size_t n)
{
    const char *e = __atomic_load_n(&dbg_cur, __ATOMIC_ACQUIRE);
    if (!e) {
        dbg_load(0);                              /* first use */
        e = __atomic_load_n(&dbg_cur, __ATOMIC_ACQUIRE);
    }
    if (!e || !*e || !n)
        return NULL;
    const size_t kl = strlen(key);
    for (const char *p = e; *p;) {
        const char *end = strchr(p, ',');
        const size_t len = end ? (size_t)(end - p) : strlen(p);
        if (len > kl && strncmp(p, key, kl) == 0 && p[kl] == '=') {
            size_t vl = len - kl - 1;
            if (vl >= n)
                vl = n - 1;
            memcpy(buf, p + kl + 1, vl);
            buf[vl] = 0;
            return buf;
        }
        if (!end)
            break;
        p = end + 1;
    }
    return NULL;
}

long pom_dbg_int(const char *key, long dflt)
{
    char buf[32];
    const char *v = pom_dbg_str(key, buf, sizeof buf);
    return v && *v ? atol(v) : dflt;
}
