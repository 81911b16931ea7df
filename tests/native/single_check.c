/* single_check.c -- the single calls' combining queue
 * (pomegranate_amd/csrc/single_queue.c) and the debug keys (host_debug.c) on
 * the CPU.  Built twice by the Makefile: under AddressSanitizer and UBSan, and
 * under ThreadSanitizer.
 *   - the selection of a group, without threads: one kind out of a mixed
 *     list, the tail fix-up, the 64-call and 256 MiB caps;
 *   - the leader protocol: 8 threads of 300 calls each over two queues, kinds
 *     rotating, with a run callback that records what it is given;
 *   - pom_dbg_str and pom_dbg_int over POM_LZO_DEBUG and the reload.
 * Prints "single_check: ok"; exits non-zero at the first failure. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "host_debug.h"
#include "lzo_mi355x.h"
#include "single_queue.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "single_check: line %d: %s\n", __LINE__, #c);     \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

/* ---- selection ----------------------------------------------------------- */
static void push(struct sc_queue *q, struct sc_req *r, enum sc_kind kind, size_t src_len, size_t room)
{
    memset(r, 0, sizeof *r);
    r->kind = kind;
    r->src_len = src_len;
    r->room = room;
    if (q->tail)
        q->tail->next = r;
    else
        q->head = r;
    q->tail = r;
}

static void selection(void)
{
    struct sc_req r[65], *g[kScGroup];
    struct sc_queue q;
    /* kinds A B A A B: the three A in order; B B left in order, tail at the last B */
    const enum sc_kind A = SC_SAFE, B = SC_COMPRESS;
    const enum sc_kind mixed[5] = {A, B, A, A, B};
    memset(&q, 0, sizeof q);
    for (int i = 0; i < 5; i++)
        push(&q, &r[i], mixed[i], 100, 100);
    CHECK(sc_queue_select(&q, g) == 3);
    CHECK(g[0] == &r[0] && g[1] == &r[2] && g[2] == &r[3]);
    CHECK(!g[0]->next && !g[1]->next && !g[2]->next);
    CHECK(q.head == &r[1] && r[1].next == &r[4] && !r[4].next && q.tail == &r[4]);
    CHECK(sc_queue_select(&q, g) == 2 && g[0] == &r[1] && g[1] == &r[4] && !q.head && !q.tail);
    /* the tail is taken, another kind stays: the tail moves back to it */
    push(&q, &r[0], A, 1, 1);
    push(&q, &r[1], B, 1, 1);
    push(&q, &r[2], A, 1, 1);
    CHECK(sc_queue_select(&q, g) == 2 && g[0] == &r[0] && g[1] == &r[2]);
    CHECK(q.head == &r[1] && q.tail == &r[1] && !r[1].next);
    CHECK(sc_queue_select(&q, g) == 1 && g[0] == &r[1] && !q.head && !q.tail);
    /* one queued call */
    push(&q, &r[0], SC_UNCHECKED, 0, 0);
    CHECK(sc_queue_select(&q, g) == 1 && g[0] == &r[0] && !q.head && !q.tail);
    /* 65 of a kind: 64 taken, one left */
    for (int i = 0; i < 65; i++)
        push(&q, &r[i], A, 10, 10);
    CHECK(sc_queue_select(&q, g) == kScGroup);
    for (int i = 0; i < kScGroup; i++)
        CHECK(g[i] == &r[i]);
    CHECK(q.head == &r[64] && q.tail == &r[64] && !r[64].next);
    CHECK(sc_queue_select(&q, g) == 1 && g[0] == &r[64] && !q.head && !q.tail);
    /* the byte cap: the first call is taken even above it */
    push(&q, &r[0], A, kScGroupBytes, 1);
    push(&q, &r[1], A, 1, 1);
    CHECK(sc_queue_select(&q, g) == 1 && g[0] == &r[0] && q.head == &r[1] && q.tail == &r[1]);
    CHECK(sc_queue_select(&q, g) == 1 && !q.head && !q.tail);
    /* a later call that would pass the cap stays queued, in order; smaller ones behind it still go */
    const size_t half = kScGroupBytes / 2;
    push(&q, &r[0], A, half - 8, 8);            /* half */
    push(&q, &r[1], A, half, 1);                /* half + 1: would pass the cap */
    push(&q, &r[2], B, 1, 1);
    push(&q, &r[3], A, half - 1, 1);            /* exactly to the cap */
    push(&q, &r[4], A, 0, 1);                   /* one byte past it */
    CHECK(sc_queue_select(&q, g) == 2 && g[0] == &r[0] && g[1] == &r[3]);
    CHECK(q.head == &r[1] && r[1].next == &r[2] && r[2].next == &r[4] && !r[4].next && q.tail == &r[4]);
    CHECK(sc_queue_select(&q, g) == 2 && g[0] == &r[1] && g[1] == &r[4] && q.head == &r[2] && q.tail == &r[2]);
    CHECK(sc_queue_select(&q, g) == 1 && g[0] == &r[2] && !q.head && !q.tail);
}

/* ---- threads ------------------------------------------------------------- */
enum { kThreads = 8, kCalls = 300, kQueues = 2 };

struct stats {
    int running, max_running;   /* groups inside the callback (atomics) */
    long groups, calls, max_k, bad;     /* the leader flag serialises the callback: plain */
};

static struct sc_queue Q[kQueues];
static struct stats S[kQueues];
static int ran[kThreads * kCalls];

/* The call's id rides in room; its results are functions of id and kind. */
static size_t want_produced(size_t id) { return id * 3 + 1; }
static int want_rc(enum sc_kind kind, size_t id) { return (int)kind * 1000 + (int)(id % 1000); }

static void record_run(struct sc_req **g, int k, void *ctx)
{
    struct stats *s = ctx;
    const int now = __atomic_add_fetch(&s->running, 1, __ATOMIC_SEQ_CST);
    int seen = __atomic_load_n(&s->max_running, __ATOMIC_SEQ_CST);
    while (now > seen && !__atomic_compare_exchange_n(&s->max_running, &seen, now, 0, __ATOMIC_SEQ_CST,
                                                      __ATOMIC_SEQ_CST))
        ;
    s->groups++;
    s->calls += k;
    if (k > s->max_k)
        s->max_k = k;
    if (k < 1 || k > kScGroup)
        s->bad++;
    for (int i = 0; i < k; i++) {
        if (g[i]->kind != g[0]->kind || g[i]->next || g[i]->done)
            s->bad++;
        __atomic_add_fetch(&ran[g[i]->room], 1, __ATOMIC_SEQ_CST);
        g[i]->produced = want_produced(g[i]->room);
        g[i]->rc = want_rc(g[i]->kind, g[i]->room);
    }
    const struct timespec launch = {0, 20000};  /* (a launch takes a while: calls queue up behind it) */
    nanosleep(&launch, NULL);
    __atomic_sub_fetch(&s->running, 1, __ATOMIC_SEQ_CST);
}

static void *caller(void *arg)
{
    const size_t t = (size_t)arg;
    const int qi = (int)(t % kQueues);
    uint64_t last_group = 0;                    /* this thread's word for its queue */
    long wrong = 0;
    for (size_t c = 0; c < kCalls; c++) {
        const size_t id = t * kCalls + c;
        const enum sc_kind kind = (enum sc_kind)((t + c) % 3);
        struct sc_req r = {kind, NULL, 100, NULL, id, 0, -1, 0, 0, NULL};
        sc_queue_call(&Q[qi], &r, &last_group, record_run, &S[qi]);
        wrong += !r.done || r.produced != want_produced(id) || r.rc != want_rc(kind, id) || r.group == 0 ||
                 last_group != r.group;
    }
    return (void *)wrong;
}

static void threads(void)
{
    pthread_t th[kThreads];
    for (int i = 0; i < kQueues; i++)
        sc_queue_init(&Q[i]);
    alarm(120);                                 /* a lost wake-up ends the program, not the suite's patience */
    for (size_t t = 0; t < kThreads; t++)
        CHECK(pthread_create(&th[t], NULL, caller, (void *)t) == 0);
    for (size_t t = 0; t < kThreads; t++) {
        void *wrong = NULL;
        CHECK(pthread_join(th[t], &wrong) == 0);
        CHECK(wrong == NULL);                   /* every call returned what its callback wrote */
    }
    alarm(0);
    for (int i = 0; i < kThreads * kCalls; i++)
        CHECK(ran[i] == 1);                     /* every call ran exactly once */
    for (int i = 0; i < kQueues; i++) {
        CHECK(S[i].bad == 0 && S[i].max_k <= kScGroup);
        CHECK(S[i].max_k > 1);                  /* (calls did queue up behind a running group) */
        CHECK(S[i].max_running == 1 && S[i].running == 0);
        CHECK(S[i].calls == (long)kThreads / kQueues * kCalls);
        CHECK(Q[i].seq == (uint64_t)S[i].groups && !Q[i].head && !Q[i].tail && !Q[i].leader);
        printf("single_check: queue %d: %ld groups, largest %ld\n", i, S[i].groups, S[i].max_k);
    }
}

/* ---- debug keys ---------------------------------------------------------- */
/* A reload does not free the copy it replaces (host_debug.c: a lookup may
 * still be reading it): LeakSanitizer is told of that one allocation site. */
const char *__lsan_default_suppressions(void);
const char *__lsan_default_suppressions(void)
{
    return "leak:dbg_load\n";
}

const char *__lsan_default_options(void);
const char *__lsan_default_options(void)
{
    return "print_suppressions=0";
}

static void debug_keys(void)
{
    char buf[16];
    setenv("POM_LZO_DEBUG", "sc_lat=0,sc_lat_min=77", 1);
    lzo_mi355x_debug_reload();
    CHECK(pom_dbg_int("sc_lat", 1) == 0 && pom_dbg_int("sc_lat_min", 2048) == 77);
    CHECK(strcmp(pom_dbg_str("sc_lat_min", buf, sizeof buf), "77") == 0);
    CHECK(pom_dbg_str("sc_combine", buf, sizeof buf) == NULL && pom_dbg_int("sc_combine", 1) == 1);
    /* only sc_lat_min: sc_lat (a prefix of it) takes its default */
    setenv("POM_LZO_DEBUG", "sc_lat_min=5", 1);
    lzo_mi355x_debug_reload();
    CHECK(pom_dbg_int("sc_lat", 1) == 1 && pom_dbg_int("sc_lat_min", 2048) == 5);
    CHECK(pom_dbg_str("sc_lat", buf, sizeof buf) == NULL);
    /* an empty string, an unset variable */
    setenv("POM_LZO_DEBUG", "", 1);
    lzo_mi355x_debug_reload();
    CHECK(pom_dbg_int("sc_lat", 1) == 1 && pom_dbg_int("sc_lat_min", 2048) == 2048);
    CHECK(pom_dbg_str("decoder", buf, sizeof buf) == NULL);
    unsetenv("POM_LZO_DEBUG");
    lzo_mi355x_debug_reload();
    CHECK(pom_dbg_int("sc_lat", 1) == 1 && pom_dbg_int("sc_lat_min", 2048) == 2048);
    CHECK(pom_dbg_str("decoder", buf, sizeof buf) == NULL);
    /* an empty value is present as a string and the default as a number */
    setenv("POM_LZO_DEBUG", "decoder=,slots=3", 1);
    lzo_mi355x_debug_reload();
    CHECK(strcmp(pom_dbg_str("decoder", buf, sizeof buf), "") == 0 && pom_dbg_int("decoder", 9) == 9);
    CHECK(pom_dbg_int("slots", 4) == 3);
    /* a value longer than the buffer is cut, not overrun */
    struct {
        char before[8], buf[8], after[8];
    } guard;
    memset(&guard, 0x5A, sizeof guard);
    setenv("POM_LZO_DEBUG", "decoder=0123456789abcdefghijklmnopqrstuvwxyz0123456789,sc_lat_min=12345678901", 1);
    lzo_mi355x_debug_reload();
    CHECK(pom_dbg_str("decoder", guard.buf, sizeof guard.buf) == guard.buf);
    CHECK(strcmp(guard.buf, "0123456") == 0);
    for (size_t i = 0; i < 8; i++)
        CHECK(guard.before[i] == 0x5A && guard.after[i] == 0x5A);
    CHECK(pom_dbg_str("decoder", guard.buf, 1) == guard.buf && guard.buf[0] == 0 && guard.buf[1] == '1');
    CHECK(pom_dbg_str("decoder", guard.buf, 0) == NULL);
    CHECK(pom_dbg_int("sc_lat_min", 1) == 12345678901L);
    unsetenv("POM_LZO_DEBUG");
    lzo_mi355x_debug_reload();
}

int main(void)
{
    selection();
    threads();
    debug_keys();
    printf("single_check: ok\n");
    return 0;
}
