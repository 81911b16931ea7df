/* single_queue.c -- the combining queue of single_queue.h: the request list,
 * the selection of a group and the leader protocol.  What a group does is the
 * caller's run callback (host_single.c: one GPU launch). */
#include <time.h>

#include "single_queue.h"

void sc_queue_init(struct sc_queue *q)
{
    pthread_mutex_init(&q->mu, NULL);
    /* the leader's ~50 us wait for company is a relative time: measure
     * it on CLOCK_MONOTONIC, which wall-clock adjustments do not move */
    pthread_condattr_t ca;
    pthread_condattr_init(&ca);
    pthread_condattr_setclock(&ca, CLOCK_MONOTONIC);
    pthread_cond_init(&q->cv, &ca);
    pthread_condattr_destroy(&ca);
}

int sc_queue_select(struct sc_queue *q, struct sc_req **g)
{
    int k = 0;
    size_t bytes = 0;
    const enum sc_kind gk = q->head->kind;
    struct sc_req **pp = &q->head, *prev = NULL;
    while (*pp && k < kScGroup) {
        struct sc_req *x = *pp;
        const size_t xb = x->room + x->src_len;
        if (x->kind != gk || (k > 0 && bytes + xb > kScGroupBytes)) {
            prev = x;
            pp = &x->next;
            continue;
        }
        *pp = x->next;
        if (q->tail == x)
            q->tail = prev;
        x->next = NULL;
        g[k++] = x;
        bytes += xb;
    }
    return k;
}

void sc_queue_call(struct sc_queue *q, struct sc_req *r, uint64_t *last_group, sc_run_fn run, void *ctx)
{
    r->done = 0;
    r->next = NULL;
    pthread_mutex_lock(&q->mu);
    if (q->tail)
        q->tail->next = r;
    else
        q->head = r;
    q->tail = r;
    if (q->leader)
        pthread_cond_broadcast(&q->cv);         /* (a leader may be waiting for company) */
    while (!r->done) {
        if (q->leader) {
            pthread_cond_wait(&q->cv, &q->mu);
            continue;
        }
        /* lead: the queue's oldest calls of the oldest call's kind.  When this
         * thread's previous call was in the last group and that group had
         * company, the other callers are probably between two calls: give
         * them ~50 us to queue.  (A thread that was not in it -- a lone caller
         * after a burst of others -- does not wait.) */
        q->leader = 1;
        if (q->last_k > 1 && q->head == q->tail && *last_group == q->seq) {
            struct timespec ts;
            clock_gettime(CLOCK_MONOTONIC, &ts);
            ts.tv_nsec += 50000;
            if (ts.tv_nsec >= 1000000000L) {
                ts.tv_sec++;
                ts.tv_nsec -= 1000000000L;
            }
            pthread_cond_timedwait(&q->cv, &q->mu, &ts);
        }
        struct sc_req *g[kScGroup];
        const int k = sc_queue_select(q, g);
        pthread_mutex_unlock(&q->mu);
        run(g, k, ctx);
        pthread_mutex_lock(&q->mu);
        q->seq++;
        for (int i = 0; i < k; i++) {
            g[i]->done = 1;
            g[i]->group = q->seq;
        }
        q->leader = 0;
        q->last_k = k;
        pthread_cond_broadcast(&q->cv);
    }
    pthread_mutex_unlock(&q->mu);
    *last_group = r->group;
}
