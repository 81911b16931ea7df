/* single_queue.h -- the combining queue of the single calls (single_queue.c).
 * Internal to liblzo_mi355x.so; C and pthreads only, no HIP, so that
 * tests/native/single_check.c runs it on the CPU under the sanitizers.
 *
 * Calls that arrive together from several threads on the same GPU are
 * COMBINED: the first caller becomes the leader and runs every call queued
 * behind it (of the oldest call's kind, up to kScGroup calls and
 * kScGroupBytes) as one group through the run callback; the others sleep
 * until their result is in their request.  A lone call is a group of one. */
#ifndef POM_SINGLE_QUEUE_H
#define POM_SINGLE_QUEUE_H 1

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

enum { kScGroup = 64 };
#define kScGroupBytes ((size_t)256 << 20)

enum sc_kind { SC_COMPRESS, SC_SAFE, SC_UNCHECKED };

/* One call.  The queue reads kind, src_len and room and owns done, group and
 * next; the run callback fills rc and produced (and the bytes at dst). */
struct sc_req {
    enum sc_kind kind;
    const uint8_t *src;
    size_t src_len;
    uint8_t *dst;
    size_t room;
    size_t produced;
    int rc;
    int done;
    uint64_t group;             /* sequence number of the group that ran it */
    struct sc_req *next;
};

struct sc_queue {
    pthread_mutex_t mu;
    pthread_cond_t cv;
    struct sc_req *head, *tail;
    int leader;
    int last_k;                 /* size of the last group (a hint that callers come together) */
    uint64_t seq;               /* groups run so far */
};

/* Runs the k calls g[0, k), all of one kind; one group at a time per queue. */
typedef void (*sc_run_fn)(struct sc_req **g, int k, void *ctx);

void sc_queue_init(struct sc_queue *q);

/* Unlinks the next group into g[0, kScGroup): the queue's oldest calls of the
 * oldest call's kind, in order, while they fit kScGroup and kScGroupBytes of
 * input plus room (the first is always taken).  The others stay queued in
 * order.  Returns how many; the queue must not be empty.  No locking: the
 * caller holds q->mu (or has no other threads). */
int sc_queue_select(struct sc_queue *q, struct sc_req **g);

/* Queues r and returns once a group has run it: as the leader of that group
 * or asleep behind another.  *last_group is the calling thread's own word for
 * this queue (zero at first): the group of its previous call. */
void sc_queue_call(struct sc_queue *q, struct sc_req *r, uint64_t *last_group, sc_run_fn run, void *ctx);

#endif
