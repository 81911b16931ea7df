/* host_requests.c -- host_requests.h: the header checks, the selection and
 * grouping of a call's requests, and a chunk's staging and scatter, for the
 * lookups and the key/value gets alike.  Plain pointer arithmetic: neither HIP
 * nor threads (lookup.c and kvget.c call the halves, host_records.c the chunk
 * parts from its callbacks). */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "host_requests.h"
#include "minilzo.h"
#include "pom_itb.h"
#include "pom_kvget.h"
#include "pom_lookup.h"

static uint32_t rd32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

static uint16_t rd16(const uint8_t *p)
{
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}

int pom_itb_walk_header(const uint8_t *rec, size_t rec_len, struct pom_walk_block *w)
{
    if (rec_len < POM_ITBH_SIZE)
        return -EINVAL;
    const uint32_t len = rd32(rec + POM_ITBH_LEN_OFF), zlen = rd32(rec + POM_ITBH_ZLEN_OFF);
    const uint16_t algo = rd16(rec + POM_ITBH_ALGO_OFF);
    const uint8_t ad = rec[POM_ITBH_ADEPTH_OFF];
    if (len < POM_ITBH_SIZE || len > rec_len || (algo != POM_COMPR_NONE && algo != POM_COMPR_LZO) ||
        ad == 0 || ad > POM_ITB_ADEPTH_MAX)
        return -EINVAL;
    if (algo == POM_COMPR_LZO &&
        (zlen <= POM_ITBH_SIZE || zlen - POM_ITBH_SIZE > POM_ITB_PAYLOAD_MAX))
        return -EINVAL;
    w->src = rec + POM_ITBH_SIZE;
    w->src_len = len - POM_ITBH_SIZE;
    w->is_lzo = algo == POM_COMPR_LZO;
    w->cap = w->is_lzo ? zlen - POM_ITBH_SIZE : 0;
    w->adepth = ad;
    w->entries = (int32_t)rd32(rec + POM_ITBH_ENTRIES_OFF);
    return 0;
}

void pom_walk_bufs_free(struct pom_walk_buf **bufs)
{
    while (*bufs) {
        struct pom_walk_buf *next = (*bufs)->next;
        free(*bufs);
        *bufs = next;
    }
}

size_t pom_group_requests(const size_t *key, size_t nreq, size_t m, size_t *first, size_t *ids)
{
    memset(first, 0, (m + 1) * sizeof(*first));
    for (size_t r = 0; r < nreq; r++)
        if (key[r] < m)
            first[key[r] + 1]++;
    for (size_t k = 0; k < m; k++)
        first[k + 1] += first[k];
    /* first[k] runs from group k's start to its end, which is group k + 1's start */
    for (size_t r = 0; r < nreq; r++)
        if (key[r] < m)
            ids[first[key[r]]++] = r;
    for (size_t k = m; k > 0; k--)
        first[k] = first[k - 1];
    first[0] = 0;
    return first[m];
}

/* ------------------------------------------------------------------------ */
/* The kinds                                                                 */
/* ------------------------------------------------------------------------ */
/* lookup: namelen <= 255.  get: POM_KV_STR set and sklen <= 320 (skey_off is
 * read by string gets of sklen <= 320 only). */
const struct req_spec pom_req_lookup = {
    .o_itb = offsetof(struct pom_lookup_req, itb), .o_blob = offsetof(struct pom_lookup_req, name_off),
    .o_len = offsetof(struct pom_lookup_req, namelen), .len_bytes = 2, .len_max = 255,
    .nwords = RW_DEPTH + 1, .rec_fixed = POM_LK_REC_SIZE};
/* unlink: the lookup's request and record, and a fourth word, `what` */
const struct req_spec pom_req_unlink = {
    .o_itb = offsetof(struct pom_lookup_req, itb), .o_blob = offsetof(struct pom_lookup_req, name_off),
    .o_len = offsetof(struct pom_lookup_req, namelen), .len_bytes = 2, .len_max = 255,
    .nwords = RW_LEN + 1, .rec_fixed = POM_LK_REC_SIZE};
const struct req_spec pom_req_kvget = {
    .o_itb = offsetof(struct pom_kvget_req, itb), .o_blob = offsetof(struct pom_kvget_req, skey_off),
    .o_len = offsetof(struct pom_kvget_req, sklen), .len_bytes = 4, .len_max = POM_KV_VALUE_MAX,
    .o_flag = offsetof(struct pom_kvget_req, kvflag), .flag_mask = POM_KV_STR,
    .nwords = RW_LEN + 1, .lease = 1, .rec_max = POM_KG_REC_MAX};

/* ------------------------------------------------------------------------ */
/* A chunk's requests                                                        */
/* ------------------------------------------------------------------------ */
/* (The loops below run once per request and bound a call of many requests an
 * ITB, DESIGN 5.9: the spec is copied into a local, which no store through a
 * byte pointer can alias, and a block's results are scattered array by array.) */
/* The blob bytes request q reads, or POM_REQ_REFUSED: by the kind's rule, or
 * because they are not all inside the call's blob. */
#define POM_REQ_REFUSED ((size_t)-1)
static inline size_t blob_bytes(const struct req_spec *Q, size_t blob_len, const uint8_t *q)
{
    const size_t n = Q->len_bytes == 2 ? rd16(q + Q->o_len) : rd32(q + Q->o_len);
    if (n > Q->len_max || (Q->flag_mask && !(rd32(q + Q->o_flag) & Q->flag_mask)))
        return POM_REQ_REFUSED;
    return (size_t)rd32(q + Q->o_blob) + n <= blob_len ? n : POM_REQ_REFUSED;
}

size_t pom_req_block(const struct pom_req_sink *K, size_t b, size_t *blob)
{
    const struct req_spec Q = *K->spec;
    size_t sum = 0;
    for (size_t k = K->req_first[b]; k < K->req_first[b + 1]; k++) {
        const size_t n = blob_bytes(&Q, K->blob_len, K->req + POM_REQ_SIZE * K->req_ids[k]);
        sum += n != POM_REQ_REFUSED ? n : 0;
    }
    *blob += sum;
    return K->req_first[b + 1] - K->req_first[b];
}

int pom_req_stage(const struct layout *L, uint8_t *h, const struct pom_req_sink *K)
{
    const struct req_spec Q = *K->spec;
    const struct req_layout *Y = &L->u.req;
    if (Y->nreq > 0xFFFFFFFFu / (Q.rec_max ? Q.rec_max : 1) || Y->blob_bytes > 0xFFFFFFF0u)
        return -1;
    const uint8_t *req = K->req, *from = K->blob;
    const size_t *ids = K->req_ids, blob_len = K->blob_len;
    uint8_t *rq = h + Y->o_req, *blob = h + Y->o_blob;
    size_t at = 0;
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i], end = K->req_first[b + 1];
        for (size_t k = K->req_first[b]; k < end; k++, rq += POM_REQ_SIZE) {
            const uint8_t *q = req + POM_REQ_SIZE * ids[k];
            const size_t n = blob_bytes(&Q, blob_len, q);
            const uint32_t itb = (uint32_t)i;   /* the chunk's own ITB index */
            const uint32_t off = n != POM_REQ_REFUSED ? (uint32_t)at : 0xFFFFFFFFu;
            memcpy(rq, q, POM_REQ_SIZE);
            memcpy(rq + Q.o_itb, &itb, 4);
            memcpy(rq + Q.o_blob, &off, 4);
            if (n != POM_REQ_REFUSED && n) {
                memcpy(blob + at, from + rd32(q + Q.o_blob), n);
                at += n;
            }
        }
    }
    return 0;
}

void pom_req_scatter(const struct layout *L, const uint8_t *h, struct pom_req_sink *K, const uint8_t *bytes,
                     size_t packed)
{
    const struct req_spec Q = *K->spec;
    const struct req_layout *Y = &L->u.req;
    const uint8_t *res = h + Y->o_hres, *fixed = res + Y->res_hdr;
    const uint64_t *lease = (const uint64_t *)(res + Y->r_lease);
    const uint32_t *len = (const uint32_t *)(res + Y->r_word[RW_LEN]);
    size_t j = 0, at = 0;
    for (size_t i = 0; i < L->nb; i++) {
        const size_t b = L->ids[i], n = K->req_first[b + 1] - K->req_first[b];
        const size_t *ids = K->req_ids + K->req_first[b];   /* the block's requests are the chunk's j ... j + n - 1 */
        K->status[b] = 0;                       /* delivered; the decoder's code is in the requests' err */
        for (size_t w = 0; w < Q.nwords; w++) {
            const uint32_t *from = (const uint32_t *)(res + Y->r_word[w]) + j;
            uint32_t *to = K->word[w];
            for (size_t k = 0; k < n; k++)
                to[ids[k]] = from[k];
        }
        for (size_t k = 0; k < n && Q.lease; k++)
            K->lease[ids[k]] = lease[j + k];
        for (size_t k = 0; k < n && Q.rec_fixed; k++)
            memcpy(K->fixed + Q.rec_fixed * ids[k], fixed + Q.rec_fixed * (j + k), Q.rec_fixed);
        for (size_t k = 0; k < n && Q.rec_max; k++) {
            const size_t m = len[j + k];
            K->recs[ids[k]] = K->records && m && at + m <= packed ? bytes + at : NULL;
            at += m;
        }
        j += n;
    }
}

/* ------------------------------------------------------------------------ */
/* A call's two halves                                                       */
/* ------------------------------------------------------------------------ */
/* mds/itb.c:1754-1755 in u64: the request's hash (a get's key) belongs to this ITB. */
static int itbid_matches(const uint8_t *rec, const uint8_t *q)
{
    const uint8_t depth = rec[POM_ITBH_DEPTH_OFF];
    uint64_t itbid, hash;
    memcpy(&itbid, rec + POM_ITBH_ITBID_OFF, 8);
    memcpy(&hash, q, 8);
    const uint64_t mask = depth >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << depth) - 1;
    return ((hash >> POM_ITB_ADEPTH_MAX) & mask) == itbid;
}

int pom_req_begin(struct pom_req_batch *W, const struct req_spec *Q, const uint8_t *const *rec,
                  const size_t *rec_len, size_t n, int itbid_check, const void *req, size_t nreq,
                  const uint8_t *blob, size_t blob_len, uint32_t *const word[RW_N], uint64_t *lease)
{
    memset(W, 0, sizeof *W);
    size_t *slot = malloc((n + 1) * sizeof(*slot));             /* ITB -> k, or a code below */
    W->key = malloc((nreq + 1) * sizeof(*W->key));              /* request -> k, or none */
    W->first = malloc((n + 2) * sizeof(*W->first));
    W->ids = malloc((nreq + 1) * sizeof(*W->ids));
    W->src = malloc((n + 1) * sizeof(*W->src));
    W->slen = malloc((n + 1) * sizeof(*W->slen));
    W->cap = malloc((n + 1) * sizeof(*W->cap));
    W->flags = malloc(2 * n + 1);                               /* is_lzo[m], adepth[m] */
    W->st = malloc((n + 1) * sizeof(*W->st));
    W->recs = Q->rec_max ? calloc(nreq + 1, sizeof(*W->recs)) : NULL;
    if (!slot || !W->key || !W->first || !W->ids || !W->src || !W->slen || !W->cap || !W->flags || !W->st ||
        (Q->rec_max && !W->recs)) {
        free(slot);
        return LZO_E_OUT_OF_MEMORY;
    }
    uint8_t *is_lzo = W->flags, *adepth = W->flags + n;
    int32_t *err = (int32_t *)word[RW_ERR];
    const size_t kUnseen = (size_t)-1, kBadHeader = (size_t)-2, kGood = (size_t)-3;
    for (size_t b = 0; b < n; b++)
        slot[b] = kUnseen;
    for (size_t w = RW_ERR + 1; w < Q->nwords; w++)
        memset(word[w], 0, nreq * sizeof(*word[w]));
    if (Q->lease)
        memset(lease, 0, nreq * sizeof(*lease));
    /* a request goes to the GPU when its ITB's header is good and the itbid check lets it walk */
    const size_t o_itb = Q->o_itb;
    size_t *key = W->key, m = 0;
    for (size_t r = 0; r < nreq; r++) {
        const uint8_t *q = (const uint8_t *)req + POM_REQ_SIZE * r;
        const size_t b = rd32(q + o_itb);
        key[r] = kUnseen;
        err[r] = -EINVAL;
        struct pom_walk_block w;
        if (b < n && slot[b] == kUnseen)
            slot[b] = pom_itb_walk_header(rec[b], rec_len[b], &w) == 0 ? kGood : kBadHeader;
        if (b >= n || slot[b] == kBadHeader)
            continue;                           /* decided here, and a bad header before the check */
        if (itbid_check && !itbid_matches(rec[b], q)) {
            err[r] = POM_LK_E_SPLIT;
            continue;
        }
        if (slot[b] == kGood) {
            pom_itb_walk_header(rec[b], rec_len[b], &w);
            slot[b] = m;
            W->src[m] = w.src;
            W->slen[m] = w.src_len;
            is_lzo[m] = w.is_lzo;
            W->cap[m] = w.cap;
            adepth[m] = w.adepth;
            m++;
        }
        key[r] = slot[b];
        err[r] = LZO_E_ERROR;                   /* until its chunk delivers */
    }
    free(slot);
    W->m = m;
    W->ngpu = pom_group_requests(W->key, nreq, m, W->first, W->ids);
    W->G = (struct pom_req_sink){.spec = Q, .is_lzo = is_lzo, .cap = W->cap, .adepth = adepth, .req_first = W->first,
                                 .req_ids = W->ids, .req = req, .blob = blob, .blob_len = blob_len, .lease = lease,
                                 .recs = W->recs, .status = W->st};
    memcpy(W->G.word, word, sizeof W->G.word);
    return LZO_E_OK;
}

int pom_req_finish(struct pom_req_batch *W, int rc, const uint8_t *const *rec)
{
    const struct pom_req_sink *G = &W->G;
    /* (the requests of chunks that were not delivered keep LZO_E_ERROR) */
    if (rc == LZO_E_OK) {
        /* mds/itb.c:2030-2033: a miss on an ITB that has just split */
        int32_t *err = (int32_t *)G->word[RW_ERR];
        for (size_t j = 0; j < W->ngpu; j++) {
            const size_t r = W->ids[j];
            if (err[r] == POM_LK_E_NOENT &&
                rec[rd32(G->req + POM_REQ_SIZE * r + G->spec->o_itb)][POM_ITBH_FLAG_OFF] == POM_ITB_JUST_SPLIT)
                err[r] = POM_LK_E_SPLIT;
        }
    }
    pom_walk_bufs_free(&W->G.bufs);
    free(W->key);
    free(W->first);
    free(W->ids);
    free(W->src);
    free(W->slen);
    free(W->cap);
    free(W->flags);
    free(W->st);
    free(W->recs);
    return rc;
}
