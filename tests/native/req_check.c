/* req_check.c -- the host arithmetic of the request operations
 * (pomegranate_amd/csrc/host_requests.c) on the CPU, under AddressSanitizer
 * and UBSan, for both kinds (lookup, key/value get):
 *   - selection and grouping (pom_req_begin) over handmade 264-byte ITB
 *     headers, against a naive model written here that scans all ITBs for
 *     every request;
 *   - the JUST_SPLIT pass (pom_req_finish);
 *   - the staging of a chunk's requests and blob (pom_req_stage) into a buffer
 *     of exactly htotal bytes, refused requests included;
 *   - the scatter of a chunk's results into the caller's request order
 *     (pom_req_scatter).
 * Records and buffers are allocated at their exact sizes, so that a read or
 * write past one is ASan's.  Prints the number of comparisons made; exits
 * non-zero at the first failure. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host_requests.h"
#include "minilzo.h"
#include "pom_itb.h"
#include "pom_kvget.h"
#include "pom_lookup.h"

static const char *what;
static unsigned long checked;

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "req_check: %s: line %d: %s\n", what, __LINE__, #cond);          \
            exit(1);                                                                         \
        }                                                                                    \
        checked++;                                                                           \
    } while (0)

static void *xmalloc(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (!p)
        exit(2);
    return p;
}

/* ------------------------------------------------------------------------ */
/* Handmade records                                                          */
/* ------------------------------------------------------------------------ */
struct hdr {
    size_t rec_len;             /* bytes allocated */
    uint32_t len, zlen;
    uint16_t algo;
    uint8_t adepth, depth, flag;
    uint64_t itbid;
};

static uint8_t *make_rec(const struct hdr *H)
{
    uint8_t *rec = xmalloc(H->rec_len);
    uint8_t full[POM_ITBH_SIZE];
    memset(full, 0, sizeof full);
    memset(rec, 0x5A, H->rec_len);
    full[POM_ITBH_FLAG_OFF] = H->flag;
    full[POM_ITBH_DEPTH_OFF] = H->depth;
    full[POM_ITBH_ADEPTH_OFF] = H->adepth;
    memcpy(full + POM_ITBH_ITBID_OFF, &H->itbid, 8);
    memcpy(full + POM_ITBH_LEN_OFF, &H->len, 4);
    memcpy(full + POM_ITBH_ZLEN_OFF, &H->zlen, 4);
    memcpy(full + POM_ITBH_ALGO_OFF, &H->algo, 2);
    memcpy(rec, full, H->rec_len < sizeof full ? H->rec_len : sizeof full);
    return rec;
}

/* The model's header rule, from the description in include/pom_gc.h. */
static int model_header_ok(const struct hdr *H)
{
    if (H->rec_len < 264 || H->len < 264 || H->len > H->rec_len)
        return 0;
    if (H->algo != POM_COMPR_NONE && H->algo != POM_COMPR_LZO)
        return 0;
    if (H->adepth < 1 || H->adepth > 10)
        return 0;
    if (H->algo == POM_COMPR_LZO && (H->zlen <= 264 || H->zlen - 264 > POM_ITB_PAYLOAD_MAX))
        return 0;
    return 1;
}

/* The model's itbid rule, bit by bit: the low `depth` bits of hash >> 10 are itbid's, its others are 0. */
static int model_itbid_ok(const struct hdr *H, uint64_t hash)
{
    for (unsigned i = 0; i < 64; i++) {
        const unsigned want = i < H->depth && i + 10 < 64 ? (unsigned)(hash >> (i + 10)) & 1 : 0;
        if (((H->itbid >> i) & 1) != want)
            return 0;
    }
    return 1;
}

/* ------------------------------------------------------------------------ */
/* Requests of either kind                                                   */
/* ------------------------------------------------------------------------ */
struct kind {
    const char *name;
    const struct req_spec *Q;
};
static const struct kind kKinds[2] = {{"lookup", &pom_req_lookup}, {"kvget", &pom_req_kvget}};

/* blob_len: namelen or sklen; str: a get's POM_KV_STR */
static void make_req(const struct kind *K, uint8_t *q, uint64_t hash, uint32_t itb, uint32_t blob_off,
                     uint32_t blob_len, int str)
{
    if (K->Q == &pom_req_lookup) {
        const struct pom_lookup_req r = {.hash = hash, .uuid = 77, .itb = itb, .flag = POM_LK_BY_NAME,
                                         .name_off = blob_off, .namelen = (uint16_t)blob_len, .column = 3};
        memcpy(q, &r, sizeof r);
    } else {
        const struct pom_kvget_req r = {.key = hash, .itb = itb, .flag = POM_KG_KV,
                                        .kvflag = (str ? POM_KV_STR : POM_KV_NORMAL) | 2, .skey_off = blob_off,
                                        .sklen = blob_len, .reserved = 9};
        memcpy(q, &r, sizeof r);
    }
}

static uint32_t field32(const uint8_t *q, size_t off)
{
    uint32_t v;
    memcpy(&v, q + off, 4);
    return v;
}

/* ------------------------------------------------------------------------ */
/* Selection and grouping against the model                                  */
/* ------------------------------------------------------------------------ */
static void select_case(const char *name, const struct kind *K, const struct hdr *H, size_t n, int itbid_check,
                        const uint32_t *itb, const uint64_t *hash, size_t nreq)
{
    what = name;
    const uint8_t **rec = xmalloc(n * sizeof(*rec));
    size_t *rec_len = xmalloc(n * sizeof(*rec_len));
    for (size_t b = 0; b < n; b++) {
        rec[b] = make_rec(&H[b]);
        rec_len[b] = H[b].rec_len;
    }
    uint8_t *req = xmalloc(POM_REQ_SIZE * nreq);
    for (size_t r = 0; r < nreq; r++)
        make_req(K, req + POM_REQ_SIZE * r, hash[r], itb[r], 0, 0, 1);
    int *err = xmalloc(nreq * sizeof(*err));
    uint32_t *words = xmalloc(3 * nreq * sizeof(*words));
    uint64_t *lease = xmalloc(nreq * sizeof(*lease));
    memset(err, 0x77, nreq * sizeof(*err));
    memset(words, 0x77, 3 * nreq * sizeof(*words));
    memset(lease, 0x77, nreq * sizeof(*lease));
    uint32_t *const word[RW_N] = {(uint32_t *)err, words, words + nreq, words + 2 * nreq};

    struct pom_req_batch W;
    CHECK(pom_req_begin(&W, K->Q, rec, rec_len, n, itbid_check, req, nreq, NULL, 0, word, lease) == LZO_E_OK);

    /* the model: every request scans all ITBs for its own */
    int *want = xmalloc(nreq * sizeof(*want));
    size_t *order = xmalloc(nreq * sizeof(*order));      /* the selected ITBs, by first GPU-bound request */
    size_t m = 0, ngpu = 0;
    for (size_t r = 0; r < nreq; r++) {
        want[r] = -EINVAL;
        for (size_t b = 0; b < n; b++)
            if (b == itb[r] && model_header_ok(&H[b]))
                want[r] = itbid_check && !model_itbid_ok(&H[b], hash[r]) ? POM_LK_E_SPLIT : LZO_E_ERROR;
        if (want[r] != LZO_E_ERROR)
            continue;
        ngpu++;
        size_t k = 0;
        while (k < m && order[k] != itb[r])
            k++;
        if (k == m)
            order[m++] = itb[r];
    }
    CHECK(W.m == m);
    CHECK(W.ngpu == ngpu);
    for (size_t r = 0; r < nreq; r++) {
        CHECK(err[r] == want[r]);               /* every request not GPU-bound has its final code */
        for (size_t w = 1; w < K->Q->nwords; w++)
            CHECK(word[w][r] == 0);
        if (K->Q->lease)
            CHECK(lease[r] == 0);
        else
            CHECK(lease[r] == 0x7777777777777777u);
    }
    const struct pom_req_sink *G = &W.G;
    CHECK(G->req_first[0] == 0);
    CHECK(G->req_first[m] == ngpu);
    size_t j = 0;
    for (size_t k = 0; k < m; k++) {
        const struct hdr *h = &H[order[k]];
        CHECK(G->req_first[k] <= G->req_first[k + 1]);
        CHECK(G->req_first[k] == j);
        CHECK(W.src[k] == rec[order[k]] + 264);
        CHECK(W.slen[k] == h->len - 264);
        CHECK(G->is_lzo[k] == (h->algo == POM_COMPR_LZO));
        CHECK(G->cap[k] == (h->algo == POM_COMPR_LZO ? h->zlen - 264 : 0));
        CHECK(G->adepth[k] == h->adepth);
        /* exactly this ITB's GPU-bound requests, in the caller's order */
        for (size_t r = 0; r < nreq; r++)
            if (want[r] == LZO_E_ERROR && itb[r] == order[k]) {
                CHECK(j < G->req_first[k + 1]);
                CHECK(G->req_ids[j] == r);
                j++;
            }
        CHECK(j == G->req_first[k + 1]);
    }
    CHECK(j == ngpu);
    CHECK(G->spec == K->Q && G->req == req && G->status == W.st && G->bufs == NULL);
    CHECK((G->recs != NULL) == (K->Q->rec_max != 0));

    /* the back half: a miss on a just-split ITB, among the GPU-bound requests alone */
    for (size_t r = 0; r < nreq; r++)
        if (err[r] == LZO_E_ERROR)
            err[r] = r % 2 ? POM_LK_E_NOENT : 0;
    CHECK(pom_req_finish(&W, LZO_E_OK, rec) == LZO_E_OK);
    for (size_t r = 0; r < nreq; r++) {
        if (want[r] != LZO_E_ERROR)
            CHECK(err[r] == want[r]);
        else if (r % 2)
            CHECK(err[r] == (H[itb[r]].flag == POM_ITB_JUST_SPLIT ? POM_LK_E_SPLIT : POM_LK_E_NOENT));
        else
            CHECK(err[r] == 0);
    }
    for (size_t b = 0; b < n; b++)
        free((void *)rec[b]);
    free(rec);
    free(rec_len);
    free(req);
    free(err);
    free(words);
    free(lease);
    free(want);
    free(order);
}

enum { kGoodLen = 264 + 40 };
#define GOOD(dep, id) {kGoodLen, kGoodLen, 0, POM_COMPR_NONE, 4, dep, 0, id}

static void selection(const struct kind *K)
{
    /* the world: good and bad headers, every way one fails */
    const uint64_t deep = 0x2AAAAAAAAAAAAAull;          /* 54 bits: hash >> 10 of ~0 is 2^54 - 1 */
    const struct hdr H[] = {
        GOOD(0, 0),                                                             /* 0 */
        {kGoodLen, kGoodLen, 264 + 5000, POM_COMPR_LZO, 10, 3, POM_ITB_JUST_SPLIT, 5},      /* 1 */
        GOOD(64, deep),                                                         /* 2 */
        {100, 100, 0, POM_COMPR_NONE, 4, 0, 0, 0},                              /* 3: rec_len < 264 */
        {kGoodLen, kGoodLen + 1, 0, POM_COMPR_NONE, 4, 0, 0, 0},                /* 4: len > rec_len */
        {kGoodLen, kGoodLen, 0, 2, 4, 3, 0, 6},                                 /* 5: algo neither value; depth 3, itbid 6 */
        {kGoodLen, kGoodLen, 0, POM_COMPR_NONE, 0, 0, 0, 0},                    /* 6: adepth 0 */
        {kGoodLen, kGoodLen, 0, POM_COMPR_NONE, 11, 0, 0, 0},                   /* 7: adepth 11 */
        {kGoodLen, kGoodLen, 264, POM_COMPR_LZO, 4, 0, 0, 0},                   /* 8: LZO, zlen <= 264 */
        {kGoodLen, kGoodLen, 264 + POM_ITB_PAYLOAD_MAX + 1, POM_COMPR_LZO, 4, 0, 0, 0},     /* 9: above the maximum */
        GOOD(0, 0),                                                             /* 10: named by no request */
        GOOD(3, 2),                                                             /* 11: named only by requests that fail the check */
        {kGoodLen, 263, 0, POM_COMPR_NONE, 4, 0, 0, 0},                         /* 12: len < 264 */
        {264, 264, 264 + POM_ITB_PAYLOAD_MAX, POM_COMPR_LZO, 1, 0, POM_ITB_JUST_SPLIT, 0},  /* 13: the largest capacity, no payload */
    };
    const size_t n = sizeof H / sizeof H[0];
    const uint32_t itb[] = {1,  13, 0, 3,  4,  5,  6, 7, 8, 9,          12,         1,          2,
                            2,  11, 11, 5, 0,  1,  (uint32_t)n, (uint32_t)n + 5, 0xFFFFFFFFu, 2, 13, 1};
    const uint64_t hash[] = {5ull << 10, 0,  ~0ull, 0, 0, 0, 0, 0, 0, 0, 0, (5ull << 10) | (1ull << 13), deep << 10,
                             (deep << 10) ^ (1ull << 63), 5ull << 10, 3ull << 10, 1ull << 10 /* bad header 5, and itbid 1 is not its 6: -EINVAL wins */,
                             123, (13ull << 10) | 1023, 0, 0, 0, (deep << 10) | 7, 1ull << 10, 4ull << 10};
    const size_t nreq = sizeof itb / sizeof itb[0];
    for (int check = 0; check < 2; check++) {
        select_case(check ? "world, itbid check on" : "world, itbid check off", K, H, n, check, itb, hash, nreq);
        select_case("n = 0 with requests", K, H, 0, check, itb, hash, nreq);
        select_case("nreq = 0", K, H, n, check, itb, hash, 0);
        select_case("one request", K, H, n, check, itb, hash, 1);
    }

    /* 300 shuffled requests over 7 ITBs, one of which holds 200 of them */
    struct hdr H7[7];
    uint32_t itb7[300];
    uint64_t hash7[300];
    for (size_t b = 0; b < 7; b++)
        H7[b] = (struct hdr)GOOD(3, b);
    H7[5].adepth = 0;                           /* one bad header among them */
    H7[2].flag = POM_ITB_JUST_SPLIT;
    for (size_t r = 0; r < 300; r++)
        itb7[r] = r < 200 ? 4 : (uint32_t)(r % 7);
    uint32_t x = 12345;
    for (size_t r = 299; r > 0; r--) {
        x = x * 1664525u + 1013904223u;
        const size_t s = (x >> 8) % (r + 1);
        const uint32_t t = itb7[r];
        itb7[r] = itb7[s];
        itb7[s] = t;
    }
    for (size_t r = 0; r < 300; r++) {
        x = x * 1664525u + 1013904223u;
        hash7[r] = ((uint64_t)(x % 5 ? itb7[r] : (itb7[r] + 1) % 8) << 10) | (x & 1023) | ((uint64_t)x << 40);
    }
    select_case("300 over 7, check off", K, H7, 7, 0, itb7, hash7, 300);
    select_case("300 over 7, check on", K, H7, 7, 1, itb7, hash7, 300);
}

/* ------------------------------------------------------------------------ */
/* Staging and scatter of the chunk {2, 0} of three blocks                   */
/* ------------------------------------------------------------------------ */
enum { kBlob = 700, kNreq = 9 };

struct want_req {
    uint32_t itb, off, len;     /* the caller's block; its blob offset and length */
    int str, ok;                /* a get's POM_KV_STR; accepted */
};

static void chunk_case(const struct kind *K, int records)
{
    what = K->name;
    const int lk = K->Q == &pom_req_lookup;
    const uint32_t big = lk ? 255 : 320;
    /* in the caller's order; blocks 2 and 0 make the chunk, block 1 stays out */
    const struct want_req R[kNreq] = {
        {0, 0xFFFFFFFFu, 1, 1, 0},              /* 0: the offset wraps in u32 arithmetic */
        {2, 10, 0, 1, 1},                       /* 1: zero length */
        {1, 20, 5, 1, 1},                       /* 2: not in the chunk */
        {2, kBlob - big, big, 1, 1},            /* 3: the longest, ending at the blob's end */
        {2, 40, big + 1, 1, 0},                 /* 4: too long */
        {0, 300, 4, 1, 1},                      /* 5 */
        {2, kBlob - 5, 6, 1, 0},                /* 6: one past the blob */
        {2, 50, 7, 0, lk},                      /* 7: a get that is no string get */
        {0, 60, 9, 1, 1},                       /* 8 */
    };
    uint8_t *blob = xmalloc(kBlob);
    for (size_t i = 0; i < kBlob; i++)
        blob[i] = (uint8_t)(i * 7 + 1);
    uint8_t *req = xmalloc(POM_REQ_SIZE * kNreq);
    for (size_t r = 0; r < kNreq; r++)
        make_req(K, req + POM_REQ_SIZE * r, 1000 + r, R[r].itb, R[r].off, R[r].len, R[r].str);
    /* grouped as pom_req_begin groups: block k's requests in the caller's order */
    size_t first[4] = {0}, rid[kNreq], nid = 0;
    for (uint32_t b = 0; b < 3; b++) {
        for (size_t r = 0; r < kNreq; r++)
            if (R[r].itb == b)
                rid[nid++] = r;
        first[b + 1] = nid;
    }
    int err[kNreq];
    uint32_t nr[kNreq], depth[kNreq], len[kNreq];
    uint64_t lease[kNreq];
    const uint8_t *recs[kNreq];
    uint8_t *fixed = xmalloc(POM_LK_REC_SIZE * kNreq);
    int32_t st[3] = {-9, -9, -9};
    struct pom_req_sink S = {.spec = K->Q, .req_first = first, .req_ids = rid, .req = req, .blob = blob,
                             .blob_len = kBlob, .records = records, .word = {(uint32_t *)err, nr, depth, len},
                             .lease = lease, .fixed = fixed, .recs = recs, .status = st};

    /* the chunk, in chunk order, and what the layout is sized with */
    const size_t ids[2] = {2, 0}, src_len[3] = {100, 50, 4000}, cap[3] = {0, 0, 9000};
    size_t chunk[kNreq], nchunk = 0, want_blob = 0, got_blob = 0, nreq = 0;
    for (size_t i = 0; i < 2; i++)
        for (size_t r = 0; r < kNreq; r++)
            if (R[r].itb == ids[i]) {
                chunk[nchunk++] = r;
                want_blob += R[r].ok ? R[r].len : 0;
            }
    for (size_t i = 0; i < 2; i++)
        nreq += pom_req_block(&S, ids[i], &got_blob);
    CHECK(nreq == nchunk);
    CHECK(got_blob == want_blob);
    struct layout L;
    pom_layout_req(&L, ids, 2, 1, src_len, cap, K->Q, nreq, got_blob, records, 1000);
    const struct req_layout *Y = &L.u.req;
    uint8_t *h = xmalloc(L.htotal), *ref = xmalloc(L.htotal);
    memset(h, 0xA5, L.htotal);
    CHECK(pom_req_stage(&L, h, &S) == 0);

    /* requests renumbered to 0 and 1 in chunk order, the blob repacked in that order */
    memset(ref, 0xA5, L.htotal);
    size_t at = 0;
    for (size_t j = 0; j < nchunk; j++) {
        const struct want_req *w = &R[chunk[j]];
        uint8_t *q = ref + Y->o_req + POM_REQ_SIZE * j;
        make_req(K, q, 1000 + chunk[j], w->itb == 2 ? 0 : 1, w->ok ? (uint32_t)at : 0xFFFFFFFFu, w->len, w->str);
        CHECK(field32(h + Y->o_req + POM_REQ_SIZE * j, K->Q->o_itb) == (w->itb == 2 ? 0u : 1u));
        CHECK(field32(h + Y->o_req + POM_REQ_SIZE * j, K->Q->o_blob) == (w->ok ? (uint32_t)at : 0xFFFFFFFFu));
        if (w->ok) {
            memcpy(ref + Y->o_blob + at, blob + w->off, w->len);
            at += w->len;
        }
    }
    CHECK(at == Y->blob_bytes);
    CHECK(memcmp(h, ref, L.htotal) == 0);       /* and not a byte elsewhere */

    /* results in chunk order in a fake staging land at the caller's indices */
    uint8_t *res = h + Y->o_hres;
    size_t packed = 0;
    for (size_t j = 0; j < nchunk; j++) {
        const uint32_t v[RW_N] = {(uint32_t)(-100 - (int)j), 1000 + (uint32_t)j, 2000 + (uint32_t)j,
                                  j % 3 ? 10 + (uint32_t)j : 0};
        const uint64_t ls = 0xABC00000000ull + j;
        for (size_t w = 0; w < K->Q->nwords; w++)
            memcpy(res + Y->r_word[w] + 4 * j, &v[w], 4);
        if (K->Q->lease)
            memcpy(res + Y->r_lease + 8 * j, &ls, 8);
        if (K->Q->rec_fixed)
            memset(res + Y->res_hdr + K->Q->rec_fixed * j, (int)j + 1, K->Q->rec_fixed);
        if (K->Q->rec_max)
            packed += v[RW_LEN];
    }
    uint8_t *bytes = xmalloc(packed);
    for (size_t r = 0; r < kNreq; r++) {
        err[r] = 7;
        nr[r] = depth[r] = len[r] = 7;
        lease[r] = 7;
        recs[r] = blob;
    }
    memset(fixed, 0xEE, POM_LK_REC_SIZE * kNreq);
    pom_req_scatter(&L, h, &S, bytes, records ? packed : 0);
    CHECK(st[2] == 0 && st[0] == 0 && st[1] == -9);
    at = 0;
    for (size_t j = 0; j < nchunk; j++) {
        const size_t r = chunk[j];
        const uint32_t l = j % 3 ? 10 + (uint32_t)j : 0;
        CHECK(err[r] == -100 - (int)j && nr[r] == 1000 + j && depth[r] == 2000 + j);
        if (lk) {
            for (size_t i = 0; i < POM_LK_REC_SIZE; i++)
                CHECK(fixed[POM_LK_REC_SIZE * r + i] == j + 1);
            CHECK(len[r] == 7 && lease[r] == 7 && recs[r] == blob);
        } else {
            CHECK(len[r] == l && lease[r] == 0xABC00000000ull + j);
            CHECK(recs[r] == (records && l ? bytes + at : NULL));
            at += l;
        }
    }
    for (size_t r = 0; r < kNreq; r++)
        if (R[r].itb == 1) {
            CHECK(err[r] == 7 && nr[r] == 7 && depth[r] == 7 && len[r] == 7 && lease[r] == 7 && recs[r] == blob);
            CHECK(fixed[POM_LK_REC_SIZE * r] == 0xEE && fixed[POM_LK_REC_SIZE * r + POM_LK_REC_SIZE - 1] == 0xEE);
        }
    free(bytes);
    free(h);
    free(ref);
    free(fixed);
    free(req);
    free(blob);
}

int main(void)
{
    for (size_t k = 0; k < 2; k++) {
        selection(&kKinds[k]);
        chunk_case(&kKinds[k], 1);
    }
    chunk_case(&kKinds[1], 0);                  /* a lengths-only get */
    printf("req_check: %lu checks ok\n", checked);
    return 0;
}
