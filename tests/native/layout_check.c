/* layout_check.c -- the staging layouts of the host batches
 * (pomegranate_amd/csrc/host_layout.c) checked on the CPU, under
 * AddressSanitizer and UBSan: for every operation and every combination of
 * block count, LZO prefix, sizes, request counts, blob lengths, both request
 * kinds (the get with and without records) and kvlist options below,
 *   - every array starts at a multiple of its element size;
 *   - the input bytes start at a multiple of 256, each block's at a multiple of 16;
 *   - the regions of the host staging are pairwise disjoint and end within
 *     htotal, those of the device staging within dtotal;
 *   - the H2D span [0, o_dst) holds exactly the uploaded fields (but for
 *     alignment padding);
 *   - the result D2H span is exactly the union of the operation's result fields.
 * The same rules hold for the staging of the single calls' groups
 * (pom_layout_single) of 1 to 64 calls, whose inputs and outputs are each
 * 256-byte aligned and whose only D2H span is the pre-scan's.
 * Prints the number of layouts checked; exits non-zero at the first failure. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host_layout.h"
#include "host_requests.h"
#include "pom_column.h"
#include "pom_kvlist.h"

enum { HOST = 1, DEV = 2, BOTH = 3 };
enum { PLAIN, UPLOAD, RESULT };         /* UPLOAD: inside the H2D span; RESULT: also inside the result D2H span */

struct region {
    const char *name;
    size_t off, elem, bytes;
    int side, kind;
};

static struct region R[40];
static size_t nR;
static const char *what;
static unsigned long checked;

static void fail(const char *msg, const struct region *a, const struct region *b)
{
    fprintf(stderr, "layout_check: %s: %s: %s%s%s\n", what, msg, a ? a->name : "", b ? " / " : "", b ? b->name : "");
    exit(1);
}

static void add(const char *name, size_t off, size_t elem, size_t bytes, int side, int kind)
{
    if (nR == sizeof R / sizeof R[0])
        fail("too many regions", NULL, NULL);
    R[nR++] = (struct region){name, off, elem, bytes, side, kind};
}

/* The arrays every layout has. */
static void add_shared(const struct layout *L, int outlen_kind)
{
    add("src_off", L->o_srcoff, 8, 8 * L->nb, BOTH, UPLOAD);
    add("dst_off", L->o_dstoff, 8, 8 * L->nb, BOTH, UPLOAD);
    add("src_len", L->o_srclen, 4, 4 * L->nb, BOTH, UPLOAD);
    add("dst_cap", L->o_dstcap, 4, 4 * L->nb, BOTH, UPLOAD);
    if (outlen_kind >= 0) {
        add("out_len", L->o_outlen, 4, 4 * L->nb, BOTH, outlen_kind);
        add("status", L->o_status, 4, 4 * L->nb, BOTH, outlen_kind);
    }
}

/* The inputs, the device's output slots and its scratch. */
static void add_bytes(const struct layout *L, const size_t *src_len, const size_t *cap, size_t scratch)
{
    size_t s = 0, d = 0;
    for (size_t i = 0; i < L->nb; i++) {
        if ((L->o_src + s) % 16 || (L->o_dst + d) % 16)
            fail("a block's bytes are not 16-byte aligned", NULL, NULL);
        s += POM_ALIGN_UP(src_len[L->ids[i]], 16);
        if (i < L->nlzo)
            d += POM_ALIGN_UP(cap[L->ids[i]], 16);
    }
    if (L->o_src % 256 || L->o_dst % 256)
        fail("o_src or o_dst is not a multiple of 256", NULL, NULL);
    add("src bytes", L->o_src, 1, s, BOTH, UPLOAD);
    add("dst slots", L->o_dst, 1, d, DEV, PLAIN);
    add("scratch", L->o_scr, 1, scratch, DEV, PLAIN);
}

static int overlap(const struct region *a, const struct region *b)
{
    return a->bytes && b->bytes && a->off < b->off + b->bytes && b->off < a->off + a->bytes;
}

static int by_off(const void *a, const void *b)
{
    const struct region *x = a, *y = b;
    return x->off < y->off ? -1 : x->off > y->off ? 1 : x->bytes < y->bytes ? -1 : x->bytes > y->bytes;
}

/* res_off/res_bytes: the D2H span of the RESULT regions. */
static void check(const struct layout *L, size_t res_off, size_t res_bytes)
{
    for (size_t i = 0; i < nR; i++) {
        const struct region *a = &R[i];
        if (a->off % a->elem)
            fail("misaligned", a, NULL);
        if ((a->side & HOST) && a->off + a->bytes > L->htotal)
            fail("ends beyond htotal", a, NULL);
        if ((a->side & DEV) && a->off + a->bytes > L->dtotal)
            fail("ends beyond dtotal", a, NULL);
        if (a->kind != PLAIN && a->off + a->bytes > L->o_dst)
            fail("uploaded but outside the H2D span", a, NULL);
        if (a->kind == PLAIN && a->bytes && a->off < L->o_dst)
            fail("inside the H2D span but not uploaded", a, NULL);
        for (size_t j = i + 1; j < nR; j++)
            if ((a->side & R[j].side) && overlap(a, &R[j]))
                fail("overlap", a, &R[j]);
    }
    /* the uploaded fields fill [0, o_dst) but for padding to 256; the results fill their span */
    qsort(R, nR, sizeof R[0], by_off);
    size_t at = 0, res_at = res_off, res_seen = 0;
    for (size_t i = 0; i < nR; i++) {
        if (R[i].kind != PLAIN && R[i].bytes) {
            if (R[i].off - at >= 256)
                fail("a hole in the H2D span before", &R[i], NULL);
            at = R[i].off + R[i].bytes;
        }
        if (R[i].kind == RESULT) {
            if (R[i].off != res_at)
                fail("the result span has a hole or starts elsewhere, at", &R[i], NULL);
            res_at += R[i].bytes;
            res_seen = 1;
        }
    }
    if (L->o_dst - at >= 256)
        fail("a hole at the end of the H2D span", NULL, NULL);
    if (res_seen && res_at != res_off + res_bytes)
        fail("the result span is not the union of the result fields", NULL, NULL);
    checked++;
}

/* Results that lie behind the H2D span, alike on both sides: the fields, then 16-byte aligned the payload. */
static void check_results(const struct layout *L, size_t o_res, size_t o_hres, size_t res_hdr, size_t res_bytes,
                          const struct region *fields, size_t nfields, size_t payload)
{
    size_t at = 0;
    for (size_t i = 0; i < nfields; i++) {
        if (fields[i].off != at)
            fail("result header field out of place", &fields[i], NULL);
        at += fields[i].bytes;
        add(fields[i].name, o_res + fields[i].off, fields[i].elem, fields[i].bytes, DEV, PLAIN);
        add(fields[i].name, o_hres + fields[i].off, fields[i].elem, fields[i].bytes, HOST, PLAIN);
    }
    if (res_hdr != POM_ALIGN_UP(at, 16) || res_bytes != res_hdr + payload || o_res % 16 || o_hres % 16)
        fail("result span is not its fields plus the payload", NULL, NULL);
    add("result payload", o_res + res_hdr, 16, payload, DEV, PLAIN);
    add("result payload", o_hres + res_hdr, 16, payload, HOST, PLAIN);
    check(L, 0, 0);
}

static const size_t kSizes[] = {0, 1, 15, 16, 17, 4096, 11904 + 512 + 5};      /* the last: room for one ITE */
static const size_t kScratch[] = {0, 1000};
static const size_t kReqs[] = {0, 1, 3};
static const uint8_t kGc[] = {WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_ERR};
static const uint8_t kRd[] = {WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_BYTES, WW_ERR};
static const uint8_t kKv[] = {WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_BYTES, WW_KEYBYTES, WW_ERR};
static const char *kWord[WW_N] = {"status", "out_len", "live", "count", "bytes", "keybytes", "err"};

static void walk_case(const char *name, const struct walk_spec *W, const size_t *ids, size_t nb, size_t nlzo,
                      const size_t *src_len, const size_t *cap, size_t scratch)
{
    struct layout L;
    what = name;
    nR = 0;
    pom_layout_walk(&L, ids, nb, nlzo, src_len, cap, W, scratch);
    const struct walk_layout *K = &L.u.walk;
    size_t ites = 0;
    for (size_t i = 0; i < nb; i++)
        ites += pom_walk_max_ites(i < nlzo ? cap[ids[i]] : src_len[ids[i]]);
    if (K->rcap != ites * W->per_ite || L.o_status != K->o_word[WW_STATUS] || L.o_outlen != K->o_word[WW_OUTLEN])
        fail("record room or the decoders' words", NULL, NULL);
    add_shared(&L, -1);
    add("scan_off", K->scan.o_scanoff, 8, 8 * nb, BOTH, UPLOAD);
    add("first", K->o_first, 8, 8 * (nb + 1), BOTH, UPLOAD);
    for (size_t w = 0; w < W->nwords; w++)
        add(kWord[W->words[w]], K->o_word[W->words[w]], 4, 4 * nb, BOTH, RESULT);
    add("adepth", K->scan.o_adepth, 1, nb, BOTH, UPLOAD);
    if (W->needle)
        add("needle", K->o_needle, 1, 256, BOTH, UPLOAD);
    add_bytes(&L, src_len, cap, scratch);
    if (W->masks)
        add("masks", K->o_mask, 8, 8 * POM_KV_MASK_WORDS * nb, DEV, PLAIN);
    add("records", K->o_pack, 16, K->rcap, DEV, PLAIN);
    if (W->host_masks)
        add("host masks", K->o_hmask, 8, 8 * POM_KV_MASK_WORDS * nb, HOST, PLAIN);
    if (W->host_records)
        add("host records", K->o_hrec, 16, K->rcap, HOST, PLAIN);
    check(&L, K->res_off, K->res_bytes);
}

/* A request operation's chunk: nreq requests of bloblen blob bytes each. */
static void req_case(const char *name, const struct req_spec *Q, const size_t *ids, size_t nb, size_t nlzo,
                     const size_t *src_len, const size_t *cap, size_t nreq, size_t bloblen, int records, size_t scratch)
{
    static const char *kReqWord[RW_N] = {"err", "nr", "depth", "len"};
    struct layout L;
    what = name;
    nR = 0;
    pom_layout_req(&L, ids, nb, nlzo, src_len, cap, Q, nreq, nreq * bloblen, records, scratch);
    const struct req_layout *K = &L.u.req;
    add_shared(&L, UPLOAD);
    add("scan_off", K->scan.o_scanoff, 8, 8 * nb, BOTH, UPLOAD);
    add("requests", K->o_req, 8, POM_REQ_SIZE * nreq, BOTH, UPLOAD);
    add("adepth", K->scan.o_adepth, 1, nb, BOTH, UPLOAD);
    add_bytes(&L, src_len, cap, scratch);
    add("blob", K->o_blob, 1, nreq * bloblen, BOTH, UPLOAD);
    if (K->nreq != nreq || K->blob_bytes != nreq * bloblen)
        fail("request or blob count", NULL, NULL);
    if (K->rcap != (Q->rec_max && records ? POM_ALIGN_UP(Q->rec_max * nreq, 16) : 0))
        fail("record room", NULL, NULL);
    struct region f[2 + RW_N];
    size_t nf = 0, at = 0;
    if (Q->rec_max) {
        /* device first[nreq + 1]: its last entry is the chunk total, the first word that comes back */
        add("first", K->o_first, 8, 8 * nreq, DEV, PLAIN);
        if (K->o_first + 8 * nreq != K->o_res)
            fail("first[nreq] is not the results' first word", NULL, NULL);
        f[nf++] = (struct region){"total", 0, 8, 8, 0, 0};
    }
    for (size_t w = 0; w < Q->nwords; w++)
        f[nf++] = (struct region){kReqWord[w], K->r_word[w], 4, 4 * nreq, 0, 0};
    if (Q->lease)
        f[nf++] = (struct region){"lease", K->r_lease, 8, 8 * nreq, 0, 0};
    if (Q->rec_fixed) {
        check_results(&L, K->o_res, K->o_hres, K->res_hdr, K->res_bytes, f, nf, Q->rec_fixed * nreq);
        return;
    }
    /* variable records: the fields alone are the first copy, the packed records a second, 16-byte aligned */
    for (size_t i = 0; i < nf; i++) {
        if (f[i].off != at)
            fail("result header field out of place", &f[i], NULL);
        at += f[i].bytes;
        add(f[i].name, K->o_res + f[i].off, f[i].elem, f[i].bytes, DEV, PLAIN);
        add(f[i].name, K->o_hres + f[i].off, f[i].elem, f[i].bytes, HOST, PLAIN);
    }
    if (K->res_bytes != at)
        fail("result span is not its fields", NULL, NULL);
    /* (the device's lie behind first[] and the results, 8-byte aligned: the emit kernel takes any alignment) */
    add("records", K->o_pack, 8, K->rcap, DEV, PLAIN);
    add("host records", K->o_hrec, 16, K->rcap, HOST, PLAIN);
    check(&L, 0, 0);
}

/* A group of k single calls: call i has the a + i-th size as input, the c + 2i-th as room. */
static const size_t kScSizes[] = {0, 1, 255, 256, 257, (3u << 20) + 5, 5u << 20};

static void single_case(size_t k, size_t a, size_t c)
{
    const size_t ns = sizeof kScSizes / sizeof kScSizes[0];
    size_t src_len[64], room[64], o_src[64], o_out[64];
    for (size_t i = 0; i < k; i++) {
        src_len[i] = kScSizes[(a + i) % ns];
        room[i] = kScSizes[(c + 2 * i) % ns];
    }
    struct single_layout S;
    what = "single calls";
    nR = 0;
    pom_layout_single(&S, k, src_len, room, o_src, o_out);
    /* the header is ALIGN_UP(44k + 4, 256); inputs, then outputs, one behind the other, each 256-aligned */
    size_t at = POM_ALIGN_UP(44 * k + 4, 256);
    if (S.o_src != at)
        fail("the header is not 44k + 4 bytes, rounded up to 256", NULL, NULL);
    for (size_t i = 0; i < k; i++) {
        if (o_src[i] != at || at % 256)
            fail("an input is out of place", NULL, NULL);
        at += POM_ALIGN_UP(src_len[i], 256);
    }
    if (S.o_dst != at || S.dtotal != at)
        fail("the H2D span or the device side does not end with the inputs", NULL, NULL);
    for (size_t i = 0; i < k; i++) {
        if (o_out[i] != at || at % 256)
            fail("an output is out of place", NULL, NULL);
        at += POM_ALIGN_UP(room[i], 256);
    }
    if (S.htotal != at)
        fail("the host side does not end with the outputs", NULL, NULL);
    /* out_len and status go up with the header (zero and -1) and are read on the
     * host side, where the kernels write them: no D2H but the pre-scan's */
    add("src_off", S.o_srcoff, 8, 8 * k, BOTH, UPLOAD);
    add("dst_off", S.o_dstoff, 8, 8 * k, BOTH, UPLOAD);
    add("src_len", S.o_srclen, 4, 4 * k, BOTH, UPLOAD);
    add("dst_cap", S.o_dstcap, 4, 4 * k, BOTH, UPLOAD);
    add("out_len", S.o_outlen, 4, 4 * k, BOTH, UPLOAD);
    add("status", S.o_status, 4, 4 * k, BOTH, UPLOAD);
    add("plen", S.o_plen, 4, 4 * k, BOTH, RESULT);
    add("pstatus", S.o_pstatus, 4, 4 * k, BOTH, RESULT);
    add("fallback list", S.o_fb, 4, 4 * (1 + k), BOTH, UPLOAD);
    add("inputs", S.o_src, 1, S.o_dst - S.o_src, BOTH, UPLOAD);
    add("outputs", S.o_dst, 1, S.htotal - S.o_dst, HOST, PLAIN);
    const struct layout L = {.o_dst = S.o_dst, .htotal = S.htotal, .dtotal = S.dtotal};
    check(&L, S.pre_off, S.pre_bytes);
}

int main(void)
{
    static const size_t kScK[] = {1, 2, 8, 9, 63, 64};
    for (size_t n = 0; n < sizeof kScK / sizeof kScK[0]; n++)
        for (size_t a = 0; a < sizeof kScSizes / sizeof kScSizes[0]; a++)
            for (size_t c = 0; c < sizeof kScSizes / sizeof kScSizes[0]; c++)
                single_case(kScK[n], a, c);
    static const size_t kNb[] = {1, 2, 5};
    const size_t ns = sizeof kSizes / sizeof kSizes[0];
    size_t ids[5], src_len[8], cap[8];
    for (size_t n = 0; n < 3; n++)
    for (size_t a = 0; a < ns; a++)
    for (size_t c = 0; c < ns; c++)
    for (size_t x = 0; x < 2; x++) {
        const size_t nb = kNb[n], scratch = kScratch[x];
        /* the chunk's blocks are the caller's 7, 6, ...: block i has the a + i-th src_len, the c + 2i-th cap */
        for (size_t i = 0; i < nb; i++) {
            ids[i] = 7 - i;
            src_len[ids[i]] = kSizes[(a + i) % ns];
            cap[ids[i]] = kSizes[(c + 2 * i) % ns];
        }
        struct layout L;
        what = "codec";
        nR = 0;
        pom_layout_codec(&L, ids, nb, src_len, cap, scratch);
        add_shared(&L, RESULT);
        add("packed offset", L.u.codec.o_poff, 8, 8 * nb, BOTH, UPLOAD);
        add_bytes(&L, src_len, cap, scratch);
        const size_t slots = R[nR - 2].bytes;       /* (add_bytes: src bytes, dst slots, scratch) */
        add("host dst", L.o_dst, 16, slots, HOST, PLAIN);
        add("packed", L.u.codec.o_pack, 16, slots, DEV, PLAIN);
        check(&L, L.u.codec.res_off, L.u.codec.res_bytes);

        for (size_t q = 0; q < 3; q++) {
            const size_t nreq = nb * kReqs[q];
            size_t slices = 0;
            for (size_t i = 0; i < nb; i++)
                slices += kReqs[q] * POM_ALIGN_UP(cap[ids[i]], 16);
            what = "column read";
            nR = 0;
            pom_layout_col(&L, ids, nb, src_len, cap, nreq, slices, scratch);
            const struct col_layout *C = &L.u.col;
            add_shared(&L, -1);
            add("want", C->o_want, 8, 8 * nb, BOTH, UPLOAD);
            add("out_off", C->o_outoff, 8, 8 * nreq, BOTH, UPLOAD);
            add("requests", C->o_req, 8, sizeof(struct pom_col_req) * nreq, BOTH, UPLOAD);
            add_bytes(&L, src_len, cap, scratch);
            if (L.o_status != C->o_res + C->r_status || L.o_outlen != C->o_res + C->r_outlen || C->nreq != nreq)
                fail("the decoders' words are not the results' first two", NULL, NULL);
            const struct region cf[] = {{"status", C->r_status, 4, 4 * nb, 0, 0}, {"out_len", C->r_outlen, 4, 4 * nb, 0, 0},
                                        {"slice len", C->r_len, 4, 4 * nreq, 0, 0}, {"slice err", C->r_err, 4, 4 * nreq, 0, 0}};
            check_results(&L, C->o_res, C->o_hres, C->res_hdr, C->res_bytes, cf, 4, slices);
        }

        for (size_t nlzo = 0; nlzo <= nb; nlzo++) {
            const struct walk_spec gc = {kGc, sizeof kGc, 16, 16, 0, 0, 0, 1};
            const struct walk_spec rd = {kRd, sizeof kRd, POM_DENT_HDR + POM_ITE_NAME_MAX, 1, 0, 0, 0, 1};
            walk_case("gc scan", &gc, ids, nb, nlzo, src_len, cap, scratch);
            walk_case("readdir", &rd, ids, nb, nlzo, src_len, cap, scratch);
            for (int mask = 0; mask < 2; mask++)
                for (int count_only = 0; count_only < 2; count_only++) {
                    const struct walk_spec kv = {kKv, sizeof kKv, 4 + POM_KV_VALUE_MAX, 1, 1, 1, mask, !count_only};
                    walk_case("kvlist", &kv, ids, nb, nlzo, src_len, cap, scratch);
                }
            for (size_t q = 0; q < 3; q++)
                for (size_t bloblen = 0; bloblen <= 255; bloblen += 255) {
                    req_case("lookup", &pom_req_lookup, ids, nb, nlzo, src_len, cap, nb * kReqs[q], bloblen, 0, scratch);
                    for (int records = 0; records < 2; records++)
                        req_case("kvget", &pom_req_kvget, ids, nb, nlzo, src_len, cap, nb * kReqs[q], bloblen, records,
                                 scratch);
                }
        }
    }
    printf("layout_check: %lu layouts ok\n", checked);
    return 0;
}
