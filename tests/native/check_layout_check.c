/* check_layout_check.c -- the ITB check's staging layout
 * (pomegranate_amd/csrc/host_layout.c pom_layout_check) checked on the CPU,
 * under AddressSanitizer and UBSan, by layout_check.c's rules: for every
 * combination of block count, LZO prefix, sizes and masks below,
 *   - every array starts at a multiple of its element size;
 *   - the input bytes start at a multiple of 256, each block's at a multiple of 16;
 *   - the regions of the host staging are pairwise disjoint and end within
 *     htotal, those of the device staging within dtotal;
 *   - the H2D span [0, o_dst) holds exactly the uploaded fields (but for
 *     alignment padding), and no result lies inside it;
 *   - the results are one span of res_bytes, alike on both sides, that is
 *     exactly the union of the result fields (but for alignment padding),
 *     with status and out_len adjacent in it as they are among the inputs;
 *   - without masks the results have no room for them.
 * Prints the number of layouts checked; exits non-zero at the first failure. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host_layout.h"

enum { HOST = 1, DEV = 2, BOTH = 3 };

struct region {
    const char *name;
    size_t hoff, doff, elem, bytes;
    int side, upload;
};

static struct region R[24];
static size_t nR;
static char what[128];

static void fail(const char *msg, const char *a, const char *b)
{
    fprintf(stderr, "check_layout_check: %s: %s: %s%s%s\n", what, msg, a ? a : "", b ? " / " : "", b ? b : "");
    exit(1);
}

static void add(const char *name, size_t hoff, size_t doff, size_t elem, size_t bytes, int side, int upload)
{
    if (nR == sizeof R / sizeof R[0])
        fail("too many regions", NULL, NULL);
    R[nR++] = (struct region){name, hoff, doff, elem, bytes, side, upload};
}

static void check_side(const struct layout *L, int side)
{
    const size_t total = side == HOST ? L->htotal : L->dtotal;
    for (size_t i = 0; i < nR; i++) {
        if (!(R[i].side & side) || !R[i].bytes)
            continue;
        const size_t a = side == HOST ? R[i].hoff : R[i].doff;
        if (a % R[i].elem)
            fail("misaligned", R[i].name, NULL);
        if (a + R[i].bytes > total)
            fail("past the staging's end", R[i].name, NULL);
        if (R[i].upload ? a + R[i].bytes > L->o_dst : a < L->o_dst)
            fail("on the wrong side of the H2D span's end", R[i].name, NULL);
        for (size_t j = i + 1; j < nR; j++) {
            if (!(R[j].side & side) || !R[j].bytes)
                continue;
            const size_t b = side == HOST ? R[j].hoff : R[j].doff;
            if (a < b + R[j].bytes && b < a + R[i].bytes)
                fail("overlap", R[i].name, R[j].name);
        }
    }
}

static unsigned long one(size_t nb, size_t nlzo, const size_t *src_len, const size_t *cap, int masks, size_t scratch)
{
    size_t ids[64];
    struct layout L;
    for (size_t i = 0; i < nb; i++)
        ids[i] = nb - 1 - i;                    /* the chunk's order is not the caller's */
    snprintf(what, sizeof what, "nb=%zu nlzo=%zu masks=%d scratch=%zu", nb, nlzo, masks, scratch);
    pom_layout_check(&L, ids, nb, nlzo, src_len, cap, masks, scratch);
    const struct itb_check_layout *K = &L.u.check;
    if (L.nb != nb || L.nlzo != nlzo || L.ids != ids || K->masks != (masks != 0))
        fail("the layout's own fields", NULL, NULL);
    size_t s = 0, d = 0, up = 0;
    for (size_t i = 0; i < nb; i++) {
        if ((L.o_src + s) % 16 || (L.o_dst + d) % 16)
            fail("a block's bytes are not 16-byte aligned", NULL, NULL);
        s += POM_ALIGN_UP(src_len[ids[i]], 16);
        if (i < nlzo)
            d += POM_ALIGN_UP(cap[ids[i]], 16);
    }
    if (L.o_src % 256 || L.o_dst % 256 || K->o_res % 256 || K->o_hres % 256)
        fail("o_src, o_dst, o_res or o_hres is not a multiple of 256", NULL, NULL);
    nR = 0;
    add("src_off", L.o_srcoff, L.o_srcoff, 8, 8 * nb, BOTH, 1);
    add("dst_off", L.o_dstoff, L.o_dstoff, 8, 8 * nb, BOTH, 1);
    add("scan_off", K->scan.o_scanoff, K->scan.o_scanoff, 8, 8 * nb, BOTH, 1);
    add("header facts", K->o_hdr, K->o_hdr, 8, 32 * nb, BOTH, 1);
    add("src_len", L.o_srclen, L.o_srclen, 4, 4 * nb, BOTH, 1);
    add("dst_cap", L.o_dstcap, L.o_dstcap, 4, 4 * nb, BOTH, 1);
    add("status", L.o_status, L.o_status, 4, 4 * nb, BOTH, 1);
    add("out_len", L.o_outlen, L.o_outlen, 4, 4 * nb, BOTH, 1);
    add("adepth", K->scan.o_adepth, K->scan.o_adepth, 1, nb, BOTH, 1);
    add("src bytes", L.o_src, L.o_src, 1, s, BOTH, 1);
    for (size_t i = 0; i < nR; i++)
        up += R[i].bytes;
    add("dst slots", 0, L.o_dst, 1, d, DEV, 0);
    add("scratch", 0, L.o_scr, 256, scratch, DEV, 0);
    const size_t first_result = nR;
    add("r status", K->o_hres + K->r_status, K->o_res + K->r_status, 4, 4 * nb, BOTH, 0);
    add("r out_len", K->o_hres + K->r_outlen, K->o_res + K->r_outlen, 4, 4 * nb, BOTH, 0);
    add("r err", K->o_hres + K->r_err, K->o_res + K->r_err, 4, 4 * nb, BOTH, 0);
    add("reports", K->o_hres + K->r_report, K->o_res + K->r_report, 8, 48 * nb, BOTH, 0);
    add("slot masks", K->o_hres + K->r_smask, K->o_res + K->r_smask, 8, masks ? 256 * nb : 0, BOTH, 0);
    add("ITE masks", K->o_hres + K->r_imask, K->o_res + K->r_imask, 8, masks ? 128 * nb : 0, BOTH, 0);
    check_side(&L, HOST);
    check_side(&L, DEV);
    /* the H2D span: the uploaded fields and padding (below 256 per alignment step, 16 per block) */
    if (L.o_dst < up || L.o_dst - up > 2 * 256 + 16 * nb)
        fail("the H2D span is not the uploaded fields", NULL, NULL);
    /* the results: one span, nothing else in it */
    size_t res = 0;
    for (size_t i = first_result; i < nR; i++) {
        res += R[i].bytes;
        if (R[i].bytes && (R[i].hoff < K->o_hres || R[i].hoff + R[i].bytes > K->o_hres + K->res_bytes))
            fail("outside the result span", R[i].name, NULL);
    }
    if (K->res_bytes < res || K->res_bytes - res > 8)
        fail("the result span is not the union of the results", NULL, NULL);
    if (K->r_outlen != K->r_status + 4 * nb || L.o_outlen != L.o_status + 4 * nb)
        fail("status and out_len are not adjacent, in this order", NULL, NULL);
    if (!masks && K->res_bytes > 12 * nb + 8 + 48 * nb)
        fail("room for masks nobody asked for", NULL, NULL);
    if (L.htotal != K->o_hres + K->res_bytes)
        fail("htotal", NULL, NULL);
    return 1;
}

int main(void)
{
    static const size_t sizes[] = {1, 15, 16, 17, 255, 256, 4097, 12416, 65536, 536192};
    size_t src_len[64], cap[64];
    unsigned long checked = 0;
    unsigned seed = 12345;
    for (size_t nb = 1; nb <= 64; nb = nb < 9 ? nb + 1 : nb * 2 - 1)
        for (size_t nlzo = 0; nlzo <= nb; nlzo += nb < 9 ? 1 : nb / 3 + 1)
            for (int masks = 0; masks < 2; masks++)
                for (int round = 0; round < 6; round++) {
                    for (size_t i = 0; i < nb; i++) {
                        seed = seed * 1103515245u + 12345u;
                        src_len[i] = sizes[(seed >> 16) % 10];
                        seed = seed * 1103515245u + 12345u;
                        cap[i] = sizes[(seed >> 16) % 10];
                    }
                    checked += one(nb, nlzo, src_len, cap, masks, round % 3 ? 4096 * nb + 64 : 0);
                }
    printf("check_layout_check: ok (%lu layouts)\n", checked);
    return 0;
}
