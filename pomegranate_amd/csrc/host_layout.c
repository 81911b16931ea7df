/* host_layout.c -- the staging layouts of host_layout.h: plain arithmetic, no
 * HIP.  Each builder lays the arrays out in the order its operation's staging
 * diagram gives (lzo_host.c for the codec, host_single.c for the single calls,
 * host_records.c for the others). */
#include <string.h>

#include "host_layout.h"
#include "pom_column.h"
#include "pom_kvlist.h"

size_t pom_walk_max_ites(size_t n)
{
    const size_t ites = n > POM_ITB_ITE_OFF ? (n - POM_ITB_ITE_OFF) / POM_ITE_SIZE : 0;
    return ites < 1024 ? ites : 1024;
}

size_t pom_gc_max_ranges(size_t n, unsigned adepth)
{
    const size_t ites = pom_walk_max_ites(n);
    if (adepth < 1 || adepth > 10)
        return 0;
    return ites < ((size_t)1 << adepth) ? ites : (size_t)1 << adepth;
}

/* The next `bytes` of the staging: their offset. */
static size_t take(size_t *o, size_t bytes)
{
    const size_t at = *o;
    *o += bytes;
    return at;
}

/* What every layout starts from; the inputs' and the output slots' sizes. */
static void layout_start(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                         const size_t *cap, size_t *in_bytes, size_t *out_bytes)
{
    memset(L, 0, sizeof(*L));
    L->nb = nb;
    L->ids = ids;
    L->nlzo = nlzo;
    size_t s = 0, d = 0;
    for (size_t i = 0; i < nb; i++) {
        s += POM_ALIGN_UP(src_len[ids[i]], 16);
        if (i < nlzo)
            d += POM_ALIGN_UP(cap[ids[i]], 16);
    }
    *in_bytes = POM_ALIGN_UP(s, 256);
    *out_bytes = POM_ALIGN_UP(d, 256);
}

void pom_layout_codec(struct layout *L, const size_t *ids, size_t nb, const size_t *src_len,
                      const size_t *cap, size_t scratch)
{
    size_t in, out, o = 0;
    layout_start(L, ids, nb, nb, src_len, cap, &in, &out);
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    L->u.codec.res_off = o;
    L->o_outlen = take(&o, 4 * nb);
    L->o_status = take(&o, 4 * nb);
    L->u.codec.res_bytes = o - L->u.codec.res_off;
    L->u.codec.o_poff = take(&o, 8 * nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    L->o_dst = take(&o, out);
    L->htotal = o;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    L->u.codec.o_pack = take(&o, out);
    L->dtotal = o;
}

void pom_layout_single(struct single_layout *L, size_t k, const size_t *src_len, const size_t *room,
                       size_t *o_src, size_t *o_out)
{
    size_t o = 0;
    L->o_srcoff = take(&o, 8 * k);
    L->o_dstoff = take(&o, 8 * k);
    L->o_srclen = take(&o, 4 * k);
    L->o_dstcap = take(&o, 4 * k);
    L->o_outlen = take(&o, 4 * k);
    L->o_status = take(&o, 4 * k);
    L->pre_off = o;
    L->o_plen = take(&o, 4 * k);
    L->o_pstatus = take(&o, 4 * k);
    L->pre_bytes = o - L->pre_off;
    L->o_fb = take(&o, 4 * (1 + k));
    o = POM_ALIGN_UP(o, 256);
    L->o_src = o;
    for (size_t i = 0; i < k; i++)
        o_src[i] = take(&o, POM_ALIGN_UP(src_len[i], 256));
    L->o_dst = o;
    L->dtotal = o;
    for (size_t i = 0; i < k; i++)
        o_out[i] = take(&o, POM_ALIGN_UP(room[i], 256));
    L->htotal = o;
}

void pom_layout_walk(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                     const size_t *cap, const struct walk_spec *W, size_t scratch)
{
    size_t in, out, o = 0, r = 0;
    layout_start(L, ids, nb, nlzo, src_len, cap, &in, &out);
    struct walk_layout *K = &L->u.walk;
    for (size_t i = 0; i < nb; i++)
        r += pom_walk_max_ites(i < nlzo ? cap[ids[i]] : src_len[ids[i]]) * W->per_ite;
    const size_t masks = W->masks ? POM_ALIGN_UP(8 * POM_KV_MASK_WORDS * nb, 256) : 0;
    K->rcap = r;
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    K->scan.o_scanoff = take(&o, 8 * nb);
    K->o_first = take(&o, 8 * (nb + 1));
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    K->res_off = o;
    for (size_t w = 0; w < W->nwords; w++)
        K->o_word[W->words[w]] = take(&o, 4 * nb);
    K->res_bytes = o - K->res_off;
    L->o_status = K->o_word[WW_STATUS];
    L->o_outlen = K->o_word[WW_OUTLEN];
    K->scan.o_adepth = take(&o, nb);
    o = POM_ALIGN_UP(o, 256);
    K->o_needle = take(&o, W->needle ? 256 : 0);
    L->o_src = take(&o, in);
    L->o_dst = o;
    K->o_hmask = o;
    K->o_hrec = o + (W->host_masks ? masks : 0);
    L->htotal = K->o_hrec + (W->host_records ? r : 0);
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    K->o_mask = take(&o, masks);
    K->o_pack = take(&o, r);
    L->dtotal = o;
}

void pom_layout_gcstat(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                       const size_t *cap, const struct walk_spec *W, size_t scratch, size_t nmerge,
                       size_t merge_scratch)
{
    size_t in, out, o = 0;
    layout_start(L, ids, nb, nlzo, src_len, cap, &in, &out);
    struct gcstat_layout *G = &L->u.gcstat;
    struct walk_layout *K = &G->walk;
    const size_t r = nmerge * 16;
    G->nmerge = nmerge;
    K->rcap = r;
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    K->scan.o_scanoff = take(&o, 8 * nb);
    K->o_first = take(&o, 8 * (nb + 1));
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    K->res_off = o;
    for (size_t w = 0; w < W->nwords; w++)
        K->o_word[W->words[w]] = take(&o, 4 * nb);
    o = POM_ALIGN_UP(o, 8);
    G->o_stat = take(&o, 5 * 8);
    K->res_bytes = o - K->res_off;
    L->o_status = K->o_word[WW_STATUS];
    L->o_outlen = K->o_word[WW_OUTLEN];
    K->scan.o_adepth = take(&o, nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    L->o_dst = o;
    K->o_hmask = o;
    K->o_hrec = o;
    L->htotal = o + r;
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    K->o_mask = o;
    K->o_pack = take(&o, POM_ALIGN_UP(r, 256));
    G->mscr_bytes = merge_scratch;
    G->o_mscr = take(&o, POM_ALIGN_UP(merge_scratch, 256));
    G->o_merged = take(&o, r);
    L->dtotal = o;
}

void pom_layout_col(struct layout *L, const size_t *ids, size_t nb, const size_t *src_len,
                    const size_t *cap, size_t nreq, size_t slice_bytes, size_t scratch)
{
    size_t in, out, o = 0, r = 0;
    layout_start(L, ids, nb, nb, src_len, cap, &in, &out);
    struct col_layout *C = &L->u.col;
    C->nreq = nreq;
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    C->o_want = take(&o, 8 * nb);
    C->o_outoff = take(&o, 8 * nreq);
    C->o_req = take(&o, sizeof(struct pom_col_req) * nreq);
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    L->o_dst = o;
    C->r_status = take(&r, 4 * nb);
    C->r_outlen = take(&r, 4 * nb);
    C->r_len = take(&r, 4 * nreq);
    C->r_err = take(&r, 4 * nreq);
    C->res_hdr = POM_ALIGN_UP(r, 16);
    C->res_bytes = C->res_hdr + slice_bytes;
    C->o_hres = o;
    L->htotal = o + C->res_bytes;
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    C->o_res = take(&o, C->res_bytes);
    L->o_status = C->o_res + C->r_status;
    L->o_outlen = C->o_res + C->r_outlen;
    L->dtotal = o;
}

void pom_layout_req(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                    const size_t *cap, const struct req_spec *Q, size_t nreq, size_t blob_bytes, int records,
                    size_t scratch)
{
    size_t in, out, o = 0, r = Q->rec_max ? 8 : 0;
    layout_start(L, ids, nb, nlzo, src_len, cap, &in, &out);
    struct req_layout *K = &L->u.req;
    K->nreq = nreq;
    K->blob_bytes = blob_bytes;
    K->rcap = records ? POM_ALIGN_UP(Q->rec_max * nreq, 16) : 0;
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    K->scan.o_scanoff = take(&o, 8 * nb);
    K->o_req = take(&o, POM_REQ_SIZE * nreq);
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    L->o_status = take(&o, 4 * nb);
    L->o_outlen = take(&o, 4 * nb);
    K->scan.o_adepth = take(&o, nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    K->o_blob = take(&o, POM_ALIGN_UP(blob_bytes, 256));
    L->o_dst = o;
    for (size_t w = 0; w < Q->nwords; w++)
        K->r_word[w] = take(&r, 4 * nreq);
    r = POM_ALIGN_UP(r, 8);
    K->r_lease = take(&r, Q->lease ? 8 * nreq : 0);
    K->res_hdr = POM_ALIGN_UP(r, 16);
    K->res_bytes = Q->rec_fixed ? K->res_hdr + Q->rec_fixed * nreq : r;
    K->o_hres = o;
    K->o_hrec = POM_ALIGN_UP(o + K->res_bytes, 16);
    L->htotal = K->o_hrec + K->rcap;
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    K->o_first = take(&o, Q->rec_max ? 8 * nreq : 0);
    K->o_res = take(&o, POM_ALIGN_UP(K->res_bytes, 256));
    K->o_pack = take(&o, K->rcap);
    L->dtotal = o;
}

void pom_layout_check(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                      const size_t *cap, int masks, size_t scratch)
{
    size_t in, out, o = 0, r = 0;
    layout_start(L, ids, nb, nlzo, src_len, cap, &in, &out);
    struct itb_check_layout *K = &L->u.check;
    K->masks = masks != 0;
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    K->scan.o_scanoff = take(&o, 8 * nb);
    K->o_hdr = take(&o, 32 * nb);
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    L->o_status = take(&o, 4 * nb);
    L->o_outlen = take(&o, 4 * nb);
    K->scan.o_adepth = take(&o, nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    L->o_dst = o;
    K->r_status = take(&r, 4 * nb);
    K->r_outlen = take(&r, 4 * nb);
    K->r_err = take(&r, 4 * nb);
    r = POM_ALIGN_UP(r, 8);
    K->r_report = take(&r, 48 * nb);
    K->r_smask = take(&r, K->masks ? 256 * nb : 0);
    K->r_imask = take(&r, K->masks ? 128 * nb : 0);
    K->res_bytes = r;
    K->o_hres = o;
    L->htotal = o + K->res_bytes;
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    K->o_res = take(&o, POM_ALIGN_UP(K->res_bytes, 256));
    L->dtotal = o;
}

size_t pom_split_stream_room(size_t n)
{
    return POM_ALIGN_UP(n + n / 16 + 64 + 3, 16);
}

void pom_layout_split(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                      const size_t *cap, size_t scratch, size_t split_scratch, size_t enc_scratch)
{
    size_t in, out, o = 0, r = 0, news = 0, streams = 0;
    layout_start(L, ids, nb, nlzo, src_len, cap, &in, &out);
    struct itb_split_layout *K = &L->u.split;
    for (size_t i = 0; i < nb; i++) {
        const size_t dl = i < nlzo ? cap[ids[i]] : src_len[ids[i]];
        news += POM_ALIGN_UP(dl, 16);
        streams += 2 * pom_split_stream_room(dl);
    }
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    K->scan.o_scanoff = take(&o, 8 * nb);
    K->o_newoff = take(&o, 8 * nb);
    K->o_esrcoff = take(&o, 16 * nb);
    K->o_edstoff = take(&o, 16 * nb);
    K->o_pfrom = take(&o, 16 * nb);
    K->o_pto = take(&o, 16 * nb);
    K->o_hdr = take(&o, 32 * nb);
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    L->o_status = take(&o, 4 * nb);
    L->o_outlen = take(&o, 4 * nb);
    K->o_newcap = take(&o, 4 * nb);
    K->o_edstcap = take(&o, 8 * nb);
    K->o_plen = take(&o, 8 * nb);
    K->scan.o_adepth = take(&o, nb);
    K->o_sd = take(&o, nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    L->o_dst = o;
    K->r_status = take(&r, 4 * nb);
    K->r_outlen = take(&r, 4 * nb);
    r = POM_ALIGN_UP(r, 8);
    K->r_result = take(&r, 48 * nb);
    K->r_elen = take(&r, 8 * nb);
    K->r_est = take(&r, 8 * nb);
    K->res_bytes = r;
    K->pcap = 2 * news;
    K->o_hres = o;
    K->o_hrec = POM_ALIGN_UP(o + r, 256);
    L->htotal = K->o_hrec + K->pcap;
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    K->o_new = take(&o, POM_ALIGN_UP(news, 256));
    K->o_sscr = take(&o, POM_ALIGN_UP(split_scratch, 256));
    K->o_esrclen = take(&o, POM_ALIGN_UP(8 * nb, 256));
    K->escr_bytes = enc_scratch;
    K->o_escr = take(&o, POM_ALIGN_UP(enc_scratch, 256));
    K->o_z = take(&o, POM_ALIGN_UP(streams, 256));
    K->o_res = take(&o, POM_ALIGN_UP(r, 256));
    K->o_pack = take(&o, POM_ALIGN_UP(K->pcap, 256));
    L->dtotal = o;
}

void pom_layout_sweep(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                      const size_t *cap, size_t scratch, size_t sweep_scratch, size_t enc_scratch)
{
    size_t in, out, o = 0, r = 0, payloads = 0, streams = 0;
    layout_start(L, ids, nb, nlzo, src_len, cap, &in, &out);
    struct itb_sweep_layout *K = &L->u.sweep;
    for (size_t i = 0; i < nb; i++) {
        const size_t dl = i < nlzo ? cap[ids[i]] : src_len[ids[i]];
        payloads += POM_ALIGN_UP(dl, 16);
        streams += pom_split_stream_room(dl);
    }
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    K->scan.o_scanoff = take(&o, 8 * nb);
    K->o_edstoff = take(&o, 8 * nb);
    K->o_pfrom = take(&o, 8 * nb);
    K->o_pto = take(&o, 8 * nb);
    K->o_hdr = take(&o, 32 * nb);
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    L->o_status = take(&o, 4 * nb);
    L->o_outlen = take(&o, 4 * nb);
    K->o_budget = take(&o, 4 * nb);
    K->o_edstcap = take(&o, 4 * nb);
    K->o_plen = take(&o, 4 * nb);
    K->scan.o_adepth = take(&o, nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    L->o_dst = o;
    K->r_status = take(&r, 4 * nb);
    K->r_outlen = take(&r, 4 * nb);
    r = POM_ALIGN_UP(r, 8);
    K->r_result = take(&r, 32 * nb);
    K->r_elen = take(&r, 4 * nb);
    K->r_est = take(&r, 4 * nb);
    K->res_bytes = r;
    K->pcap = payloads;
    K->o_hres = o;
    K->o_hrec = POM_ALIGN_UP(o + r, 256);
    L->htotal = K->o_hrec + K->pcap;
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    K->o_sscr = take(&o, POM_ALIGN_UP(sweep_scratch, 256));
    K->o_esrclen = take(&o, POM_ALIGN_UP(4 * nb, 256));
    K->escr_bytes = enc_scratch;
    K->o_escr = take(&o, POM_ALIGN_UP(enc_scratch, 256));
    K->o_z = take(&o, POM_ALIGN_UP(streams, 256));
    K->o_res = take(&o, POM_ALIGN_UP(r, 256));
    K->o_pack = take(&o, POM_ALIGN_UP(K->pcap, 256));
    L->dtotal = o;
}

void pom_layout_unlink(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                       const size_t *cap, const struct req_spec *Q, size_t nreq, size_t blob_bytes, size_t scratch,
                       size_t unlink_scratch, size_t enc_scratch)
{
    size_t in, out, o = 0, r = 0, payloads = 0, streams = 0;
    layout_start(L, ids, nb, nlzo, src_len, cap, &in, &out);
    struct itb_unlink_layout *K = &L->u.unlink;
    struct req_layout *Y = &K->req;
    for (size_t i = 0; i < nb; i++) {
        const size_t dl = i < nlzo ? cap[ids[i]] : src_len[ids[i]];
        payloads += POM_ALIGN_UP(dl, 16);
        streams += pom_split_stream_room(dl);
    }
    Y->nreq = nreq;
    Y->blob_bytes = blob_bytes;
    L->o_srcoff = take(&o, 8 * nb);
    L->o_dstoff = take(&o, 8 * nb);
    Y->scan.o_scanoff = take(&o, 8 * nb);
    K->o_edstoff = take(&o, 8 * nb);
    K->o_pfrom = take(&o, 8 * nb);
    K->o_pto = take(&o, 8 * nb);
    K->o_hdr = take(&o, 32 * nb);
    Y->o_req = take(&o, POM_REQ_SIZE * nreq);
    L->o_srclen = take(&o, 4 * nb);
    L->o_dstcap = take(&o, 4 * nb);
    L->o_status = take(&o, 4 * nb);
    L->o_outlen = take(&o, 4 * nb);
    K->o_reqfirst = take(&o, 4 * (nb + 1));
    K->o_edstcap = take(&o, 4 * nb);
    K->o_plen = take(&o, 4 * nb);
    Y->scan.o_adepth = take(&o, nb);
    o = POM_ALIGN_UP(o, 256);
    L->o_src = take(&o, in);
    Y->o_blob = take(&o, POM_ALIGN_UP(blob_bytes, 256));
    L->o_dst = o;
    K->r_status = take(&r, 4 * nb);
    K->r_outlen = take(&r, 4 * nb);
    r = POM_ALIGN_UP(r, 8);
    K->r_result = take(&r, 32 * nb);
    K->r_elen = take(&r, 4 * nb);
    K->r_est = take(&r, 4 * nb);
    for (size_t w = 0; w < Q->nwords; w++)
        Y->r_word[w] = take(&r, 4 * nreq);
    Y->r_lease = r;
    Y->res_hdr = POM_ALIGN_UP(r, 16);
    Y->res_bytes = Y->res_hdr + Q->rec_fixed * nreq;
    K->pcap = payloads;
    Y->o_hres = o;
    K->o_hrec = POM_ALIGN_UP(o + Y->res_bytes, 256);
    L->htotal = K->o_hrec + K->pcap;
    o += out;
    L->o_scr = take(&o, POM_ALIGN_UP(scratch, 256));
    K->o_sscr = take(&o, POM_ALIGN_UP(unlink_scratch, 256));
    K->o_esrclen = take(&o, POM_ALIGN_UP(4 * nb, 256));
    K->escr_bytes = enc_scratch;
    K->o_escr = take(&o, POM_ALIGN_UP(enc_scratch, 256));
    K->o_z = take(&o, POM_ALIGN_UP(streams, 256));
    Y->o_res = take(&o, POM_ALIGN_UP(Y->res_bytes, 256));
    K->o_pack = take(&o, POM_ALIGN_UP(K->pcap, 256));
    L->dtotal = o;
}
