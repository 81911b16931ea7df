/* host_layout.h -- where everything lies in the staging of one chunk of a host
 * batch (internal to liblzo_mi355x.so; plain C, no HIP, so that
 * tests/native/layout_check.c checks the arithmetic on the CPU).
 *
 * A chunk's staging is one region of pinned host memory and one of device
 * memory, laid out alike from byte 0 to the end of the inputs, so that one
 * H2D copy of [0, o_dst) brings up everything the kernels read.  What lies
 * behind differs per side and per operation.  Block i of the chunk is the
 * caller's block ids[i]; blocks [0, nlzo) are LZO1X streams the decoders run
 * over, the others are stored payloads that ride along and are walked where
 * they are staged (codec and column chunks: nlzo = nb).
 */
#ifndef POM_HOST_LAYOUT_H
#define POM_HOST_LAYOUT_H 1

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POM_ALIGN_UP(x, a) (((x) + (size_t)(a) - 1) & ~((size_t)(a) - 1))

/* Codec chunks: the kernels write each block into its capacity-sized dst slot;
 * only the produced bytes come back, packed (pack kernel), in one D2H copy
 * into the host's dst region. */
struct codec_layout {
    size_t res_off, res_bytes;  /* out_len and status: the D2H behind the kernels */
    size_t o_poff;              /* u64 per block: its place among the packed bytes */
    size_t o_pack;              /* device only: the packed output */
};

/* Operations whose kernel walks payloads where they lie: decoded, or stored
 * uncompressed and staged among the inputs. */
struct scan_layout {
    size_t o_scanoff;           /* u64 per block: the payload's offset in the device staging */
    size_t o_adepth;            /* u8 per block */
};

/* The per-block result words of the walks (u32 or i32 each).  An operation
 * names the ones it has, in staging order (struct walk_spec); they lie one
 * array behind the other and come back in one D2H copy. */
enum walk_word { WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_BYTES, WW_KEYBYTES, WW_ERR, WW_N };

struct walk_spec {
    const uint8_t *words;       /* enum walk_word, in staging order */
    size_t nwords;
    size_t per_ite;             /* bytes of record room per ITE a payload can hold */
    size_t unit;                /* the records' unit: 16 (ranges, WW_COUNT of them) or 1 (bytes, WW_BYTES of them) */
    int needle;                 /* a 256-byte needle is staged with the inputs */
    int masks;                  /* emit masks, 128 bytes per block, on the device ... */
    int host_masks;             /* ... and copied back */
    int host_records;           /* the records are copied back (not count-only) */
};

struct walk_layout {
    struct scan_layout scan;
    size_t o_first;             /* u64, nb + 1 */
    size_t o_word[WW_N];        /* the result words the operation has */
    size_t res_off, res_bytes;  /* their span: the D2H behind the kernels */
    size_t o_needle;
    size_t rcap;                /* record room, in bytes */
    size_t o_mask, o_pack;      /* device only: masks, records */
    size_t o_hmask, o_hrec;     /* host only: masks, records */
};

/* The GC data stat: the GC scan's walk with the merge of its ranges behind it
 * (gc_merge.hip).  The walk's layout comes first, so that what serves the walks
 * serves this chunk too; its records' room is the merge's input, nmerge ranges
 * (zeroed before the scan, so that the places the scan leaves are dropped
 * ranges).  The chunk's struct pom_gc_stat lies behind the result words, 8-byte
 * aligned, inside their D2H span; the merged map comes back in a second copy
 * sized by its nout. */
struct gcstat_layout {
    struct walk_layout walk;    /* o_pack: the ranges; o_hrec: the host's merged map; rcap: 16 * nmerge */
    size_t nmerge;              /* ranges the chunk's ITBs can emit at the most */
    size_t o_stat;              /* struct pom_gc_stat, host and device alike */
    size_t o_mscr, mscr_bytes;  /* device only: the merge's scratch */
    size_t o_merged;            /* device only: the merged map, room for nmerge extents */
};

/* Column reads.  The results -- a header of four arrays, then the slices --
 * lie alike on both sides (device o_res, host o_hres) and come back in one
 * copy; the r_ offsets are relative to the results' start. */
struct col_layout {
    size_t nreq;
    size_t o_want;              /* u64 per block */
    size_t o_outoff;            /* u64 per request: its slice's place among the slices */
    size_t o_req;               /* struct pom_col_req per request */
    size_t o_res, o_hres;
    size_t r_status, r_outlen;  /* i32, u32 per block */
    size_t r_len, r_err;        /* u32, i32 per request */
    size_t res_hdr, res_bytes;  /* the slices start at res_hdr; the whole is res_bytes */
};

/* The request operations: lookups and key/value gets.  A kind is told by where
 * its 32-byte request keeps its ITB number, its offset into the call's blob
 * (names, keys) and the length it reads there, by the rule that refuses a
 * request its blob bytes, and by its results: the first nwords of enum
 * req_word per request, a u64 lease, and records that are either rec_fixed
 * bytes each or packed, of at most rec_max bytes each. */
enum req_word { RW_ERR, RW_NR, RW_DEPTH, RW_LEN, RW_N };
#define POM_REQ_SIZE 32u

struct req_spec {
    size_t o_itb, o_blob;       /* the request's u32 fields: its ITB, its offset into the blob */
    size_t o_len, len_bytes;    /* its blob length: a u16 or u32 field; above len_max the request is refused */
    uint32_t len_max;
    size_t o_flag;              /* a u32 field that must have a bit of flag_mask set, else refused (mask 0: no such rule) */
    uint32_t flag_mask;
    size_t nwords;              /* err, nr, depth (lookup), len (get): i32, then u32 each */
    int lease;                  /* a u64 per request behind the words */
    size_t rec_fixed;           /* fixed records of this many bytes, behind the words in the same D2H span; or 0: */
    size_t rec_max;             /* variable ones, packed on the device behind first[], at most this long */
};

/* The results -- the words, the lease, fixed records 16-byte aligned behind
 * them -- lie alike on both sides (device o_res, host o_hres) and come back in
 * one copy; the r_ offsets are relative to their start.  Variable records: the
 * results start with the chunk's record total (on the device the last entry of
 * first[]), and the packed records follow in a second copy sized by it. */
struct req_layout {
    struct scan_layout scan;
    size_t nreq, blob_bytes;
    size_t o_req;               /* POM_REQ_SIZE per request */
    size_t o_blob;              /* the chunk's own blob, behind the inputs */
    size_t o_first;             /* device only, variable records: u64, nreq + 1; first[nreq] is the results' first word */
    size_t o_res, o_hres;
    size_t r_word[RW_N];        /* i32 or u32 per request */
    size_t r_lease;             /* u64 per request */
    size_t res_hdr, res_bytes;  /* fixed records start at res_hdr; the whole copy is res_bytes */
    size_t rcap;                /* room for the variable records, in bytes (0: none come back) */
    size_t o_pack, o_hrec;      /* device, host: the packed records */
};

/* The ITB check.  The walks' partition and inputs, with 32 bytes of header
 * facts per block among them; the decoders' two words lie among the inputs
 * (a stored block's are staged).  The results -- the three per-block words,
 * then the 48-byte reports, then the masks when the caller asked for them --
 * lie alike on both sides (device o_res, host o_hres) outside the inputs, so
 * that nothing of them is uploaded, and come back in one copy; the r_ offsets
 * are relative to their start.  The kernels' status and out_len are copied
 * into the results on the device. */
struct itb_check_layout {
    struct scan_layout scan;
    size_t o_hdr;               /* struct pom_check_hdr per block */
    size_t o_res, o_hres;
    size_t r_status, r_outlen;  /* i32, u32 per block: adjacent, in this order */
    size_t r_err;               /* i32 per block */
    size_t r_report;            /* 48 bytes per block, 8-byte aligned */
    size_t r_smask, r_imask;    /* 256 and 128 bytes per block, when masks != 0 */
    size_t res_bytes;
    int masks;
};

/* The ITB split: the check's partition and inputs, and what a writer adds.
 * dl(i), block i's decoded length, is its capacity (LZO) or its staged length
 * (stored); a stored block is split where it is staged.  Among the inputs, so
 * that one H2D brings them up: the split depths, each new payload's place and
 * capacity (dl), and for the encoder's 2 * nb blocks -- half 0 the old
 * payloads, half 1 the new ones -- their sources, stream slots and slot sizes;
 * the three pack arrays are filled and uploaded once the results are back.
 * Device only: the new payloads, the split's scratch, the encoder's lengths
 * (gathered from the results on the device) and scratch, the stream slots,
 * the packed output.  The results -- the decoders' two words, the 48-byte
 * results, the encoder's out_len and status -- lie alike on both sides and
 * come back in one copy; what each half is stored as is decided from them, and
 * exactly those bytes follow in a second one. */
struct itb_split_layout {
    struct scan_layout scan;
    size_t o_hdr, o_sd;             /* struct pom_check_hdr, u8 per block */
    size_t o_newoff, o_newcap;      /* u64, u32 per block: from the device staging's start */
    size_t o_esrcoff, o_edstoff;    /* u64, 2 * nb */
    size_t o_edstcap;               /* u32, 2 * nb */
    size_t o_pfrom, o_pto, o_plen;  /* u64, u64, u32, 2 * nb: the pack of what is delivered */
    size_t o_new, o_sscr;           /* device only */
    size_t o_esrclen;               /* device only: u32, 2 * nb */
    size_t o_escr, escr_bytes;
    size_t o_z;                     /* device only: the stream slots */
    size_t o_res, o_hres;
    size_t r_status, r_outlen;      /* i32, u32 per block: adjacent, in this order */
    size_t r_result;                /* 48 bytes per block, 8-byte aligned */
    size_t r_elen, r_est;           /* u32, i32, 2 * nb */
    size_t res_bytes;
    size_t pcap;                    /* room for the delivered halves */
    size_t o_pack, o_hrec;          /* device, host */
};

/* The ITB sweep: the split's staging without a second half.  A payload is
 * swept where it was decoded (or staged) and encoded from there, so the
 * encoder's sources are the scan offsets; among the inputs, beside the
 * check's: the budgets, each stream slot and its size; the three pack arrays
 * are filled and uploaded once the results are back.  Device only: the
 * sweep's scratch, the encoder's lengths (gathered from the results on the
 * device) and scratch, the stream slots, the packed output.  The results --
 * the decoders' two words, the 32-byte results, the encoder's out_len and
 * status -- lie alike on both sides and come back in one copy; what each
 * record is stored as is decided from them, and exactly those bytes follow in
 * a second one. */
struct itb_sweep_layout {
    struct scan_layout scan;
    size_t o_hdr, o_budget;         /* struct pom_check_hdr, u32 per block */
    size_t o_edstoff, o_edstcap;    /* u64, u32 per block */
    size_t o_pfrom, o_pto, o_plen;  /* u64, u64, u32 per block: the pack of what is delivered */
    size_t o_sscr;                  /* device only */
    size_t o_esrclen;               /* device only: u32 per block */
    size_t o_escr, escr_bytes;
    size_t o_z;                     /* device only: the stream slots */
    size_t o_res, o_hres;
    size_t r_status, r_outlen;      /* i32, u32 per block: adjacent, in this order */
    size_t r_result;                /* 32 bytes per block, 8-byte aligned */
    size_t r_elen, r_est;           /* u32, i32 per block */
    size_t res_bytes;
    size_t pcap;                    /* room for the delivered payloads */
    size_t o_pack, o_hrec;          /* device, host */
};

/* The ITB unlink: the request operations' staging -- the requests and the
 * chunk's own blob among the inputs, four words and a 136-byte record a
 * request among the results (struct req_layout comes first, so that
 * pom_req_stage and pom_req_scatter serve this chunk too) -- with the sweep's
 * writer half: among the inputs the header facts, each group's first request
 * (u32, nb + 1), each stream slot and its size, and the three pack arrays,
 * filled and uploaded once the results are back.  Device only: the unlink's
 * scratch, the encoder's lengths and scratch, the stream slots, the packed
 * output.  The results -- the decoders' two words, the 32-byte results, the
 * encoder's out_len and status, then the requests' words and records -- lie
 * alike on both sides and come back in one copy; what each record is stored
 * as is decided from them, and exactly those bytes follow in a second one. */
struct itb_unlink_layout {
    struct req_layout req;          /* (no variable records: its o_first, rcap, o_pack and o_hrec stay 0) */
    size_t o_hdr, o_reqfirst;       /* struct pom_check_hdr per block; u32, nb + 1 */
    size_t o_edstoff, o_edstcap;    /* u64, u32 per block */
    size_t o_pfrom, o_pto, o_plen;  /* u64, u64, u32 per block: the pack of what is delivered */
    size_t o_sscr;                  /* device only */
    size_t o_esrclen;               /* device only: u32 per block */
    size_t o_escr, escr_bytes;
    size_t o_z;                     /* device only: the stream slots */
    size_t r_status, r_outlen;      /* i32, u32 per block: adjacent, in this order */
    size_t r_result;                /* 32 bytes per block, 8-byte aligned */
    size_t r_elen, r_est;           /* u32, i32 per block */
    size_t pcap;                    /* room for the delivered payloads */
    size_t o_pack, o_hrec;          /* device, host */
};

struct layout {
    size_t nb;
    const size_t *ids;
    size_t nlzo;
    int collected;              /* the D2H behind the kernels is queued */
    size_t packed;              /* its bytes */
    size_t o_srcoff, o_dstoff;  /* u64 per block */
    size_t o_srclen, o_dstcap;  /* u32 per block */
    size_t o_outlen, o_status;  /* u32, i32 per block: the decoders' results, on the device */
    size_t o_src;               /* the blocks' input bytes, each 16-byte aligned */
    size_t o_dst;               /* end of the H2D; on the device the output (or decoded payload) slots */
    size_t o_scr;               /* device only: scratch of the kernels */
    size_t htotal, dtotal;
    union {
        struct codec_layout codec;
        struct walk_layout walk;
        struct gcstat_layout gcstat;    /* (starts with the walk's) */
        struct col_layout col;
        struct req_layout req;
        struct itb_check_layout check;
        struct itb_split_layout split;
        struct itb_sweep_layout sweep;
        struct itb_unlink_layout unlink;    /* (starts with the requests') */
    } u;
};

/* src_len[] and cap[] are indexed by the caller's block ids; a block behind
 * nlzo takes no output slot.  scratch: bytes of device scratch the chunk's
 * kernels need (the encoder's or the decoders', for the blocks they run over). */
void pom_layout_codec(struct layout *L, const size_t *ids, size_t nb, const size_t *src_len,
                      const size_t *cap, size_t scratch);
void pom_layout_walk(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                     const size_t *cap, const struct walk_spec *W, size_t scratch);
/* The GC scan's walk layout (W: its spec) with the merge behind it: nmerge
 * ranges at the most, merge_scratch bytes of scratch for them. */
void pom_layout_gcstat(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                       const size_t *cap, const struct walk_spec *W, size_t scratch, size_t nmerge,
                       size_t merge_scratch);
/* slice_bytes: the requests' clamped lengths, each rounded up to 16 */
void pom_layout_col(struct layout *L, const size_t *ids, size_t nb, const size_t *src_len,
                    const size_t *cap, size_t nreq, size_t slice_bytes, size_t scratch);
/* records != 0: room for every request's longest variable record on both sides */
void pom_layout_req(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                    const size_t *cap, const struct req_spec *Q, size_t nreq, size_t blob_bytes, int records,
                    size_t scratch);

/* masks != 0: the results have room for the slot and ITE masks */
void pom_layout_check(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                      const size_t *cap, int masks, size_t scratch);

/* split_scratch, enc_scratch: what the split of nb blocks and the encoder of
 * 2 * nb blocks need. */
void pom_layout_split(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                      const size_t *cap, size_t scratch, size_t split_scratch, size_t enc_scratch);
/* The room an LZO1X-1 stream of n bytes can take, rounded up to 16. */
size_t pom_split_stream_room(size_t n);

/* sweep_scratch, enc_scratch: what the sweep and the encoder of nb blocks need. */
void pom_layout_sweep(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                      const size_t *cap, size_t scratch, size_t sweep_scratch, size_t enc_scratch);

/* Q: the unlink's kind (fixed records, no lease); unlink_scratch, enc_scratch:
 * what the unlink and the encoder of nb blocks need. */
void pom_layout_unlink(struct layout *L, const size_t *ids, size_t nb, size_t nlzo, const size_t *src_len,
                       const size_t *cap, const struct req_spec *Q, size_t nreq, size_t blob_bytes, size_t scratch,
                       size_t unlink_scratch, size_t enc_scratch);

/* The staging of a group of k single calls (host_single.c).  The header
 * arrays, then the inputs, lie alike on both sides and go up in one H2D copy
 * of [0, o_dst); the outputs lie behind, in the pinned host staging only: the
 * kernels write them, out_len and status there directly, so nothing but the
 * rare pre-scan's words is ever copied back. */
struct single_layout {
    size_t o_srcoff, o_dstoff;  /* u64 per call */
    size_t o_srclen, o_dstcap;  /* u32 per call */
    size_t o_outlen, o_status;  /* u32, i32 per call: read on the host side */
    size_t o_plen, o_pstatus;   /* u32, i32 per call: the pre-scan's decoded length and status */
    size_t pre_off, pre_bytes;  /* their span: the D2H behind the pre-scan */
    size_t o_fb;                /* u32, 1 + k: the decoders' fallback list, count then ids */
    size_t o_src;               /* the header's end: the first input */
    size_t o_dst;               /* end of the H2D; host only: the first output */
    size_t htotal, dtotal;
};

/* Call i has src_len[i] bytes of input at o_src[i] and room[i] bytes of output
 * at o_out[i], each 256-byte aligned. */
void pom_layout_single(struct single_layout *L, size_t k, const size_t *src_len, const size_t *room,
                       size_t *o_src, size_t *o_out);

/* The ITEs a payload of n bytes can hold: what a walk can emit at the most. */
size_t pom_walk_max_ites(size_t n);
/* The ranges the GC scan can emit for an ITB of that payload size and adepth:
 * one per ITE it holds and per bitmap bit below 1 << adepth (none for an
 * adepth outside 1 ... 10). */
size_t pom_gc_max_ranges(size_t n, unsigned adepth);

#ifdef __cplusplus
}
#endif

#endif
