/* CPU restatement of the encoder's window protocol (lzo1x_encode_fast.hip,
 * parse_wave): every active lane of a 64-lane window probes the pre-window
 * dictionary and posts (tag, lane) for the slot it would write into a
 * 1024-entry min table, once; "the lowest poster of a slot I read is below me"
 * is a fixed per-lane flag; the rounds take the lowest flagged unresolved path
 * lane, search its writer among the path lanes below it, and either drop it (a
 * false alarm) or decide it again from the writer and walk the path again;
 * after FWD forwardings the window ends at the next flagged lane.  A lane that
 * moves from its secondary slot to its primary one writes a slot it did not
 * post: the readers of that slot above it (`extra`) are asserted to carry a
 * flag already, which is why the kernel keeps no such mask.  The matches it
 * produces are asserted equal to the sequential parse (lib/minilzo.c
 * lzo1x_1_compress with a zeroed wrkmem), block by block.
 * Prints windows, path lanes, true conflicts, false alarms and rounds.
 *   gcc -O2 -o /tmp/s scripts/dbg/enc_claims_sim.c
 *   /tmp/s FILE [BLOCKSIZE]    raw concatenated blocks (default 65536 each)
 *   /tmp/s --framed FILE       blocks as [u32 length][bytes] (little endian)
 * Exit status 1 on the first block whose parse differs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
enum { SLOTS = 1u << 14, FAR = 0xBFFF, NEAR = 0x0800, GUARD = 13, WAVE = 64, PATHMAX = 6, FWD = 8,
       CLAIM = 1024 };
typedef struct { uint32_t pos, len, off; } Match;
typedef struct { Match *m; size_t n, cap; } Matches;
static void add(Matches *M, uint32_t pos, uint32_t len, uint32_t off)
{
    if (M->n == M->cap) {
        M->cap = M->cap ? 2 * M->cap : 1024;
        M->m = realloc(M->m, M->cap * sizeof(Match));
        if (!M->m) { perror("realloc"); exit(2); }
    }
    M->m[M->n++] = (Match){pos, len, off};
}
static uint32_t h1_of(const uint8_t *p)
{
    uint32_t v = ((((uint32_t)p[3] << 6) ^ p[2]) << 5) ^ p[1];
    v = (v << 5) ^ p[0];
    return ((v * 33u) >> 5) & (SLOTS - 1);
}
static uint32_t h2_of(uint32_t h) { return (h & 0x7FFu) ^ 0x201Fu; }
static uint32_t claim_index(uint32_t s) { return (s ^ (s >> 9)) & (CLAIM - 1); }
static uint32_t match_len(const uint8_t *in, size_t n, size_t c, size_t p)
{
    uint32_t len = 0;
    while (p + len < n && in[c + len] == in[p + len]) len++;
    return len;
}

/* the sequential parse: dict holds position (0: empty, positions start at 4) */
static void parse_seq(const uint8_t *in, size_t n, Matches *M)
{
    static uint32_t dict[SLOTS];
    memset(dict, 0, sizeof dict);
    if (n <= GUARD) return;
    size_t ip_end = n - GUARD, ip = 4;
    while (ip < ip_end) {
        uint32_t a = h1_of(in + ip), slot = a;
        size_t c = dict[a];
        int ok = 0;
        if (c && ip - c <= FAR) {
            if (ip - c <= NEAR || in[c + 3] == in[ip + 3]) ok = 1;
            else {
                slot = h2_of(a);
                c = dict[slot];
                if (c && ip - c <= FAR && (ip - c <= NEAR || in[c + 3] == in[ip + 3])) ok = 1;
            }
        }
        if (ok && !(in[c] == in[ip] && in[c + 1] == in[ip + 1] && in[c + 2] == in[ip + 2])) ok = 0;
        dict[slot] = (uint32_t)ip;
        if (!ok) { ip++; continue; }
        uint32_t len = match_len(in, n, c, ip);
        add(M, (uint32_t)ip, len, (uint32_t)(ip - c));
        ip += len;
    }
}

static double s_blocks, s_win, s_path, s_true, s_false, s_capped, s_extra;

/* lane state of one window */
static uint32_t H1[WAVE], H2[WAVE], SLOT[WAVE], CAND[WAVE], MLEN[WAVE];
static uint64_t okm, path, mstart;
static uint32_t end_, nmatch, nact;
static uint64_t bit_range(uint32_t off, uint32_t width)      /* width < 64 */
{
    return width ? (((1ull << width) - 1) << off) : 0;
}
static void walk(uint32_t from)
{
    end_ = from;
    uint64_t rem = okm & (~0ull << from);
    uint32_t nm = nmatch;
    for (int it = 0; it < PATHMAX; it++) {
        if (nm >= PATHMAX) break;
        if (!rem) {
            if (end_ < nact) {
                path |= nact - end_ >= 64 ? ~0ull : bit_range(end_, nact - end_);
                end_ = nact;
            }
            break;
        }
        uint32_t q = (uint32_t)__builtin_ctzll(rem);
        path |= bit_range(end_, q - end_) | (1ull << q);
        mstart |= 1ull << q;
        end_ = q + MLEN[q];
        nm++;
        uint32_t e = end_ < 64u ? end_ : 64u;
        rem &= e < 64 ? bit_range(e, 64u - e) : 0;
    }
    nmatch = nm;
}

static void parse_win(const uint8_t *in, size_t n, Matches *M)
{
    static uint32_t dict[SLOTS], claim[CLAIM];
    memset(dict, 0, sizeof dict);
    memset(claim, 0xFF, sizeof claim);
    if (n <= GUARD) return;
    const uint32_t ip_end = (uint32_t)n - GUARD;
    uint32_t ip = 4, wtag = 0xFFFFFEu;
    for (;;) {
        s_win++;
        uint64_t um2 = 0, active = 0;
        okm = 0;
        nact = 0;
        for (uint32_t l = 0; l < WAVE; l++) {
            uint32_t p = ip + l;
            int act = l == 0 || p < ip_end;
            H1[l] = H2[l] = SLOT[l] = CAND[l] = MLEN[l] = 0;
            if (!act) continue;
            active |= 1ull << l;
            nact++;
            uint32_t a = h1_of(in + p), b = h2_of(a);
            uint32_t w1 = dict[a], w2 = dict[b];
            int v1 = w1 != 0 && p - w1 <= FAR;
            int v2 = v1 && w2 != 0 && p - w2 <= FAR;
            int c1pass = v1 && (p - w1 <= NEAR || in[w1 + 3] == in[p + 3]);
            int use2 = v1 && !c1pass;
            int c2pass = use2 && v2 && (p - w2 <= NEAR || in[w2 + 3] == in[p + 3]);
            uint32_t cand = c2pass ? w2 : w1;
            int ok = (c1pass || c2pass) && in[cand] == in[p] && in[cand + 1] == in[p + 1] &&
                     in[cand + 2] == in[p + 2];
            H1[l] = a; H2[l] = b; SLOT[l] = use2 ? b : a; CAND[l] = cand;
            MLEN[l] = ok ? match_len(in, n, cand, p) : 0;
            if (use2) um2 |= 1ull << l;
            if (ok) okm |= 1ull << l;
        }
        /* one post per window from every active lane, then the two reads */
        for (uint32_t l = 0; l < WAVE; l++)
            if ((active >> l) & 1) {
                uint32_t *e = &claim[claim_index(SLOT[l])], mine = (wtag << 8) | l;
                if (mine < *e) *e = mine;
            }
        uint64_t f1 = 0, f2 = 0;
        for (uint32_t l = 0; l < WAVE; l++) {
            uint32_t t1 = claim[claim_index(H1[l])], t2 = claim[claim_index(H2[l])];
            if ((t1 >> 8) == wtag && (t1 & 0xFF) < l) f1 |= 1ull << l;
            if ((t2 >> 8) == wtag && (t2 & 0xFF) < l) f2 |= 1ull << l;
        }
        wtag--;
        path = mstart = 0;
        nmatch = 0;
        walk(0);
        uint64_t resolved = 0, superseded = 0;
        for (uint32_t fwd = 0;;) {
            uint64_t cm = path & ~resolved & (f1 | (um2 & f2));
            if (!cm) break;
            uint32_t c = (uint32_t)__builtin_ctzll(cm);
            if (c == 0) { fprintf(stderr, "lane 0 flagged\n"); exit(1); }
            if (fwd >= FWD) { end_ = c; s_capped++; break; }
            resolved |= 1ull << c;
            uint64_t below_c = (1ull << c) - 1, pm = path & below_c, wm1 = 0, wm2 = 0;
            int u2c = (um2 >> c) & 1;
            for (uint32_t l = 0; l < c; l++)
                if ((pm >> l) & 1) {
                    if (SLOT[l] == H1[c]) wm1 |= 1ull << l;
                    if (u2c && SLOT[l] == H2[c]) wm2 |= 1ull << l;
                }
            if (!wm1 && !wm2) { s_false++; continue; }
            fwd++;
            s_true++;
            int via2 = wm1 == 0;
            uint32_t j = 63u - (uint32_t)__builtin_clzll(via2 ? wm2 : wm1);
            superseded |= 1ull << j;
            uint32_t pc = ip + c, pj = ip + j;
            int ok = in[pj] == in[pc] && in[pj + 1] == in[pc + 1] && in[pj + 2] == in[pc + 2];
            uint64_t bitc = 1ull << c;
            okm = (okm & ~bitc) | (ok ? bitc : 0);
            if (u2c && !via2) {
                uint64_t x = 0;
                for (uint32_t l = c + 1; l < WAVE; l++)
                    if ((active >> l) & 1)
                        if (H1[l] == H1[c] || (((um2 >> l) & 1) && H2[l] == H1[c])) x |= 1ull << l;
                s_extra += __builtin_popcountll(x);
                if (x & ~(f1 | (um2 & f2))) { fprintf(stderr, "an unflagged reader of a moved slot\n"); exit(1); }
            }
            um2 = via2 ? um2 | bitc : um2 & ~bitc;
            MLEN[c] = match_len(in, n, pj, pc);
            CAND[c] = pj;
            SLOT[c] = via2 ? H2[c] : H1[c];
            path &= below_c;
            mstart &= below_c;
            nmatch = (uint32_t)__builtin_popcountll(mstart);
            walk(c);
        }
        const uint64_t keep = end_ >= 64 ? ~0ull : ((1ull << end_) - 1);
        uint64_t km = mstart & keep;
        int done = 0;
        for (uint32_t l = 0; l < WAVE; l++)
            if ((km >> l) & 1) {
                add(M, ip + l, MLEN[l], ip + l - CAND[l]);
                if (ip + l + MLEN[l] >= ip_end) { done = 1; break; }
            }
        s_path += __builtin_popcountll(path & keep);
        for (uint32_t l = 0; l < WAVE; l++)
            if (((path & keep & ~superseded) >> l) & 1) dict[SLOT[l]] = ip + l;
        if (done) break;
        ip += end_;
        if (ip >= ip_end) break;
    }
}

static int check(const uint8_t *in, size_t n, size_t id)
{
    static Matches A, B;
    A.n = B.n = 0;
    parse_seq(in, n, &A);
    parse_win(in, n, &B);
    s_blocks++;
    if (A.n == B.n && (A.n == 0 || memcmp(A.m, B.m, A.n * sizeof(Match)) == 0)) return 0;
    size_t i = 0;
    while (i < A.n && i < B.n && memcmp(&A.m[i], &B.m[i], sizeof(Match)) == 0) i++;
    fprintf(stderr, "block %zu (%zu bytes): parse differs at match %zu of %zu / %zu", id, n, i, A.n, B.n);
    if (i < A.n) fprintf(stderr, "; sequential (%u, %u, %u)", A.m[i].pos, A.m[i].len, A.m[i].off);
    if (i < B.n) fprintf(stderr, "; window (%u, %u, %u)", B.m[i].pos, B.m[i].len, B.m[i].off);
    fprintf(stderr, "\n");
    return 1;
}

int main(int argc, char **argv)
{
    int framed = argc > 2 && strcmp(argv[1], "--framed") == 0;
    if (argc < 2) { fprintf(stderr, "usage: %s FILE [BLOCKSIZE] | --framed FILE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[framed ? 2 : 1], "rb");
    if (!f) { perror("open"); return 2; }
    size_t bs = !framed && argc > 2 ? strtoul(argv[2], 0, 0) : 65536, nb = 0;
    uint8_t *buf = NULL;
    for (;;) {
        uint32_t len = (uint32_t)bs;
        if (framed && fread(&len, 4, 1, f) != 1) break;
        /* (the probes read 4 bytes at positions below n - 13: no padding needed) */
        uint8_t *nbuf = malloc(len ? len : 1);
        if (!nbuf) { perror("malloc"); return 2; }
        free(buf);
        buf = nbuf;
        if (fread(buf, 1, len, f) != len) break;
        if (check(buf, len, nb)) return 1;
        nb++;
    }
    free(buf);
    fclose(f);
    if (!nb) { fprintf(stderr, "no blocks\n"); return 2; }
    printf("%zu blocks identical to the sequential parse; per block: windows %.1f, true conflicts %.1f, "
           "false alarms %.1f, rounds %.1f, capped windows %.2f; per window: path lanes %.1f, true %.2f, "
           "false %.2f, readers of moved slots (all flagged) %.3f\n",
           nb, s_win / s_blocks, s_true / s_blocks, s_false / s_blocks, (s_true + s_false) / s_blocks,
           s_capped / s_blocks, s_path / s_win, s_true / s_win, s_false / s_win, s_extra / s_win);
    return 0;
}
