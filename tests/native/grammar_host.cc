// grammar_host.cc -- pomegranate_amd/csrc/lzo1x_grammar.h on the CPU (never
// part of the product library).  No statement of the grammar lives here:
// both builds only call the header.
//   libgrammar_host.so  grammar_decode(): a sequential decoder that steps
//                       through a stream with the shared functions
//                       (tests/test_grammar.py)
//   grammar_check       (-DGRAMMAR_CHECK) the branch-free form against the
//                       general form over instruction words, states and ends
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "lzo1x_grammar.h"

namespace {

// modes: the zero-run policy, | GM_GENERAL: the general form only (else the
// branch-free form, and the general form where it asks for it)
enum { GM_FAST = 0, GM_WIN_SPEC = 1, GM_WIN_TRUE = 2, GM_LAT = 3, GM_GENERAL = 4 };
enum { GR_DONE = 0, GR_REFUSED = 1, GR_CAPACITY = 2, GR_LOOKBEHIND = 3 };

// the windowed decoder's true path: aligned 16-byte zero scan (no piece is
// staged here, so from the first byte on)
struct HostWinRun {
    const uint8_t* in;
    uint32_t limit;
    uint32_t bulk(uint32_t p, uint32_t z) const
    {
        static const uint8_t zero[16] = {0};
        return p + 16 <= z && ((uintptr_t)(in + p) & 15u) == 0 && memcmp(in + p, zero, 16) == 0 ? 16u : 0u;
    }
};

Lzo1xIns step(const uint8_t* in, uint32_t z, uint32_t pos, uint32_t st, int mode)
{
    auto rd = [&](uint32_t p) -> uint32_t { return p < z ? in[p] : 0u; };
    if (!(mode & GM_GENERAL)) {
        const uint32_t lo = rd(pos) | rd(pos + 1) << 8 | rd(pos + 2) << 16 | rd(pos + 3) << 24;
        bool general;
        const Lzo1xIns r = lzo1x_decode_word<false>(lo, pos, st, z, general);
        if (!general)
            return r;
    }
    switch (mode & 3) {
    case GM_WIN_SPEC: return lzo1x_decode_general(rd, Lzo1xZeroRun{kLzoZerosWinSpec}, pos, st, z);
    case GM_WIN_TRUE: return lzo1x_decode_general(rd, HostWinRun{in, kLzoZerosWinTrue}, pos, st, z);
    case GM_LAT: return lzo1x_decode_general(rd, Lzo1xZeroRun{kLzoZerosLat}, pos, st, z);
    default: return lzo1x_decode_general(rd, Lzo1xZeroRun{kLzoZerosAny}, pos, st, z);
    }
}

}  // namespace

// Decodes in[0, z) into out[0, cap); *out_len = bytes written (on every
// return).  GR_DONE at the EOF marker, GR_REFUSED on a bad instruction,
// GR_CAPACITY / GR_LOOKBEHIND when an op does not fit or reaches before out.
extern "C" int grammar_decode(const uint8_t* in, uint32_t z, uint8_t* out, uint32_t cap, int mode,
                              uint32_t* out_len)
{
    uint32_t pos = 0, st = ST_F, o = 0;
    int rc;
    for (;;) {
        const Lzo1xIns r = step(in, z, pos, st, mode);
        if (r.bad || r.eof) {
            rc = r.bad ? GR_REFUSED : GR_DONE;
            break;
        }
        const uint32_t len[2] = {r.aL, r.bL}, src[2] = {r.aS, r.bS};
        rc = GR_DONE;
        for (int i = 0; i < 2 && rc == GR_DONE; i++) {
            if (len[i] > cap - o)
                rc = GR_CAPACITY;
            else if (src[i] & kLzoLit)
                memcpy(out + o, in + (src[i] & ~kLzoLit), len[i]);   // (not bad: the literals end by z)
            else if (src[i] > o)
                rc = GR_LOOKBEHIND;
            else
                for (uint32_t j = 0; j < len[i]; j++)
                    out[o + j] = out[o + j - src[i]];
            if (rc == GR_DONE)
                o += len[i];
        }
        if (rc != GR_DONE)
            break;
        pos = r.pos;
        st = r.st;
    }
    *out_len = o;
    return rc;
}

#ifdef GRAMMAR_CHECK
namespace {

struct Tally {
    unsigned long long words, compared, general;
};

bool same(const Lzo1xIns& a, const Lzo1xIns& b)
{
    // (the source of an op of length 0 means nothing)
    return a.pos == b.pos && a.st == b.st && a.aL == b.aL && (a.aL == 0 || a.aS == b.aS) && a.bL == b.bL &&
           (a.bL == 0 || a.bS == b.bS) && a.eof == b.eof && a.bad == b.bad;
}

// One word in one state: the instruction's end from the word alone, then z
// one byte before it, at it and one past it (the `bad` and `eof` rules).
bool check(const uint8_t w[4], uint32_t st, Tally& n)
{
    constexpr uint32_t pos = 16;
    uint8_t in[pos + 8] = {0};
    memcpy(in + pos, w, 4);
    bool general;
    const uint32_t whole = w[0] | w[1] << 8 | w[2] << 16 | (uint32_t)w[3] << 24;
    const uint32_t end = lzo1x_decode_word<false>(whole, pos, st, 1u << 20, general).pos;
    for (uint32_t z = end - 1; z <= end + 1; z++) {
        auto rd = [&](uint32_t p) -> uint32_t { return p < z && p < sizeof in ? in[p] : 0u; };
        const uint32_t lo = rd(pos) | rd(pos + 1) << 8 | rd(pos + 2) << 16 | rd(pos + 3) << 24;
        bool ga, gb;
        const Lzo1xIns a = lzo1x_decode_word<false>(lo, pos, st, z, ga);
        const Lzo1xIns b = lzo1x_decode_word<true>(lo, pos, st, z, gb);
        n.words++;
        if (ga != gb || !same(a, b)) {
            printf("extraction variants differ: word %08x st %u z %u\n", lo, st, z);
            return false;
        }
        if (ga) {
            n.general++;
            continue;
        }
        const Lzo1xIns g = lzo1x_decode_general(rd, Lzo1xZeroRun{kLzoZerosAny}, pos, st, z);
        n.compared++;
        // (the fields of a refused instruction mean nothing)
        if (a.bad != g.bad || (!a.bad && !same(a, g))) {
            printf("forms differ: word %08x st %u z %u: word form pos %u st %u A %u/%08x B %u/%08x eof %d bad %d, "
                   "general form pos %u st %u A %u/%08x B %u/%08x eof %d bad %d\n", lo, st, z,
                   a.pos, a.st, a.aL, a.aS, a.bL, a.bS, a.eof, a.bad, g.pos, g.st, g.aL, g.aS, g.bL, g.bS, g.eof, g.bad);
            return false;
        }
    }
    return true;
}

}  // namespace

int main()
{
    static const uint8_t pick[7] = {0, 1, 3, 4, 0x7F, 0xFC, 0xFF};
    Tally n = {};
    // every first byte in every state; each other byte swept over all values
    // in turn, the remaining two from `pick`
    for (uint32_t st = 0; st < 4; st++)
        for (uint32_t b0 = 0; b0 < 256; b0++)
            for (int sweep = 1; sweep < 4; sweep++)
                for (uint32_t v = 0; v < 256; v++)
                    for (int i = 0; i < 7; i++)
                        for (int j = 0; j < 7; j++) {
                            uint8_t w[4] = {(uint8_t)b0, 0, 0, 0};
                            const int o1 = sweep == 1 ? 2 : 1, o2 = sweep == 3 ? 2 : 3;
                            w[sweep] = (uint8_t)v;
                            w[o1] = pick[i];
                            w[o2] = pick[j];
                            if (!check(w, st, n))
                                return 1;
                        }
    printf("grammar_check: ok, %llu (word, state, end) cases, %llu compared with the general form, "
           "%llu that ask for it\n", n.words, n.compared, n.general);
    return n.compared > n.general ? 0 : 1;
}
#endif
