// gc_merge_host.cc -- pomegranate_amd/csrc/gc_merge.h on the CPU, with the host
// fold of gc_fold.c (never part of the product library).
//   libgc_merge_host.so  gc_merge_host(): the merge as gc_merge.hip stages it
//                        -- tiles, histogram table, scans with aggregates and
//                        a carry, stable scatter -- one tile and one element
//                        at a time, out of the header's functions alone;
//                        gc_merge_const(): the tile constants; pom_gc_fold.
//   gc_merge_check       (-DGC_MERGE_CHECK) that composition and the fold
//                        against a second, naive merge written below
//                        (std::stable_sort and a sweep), over directed and
//                        seeded random range sets; and the GC stat chunk's
//                        staging layout (host_layout.c).  Inputs and outputs are heap
//                        blocks of exactly their size, so a sanitizer build
//                        sees any access past them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gc_fold.h"
#include "gc_merge.h"
#ifdef GC_MERGE_CHECK
#include "host_layout.h"
#endif

namespace {

// The scan primitive as the kernels stage it: a reduce per tile, the
// aggregates' exclusive scan in passes of kGcAggThreads with a carry, a
// downsweep per tile.  load(i) is element i; op combines; out gets the
// inclusive or the exclusive scan.
template <class T, class Load, class Op>
void tiled_scan(uint32_t n, Load load, Op op, T identity, bool exclusive, std::vector<T>& out)
{
    const uint32_t tiles = gc_merge_tiles(n, kGcScanTile);
    std::vector<T> agg(tiles + 1, identity);
    for (uint32_t t = 0; t < tiles; t++) {
        T sum = identity;
        for (uint32_t i = t * kGcScanTile; i < n && i < (t + 1) * kGcScanTile; i++)
            sum = op(sum, load(i));
        agg[t] = sum;
    }
    T carry = identity;
    for (uint32_t base = 0; base < tiles; base += kGcAggThreads) {
        T run = identity;
        for (uint32_t t = base; t < tiles && t < base + kGcAggThreads; t++) {
            const T v = agg[t];
            agg[t] = op(carry, run);
            run = op(run, v);
        }
        carry = op(carry, run);
    }
    agg[tiles] = carry;
    out.assign(n, identity);
    for (uint32_t t = 0; t < tiles; t++) {
        T run = agg[t];
        for (uint32_t i = t * kGcScanTile; i < n && i < (t + 1) * kGcScanTile; i++) {
            const T incl = op(run, load(i));
            out[i] = exclusive ? run : incl;
            run = incl;
        }
    }
}

}  // namespace

extern "C" uint32_t gc_merge_const(int which)
{
    const uint32_t c[] = {kGcSortTile, kGcScanTile, kGcAggThreads, kGcMergeMaxN, kGcRadixBits, kGcPasses};
    return which >= 0 && which < 6 ? c[which] : 0;
}

// in: n {low, high} pairs; out: room for out_cap pairs; stat: valid, max, nout, nin, nwrapped.
extern "C" int gc_merge_host(const uint64_t* in, uint32_t n, uint64_t* out, uint64_t out_cap, uint64_t* stat)
{
    static_assert(sizeof(pom_gc_range) == 16 && sizeof(pom_gc_stat) == 40, "u64 fields");
    if (n > kGcMergeMaxN)
        return -1;
    std::vector<uint64_t> key[2], val[2];
    for (int k = 0; k < 2; k++) {
        key[k].resize(n);
        val[k].resize(n);
    }
    for (uint32_t i = 0; i < n; i++) {
        key[0][i] = gc_merge_key(in[2 * i], in[2 * i + 1]);
        val[0][i] = in[2 * i + 1];
    }
    const uint32_t tiles = gc_merge_tiles(n, kGcSortTile);
    std::vector<uint32_t> table, base;
    for (uint32_t pass = 0; n && pass < kGcPasses; pass++) {
        const uint32_t a = pass & 1u, b = a ^ 1u;
        table.assign((size_t)tiles * kGcRadix, 0);
        for (uint32_t i = 0; i < n; i++)
            table[(size_t)gc_merge_digit(key[a][i], pass) * tiles + i / kGcSortTile]++;
        tiled_scan<uint32_t>((uint32_t)table.size(), [&](uint32_t i) { return table[i]; },
                             [](uint32_t x, uint32_t y) { return x + y; }, 0u, true, base);
        for (uint32_t t = 0; t < tiles; t++) {
            uint32_t at[kGcRadix];
            for (uint32_t d = 0; d < kGcRadix; d++)
                at[d] = base[(size_t)d * tiles + t];
            const uint32_t end = n < (t + 1) * kGcSortTile ? n : (t + 1) * kGcSortTile;
            for (uint32_t r0 = t * kGcSortTile; r0 < end; r0 += kGcRound) {
                const uint32_t r1 = r0 + kGcRound < end ? r0 + kGcRound : end;
                uint32_t in_round[kGcRadix] = {0}, before[kGcRadix] = {0};
                for (uint32_t i = r0; i < r1; i++)
                    in_round[gc_merge_digit(key[a][i], pass)]++;
                for (uint32_t i = r0; i < r1; i++) {
                    const uint32_t d = gc_merge_digit(key[a][i], pass);
                    const uint32_t to = gc_merge_slot(at[d], before[d]++, in_round[d]);
                    if (to >= n)
                        return -2;          // (a scatter rule that leaves the array)
                    key[b][to] = key[a][i];
                    val[b][to] = val[a][i];
                }
                for (uint32_t d = 0; d < kGcRadix; d++)
                    at[d] += in_round[d];
            }
        }
    }
    const std::vector<uint64_t>&K = key[0], &V = val[0];
    std::vector<uint64_t> runmax;
    tiled_scan<uint64_t>(n, [&](uint32_t i) { return gc_merge_high(K[i], V[i]); },
                         [](uint64_t x, uint64_t y) { return gc_merge_max(x, y); }, 0ull, false, runmax);
    std::vector<uint32_t> kidx;
    tiled_scan<uint32_t>(n, [&](uint32_t i) { return gc_merge_head(i, K[i], i ? runmax[i - 1] : 0ull) ? 1u : 0u; },
                         [](uint32_t x, uint32_t y) { return x + y; }, 0u, true, kidx);
    uint64_t valid = 0, heads = 0, kept = 0;
    for (uint32_t i = 0; i < n; i++) {
        kept += gc_merge_key_kept(K[i]);
        const bool head = gc_merge_head(i, K[i], i ? runmax[i - 1] : 0ull);
        const uint32_t x = gc_merge_extent(kidx[i], head);
        if (head) {
            heads++;
            valid -= K[i];
            if (x < out_cap)
                out[2 * (size_t)x] = K[i];
        }
        if (gc_merge_last(i, n, K[i], i + 1 < n ? K[i + 1] : 0ull, runmax[i])) {
            valid += runmax[i];
            if (x < out_cap)
                out[2 * (size_t)x + 1] = runmax[i];
        }
    }
    stat[0] = valid;
    stat[1] = n ? runmax[n - 1] : 0;
    stat[2] = heads;
    stat[3] = n;
    stat[4] = n - kept;
    return 0;
}

#ifdef GC_MERGE_CHECK
namespace {

struct Want {
    std::vector<uint64_t> out;      // pairs
    uint64_t valid = 0, max = 0, nwrapped = 0;
};

Want naive(const std::vector<uint64_t>& in)
{
    Want W;
    std::vector<std::pair<uint64_t, uint64_t>> r;
    for (size_t i = 0; i < in.size() / 2; i++) {
        if (in[2 * i + 1] <= in[2 * i])
            W.nwrapped++;
        else
            r.emplace_back(in[2 * i], in[2 * i + 1]);
    }
    std::stable_sort(r.begin(), r.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (const auto& x : r) {
        if (!W.out.empty() && x.first <= W.out.back()) {
            W.out.back() = std::max(W.out.back(), x.second);
        } else {
            W.out.push_back(x.first);
            W.out.push_back(x.second);
        }
    }
    for (size_t k = 0; k < W.out.size() / 2; k++)
        W.valid += W.out[2 * k + 1] - W.out[2 * k];
    W.max = W.out.empty() ? 0 : W.out.back();
    return W;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int failures = 0, checks = 0;
const uint64_t kPoison = 0xA5A5A5A5A5A5A5A5ull;

void check(const std::vector<uint64_t>& in, const char* what)
{
    const uint32_t n = (uint32_t)(in.size() / 2);
    const Want W = naive(in);
    const uint64_t nout = W.out.size() / 2;
    uint64_t* exact_in = static_cast<uint64_t*>(malloc(16 * (size_t)n + (n == 0)));
    if (n)
        memcpy(exact_in, in.data(), 16 * (size_t)n);
    for (uint64_t cap : {nout, nout ? nout - 1 : 0, (uint64_t)0}) {
        uint64_t* out = static_cast<uint64_t*>(malloc(16 * cap + 8));
        for (uint64_t i = 0; i < 2 * cap + 1; i++)
            out[i] = kPoison;
        uint64_t st[5] = {7, 7, 7, 7, 7};
        const int rc = gc_merge_host(exact_in, n, out, cap, st);
        const uint64_t fit = nout < cap ? nout : cap;
        const bool ok = rc == 0 && st[0] == W.valid && st[1] == W.max && st[2] == nout && st[3] == n &&
                        st[4] == W.nwrapped && (fit == 0 || memcmp(out, W.out.data(), 16 * fit) == 0) &&
                        out[2 * fit] == kPoison && (n == 0 || memcmp(exact_in, in.data(), 16 * (size_t)n) == 0);
        checks++;
        if (!ok) {
            failures++;
            fprintf(stderr, "%s: n=%u cap=%llu: rc %d valid %llu/%llu max %llu/%llu nout %llu/%llu wrapped %llu/%llu\n",
                    what, n, (unsigned long long)cap, rc, (unsigned long long)st[0], (unsigned long long)W.valid,
                    (unsigned long long)st[1], (unsigned long long)W.max, (unsigned long long)st[2],
                    (unsigned long long)nout, (unsigned long long)st[4], (unsigned long long)W.nwrapped);
        }
        free(out);
    }
    free(exact_in);
}

// n ranges of one family
std::vector<uint64_t> family(int kind, uint32_t n)
{
    std::vector<uint64_t> v(2 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t lo = 0, hi = 1;
        switch (kind) {
        case 0: case 1: case 2: case 3: case 4: case 5: case 6: case 7:   // keys differ in one byte only
            lo = 0x0101010101010101ull * 0x11 ^ ((rnd() & 0xFF) << (8 * kind));
            hi = lo + 1 + (rnd() & 3);
            if (hi <= lo)
                hi = ~0ull;
            break;
        case 8:                     // all keys equal
            lo = 1000, hi = 1001 + (rnd() & 0xFF);
            break;
        case 9:                     // descending, touching
            lo = 10ull * (n - 1 - i), hi = lo + 10;
            break;
        case 10:                    // gap of one, shuffled by a stride
            lo = 10ull * ((i * 7919ull) % n), hi = lo + 9;
            break;
        case 11:                    // random, with wrapped ranges mixed in
            lo = rnd() >> (rnd() & 63), hi = lo + (rnd() & 0xFFFF);
            if (rnd() % 7 == 0)
                hi = rnd() % 2 ? lo : lo - (rnd() & 0xFF);
            break;
        default:                    // sparse random over 2^40
            lo = rnd() & ((1ull << 40) - 1), hi = lo + 1 + (rnd() & 0xFFFFF);
        }
        v[2 * i] = lo;
        v[2 * i + 1] = hi;
    }
    return v;
}

void check_fold()
{
    // the fold equals the naive merge of everything put together, however it is cut into maps
    for (uint32_t t = 0; t < 200; t++) {
        std::vector<uint64_t> all;
        std::vector<std::vector<pom_gc_range>> maps(1 + rnd() % 4);
        for (auto& m : maps) {
            const std::vector<uint64_t> part = family(12, (uint32_t)(rnd() % 50));
            const Want w = naive(part);
            for (size_t k = 0; k < w.out.size() / 2; k++)
                m.push_back(pom_gc_range{w.out[2 * k], w.out[2 * k + 1]});
            all.insert(all.end(), part.begin(), part.end());
        }
        std::vector<pom_gc_range> seed;
        if (t % 2) {
            const Want w = naive(family(12, (uint32_t)(rnd() % 20)));
            for (size_t k = 0; k < w.out.size() / 2; k++)
                seed.push_back(pom_gc_range{w.out[2 * k], w.out[2 * k + 1]});
            all.insert(all.end(), w.out.begin(), w.out.end());
        }
        const Want W = naive(all);
        const size_t nout = W.out.size() / 2;
        std::vector<const pom_gc_range*> ptr;
        std::vector<size_t> cnt;
        for (auto& m : maps) {
            ptr.push_back(m.data());
            cnt.push_back(m.size());
        }
        for (size_t cap : {nout, nout ? nout - 1 : (size_t)0}) {
            pom_gc_range* merged = static_cast<pom_gc_range*>(malloc(16 * cap + 1));
            pom_gc_stat st;
            const int rc = pom_gc_fold(ptr.data(), cnt.data(), ptr.size(), seed.data(), seed.size(), merged, cap, &st);
            const bool ok = rc == (cap < nout ? POM_GC_E_NOSPACE : 0) && st.valid == W.valid && st.max == W.max &&
                            st.nout == nout && (cap == 0 || memcmp(merged, W.out.data(), 16 * cap) == 0);
            checks++;
            if (!ok) {
                failures++;
                fprintf(stderr, "fold %u cap %zu: rc %d nout %llu/%zu\n", t, cap, rc, (unsigned long long)st.nout, nout);
            }
            free(merged);
        }
    }
    const pom_gc_range unsorted[] = {{10, 20}, {5, 8}}, touching[] = {{0, 5}, {5, 9}}, empty[] = {{4, 4}};
    const pom_gc_range gap1[] = {{0, 5}, {6, 9}};
    pom_gc_stat st;
    pom_gc_range room[2];
    checks += 4;
    failures += pom_gc_fold(nullptr, nullptr, 0, unsorted, 2, room, 2, &st) != -22;
    failures += pom_gc_fold(nullptr, nullptr, 0, touching, 2, room, 2, &st) != -22;
    failures += pom_gc_fold(nullptr, nullptr, 0, empty, 1, room, 2, &st) != -22;
    failures += !(pom_gc_fold(nullptr, nullptr, 0, gap1, 2, room, 2, &st) == 0 && st.nout == 2 && st.valid == 8);
}

// The GC stat chunk's staging (host_layout.c pom_layout_gcstat): the stat lies
// 8-byte aligned inside the first D2H's span, the device regions follow one
// another without overlap, and the host side has room for every extent.
void check_layout()
{
    const uint8_t words[] = {WW_STATUS, WW_OUTLEN, WW_LIVE, WW_COUNT, WW_ERR};
    const walk_spec spec = {words, sizeof words, 16, 16, 0, 0, 0, 1};
    for (size_t nb : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)1001}) {
        std::vector<size_t> ids(nb), slen(nb), cap(nb);
        size_t nm = 0;
        for (size_t i = 0; i < nb; i++) {
            ids[i] = i;
            slen[i] = 100 + rnd() % 5000;
            cap[i] = 11904 + 512 * (rnd() % 1025);
            nm += pom_gc_max_ranges(cap[i], 1 + (unsigned)(rnd() % 10));
        }
        const size_t nlzo = nb - nb / 3, dec = 4096 + 64 * nb, mscr = gc_merge_scratch_layout((uint32_t)nm).total;
        layout L;
        pom_layout_gcstat(&L, ids.data(), nb, nlzo, slen.data(), cap.data(), &spec, dec, nm, mscr);
        const gcstat_layout& G = L.u.gcstat;
        const walk_layout& K = L.u.walk;
        bool ok = G.nmerge == nm && K.rcap == 16 * nm && G.o_stat % 8 == 0 && K.res_off % 8 == 0 &&
                  G.o_stat >= K.res_off + 20 * nb && G.o_stat + 40 <= K.res_off + K.res_bytes &&
                  K.res_off + K.res_bytes <= L.o_src && L.o_src <= L.o_dst && L.htotal == K.o_hrec + 16 * nm &&
                  K.o_hrec >= L.o_dst && L.o_scr >= L.o_dst && K.o_pack >= L.o_scr + dec &&
                  G.o_mscr >= K.o_pack + 16 * nm && G.o_mscr % 256 == 0 && G.mscr_bytes == mscr &&
                  G.o_merged >= G.o_mscr + mscr && L.dtotal >= G.o_merged + 16 * nm;
        for (size_t w = 0; w < sizeof words; w++)
            ok = ok && K.o_word[words[w]] == K.res_off + 4 * nb * w;
        checks++;
        if (!ok) {
            failures++;
            fprintf(stderr, "layout nb=%zu nm=%zu\n", nb, nm);
        }
    }
    checks += 3;
    failures += pom_gc_max_ranges(11904 + 512 * 100, 10) != 100;
    failures += pom_gc_max_ranges(11904 + 512 * 100, 3) != 8;
    failures += pom_gc_max_ranges(11904 + 512 * 100, 0) != 0 || pom_gc_max_ranges(11904 + 512 * 100, 11) != 0;
}

}  // namespace

// "quick": without the long cases (for builds against deliberately wrong rules)
int main(int argc, char** argv)
{
    const bool quick = argc > 1 && strcmp(argv[1], "quick") == 0;
    const uint32_t S = kGcSortTile, C = kGcScanTile;
    const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1, S - 1, S, S + 1, 2 * S + 1};
    for (int kind = 0; kind <= 12; kind++)
        for (uint32_t n : sizes)
            check(family(kind, n), "family");
    // a wide range first in sorted order, three scan tiles of small ranges inside it; then last in the input
    {
        std::vector<uint64_t> v = family(12, 3 * C);
        v.insert(v.begin(), {0ull, 1ull << 40});
        check(v, "wide first");
        std::rotate(v.begin(), v.begin() + 2, v.end());
        check(v, "wide last");
    }
    // heads and lasts at tile edges: extents of exactly one scan tile, touching inside, a gap between
    {
        std::vector<uint64_t> v;
        for (uint32_t i = 0; i < 3 * C; i++) {
            const uint64_t lo = 4ull * i + (i / C) * 100;
            v.push_back(lo);
            v.push_back(lo + 4);
        }
        check(v, "extent per tile");
    }
    // more tile aggregates than one pass of the aggregates' workgroup is wide
    if (!quick)
        check(family(12, kGcAggThreads * C + 3 * C + 5), "carry loop");
    for (uint32_t t = 0; t < (quick ? 20u : 300u); t++)
        check(family(11 + (int)(rnd() % 2), (uint32_t)(rnd() % (3 * S))), "random");
    check_fold();
    check_layout();
    if (failures) {
        fprintf(stderr, "gc_merge_check: %d of %d FAILED\n", failures, checks);
        return 1;
    }
    printf("gc_merge_check: %d checks ok\n", checks);
    return 0;
}
#endif
