// itb_dents_host.cc -- pomegranate_amd/csrc/itb_dents.h on the CPU (never part
// of the product library).
//   libitb_dents_host.so  itb_dents_host(): itb_dents_one over one payload
//                         (itb_dents_host_batch(): over many);
//                         itb_dents_wave_host(): the emit kernel's rounds with
//                         the header's copy plan (itb_dents_granule), the 64
//                         lanes one after another (tests/test_readdir.py
//                         compares both with its oracle)
//   itb_dents_check       (-DITB_DENTS_CHECK) both against a second, naive
//                         walk written below, over directed and seeded random
//                         payloads.  Every payload and every output is a heap
//                         block of exactly its length at the residue under
//                         test, so a sanitizer build sees any load at or past
//                         a payload's end and any store outside the output.
#include <assert.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "itb_dents.h"

extern "C" int itb_dents_host(const uint8_t* payload, uint32_t n, uint32_t adepth, uint8_t* out, uint64_t cap,
                              uint32_t* live, uint32_t* dnum, uint32_t* bytes)
{
    return itb_dents_one(payload, n, adepth, out, cap, live, dnum, bytes);
}

// itb_dents_one over `count` payloads, records packed in payload order:
// first[b] = the byte offset of payload b's records, first[count] the total
// (scripts/readdir_rate.py: the host walk of its decode-and-copy-back path).
extern "C" int itb_dents_host_batch(const uint8_t* const* payload, const uint32_t* n, const uint8_t* adepth,
                                    size_t count, uint8_t* out, uint64_t cap, uint64_t* first)
{
    uint64_t at = 0;
    int worst = 0;
    for (size_t b = 0; b < count; b++) {
        uint32_t live, dnum, bytes;
        first[b] = at;
        const int err = itb_dents_one(payload[b], n[b], adepth[b], out + (at < cap ? at : cap), at < cap ? cap - at : 0,
                                      &live, &dnum, &bytes);
        if (err != 0)
            worst = err;
        at += bytes;
    }
    first[count] = at;
    return worst;
}

namespace {

struct HostOut {
    void st16(uint64_t a, const itb_dents_u128& v) const
    {
        assert((a & 15u) == 0);
        memcpy(reinterpret_cast<void*>(a), &v, 16);
    }
    void st1(uint64_t a, uint8_t b) const { *reinterpret_cast<uint8_t*>(a) = b; }
};

}  // namespace

// What itb_dents.hip does for one ITB: the count kernel's words, then the emit
// kernel's rounds writing out[at, min(at + bytes, out_cap)).
extern "C" int itb_dents_wave_host(const uint8_t* p, uint32_t n, uint32_t adepth, uint8_t* out, uint64_t at,
                                   uint64_t out_cap, uint32_t* live, uint32_t* dnum, uint32_t* bytes)
{
    *live = *dnum = *bytes = 0;
    int32_t e = itb_scan_precheck(n, adepth);
    if (e == 0)
        e = itb_scan_live(p, n, adepth, live);
    if (e != 0)
        return e;
    const uint32_t rounds = itb_scan_rounds(adepth);
    uint32_t nd = 0, nb = 0;
    bool bad = false;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t w = itb_scan_word(p, r, adepth);
        for (uint32_t lane = 0; lane < 64; lane++) {
            if (!((w >> lane) & 1u))
                continue;
            const uint64_t fn = itb_dents_flag_namelen(p, 64u * r + lane);
            if (!itb_dents_emits(fn))
                continue;
            nd++;
            bad |= !itb_dents_name_ok(itb_dents_namelen(fn));
            nb += itb_dents_name_ok(itb_dents_namelen(fn)) ? POM_DENT_HDR + itb_dents_namelen(fn) : 0u;
        }
    }
    if (bad)
        return POM_RD_E_NAME;
    *dnum = nd;
    *bytes = nb;
    if (nd == 0 || out_cap == 0)
        return 0;
    const HostOut mem;
    const uint64_t cap_end = (uint64_t)(uintptr_t)out + out_cap;
    for (uint32_t r = 0; r < rounds && at < out_cap; r++) {
        const uint64_t w = itb_scan_word(p, r, adepth);
        itb_dents_u128 hdr[64];
        uint32_t start[64], nr[64], cnt = 0, span = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            if (!((w >> lane) & 1u))
                continue;
            const uint64_t fn = itb_dents_flag_namelen(p, 64u * r + lane);
            if (!itb_dents_emits(fn))
                continue;
            hdr[cnt] = itb_dents_header(p, 64u * r + lane, itb_dents_namelen(fn));
            start[cnt] = span;
            nr[cnt] = 64u * r + lane;
            span += POM_DENT_HDR + itb_dents_namelen(fn);
            cnt++;
        }
        if (cnt == 0)
            continue;
        const uint64_t dst = (uint64_t)(uintptr_t)out + at;
        const itb_dents_round R{start, nr, hdr, cnt, span, p, dst, dst + span < cap_end ? dst + span : cap_end};
        const uint32_t granules = itb_dents_granules(R);
        for (uint32_t g = 0; g < granules; g++)
            itb_dents_granule(mem, R, g);
        at += span;
    }
    return 0;
}

#ifdef ITB_DENTS_CHECK
namespace {

struct Result {
    int err;
    uint32_t live, dnum;
    std::vector<uint8_t> bytes;
};

// mds/itb.c:2567-2585 bit by bit, with the rules of pom_readdir.h for what the
// reference leaves undefined.
Result naive(const uint8_t* p, uint32_t n, uint32_t adepth)
{
    Result R{0, 0, 0, {}};
    if (adepth < 1 || adepth > 10) {
        R.err = -22;
        return R;
    }
    if (n < 3712) {
        R.err = -4097;
        return R;
    }
    bool cut = false, longname = false;
    for (uint32_t nr = 0; nr < (1u << adepth); nr++) {
        if (!(p[3584 + nr / 8] >> (nr % 8) & 1))
            continue;
        R.live++;
        if (11904 + 512 * (uint64_t)(nr + 1) > n) {
            cut = true;
            continue;
        }
        if (cut)
            continue;
        const uint8_t* ite = p + 11904 + 512 * nr;
        uint32_t flag, namelen;
        memcpy(&flag, ite + 16, 4);
        memcpy(&namelen, ite + 20, 4);
        if ((flag & 7) != 0 || (flag & 0x01000000))
            continue;
        if (namelen > 256) {
            longname = true;
            continue;
        }
        R.dnum++;
        R.bytes.insert(R.bytes.end(), ite + 8, ite + 16);
        R.bytes.insert(R.bytes.end(), ite + 36, ite + 38);
        R.bytes.push_back((uint8_t)namelen);
        R.bytes.push_back((uint8_t)(namelen >> 8));
        R.bytes.insert(R.bytes.end(), 4, 0);
        R.bytes.insert(R.bytes.end(), ite + 104, ite + 104 + namelen);
    }
    if (cut || longname) {
        R.err = cut ? -4097 : -4099;
        R.dnum = 0;
        R.bytes.clear();
    }
    return R;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int failures = 0;

// image: a full payload; the first n bytes are walked at residue `shift`, into
// outputs at residue `oshift`, whole and under a few caps
void check(const std::vector<uint8_t>& image, uint32_t n, uint32_t adepth, uint32_t shift, uint32_t oshift,
           const char* what)
{
    // malloc gives 16-byte alignment; the payload ends where the block ends
    uint8_t* exact = static_cast<uint8_t*>(malloc(n + shift + (n + shift == 0)));
    uint8_t* base = exact + shift;
    if (n)
        memcpy(base, image.data(), n);
    const Result want = naive(base, n, adepth);
    const uint64_t total = want.bytes.size();
    std::vector<uint64_t> caps = {total, 0, 1, 15, 16, 17, total ? total - 1 : 0, total / 2, total / 3 + 7};
    for (uint64_t cap : caps) {
        if (cap > total)
            continue;
        for (int wave = 0; wave < 2; wave++) {
            // the output block ends where the cap ends, and starts at its residue
            uint8_t* oexact = static_cast<uint8_t*>(malloc(cap + oshift + (cap + oshift == 0)));
            uint8_t* out = oexact + oshift;
            memset(oexact, 0xA5, cap + oshift);
            uint32_t live = 77, dnum = 77, bytes = 77;
            const int err = wave ? itb_dents_wave_host(base, n, adepth, out, 0, cap, &live, &dnum, &bytes)
                                 : itb_dents_host(base, n, adepth, out, cap, &live, &dnum, &bytes);
            bool ok = err == want.err && dnum == want.dnum && bytes == total &&
                      live == (want.err == -22 || n < 3712 ? 0u : want.live) &&
                      (cap == 0 || memcmp(out, want.bytes.data(), cap) == 0);
            for (uint32_t i = 0; i < oshift; i++)
                ok = ok && oexact[i] == 0xA5;
            if (!ok) {
                failures++;
                fprintf(stderr, "%s (%s): n=%u adepth=%u shift=%u oshift=%u cap=%llu: err %d/%d live %u/%u dnum %u/%u "
                        "bytes %u/%llu\n", what, wave ? "wave" : "one", n, adepth, shift, oshift,
                        (unsigned long long)cap, err, want.err, live, want.live, dnum, want.dnum, bytes,
                        (unsigned long long)total);
            }
            free(oexact);
        }
    }
    free(exact);
}

void put32(std::vector<uint8_t>& img, uint32_t nr, uint32_t off, uint32_t v)
{
    memcpy(img.data() + 11904 + 512 * nr + off, &v, 4);
}

// random bytes everywhere; flags mostly active, name lengths over the whole range
std::vector<uint8_t> random_image(uint32_t density, bool long_names = false)
{
    std::vector<uint8_t> img(11904 + 512 * 1024);
    for (auto& b : img)
        b = (uint8_t)rnd();
    for (uint32_t i = 0; i < 128; i++) {
        uint8_t v = 0;
        for (int k = 0; k < 8; k++)
            v |= (rnd() % 100 < density) << k;
        img[3584 + i] = v;
    }
    static const uint32_t lens[] = {0, 1, 15, 16, 17, 255, 256, 7, 8, 9, 31, 33, 100};
    for (uint32_t nr = 0; nr < 1024; nr++) {
        const uint64_t pick = rnd() % 16;
        uint32_t flag = (uint32_t)rnd() & ~0x01000007u;
        if (pick < 3)
            flag |= 1u + (uint32_t)(rnd() % 7);           // not active
        else if (pick == 3)
            flag |= 0x01000000u;                          // KV
        put32(img, nr, 16, flag);
        uint32_t namelen = rnd() % 3 ? lens[rnd() % 13] : (uint32_t)(rnd() % 257);
        if (pick < 4 && rnd() % 2)
            namelen = 257 + (uint32_t)rnd() % 100000;     // on a skipped ITE: not examined
        if (long_names && pick >= 4 && rnd() % 200 == 0)
            namelen = 257 + (uint32_t)(rnd() % 3) * 70000;
        put32(img, nr, 20, namelen);
    }
    return img;
}

void set_bits(std::vector<uint8_t>& img, std::initializer_list<uint32_t> bits)
{
    memset(img.data() + 3584, 0, 128);
    for (uint32_t nr : bits)
        img[3584 + nr / 8] |= 1u << (nr % 8);
}

}  // namespace

int main()
{
    std::vector<uint8_t> img = random_image(50);
    const uint32_t full = (uint32_t)img.size();
    // adepth with bits above the limit; every payload residue against a moving output residue
    for (uint32_t adepth = 0; adepth <= 12; adepth++)
        for (uint32_t shift = 0; shift < 16; shift++)
            check(img, full, adepth, shift, (5 * shift + adepth) % 16, "adepth");
    // every output residue at one aligned and one odd payload
    for (uint32_t oshift = 0; oshift < 16; oshift++) {
        check(img, 11904 + 512 * 128, 7, 0, oshift, "output residue");
        check(img, 11904 + 512 * 128, 7, 3, oshift, "output residue");
    }
    // cuts around the bitmap, the first ITE, and one byte short of a live ITE's end
    set_bits(img, {0, 5, 63, 64, 200});
    for (uint32_t n : {0u, 1u, 3583u, 3711u, 3712u, 11903u, 11904u, 11904u + 511u, 11904u + 512u,
                       11904u + 512u * 201u - 1u, 11904u + 512u * 201u, 11904u + 512u * 201u + 1u})
        for (uint32_t shift : {0u, 1u, 7u, 8u, 15u})
            check(img, n, 10, shift, shift ^ 9u, "cut");
    // name lengths at the edges, active, on a lone bit and between neighbours
    for (uint32_t namelen : {0u, 1u, 15u, 16u, 17u, 255u, 256u, 257u, 65536u + 5u}) {
        set_bits(img, {9});
        put32(img, 9, 16, 0x80000000u);
        put32(img, 9, 20, namelen);
        check(img, full, 10, namelen % 16, 7, "name length");
        set_bits(img, {8, 9, 10});
        check(img, full, 10, 8, namelen % 16, "name length, neighbours");
        // the same length on an ITE that is skipped is not examined
        put32(img, 9, 16, 0x80000001u);
        check(img, full, 10, 0, 1, "name length, not active");
        put32(img, 9, 16, 0x81000000u);
        check(img, full, 10, 0, 1, "name length, KV");
        put32(img, 9, 16, 0x80000000u);
        put32(img, 9, 20, 12);
    }
    // every non-active state
    for (uint32_t state = 1; state < 8; state++) {
        set_bits(img, {0, 1, 2});
        put32(img, 1, 16, 0x40000000u | state);
        check(img, full, 10, state, state, "state");
    }
    // empty, full, single bits, alternating
    set_bits(img, {});
    check(img, full, 10, 3, 0, "empty");
    check(img, 3712, 10, 3, 0, "empty, bitmap only");
    memset(img.data() + 3584, 0xFF, 128);
    check(img, full, 10, 5, 11, "full");
    check(img, full - 1, 10, 5, 11, "full, one byte short");
    for (uint32_t nr : {0u, 63u, 64u, 1023u}) {
        set_bits(img, {nr});
        check(img, full, 10, nr % 16, 3, "single bit");
        check(img, 11904 + 512 * (nr + 1), 10, nr % 16, 3, "single bit, payload ends with its ITE");
        check(img, 11904 + 512 * (nr + 1) - 1, 10, nr % 16, 3, "single bit, one byte short");
    }
    memset(img.data() + 3584, 0x55, 128);
    check(img, full, 10, 9, 2, "alternating");
    memset(img.data() + 3584, 0xAA, 128);
    check(img, full, 10, 9, 2, "alternating");
    // the largest listing: 1,024 active entries with 256-byte names
    memset(img.data() + 3584, 0xFF, 128);
    for (uint32_t nr = 0; nr < 1024; nr++) {
        put32(img, nr, 16, 0);
        put32(img, nr, 20, 256);
    }
    check(img, full, 10, 0, 0, "maximum");
    check(img, full, 10, 13, 6, "maximum");
    // seeded random ITBs: density, adepth, length and residues all vary
    for (uint32_t t = 0; t < 300; t++) {
        std::vector<uint8_t> r = random_image((uint32_t)(rnd() % 101), t % 3 == 0);
        const uint32_t adepth = 1 + (uint32_t)(rnd() % 10);
        const uint32_t ites = (uint32_t)(rnd() % 1025);
        uint32_t n = 11904 + 512 * ites;
        if (rnd() % 4 == 0)
            n -= (uint32_t)(rnd() % 600);
        check(r, n, adepth, (uint32_t)(rnd() % 16), (uint32_t)(rnd() % 16), "random");
    }
    if (failures) {
        fprintf(stderr, "itb_dents_check: %d FAILED\n", failures);
        return 1;
    }
    printf("itb_dents_check: ok\n");
    return 0;
}
#endif
