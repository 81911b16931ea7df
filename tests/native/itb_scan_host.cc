// itb_scan_host.cc -- pomegranate_amd/csrc/itb_scan.h on the CPU (never part
// of the product library).
//   libitb_scan_host.so  itb_scan_host(): itb_scan_one over one payload
//                        (tests/test_gc_scan.py compares it with its oracle)
//   itb_scan_check       (-DITB_SCAN_CHECK) the header against a second,
//                        naive walk written below, over directed and seeded
//                        random payloads.  Every payload is a heap block of
//                        exactly its length at the residue under test, so a
//                        sanitizer build sees any load at or past its end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "itb_scan.h"

extern "C" int itb_scan_host(const uint8_t* payload, uint32_t n, uint32_t adepth, uint32_t column,
                             uint64_t* out, uint64_t cap, uint32_t* live, uint32_t* nranges)
{
    static_assert(sizeof(pom_gc_range) == 16, "two u64");
    return itb_scan_one(payload, n, adepth, column, reinterpret_cast<pom_gc_range*>(out), cap, live, nranges);
}

#ifdef ITB_SCAN_CHECK
namespace {

struct Result {
    int err;
    uint32_t live;
    std::vector<uint64_t> r;
};

uint64_t naive_u64(const uint8_t* p)
{
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--)
        v = v << 8 | p[i];
    return v;
}

// mdsl/gc.c:968-993 and :788-802 bit by bit, with the rules of pom_gc.h for
// what the reference leaves undefined.
Result naive(const uint8_t* p, uint32_t n, uint32_t adepth, uint32_t column)
{
    Result R{0, 0, {}};
    if (adepth < 1 || adepth > 10) {
        R.err = -22;
        return R;
    }
    if (n < 3712) {
        R.err = -4097;
        return R;
    }
    bool cut = false;
    for (uint32_t nr = 0; nr < (1u << adepth); nr++) {
        if (!(p[3584 + nr / 8] >> (nr % 8) & 1))
            continue;
        R.live++;
        if (11904 + 512 * (uint64_t)(nr + 1) > n) {
            cut = true;
            continue;
        }
        const uint8_t* c = p + 11904 + 512 * nr + 368 + 24 * column;
        const uint64_t len = naive_u64(c + 8), off = naive_u64(c + 16);
        if (len > 0) {
            R.r.push_back(off);
            R.r.push_back(off + len + 1);
        }
    }
    if (cut) {
        R.err = -4097;
        R.r.clear();
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

// image: a full payload; the first n bytes are scanned at residue `shift`
void check(const std::vector<uint8_t>& image, uint32_t n, uint32_t adepth, uint32_t shift, const char* what)
{
    // malloc gives 16-byte alignment; the payload ends where the block ends
    uint8_t* exact = static_cast<uint8_t*>(malloc(n + shift + (n + shift == 0)));
    uint8_t* base = exact + shift;
    if (n)
        memcpy(base, image.data(), n);
    for (uint32_t column = 0; column < 6; column++) {
        const Result want = naive(base, n, adepth, column);
        for (uint64_t cap : {(uint64_t)1024, (uint64_t)(want.r.size() / 2 ? want.r.size() / 2 - 1 : 0)}) {
            std::vector<uint64_t> got(2 * cap + 2, 0xA5A5A5A5A5A5A5A5ull);
            uint32_t live = 77, nranges = 77;
            const int err = itb_scan_host(base, n, adepth, column, got.data(), cap, &live, &nranges);
            const size_t fit = want.r.size() / 2 < cap ? want.r.size() / 2 : cap;
            bool ok = err == want.err && nranges == want.r.size() / 2 &&
                      live == (want.err == -22 || n < 3712 ? 0u : want.live) &&
                      (fit == 0 || memcmp(got.data(), want.r.data(), 16 * fit) == 0) &&
                      got[2 * fit] == 0xA5A5A5A5A5A5A5A5ull;
            if (!ok) {
                failures++;
                fprintf(stderr, "%s: n=%u adepth=%u shift=%u column=%u cap=%llu: err %d/%d live %u/%u ranges %u/%zu\n",
                        what, n, adepth, shift, column, (unsigned long long)cap, err, want.err, live, want.live,
                        nranges, want.r.size() / 2);
            }
        }
    }
    free(exact);
}

std::vector<uint8_t> random_image(uint32_t density)
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
    // a third of the columns empty, a few at the wrap
    for (uint32_t nr = 0; nr < 1024; nr++)
        for (uint32_t c = 0; c < 6; c++) {
            uint8_t* col = img.data() + 11904 + 512 * nr + 368 + 24 * c;
            const uint64_t pick = rnd() % 9;
            if (pick < 3)
                memset(col + 8, 0, 8);
            else if (pick == 3)
                memset(col + 16, 0xFF, 8);
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
    // directed: adepth with bits above the limit, every residue
    for (uint32_t adepth = 0; adepth <= 12; adepth++)
        for (uint32_t shift = 0; shift < 16; shift++)
            check(img, full, adepth, shift, "adepth");
    // cuts around the bitmap, the first ITE, and one byte short of a live ITE's end
    set_bits(img, {0, 5, 63, 64, 200});
    for (uint32_t n : {0u, 1u, 3583u, 3711u, 3712u, 11903u, 11904u, 11904u + 511u, 11904u + 512u,
                       11904u + 512u * 201u - 1u, 11904u + 512u * 201u, 11904u + 512u * 201u + 1u})
        for (uint32_t shift : {0u, 1u, 7u, 8u, 15u})
            check(img, n, 10, shift, "cut");
    // empty, full, single bits, alternating
    set_bits(img, {});
    check(img, full, 10, 3, "empty");
    check(img, 3712, 10, 3, "empty, bitmap only");
    memset(img.data() + 3584, 0xFF, 128);
    check(img, full, 10, 5, "full");
    check(img, full - 1, 10, 5, "full, one byte short");
    for (uint32_t nr : {0u, 63u, 64u, 1023u}) {
        set_bits(img, {nr});
        check(img, full, 10, nr % 16, "single bit");
        check(img, 11904 + 512 * (nr + 1), 10, nr % 16, "single bit, payload ends with its ITE");
        check(img, 11904 + 512 * (nr + 1) - 1, 10, nr % 16, "single bit, one byte short");
    }
    memset(img.data() + 3584, 0x55, 128);
    check(img, full, 10, 9, "alternating");
    memset(img.data() + 3584, 0xAA, 128);
    check(img, full, 10, 9, "alternating");
    // seeded random ITBs: density, adepth, length and residue all vary
    for (uint32_t t = 0; t < 300; t++) {
        std::vector<uint8_t> r = random_image((uint32_t)(rnd() % 101));
        const uint32_t adepth = 1 + (uint32_t)(rnd() % 10);
        const uint32_t ites = (uint32_t)(rnd() % 1025);
        uint32_t n = 11904 + 512 * ites;
        if (rnd() % 4 == 0)
            n -= (uint32_t)(rnd() % 600);
        check(r, n, adepth, (uint32_t)(rnd() % 16), "random");
    }
    if (failures) {
        fprintf(stderr, "itb_scan_check: %d FAILED\n", failures);
        return 1;
    }
    printf("itb_scan_check: ok\n");
    return 0;
}
#endif
