// itb_check_host.cc -- pomegranate_amd/csrc/itb_check.h on the CPU (never part
// of the product library).
//   libitb_check_host.so  itb_check_host(): itb_check_one over one payload;
//                         itb_check_batch_host(): a call as pom_itb_check_dev
//                         sees it, status rule included (tests/test_check.py
//                         compares both with its oracle)
//   itb_check_check       (-DITB_CHECK_CHECK) itb_check_one over directed and
//                         seeded random tables.  Every payload is a heap block
//                         of exactly its length at the residue under test, so
//                         a sanitizer build sees any load at or past its end;
//                         the results must not depend on the residue, and
//                         whatever the table holds, every count must agree
//                         with the masks.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "itb_check.h"

extern "C" int itb_check_host(const uint8_t* payload, uint32_t n, uint32_t adepth, const pom_check_hdr* hdr,
                              uint32_t flags, pom_check_report* report, uint64_t* slot_mask, uint64_t* ite_mask)
{
    return itb_check_one(payload, n, adepth, hdr, flags, report, slot_mask, ite_mask);
}

extern "C" void itb_check_batch_host(const uint8_t* payload, const uint64_t* payload_off, const uint32_t* payload_len,
                                     const int32_t* status, const uint8_t* adepth, const pom_check_hdr* hdr,
                                     uint32_t nitb, uint32_t flags, pom_check_report* report, uint64_t* slot_mask,
                                     uint64_t* ite_mask, int32_t* err)
{
    for (uint32_t b = 0; b < nitb; b++) {
        uint64_t* sm = slot_mask ? slot_mask + POM_CK_SLOT_MASK_WORDS * b : nullptr;
        uint64_t* im = ite_mask ? ite_mask + POM_CK_ITE_MASK_WORDS * b : nullptr;
        if (status && status[b] != 0) {
            report[b] = pom_check_report{};
            if (sm)
                memset(sm, 0, 8 * POM_CK_SLOT_MASK_WORDS);
            if (im)
                memset(im, 0, 8 * POM_CK_ITE_MASK_WORDS);
            err[b] = status[b];
            continue;
        }
        err[b] = itb_check_one(payload + payload_off[b], payload_len[b], adepth[b], hdr ? &hdr[b] : nullptr, flags,
                               &report[b], sm, im);
    }
}

#ifdef ITB_CHECK_CHECK
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

struct Result {
    int32_t err;
    pom_check_report rep;
    uint64_t sm[POM_CK_SLOT_MASK_WORDS], im[POM_CK_ITE_MASK_WORDS];
};

// The payload copied into a heap block that ends where the payload ends, at
// byte residue `shift`.
Result run(const uint8_t* image, uint32_t n, uint32_t adepth, const pom_check_hdr* hdr, uint32_t flags,
           uint32_t shift)
{
    void* block = nullptr;
    if (posix_memalign(&block, 16, n + shift) != 0)
        abort();
    uint8_t* p = static_cast<uint8_t*>(block) + shift;
    memcpy(p, image, n);
    Result R;
    memset(&R, 0x5A, sizeof R);
    R.err = itb_check_one(p, n, adepth, hdr, flags, &R.rep, R.sm, R.im);
    free(block);
    return R;
}

int fail(const char* what, unsigned t)
{
    fprintf(stderr, "itb_check_check: table %u: %s\n", t, what);
    return 1;
}

int popcount_words(const uint64_t* w, uint32_t n)
{
    int c = 0;
    for (uint32_t i = 0; i < n; i++)
        c += __builtin_popcountll(w[i]);
    return c;
}

}  // namespace

int main()
{
    unsigned tables = 0;
    for (unsigned t = 0; t < 400; t++) {
        const uint32_t adepth = t < 20 ? t % 12 : 1 + rnd() % 10;      // 0 and 11 among the first
        const uint32_t d = 1u << (adepth < 1 || adepth > 10 ? 1 : adepth);
        const uint32_t ites = rnd() % (d + 1);
        uint32_t n = POM_ITB_ITE_OFF + POM_ITE_SIZE * ites;
        if (t % 7 == 3)
            n -= 1 + rnd() % 600;                                       // cut: inside the last ITE or the index
        uint8_t* image = static_cast<uint8_t*>(calloc(1, POM_ITB_ITE_OFF + POM_ITE_SIZE * 1024));
        // slots: mostly plausible, now and then anything
        for (uint32_t s = 0; s < POM_ITB_INDEX_ENTRIES; s++) {
            const bool near = s < 2 * d + 2;
            if (!(near ? rnd() % 4 : rnd() % 300 == 0))
                continue;
            const bool wild = rnd() % 16 == 0;
            const uint32_t entry = wild ? rnd() % 32768 : rnd() % (d + 1);
            const uint32_t conflict = wild ? rnd() % 32768 : d + rnd() % (d + 2) - 1;
            const uint32_t w = entry | (conflict & 0x7FFF) << 15 | (uint32_t)(rnd() % 4) << 30;
            memcpy(image + POM_ITB_INDEX_OFF + 4 * s, &w, 4);
        }
        for (uint32_t nr = 0; nr < 1024; nr++)
            if (nr < ites ? rnd() % 3 != 0 : (t % 5 == 0 && rnd() % 200 == 0))
                image[POM_ITB_BITMAP_OFF + nr / 8] |= 1u << (nr % 8);
        for (uint32_t nr = 0; nr < ites; nr++) {
            const uint64_t h = rnd();
            memcpy(image + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr, &h, 8);
        }
        pom_check_hdr hdr{};
        hdr.entries = (int32_t)(rnd() % (d + 2));
        hdr.max_offset = (int32_t)(rnd() % (d + 1)) - 1;
        hdr.pseudo_conflicts = (int32_t)(rnd() % (d + 1));
        hdr.ulen = POM_ITB_SIZE + POM_ITE_SIZE * (uint32_t)(rnd() % (d + 1));
        hdr.inf = (uint16_t)(rnd() % (d + 2));
        hdr.itu = (uint16_t)(rnd() % (d + 1));
        hdr.depth = (uint8_t)(t % 9 == 0 ? 64 + rnd() % 3 : rnd() % 5);
        hdr.itbid = rnd() % 4;
        const Result base = run(image, n, adepth, &hdr, POM_CK_ITBID, 0);
        for (uint32_t shift = 1; shift < 8; shift++) {
            const Result r = run(image, n, adepth, &hdr, POM_CK_ITBID, shift);
            if (memcmp(&r, &base, sizeof r) != 0)
                return fail("the result depends on the payload's alignment", t);
        }
        const Result bare = run(image, n, adepth, nullptr, POM_CK_ITBID, 3);
        if (bare.err != base.err || (bare.rep.findings >> POM_CK_E_MISPLACED) != 0 ||
            (bare.rep.findings & 0x7FFF) != (base.rep.findings & 0x7FFF))
            return fail("hdr NULL changes more than kinds 15 ... 21", t);
        if (base.err != 0) {
            pom_check_report zero{};
            zero.live = base.rep.live;
            if (memcmp(&base.rep, &zero, sizeof zero) != 0 || popcount_words(base.sm, POM_CK_SLOT_MASK_WORDS) ||
                popcount_words(base.im, POM_CK_ITE_MASK_WORDS))
                return fail("an error with a report or masks", t);
        } else {
            // every count is at most its mask's population, every finding bit has a count
            int slot_max = 0, ite_max = 0;
            for (uint32_t k = 0; k < kItbCheckCounted; k++) {
                if (((base.rep.findings >> k) & 1u) != (base.rep.count[k] != 0))
                    return fail("findings and count[] disagree", t);
                int& m = k < kItbCheckSlotKinds ? slot_max : ite_max;
                m = base.rep.count[k] > m ? base.rep.count[k] : m;
            }
            if (slot_max > popcount_words(base.sm, POM_CK_SLOT_MASK_WORDS) ||
                ite_max > popcount_words(base.im, POM_CK_ITE_MASK_WORDS))
                return fail("a count exceeds its mask", t);
            if ((slot_max == 0) != (popcount_words(base.sm, POM_CK_SLOT_MASK_WORDS) == 0) ||
                (ite_max == 0) != (popcount_words(base.im, POM_CK_ITE_MASK_WORDS) == 0))
                return fail("a mask without a count", t);
        }
        free(image);
        tables++;
    }
    printf("itb_check_check: ok (%u tables, 9 runs each)\n", tables);
    return 0;
}
#endif
