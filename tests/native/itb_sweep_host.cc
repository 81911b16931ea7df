// itb_sweep_host.cc -- pomegranate_amd/csrc/itb_sweep.h on the CPU (never part
// of the product library).
//   libitb_sweep_host.so  itb_sweep_host(): itb_sweep_one over one payload, as
//                         the serial loop or as the kernel's pieces;
//                         itb_sweep_batch_host(): a call as pom_itb_sweep_dev
//                         sees it, status and budget rules included
//                         (tests/test_itb_sweep.py compares both forms with
//                         its oracle)
//   itb_sweep_check       (-DITB_SWEEP_CHECK) both forms over seeded tables
//                         built by the split header's add rule with random
//                         flag words, and over the same tables with a few
//                         words flipped.  A payload is a heap block of exactly
//                         its length, so a sanitizer build sees any access
//                         past it; whatever the table holds, an error leaves
//                         it untouched, both forms agree in every byte, and a
//                         sweep leaves a table the check passes and a second
//                         sweep finds nothing in.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "itb_sweep.h"

extern "C" int itb_sweep_host(uint8_t* payload, uint32_t n, uint32_t adepth, const pom_check_hdr* hdr, uint32_t budget,
                              uint64_t payload_off, int parts, pom_sweep_result* result, uint32_t* steps)
{
    return itb_sweep_one(payload, n, adepth, *hdr, budget, payload_off, parts != 0, result, steps);
}

extern "C" void itb_sweep_batch_host(uint8_t* payload, const uint64_t* payload_off, const uint32_t* payload_len,
                                     const int32_t* status, const uint8_t* adepth, const pom_check_hdr* hdr,
                                     const uint32_t* budget, uint32_t nitb, int parts, pom_sweep_result* result,
                                     uint32_t* steps)
{
    for (uint32_t b = 0; b < nitb; b++) {
        if (status && status[b] != 0) {
            result[b] = pom_sweep_result{};
            result[b].err = status[b];
            steps[b] = 0;
            continue;
        }
        itb_sweep_one(payload + payload_off[b], payload_len[b], adepth[b], hdr[b],
                      budget ? budget[b] : POM_SWEEP_NO_BUDGET, payload_off[b], parts != 0, &result[b], &steps[b]);
    }
}

#ifdef ITB_SWEEP_CHECK
namespace {

constexpr uint32_t kHeader = POM_ITB_SIZE - POM_ITB_ITE_OFF;    // sizeof(struct itbh)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int fail(const char* what, unsigned t)
{
    fprintf(stderr, "itb_sweep_check: table %u: %s\n", t, what);
    return 1;
}

uint8_t* exact_block(uint32_t n, const uint8_t* image)
{
    void* block = nullptr;
    if (posix_memalign(&block, 16, n ? n : 16) != 0)
        abort();
    memcpy(block, image, n);
    return static_cast<uint8_t*>(block);
}

}  // namespace

int main()
{
    unsigned swept = 0, refused = 0, stopped = 0;
    static itb_split_state B;
    for (unsigned t = 0; t < 600; t++) {
        const uint32_t adepth = 1 + rnd() % 10, d = 1u << adepth;
        const uint32_t m = t % 11 == 0 ? d : (uint32_t)(rnd() % (d + 1));
        const uint32_t narrow = rnd() % 2 ? d : (d / 4 ? d / 4 : 1);
        const uint32_t n = POM_ITB_ITE_OFF + POM_ITE_SIZE * m;
        const uint32_t frac = (uint32_t)(rnd() % 5);                    // marked: none, few, half, most, all
        // the table, by __itb_add_index's rule: the split state's new side is the builder
        memset(&B, 0, sizeof B);
        uint8_t* image = static_cast<uint8_t*>(malloc(n));
        for (uint32_t i = 0; i < n; i++)
            image[i] = (uint8_t)rnd();
        memset(image + POM_ITB_BITMAP_OFF, 0, POM_ITB_ITE_OFF - POM_ITB_BITMAP_OFF);
        uint32_t want = 0;
        for (uint32_t nr = 0; nr < m; nr++) {
            const uint64_t hash = (rnd() % narrow) | (rnd() << 12);
            uint8_t* ite = image + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr;
            memcpy(ite + POM_ITE_HASH_OFF, &hash, 8);
            const bool mark = frac == 4 || (frac != 0 && rnd() % 10 < (frac == 1 ? 1u : frac == 2 ? 5u : 9u));
            static const uint32_t other[] = {0u, 2u, 3u, 5u, 7u};
            uint32_t flag;
            memcpy(&flag, ite + POM_ITE_FLAG_OFF, 4);
            flag = (flag & ~POM_ITE_STATE_MASK) | (mark ? POM_ITE_UNLINKED : other[rnd() % 5]);
            memcpy(ite + POM_ITE_FLAG_OFF, &flag, 4);
            want += mark;
            B.info[nr] = (uint16_t)(hash & (d - 1u));
            if (!itb_split_add(B, d, nr))
                return fail("the builder's table is full", t);
        }
        memcpy(image + POM_ITB_BITMAP_OFF, B.nbm, sizeof B.nbm);
        memcpy(image + POM_ITB_INDEX_OFF, B.nidx, sizeof B.nidx);
        pom_check_hdr hdr{};
        hdr.entries = B.n.entries;
        hdr.max_offset = B.n.max_offset;
        hdr.pseudo_conflicts = B.n.pseudo;
        hdr.ulen = itb_split_len(B.n);
        hdr.inf = (uint16_t)B.n.inf;
        hdr.itu = (uint16_t)B.n.itu;
        const bool flipped = t % 3 == 2;
        if (flipped)                                                    // a few index words or bitmap bytes
            for (uint32_t k = 0; k < 1 + rnd() % 3; k++)
                image[POM_ITB_BITMAP_OFF + rnd() % (128 + 8 * d)] ^= (uint8_t)(1u << (rnd() % 8));
        const uint32_t budget = t % 5 == 1 ? (uint32_t)(rnd() % (want + 2)) : POM_SWEEP_NO_BUDGET;

        uint8_t* p = exact_block(n, image);
        uint8_t* q = exact_block(n, image);
        pom_sweep_result r, rq;
        uint32_t steps = 0;
        const int32_t err = itb_sweep_one(p, n, adepth, hdr, budget, 0, false, &r, &steps);
        const int32_t errq = itb_sweep_one(q, n, adepth, hdr, budget, 0, true, &rq, nullptr);
        if (err != r.err || errq != rq.err)
            return fail("the return value is not result.err", t);
        if (memcmp(&r, &rq, sizeof r) != 0 || memcmp(p, q, n) != 0)
            return fail("the serial loop and the pieces disagree", t);
        if (err != 0 || r.removed == 0) {
            refused++;
            if (memcmp(p, image, n) != 0)
                return fail("nothing is produced, yet the payload changed", t);
            if (r.dc || r.len || r.entries || r.max_offset || r.pseudo_conflicts || r.itu || r.visited)
                return fail("nothing is produced, yet the result is not zero", t);
            if (!flipped && err != 0)
                return fail("a table built by the add rule is refused", t);
            if (!flipped && want != 0 && budget == POM_SWEEP_NO_BUDGET)
                return fail("marked ITEs, yet nothing removed", t);
        } else {
            swept++;
            if (memcmp(p, image, POM_ITB_BITMAP_OFF) != 0 ||
                memcmp(p + POM_ITB_ITE_OFF, image + POM_ITB_ITE_OFF, n - POM_ITB_ITE_OFF) != 0)
                return fail("the payload changed outside its bitmap and index", t);
            const bool whole = r.visited == d && (budget == POM_SWEEP_NO_BUDGET || r.dc < budget);
            stopped += !whole;
            if (r.removed > want || (whole && !flipped && r.removed != want) || r.dc < r.removed ||
                r.dc > r.removed + d / 2 || r.len > hdr.ulen || r.visited > d || r.visited == 0 ||
                (uint32_t)r.entries + r.removed != (uint32_t)hdr.entries || steps > (uint32_t)hdr.entries + r.dc - r.removed)
                return fail("removed, dc, the length, visited or the steps", t);
            if (budget != POM_SWEEP_NO_BUDGET && r.visited < d && r.dc < budget)
                return fail("the loop stopped below its budget", t);
            // the table passes the check under its new header, and a second sweep finds nothing up to there
            pom_check_hdr nh = hdr;
            nh.entries = r.entries, nh.max_offset = r.max_offset, nh.pseudo_conflicts = r.pseudo_conflicts;
            nh.itu = r.itu, nh.ulen = r.len;
            pom_check_report rep;
            uint8_t* after = exact_block(r.len - kHeader, p);
            if (itb_check_one(after, r.len - kHeader, adepth, &nh, 0, &rep, nullptr, nullptr) || rep.findings)
                return fail("the table does not pass the check after the sweep", t);
            if (whole) {
                pom_sweep_result again;
                if (itb_sweep_one(after, r.len - kHeader, adepth, nh, POM_SWEEP_NO_BUDGET, 0, true, &again, nullptr) ||
                    again.removed)
                    return fail("a second sweep removed something", t);
            }
            free(after);
        }
        free(p);
        free(q);
        free(image);
    }
    if (swept < 200 || refused < 100 || stopped < 20)
        return fail("too few tables of one kind", swept);
    printf("itb_sweep_check: ok (%u swept, %u of them stopped by the budget, %u refused or unmarked)\n", swept, stopped,
           refused);
    return 0;
}
#endif
