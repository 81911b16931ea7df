// itb_split_host.cc -- pomegranate_amd/csrc/itb_split.h on the CPU (never part
// of the product library).
//   libitb_split_host.so  itb_split_host(): itb_split_one over one payload;
//                         itb_split_batch_host(): a call as pom_itb_split_dev
//                         sees it, status and split_depth rules included
//                         (tests/test_itb_split.py compares both with its
//                         oracle)
//   itb_split_check       (-DITB_SPLIT_CHECK) itb_split_one over seeded tables
//                         built by the header's own add rule, and over the
//                         same tables with a few words flipped.  Payload and
//                         new payload are heap blocks of exactly their
//                         lengths, so a sanitizer build sees any access past
//                         either; whatever the table holds, an error leaves
//                         both untouched, and a split leaves two tables the
//                         check passes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "itb_split.h"

extern "C" int itb_split_host(uint8_t* payload, uint32_t n, uint32_t adepth, const pom_check_hdr* hdr, uint32_t sd,
                              uint64_t payload_off, uint64_t new_off, uint8_t* new_payload, uint32_t new_cap,
                              pom_split_result* result, uint32_t* steps)
{
    return itb_split_one(payload, n, adepth, *hdr, sd, payload_off, new_off, new_payload, new_cap, result, steps);
}

extern "C" void itb_split_batch_host(uint8_t* payload, const uint64_t* payload_off, const uint32_t* payload_len,
                                     const int32_t* status, const uint8_t* adepth, const pom_check_hdr* hdr,
                                     const uint8_t* split_depth, uint32_t nitb, uint8_t* new_payload,
                                     const uint64_t* new_off, const uint32_t* new_cap, pom_split_result* result,
                                     uint32_t* steps)
{
    for (uint32_t b = 0; b < nitb; b++) {
        if (status && status[b] != 0) {
            result[b] = pom_split_result{};
            result[b].err = status[b];
            steps[b] = 0;
            continue;
        }
        const uint32_t sd = split_depth ? split_depth[b] : (uint32_t)hdr[b].depth + 1u;
        itb_split_one(payload + payload_off[b], payload_len[b], adepth[b], hdr[b], sd, payload_off[b], new_off[b],
                      new_payload + new_off[b], new_cap[b], &result[b], &steps[b]);
    }
}

#ifdef ITB_SPLIT_CHECK
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
    fprintf(stderr, "itb_split_check: table %u: %s\n", t, what);
    return 1;
}

uint8_t* exact_block(uint32_t n, const uint8_t* image, int fill)
{
    void* block = nullptr;
    if (posix_memalign(&block, 16, n ? n : 16) != 0)
        abort();
    if (image)
        memcpy(block, image, n);
    else
        memset(block, fill, n);
    return static_cast<uint8_t*>(block);
}

}  // namespace

int main()
{
    unsigned split = 0, refused = 0;
    static itb_split_state B;
    for (unsigned t = 0; t < 600; t++) {
        const uint32_t adepth = 1 + rnd() % 10, d = 1u << adepth;
        const uint32_t m = t % 11 == 0 ? d : (uint32_t)(rnd() % (d + 1));
        const uint32_t narrow = rnd() % 2 ? d : (d / 4 ? d / 4 : 1);
        const uint32_t n = POM_ITB_ITE_OFF + POM_ITE_SIZE * m;
        // the table, by __itb_add_index's rule: B's new side is the builder
        memset(&B, 0, sizeof B);
        uint8_t* image = static_cast<uint8_t*>(malloc(n));
        for (uint32_t i = 0; i < n; i++)
            image[i] = (uint8_t)rnd();
        memset(image + POM_ITB_BITMAP_OFF, 0, POM_ITB_ITE_OFF - POM_ITB_BITMAP_OFF);
        for (uint32_t nr = 0; nr < m; nr++) {
            const uint64_t hash = (rnd() % narrow) | (rnd() % 2) << 10 | (rnd() << 12);
            memcpy(image + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr, &hash, 8);
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
        uint32_t want = 0;
        for (uint32_t nr = 0; nr < m; nr++) {
            uint64_t hash;
            memcpy(&hash, image + POM_ITB_ITE_OFF + POM_ITE_SIZE * nr, 8);
            want += (image[POM_ITB_BITMAP_OFF + nr / 8] >> (nr % 8) & 1u) && itb_split_moves(hash, 1);
        }

        uint32_t cap = n;
        if (t % 13 == 5 && want)
            cap = POM_ITB_ITE_OFF + POM_ITE_SIZE * want - 1;
        uint8_t* p = exact_block(n, image, 0);
        uint8_t* np = exact_block(cap, nullptr, 0x5A);
        pom_split_result r;
        uint32_t steps = 0;
        const int32_t err = itb_split_one(p, n, adepth, hdr, 1, 0, 0, np, cap, &r, &steps);
        if (err != r.err)
            return fail("the return value is not result.err", t);
        bool np_untouched = true;
        for (uint32_t i = 0; i < cap; i++)
            np_untouched &= np[i] == 0x5A;
        if (err != 0 || r.moved == 0) {
            refused++;
            if (memcmp(p, image, n) != 0 || !np_untouched)
                return fail("nothing is produced, yet a payload changed", t);
            if (r.old_len || r.new_len || r.old_entries || r.new_entries)
                return fail("nothing is produced, yet the result is not zero", t);
            if (!flipped && cap == n && err != 0)
                return fail("a table built by the add rule is refused", t);
            if (cap != n && err != kItbSplitOverrun && !flipped)
                return fail("a capacity one byte short is not refused", t);
        } else {
            split++;
            if (memcmp(p, image, POM_ITB_BITMAP_OFF) != 0 ||
                memcmp(p + POM_ITB_ITE_OFF, image + POM_ITB_ITE_OFF, n - POM_ITB_ITE_OFF) != 0)
                return fail("O changed outside its bitmap and index", t);
            if (r.moved != want || r.new_len != POM_ITB_SIZE + POM_ITE_SIZE * r.moved || r.old_len > hdr.ulen ||
                r.new_len > hdr.ulen || steps > (uint32_t)hdr.entries + r.moved + 1u)
                return fail("moved, the lengths or the steps", t);
            for (uint32_t i = r.new_len - kHeader; i < cap; i++)
                if (np[i] != 0x5A)
                    return fail("N is written past new_len - 264", t);
            // both halves pass the check, kind 15 included
            pom_check_hdr oh = hdr, nh = hdr;
            oh.depth = nh.depth = 1;
            nh.itbid = 1;
            oh.entries = r.old_entries, oh.max_offset = r.old_max_offset, oh.pseudo_conflicts = r.old_pseudo;
            oh.itu = r.old_itu, oh.ulen = r.old_len;
            nh.entries = r.new_entries, nh.max_offset = r.new_max_offset, nh.pseudo_conflicts = r.new_pseudo;
            nh.inf = r.new_inf, nh.itu = r.new_itu, nh.ulen = r.new_len;
            pom_check_report rep;
            uint8_t* oo = exact_block(r.old_len - kHeader, p, 0);
            uint8_t* nn = exact_block(r.new_len - kHeader, np, 0);
            if (itb_check_one(oo, r.old_len - kHeader, adepth, &oh, POM_CK_ITBID, &rep, nullptr, nullptr) ||
                rep.findings)
                return fail("O does not pass the check after the split", t);
            if (itb_check_one(nn, r.new_len - kHeader, adepth, &nh, POM_CK_ITBID, &rep, nullptr, nullptr) ||
                rep.findings || rep.live != r.moved)
                return fail("N does not pass the check", t);
            free(oo);
            free(nn);
        }
        free(p);
        free(np);
        free(image);
    }
    if (split < 200 || refused < 100)
        return fail("too few tables of one kind", split);
    printf("itb_split_check: ok (%u split, %u refused or unmoved)\n", split, refused);
    return 0;
}
#endif
