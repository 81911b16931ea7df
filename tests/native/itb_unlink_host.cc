// itb_unlink_host.cc -- pomegranate_amd/csrc/itb_unlink.h on the CPU (never part
// of the product library).
//   libitb_unlink_host.so  itb_unlink_batch_host(): a call as
//                          pom_itb_unlink_dev sees it, status, grouping and
//                          order included, in the reference's form or as the
//                          kernel's rounds; itb_unlink_ite_host(): the pure
//                          ite_unlink arithmetic (tests/test_unlink.py
//                          compares both with its oracle)
//   itb_unlink_check       (-DITB_UNLINK_CHECK) both forms over seeded tables
//                          built by the split header's add rule, with seeded
//                          request lists by uuid, and over the same tables
//                          with a few words flipped.  A payload is a heap
//                          block of exactly its length, so a sanitizer build
//                          sees any access past it; whatever the table holds,
//                          an error leaves it untouched, both forms agree in
//                          every byte, and what is produced passes the check
//                          under its new header.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "itb_unlink.h"

extern "C" void itb_unlink_ite_host(uint32_t flag, uint32_t mode, uint32_t nlink, int async, uint32_t* out)
{
    const itb_unlink_step s = itb_unlink_ite(flag, mode, nlink, async != 0);
    out[0] = s.flag;
    out[1] = s.nlink;
    out[2] = s.what;
}

extern "C" void itb_unlink_batch_host(uint8_t* payload, const uint64_t* payload_off, const uint32_t* payload_len,
                                      const int32_t* status, const uint8_t* adepth, const pom_check_hdr* hdr,
                                      uint32_t nitb, int async, const pom_lookup_req* req, const uint32_t* req_first,
                                      const uint8_t* names, uint32_t names_len, int parts, int32_t* err, uint32_t* nr,
                                      uint32_t* depth, uint32_t* what, uint8_t* out, pom_unlink_result* result)
{
    for (uint32_t b = 0; b < nitb; b++) {
        const uint32_t r0 = req_first[b], cnt = req_first[b + 1] - r0;
        if (status && status[b] != 0) {
            result[b] = pom_unlink_result{};
            result[b].err = status[b];
            for (uint32_t r = r0; r < r0 + cnt; r++) {
                err[r] = req[r].itb != b ? kItbScanEinval : status[b];
                nr[r] = depth[r] = what[r] = 0;
                itb_unlink_put_record(out + POM_LK_REC_SIZE * r, nullptr);
            }
            continue;
        }
        itb_unlink_one(payload + payload_off[b], payload_len[b], adepth[b], hdr[b], async != 0, payload_off[b], b,
                       req + r0, cnt, names, names_len, parts != 0, err + r0, nr + r0, depth + r0, what + r0,
                       out + POM_LK_REC_SIZE * r0, &result[b]);
    }
}

#ifdef ITB_UNLINK_CHECK
namespace {

constexpr uint32_t kHeader = POM_ITB_SIZE - POM_ITB_ITE_OFF;    // sizeof(struct itbh)

uint64_t rng_state = 0xD1B54A32D192ED03ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int fail(const char* what, unsigned t)
{
    fprintf(stderr, "itb_unlink_check: table %u: %s\n", t, what);
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
    unsigned changed = 0, refused = 0, deleted = 0;
    static itb_split_state B;
    static const uint32_t kinds[] = {POM_ITE_FLAG_NORMAL, POM_ITE_FLAG_NORMAL | POM_ITE_FLAG_SDT, POM_ITE_FLAG_SYM,
                                     POM_ITE_FLAG_LS, POM_ITE_FLAG_KV, POM_ITE_FLAG_KV | POM_ITE_FLAG_SDT, 0u,
                                     POM_ITE_FLAG_NORMAL | POM_ITE_FLAG_KV};
    for (unsigned t = 0; t < 600; t++) {
        const uint32_t adepth = 1 + rnd() % 10, d = 1u << adepth;
        const uint32_t m = t % 11 == 0 ? d : (uint32_t)(rnd() % (d + 1));
        const uint32_t narrow = rnd() % 2 ? d : (d / 4 ? d / 4 : 1);
        const uint32_t n = POM_ITB_ITE_OFF + POM_ITE_SIZE * m;
        memset(&B, 0, sizeof B);
        uint8_t* image = static_cast<uint8_t*>(malloc(n));
        for (uint32_t i = 0; i < n; i++)
            image[i] = (uint8_t)rnd();
        memset(image + POM_ITB_BITMAP_OFF, 0, POM_ITB_ITE_OFF - POM_ITB_BITMAP_OFF);
        for (uint32_t i = 0; i < m; i++) {
            const uint64_t hash = (rnd() % narrow) | (rnd() << 12), uuid = 1000 + i;
            uint8_t* ite = image + POM_ITB_ITE_OFF + POM_ITE_SIZE * i;
            const uint32_t flag = kinds[rnd() % 8] | (uint32_t)(rnd() % 4 == 0 ? rnd() % 8 : 0);
            const uint16_t nlink = (uint16_t)(rnd() % 4), mode = (uint16_t)(rnd() % 3 ? 0100644 : 0040755);
            memcpy(ite + POM_ITE_HASH_OFF, &hash, 8);
            memcpy(ite + POM_ITE_UUID_OFF, &uuid, 8);
            memcpy(ite + POM_ITE_FLAG_OFF, &flag, 4);
            memcpy(ite + POM_ITE_MODE_OFF, &mode, 2);
            memcpy(ite + POM_ITE_NLINK_OFF, &nlink, 2);
            B.info[i] = (uint16_t)(hash & (d - 1u));
            if (!itb_split_add(B, d, i))
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
        // the requests: live ITEs by uuid (some twice), a miss now and then
        const uint32_t nreq = 1 + (uint32_t)(rnd() % 24);
        pom_lookup_req req[24] = {};
        for (uint32_t r = 0; r < nreq; r++) {
            const uint32_t i = m ? (uint32_t)(rnd() % m) : 0;
            const uint8_t* ite = image + POM_ITB_ITE_OFF + POM_ITE_SIZE * i;
            if (m)
                memcpy(&req[r].hash, ite + POM_ITE_HASH_OFF, 8);
            req[r].uuid = rnd() % 8 ? 1000 + i : 7;
            req[r].flag = POM_LK_BY_UUID | (rnd() % 4 == 0 ? POM_LK_ITE_SHADOW : 0u) | (rnd() % 2 ? POM_UL_UNLINK : 0u);
        }
        const bool flipped = t % 3 == 2;
        if (flipped)
            for (uint32_t k = 0; k < 1 + rnd() % 3; k++)
                image[POM_ITB_BITMAP_OFF + rnd() % (128 + 8 * d)] ^= (uint8_t)(1u << (rnd() % 8));
        const bool async = rnd() % 2;

        uint8_t* p = exact_block(n, image);
        uint8_t* q = exact_block(n, image);
        pom_unlink_result r, rq;
        int32_t err[2][24];
        uint32_t nr[2][24], depth[2][24], what[2][24];
        static uint8_t out[2][24 * POM_LK_REC_SIZE];
        const int32_t e = itb_unlink_one(p, n, adepth, hdr, async, 0, 0, req, nreq, nullptr, 0, false, err[0], nr[0],
                                         depth[0], what[0], out[0], &r);
        const int32_t eq = itb_unlink_one(q, n, adepth, hdr, async, 0, 0, req, nreq, nullptr, 0, true, err[1], nr[1],
                                          depth[1], what[1], out[1], &rq);
        if (e != r.err || eq != rq.err)
            return fail("the return value is not result.err", t);
        if (memcmp(&r, &rq, sizeof r) != 0 || memcmp(p, q, n) != 0 || memcmp(err[0], err[1], 4 * nreq) != 0 ||
            memcmp(nr[0], nr[1], 4 * nreq) != 0 || memcmp(depth[0], depth[1], 4 * nreq) != 0 ||
            memcmp(what[0], what[1], 4 * nreq) != 0 || memcmp(out[0], out[1], POM_LK_REC_SIZE * nreq) != 0)
            return fail("the reference's form and the rounds disagree", t);
        if (e != 0 || r.changed == 0) {
            refused++;
            if (memcmp(p, image, n) != 0)
                return fail("nothing is produced, yet the payload changed", t);
            if (r.removed || r.len || r.entries || r.max_offset || r.pseudo_conflicts || r.itu)
                return fail("nothing is produced, yet the result is not zero", t);
            if (!flipped && e != 0)
                return fail("a table built by the add rule is refused", t);
        } else {
            changed++;
            deleted += r.removed;
            if (memcmp(p, image, POM_ITB_BITMAP_OFF) != 0)
                return fail("the lock region changed", t);
            for (uint32_t i = 0; i < m; i++) {
                const uint32_t at = POM_ITB_ITE_OFF + POM_ITE_SIZE * i;
                if (memcmp(p + at, image + at, 16) != 0 || memcmp(p + at + 20, image + at + 20, 18) != 0 ||
                    memcmp(p + at + 40, image + at + 40, POM_ITE_SIZE - 40) != 0)
                    return fail("an ITE changed outside its flag and nlink", t);
            }
            if ((async && r.removed > r.changed) || (uint32_t)r.entries + r.removed != (uint32_t)hdr.entries ||
                r.len > hdr.ulen || r.hits > nreq || r.changed > r.hits)
                return fail("changed, removed, the length or hits", t);
            pom_check_hdr nh = hdr;
            nh.entries = r.entries, nh.max_offset = r.max_offset, nh.pseudo_conflicts = r.pseudo_conflicts;
            nh.itu = r.itu, nh.ulen = r.len;
            pom_check_report rep;
            uint8_t* after = exact_block(r.len - kHeader, p);
            if (itb_check_one(after, r.len - kHeader, adepth, &nh, 0, &rep, nullptr, nullptr) || rep.findings)
                return fail("the table does not pass the check after the unlinks", t);
            free(after);
        }
        free(p);
        free(q);
        free(image);
    }
    if (changed < 200 || refused < 100 || deleted < 200)
        return fail("too few tables of one kind", changed);
    printf("itb_unlink_check: ok (%u changed, %u ITEs deleted, %u refused or untouched)\n", changed, deleted, refused);
    return 0;
}
#endif
