// itb_find_host.cc -- pomegranate_amd/csrc/itb_find.h on the CPU (never part
// of the product library).
//   libitb_find_host.so  itb_find_host(): itb_find_one and the record for one
//                        request; itb_find_batch_host(): what itb_find.hip does
//                        for a whole call, wave by wave, the 64 lanes one after
//                        another -- with the header's copy plan
//                        (itb_find_granule) where `out` is 16-byte aligned, else
//                        the per-lane byte copy (tests/test_lookup.py compares
//                        both with its oracle; scripts/lookup_rate.py uses the
//                        batch as the host walk of its decode-and-copy-back leg)
//   itb_find_check       (-DITB_FIND_CHECK) both against a second, naive walk
//                        written below, over directed and seeded random
//                        payloads.  Every payload, name blob and output is a
//                        heap block that ends exactly where the data ends, at
//                        the residue under test, so a sanitizer build sees any
//                        load at or past a payload's or the blob's end and any
//                        store outside the output.
#include <assert.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "itb_find.h"

extern "C" int itb_find_host(const uint8_t* payload, uint32_t n, uint32_t adepth, const pom_lookup_req* q,
                             const uint8_t* names, uint32_t names_len, uint32_t* nr, uint32_t* depth, uint8_t* rec)
{
    const int32_t e = itb_find_one(payload, n, adepth, *q, names, names_len, nr, depth);
    itb_find_record_bytes(rec, payload, e == 0 ? POM_ITB_ITE_OFF + (uint64_t)POM_ITE_SIZE * *nr : kItbFindNoIte,
                          itb_find_column_of(*q));
    return e;
}

namespace {

struct HostSpan {
    uint8_t* span;
    void st16(uint32_t o, uint64_t lo, uint64_t hi) const
    {
        assert(((uintptr_t)(span + o) & 15u) == 0);
        memcpy(span + o, &lo, 8);
        memcpy(span + o + 8, &hi, 8);
    }
    void st8(uint32_t o, uint64_t v) const
    {
        assert(((uintptr_t)(span + o) & 7u) == 0);
        memcpy(span + o, &v, 8);
    }
};

}  // namespace

// pom_lookup_dev's arguments in host memory.  per_lane != 0 forces the byte
// copy on an aligned `out` too.
extern "C" int itb_find_batch_host(const uint8_t* payload, const uint64_t* payload_off, const uint32_t* payload_len,
                                   const int32_t* status, const uint8_t* adepth, uint32_t nitb,
                                   const pom_lookup_req* req, uint32_t nreq, const uint8_t* names, uint32_t names_len,
                                   int32_t* err, uint32_t* nr, uint32_t* depth, uint8_t* out, int per_lane)
{
    const bool bytes = per_lane || ((uintptr_t)out & 15u) != 0;
    for (uint32_t r0 = 0; r0 < nreq; r0 += 64) {
        const uint32_t cnt = nreq - r0 < 64u ? nreq - r0 : 64u;
        uint64_t ite_off[64];
        uint32_t col[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            ite_off[lane] = kItbFindNoIte;
            col[lane] = kItbFindNoColumn;
            if (lane >= cnt)
                continue;
            const uint32_t r = r0 + lane;
            const pom_lookup_req q = req[r];
            int32_t e = kItbScanEinval;
            uint32_t hit = 0, d = 0;
            if (q.itb < nitb) {
                e = status ? status[q.itb] : 0;
                if (e == 0) {
                    const uint64_t off = payload_off[q.itb];
                    e = itb_find_one(payload + off, payload_len[q.itb], adepth[q.itb], q, names, names_len, &hit, &d);
                    if (e == 0) {
                        ite_off[lane] = off + POM_ITB_ITE_OFF + (uint64_t)POM_ITE_SIZE * hit;
                        col[lane] = itb_find_column_of(q);
                    }
                }
            }
            err[r] = e;
            nr[r] = hit;
            depth[r] = d;
        }
        uint8_t* span = out + (uint64_t)POM_LK_REC_SIZE * r0;
        if (bytes) {
            for (uint32_t lane = 0; lane < cnt; lane++)
                itb_find_record_bytes(span + POM_LK_REC_SIZE * lane, payload, ite_off[lane], col[lane]);
            continue;
        }
        const HostSpan mem{span};
        const uint32_t granules = itb_find_granules(cnt);
        for (uint32_t g = 0; g < granules; g++)
            itb_find_granule(mem, payload, ite_off, col, cnt, g);
    }
    return 0;
}

#ifdef ITB_FIND_CHECK
namespace {

struct Result {
    int err;
    uint32_t nr, depth;
    uint8_t rec[POM_LK_REC_SIZE];
};

uint32_t rd32(const uint8_t* p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

uint64_t rd64(const uint8_t* p)
{
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

// mds/itb.c:1769-1814 with ite_match, slot by slot and memcmp for the name,
// with the rules of pom_lookup.h for what the reference leaves undefined.
Result naive(const uint8_t* p, uint32_t n, uint32_t adepth, const pom_lookup_req& q, const uint8_t* names,
             uint32_t names_len)
{
    Result R;
    memset(&R, 0, sizeof R);
    R.err = -22;
    if (adepth < 1 || adepth > 10)
        return R;
    R.err = POM_GC_E_TRUNCATED;
    if (n < 11904)
        return R;
    R.err = -22;
    if ((q.flag & ~0x03000053u) || q.namelen > 255 || ((q.flag & 0x40u) && q.column > 5) ||
        (uint64_t)q.name_off + q.namelen > names_len)
        return R;
    uint64_t offset = q.hash & ((1u << adepth) - 1);
    R.err = -2;
    while (offset < 2048) {
        const uint32_t ii = rd32(p + 3712 + 4 * offset);
        const uint32_t entry = ii & 0x7FFF, conflict = (ii >> 15) & 0x7FFF, flag = ii >> 30;
        if (flag == 0)
            break;
        if (R.depth == 2048) {
            R.err = POM_LK_E_LOOP;
            break;
        }
        R.depth++;
        const uint64_t at = 11904 + 512ull * entry;
        if (at + 512 > n) {
            R.err = POM_GC_E_TRUNCATED;
            break;
        }
        const uint8_t* e = p + at;
        const uint32_t state = rd32(e + 16) & 7;
        bool hit = true;
        if ((q.flag & 0x02000000u) && state != 3 && state != 1)
            hit = false;
        else if ((q.flag & 0x01000000u) && state != 0)
            hit = false;
        else if (state == 1 && !(q.flag & 0x02000000u))
            hit = false;
        else if (q.flag & 2u)
            hit = rd64(e + 8) == q.uuid && rd64(e) == q.hash;
        else if (q.flag & 1u)
            hit = rd32(e + 20) == q.namelen && memcmp(e + 104, names + q.name_off, q.namelen) == 0;
        else
            hit = false;
        if (hit) {
            R.err = 0;
            R.nr = entry;
            memcpy(R.rec, e + 8, 8);
            memcpy(R.rec + 8, e + 24, 104);
            if (q.flag & 0x40u)
                memcpy(R.rec + 112, e + 368 + 24 * q.column, 24);
            break;
        }
        if (flag == 1)
            break;
        offset = conflict;
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

// A heap block of shift + n bytes whose last n are `data`: the data ends where
// the block does and starts at residue (16-byte malloc + shift) mod 16.
struct Exact {
    uint8_t* block;
    uint8_t* at;
    Exact(const uint8_t* data, size_t n, size_t shift) : block((uint8_t*)malloc(shift + n + (shift + n == 0))), at(block + shift)
    {
        if (n && data)
            memcpy(at, data, n);
    }
    ~Exact() { free(block); }
    Exact(const Exact&) = delete;
};

void put_slot(std::vector<uint8_t>& img, uint32_t off, uint32_t entry, uint32_t conflict, uint32_t flag)
{
    const uint32_t v = (entry & 0x7FFF) | (conflict & 0x7FFF) << 15 | flag << 30;
    memcpy(&img[3712 + 4 * off], &v, 4);
}

int failures = 0, hits = 0, misses = 0, loops = 0, cuts = 0;

void check_one(const std::vector<uint8_t>& img, uint32_t n, uint32_t adepth, const pom_lookup_req& q,
               const std::vector<uint8_t>& names, uint32_t pshift, uint32_t nshift, const char* what)
{
    const Exact P(img.data(), n, pshift), N(names.data(), names.size(), nshift);
    const Result want = naive(P.at, n, adepth, q, N.at, (uint32_t)names.size());
    hits += want.err == 0;
    misses += want.err == -2;
    loops += want.err == POM_LK_E_LOOP;
    cuts += want.err == POM_GC_E_TRUNCATED;
    Result got;
    memset(&got, 0xA5, sizeof got);
    got.err = itb_find_host(P.at, n, adepth, &q, N.at, (uint32_t)names.size(), &got.nr, &got.depth, got.rec);
    if (got.err != want.err || got.nr != want.nr || got.depth != want.depth ||
        memcmp(got.rec, want.rec, POM_LK_REC_SIZE) != 0) {
        printf("itb_find_check: %s: n=%u adepth=%u flag=%#x: got (%d, %u, %u), want (%d, %u, %u)\n", what, n, adepth,
               q.flag, got.err, got.nr, got.depth, want.err, want.nr, want.depth);
        failures++;
    }
}

// The whole call, as the kernel cuts it into waves, against naive() per request.
void check_batch(const std::vector<uint8_t>& img, uint32_t n, uint32_t adepth, const std::vector<pom_lookup_req>& reqs,
                 const std::vector<uint8_t>& names, uint32_t pshift, uint32_t oshift, int per_lane)
{
    const Exact P(img.data(), n, pshift), N(names.data(), names.size(), 3);
    const uint32_t nreq = (uint32_t)reqs.size();
    const Exact O(nullptr, (size_t)POM_LK_REC_SIZE * nreq, oshift);
    std::vector<int32_t> err(nreq);
    std::vector<uint32_t> nr(nreq), depth(nreq);
    const uint64_t off[2] = {0, 0};
    const uint32_t len[2] = {n, n};
    const int32_t status[2] = {0, -6};
    const uint8_t ad[2] = {(uint8_t)adepth, (uint8_t)adepth};
    itb_find_batch_host(P.at, off, len, status, ad, 2, reqs.data(), nreq, N.at, (uint32_t)names.size(), err.data(),
                        nr.data(), depth.data(), O.at, per_lane);
    for (uint32_t r = 0; r < nreq; r++) {
        Result want = naive(P.at, n, adepth, reqs[r], N.at, (uint32_t)names.size());
        if (reqs[r].itb >= 2) {
            memset(&want, 0, sizeof want);
            want.err = -22;
        } else if (reqs[r].itb == 1) {
            memset(&want, 0, sizeof want);
            want.err = -6;
        }
        if (err[r] != want.err || nr[r] != want.nr || depth[r] != want.depth ||
            memcmp(O.at + (size_t)POM_LK_REC_SIZE * r, want.rec, POM_LK_REC_SIZE) != 0) {
            printf("itb_find_check: batch of %u (out residue %u, per_lane %d): request %u differs\n", nreq, oshift,
                   per_lane, r);
            failures++;
        }
    }
}

}  // namespace

int main()
{
    const uint32_t kFull = 11904 + 512 * 1024;
    std::vector<uint8_t> img(kFull);
    for (int round = 0; round < 40; round++) {
        for (auto& b : img)
            b = (uint8_t)rnd();
        const uint32_t adepth = 1 + rnd() % 10, n_ites = 1 + rnd() % 64;
        const uint32_t n_cut = round % 4 == 0 ? rnd() % 600 : 0;
        const uint32_t n = 11904 + 512 * n_ites - (n_cut < 512 * n_ites ? n_cut : 0);
        // a table of random slots: flags of every kind, entries and conflicts over all 15 bits now and then
        for (uint32_t o = 0; o < 2048; o++) {
            const bool wild = rnd() % 16 == 0;
            put_slot(img, o, wild ? rnd() % 32768 : rnd() % n_ites, wild ? rnd() % 32768 : rnd() % 2048, rnd() % 4);
        }
        // a handful of names, some of them the names of ITEs
        std::vector<uint8_t> names;
        std::vector<pom_lookup_req> reqs;
        std::vector<uint32_t> target;
        for (uint32_t t = 0; t < 150; t++) {
            pom_lookup_req q;
            memset(&q, 0, sizeof q);
            const uint32_t nr = rnd() % n_ites;
            uint8_t* e = &img[11904 + 512 * nr];
            static const uint32_t lens[] = {0, 1, 7, 8, 9, 16, 17, 255};
            q.namelen = (uint16_t)lens[rnd() % 8];
            if (rnd() % 2) {                    // make the ITE agree, fully or up to its last byte
                const uint32_t l = q.namelen;
                memcpy(e + 20, &l, 4);
                const uint32_t state = rnd() % 4;
                uint32_t fl = rd32(e + 16);
                fl = (fl & ~7u) | state;
                memcpy(e + 16, &fl, 4);
            }
            q.name_off = (uint32_t)names.size();
            names.insert(names.end(), e + 104, e + 104 + q.namelen);
            if (q.namelen && rnd() % 4 == 0)
                names.back() ^= 0x40;
            q.hash = rnd() % 3 ? rd64(e) : rnd();
            q.uuid = rd64(e + 8);
            static const uint32_t flags[] = {1, 2, 3, 0x11, 0x41, 0x42, 0x01000001, 0x02000001, 0x03000002, 0, 0x10, 0x81};
            q.flag = flags[rnd() % 12];
            q.column = (uint16_t)(rnd() % 7);
            q.itb = rnd() % 16 == 0 ? (uint32_t)(1 + rnd() % 3) : 0;
            reqs.push_back(q);
            target.push_back(nr);
        }
        // the home slot of every other request leads to its ITE
        for (uint32_t t = 0; t < reqs.size(); t += 2)
            put_slot(img, (uint32_t)reqs[t].hash & ((1u << adepth) - 1u), target[t], rnd() % 2048, 1 + rnd() % 3);
        for (uint32_t t = 0; t < reqs.size(); t++) {
            pom_lookup_req q = reqs[t];
            q.itb = 0;
            check_one(img, n, adepth, q, names, t % 16, (t * 5) % 8, "random");
        }
        // requests whose name lies outside the blob, by one byte and by far
        pom_lookup_req q = reqs[0];
        q.itb = 0;
        q.flag = 1;
        q.namelen = 9;
        q.name_off = (uint32_t)names.size() - 8;
        check_one(img, n, adepth, q, names, 1, 2, "name past the blob");
        q.name_off = 0xFFFFFFFFu;
        check_one(img, n, adepth, q, names, 1, 2, "name far past the blob");
        q.namelen = 0;
        q.name_off = (uint32_t)names.size();
        check_one(img, n, adepth, q, names, 1, 2, "empty name at the blob's end");
        q.namelen = 256;
        q.name_off = 0;
        check_one(img, n, adepth, q, names, 1, 2, "namelen 256");
        for (uint32_t cnt : {1u, 2u, 63u, 64u, 65u, 129u, 150u}) {
            std::vector<pom_lookup_req> some(reqs.begin(), reqs.begin() + cnt);
            check_batch(img, n, adepth, some, names, round % 16, 0, 0);
            check_batch(img, n, adepth, some, names, round % 16, 0, 1);
            check_batch(img, n, adepth, some, names, round % 16, 1 + round % 15, 0);
        }
    }
    // directed: payloads that end inside the index table, right behind it, inside an ITE
    for (auto& b : img)
        b = (uint8_t)rnd();
    for (uint32_t o = 0; o < 2048; o++)
        put_slot(img, o, o % 8, (o + 1) % 2048, 2);         // one cycle through every slot
    std::vector<uint8_t> names(8, 0x11);
    pom_lookup_req q;
    memset(&q, 0, sizeof q);
    q.flag = 1;
    q.namelen = 8;
    for (uint32_t n : {0u, 3712u, 11903u, 11904u, 11904u + 511u, 11904u + 512u, 11904u + 8u * 512u - 1u, 11904u + 8u * 512u})
        for (uint32_t shift : {0u, 1u, 8u, 15u}) {
            q.hash = shift;
            check_one(img, n, 10, q, names, shift, shift % 8, "cut payload, cyclic table");
        }
    // entry 32,767 and a conflict past the table
    put_slot(img, 5, 32767, 6, 2);
    q.hash = 5;
    check_one(img, kFull, 10, q, names, 3, 1, "entry 32767");
    put_slot(img, 5, 1, 2048, 2);
    check_one(img, kFull, 10, q, names, 3, 1, "conflict 2048");
    put_slot(img, 5, 1, 32767, 3);
    check_one(img, kFull, 10, q, names, 3, 1, "conflict 32767");
    // the cases must have reached every outcome
    if (hits < 100 || misses < 100 || loops < 1 || cuts < 10) {
        printf("itb_find_check: thin coverage: %d hits, %d misses, %d loops, %d cut\n", hits, misses, loops, cuts);
        failures++;
    }
    if (failures) {
        printf("itb_find_check: %d failures\n", failures);
        return 1;
    }
    printf("itb_find_check: ok (%d hits, %d misses, %d loops, %d cut)\n", hits, misses, loops, cuts);
    return 0;
}
#endif
