// itb_kvget_host.cc -- pomegranate_amd/csrc/itb_kvget.h on the CPU (never part
// of the product library).
//   libitb_kvget_host.so  itb_kvget_batch_host(): what itb_kvget.hip does for a
//                         whole call -- the find lane after lane, the prefix,
//                         then the emit wave by wave, its 64 lanes one after
//                         another, with the header's granule plan
//                         (itb_kvget_granule) or, per_lane != 0, the per-lane
//                         byte copy (tests/test_kvget.py compares both with its
//                         oracle)
//   itb_kvget_check       (-DITB_KVGET_CHECK) both against a second, naive walk
//                         written below, over directed and seeded random
//                         payloads.  Every payload, key blob and capped output
//                         is a heap block that ends exactly where the data
//                         ends, at the residue under test, so a sanitizer build
//                         sees any load at or past a payload's or the blob's
//                         end and any store outside the output.
#include <assert.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "itb_kvget.h"

namespace {

struct HostOut {
    uint8_t* out;
    void st16(uint64_t o, uint64_t lo, uint64_t hi) const
    {
        assert(((uintptr_t)(out + o) & 15u) == 0);
        memcpy(out + o, &lo, 8);
        memcpy(out + o + 8, &hi, 8);
    }
    void st1(uint64_t o, uint8_t v) const { out[o] = v; }
};

}  // namespace

// pom_kvget_dev's arguments in host memory.
extern "C" int itb_kvget_batch_host(const uint8_t* payload, const uint64_t* payload_off, const uint32_t* payload_len,
                                    const int32_t* status, const uint8_t* adepth, uint32_t nitb,
                                    const pom_kvget_req* req, uint32_t nreq, const uint8_t* keys, uint32_t keys_len,
                                    int32_t* err, uint32_t* nr, uint32_t* depth, uint32_t* len, uint64_t* lease,
                                    uint64_t* first, uint8_t* out, uint64_t out_cap, int per_lane)
{
    // find
    for (uint32_t r = 0; r < nreq; r++) {
        const pom_kvget_req q = req[r];
        int32_t e = kItbScanEinval;
        uint32_t hit = 0, d = 0, ln = 0;
        uint64_t ls = 0;
        if (q.itb < nitb) {
            e = status ? status[q.itb] : 0;
            if (e == 0)
                e = itb_kvget_one(payload + payload_off[q.itb], payload_len[q.itb], adepth[q.itb], q, keys, keys_len,
                                  &hit, &d, &ln, &ls);
        }
        err[r] = e;
        nr[r] = hit;
        depth[r] = d;
        len[r] = ln;
        lease[r] = ls;
    }
    // prefix
    first[0] = 0;
    for (uint32_t r = 0; r < nreq; r++)
        first[r + 1] = first[r] + len[r];
    if (out_cap == 0)
        return 0;
    // emit
    const HostOut mem{out};
    const uint32_t mis = (uint32_t)((uintptr_t)out & 15u);
    for (uint32_t r0 = 0; r0 < nreq; r0 += kItbKvgetWave) {
        const uint32_t cnt = nreq - r0 < kItbKvgetWave ? nreq - r0 : kItbKvgetWave;
        const uint64_t lo = first[r0], hi = first[r0 + cnt];
        if (lo >= hi || lo >= out_cap)
            continue;
        itb_kvget_src src[kItbKvgetWave];
        uint32_t rel[kItbKvgetWave];
        for (uint32_t lane = 0; lane < kItbKvgetWave; lane++) {
            src[lane] = itb_kvget_src{0, 0, kItbKvgetNoColumn};
            rel[lane] = (uint32_t)(hi - lo);
            if (lane >= cnt)
                continue;
            const pom_kvget_req q = req[r0 + lane];
            rel[lane] = (uint32_t)(first[r0 + lane] - lo);
            if (len[r0 + lane])
                src[lane] = itb_kvget_src_of(q, payload_off[q.itb], nr[r0 + lane], len[r0 + lane]);
        }
        if (per_lane) {
            for (uint32_t lane = 0; lane < cnt; lane++)
                itb_kvget_record_bytes(mem, lo + rel[lane], out_cap, payload, src[lane]);
            continue;
        }
        const uint32_t granules = itb_kvget_granules(mis, lo, hi);
        for (uint32_t g = 0; g < granules; g++)
            itb_kvget_granule(mem, payload, rel, src, cnt, mis, lo, hi, out_cap, g);
    }
    return 0;
}

#ifdef ITB_KVGET_CHECK
namespace {

struct Result {
    int err;
    uint32_t nr, depth, len;
    uint64_t lease;
    uint8_t rec[POM_KG_REC_MAX];
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

// mds/itb.c:1769-1814 with the INDEX_KV branch of ite_match, slot by slot and
// memcmp for the key, with the rules of pom_kvget.h for what the reference
// leaves undefined.
Result naive(const uint8_t* p, uint32_t n, uint32_t adepth, const pom_kvget_req& q, const uint8_t* keys,
             uint32_t keys_len)
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
    const bool str = q.kvflag & 0x4000u;
    if ((q.flag & ~0x40000050u) || (q.kvflag & ~0xCFFFu) || ((q.flag & 0x40u) && (q.kvflag & 0xFFFu) > 5) ||
        (str && q.sklen <= 320 && (uint64_t)q.skey_off + q.sklen > keys_len))
        return R;
    uint64_t offset = q.key & ((1u << adepth) - 1);
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
        bool hit = rd64(e + 32) == q.key;
        if (hit && str)
            hit = q.sklen <= 320 && rd32(e + 40) == q.sklen && memcmp(e + 44, keys + q.skey_off, q.sklen) == 0;
        if (hit) {
            const uint32_t vlen = rd32(e + 28);
            if (!(rd32(e + 24) & 0xC000u)) {
                R.err = -22;
            } else if (vlen > 320) {
                R.err = POM_KG_E_VALUE;
            } else {
                R.err = 0;
                R.nr = entry;
                R.len = 20 + vlen;
                R.lease = rd64(e + 80);
                memcpy(R.rec, e + 24, 20 + vlen);
                if (q.flag & 0x40u) {
                    memcpy(R.rec + R.len, e + 368 + 24 * (q.kvflag & 0xFFFu), 24);
                    R.len += 24;
                }
            }
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

int failures = 0, hits = 0, misses = 0, loops = 0, cuts = 0, refused = 0, toolong = 0, capped = 0;

// The whole call against naive() per request; the output is a heap block of
// exactly min(total, cap) bytes at residue oshift.  cap_at: where the cap
// cuts, as a fraction of the total in 1/8 (8: no cut).
void check_batch(const std::vector<uint8_t>& img, uint32_t n, uint32_t adepth, const std::vector<pom_kvget_req>& reqs,
                 const std::vector<uint8_t>& keys, uint32_t pshift, uint32_t kshift, uint32_t oshift, int per_lane,
                 uint32_t cap_at, const char* what)
{
    const Exact P(img.data(), n, pshift), N(keys.data(), keys.size(), kshift);
    const uint32_t nreq = (uint32_t)reqs.size();
    const uint64_t off[2] = {0, 0};
    const uint32_t plen[2] = {n, n};
    const int32_t status[2] = {0, -6};
    const uint8_t ad[2] = {(uint8_t)adepth, (uint8_t)adepth};
    std::vector<Result> want(nreq);
    std::vector<uint8_t> all;
    for (uint32_t r = 0; r < nreq; r++) {
        want[r] = naive(P.at, n, adepth, reqs[r], N.at, (uint32_t)keys.size());
        if (reqs[r].itb >= 2) {
            memset(&want[r], 0, sizeof(Result));
            want[r].err = -22;
        } else if (reqs[r].itb == 1) {
            memset(&want[r], 0, sizeof(Result));
            want[r].err = -6;
        }
        all.insert(all.end(), want[r].rec, want[r].rec + want[r].len);
        if (cap_at == 8 && oshift == 0 && !per_lane) {
            hits += want[r].err == 0;
            misses += want[r].err == -2;
            loops += want[r].err == POM_LK_E_LOOP;
            cuts += want[r].err == POM_GC_E_TRUNCATED;
            refused += want[r].err == -22;
            toolong += want[r].err == POM_KG_E_VALUE;
        }
    }
    const uint64_t total = all.size();
    const uint64_t cap = cap_at >= 8 ? total : total * cap_at / 8 + (cap_at ? 1 : 0);
    const uint64_t room = cap < total ? cap : total;
    capped += cap < total;
    const Exact O(nullptr, room, oshift);
    std::vector<int32_t> err(nreq);
    std::vector<uint32_t> nr(nreq), depth(nreq), len(nreq);
    std::vector<uint64_t> lease(nreq), first(nreq + 1);
    itb_kvget_batch_host(P.at, off, plen, status, ad, 2, reqs.data(), nreq, N.at, (uint32_t)keys.size(), err.data(),
                         nr.data(), depth.data(), len.data(), lease.data(), first.data(), O.at, cap, per_lane);
    uint64_t at = 0;
    for (uint32_t r = 0; r < nreq; r++) {
        if (err[r] != want[r].err || nr[r] != want[r].nr || depth[r] != want[r].depth || len[r] != want[r].len ||
            lease[r] != want[r].lease || first[r] != at) {
            printf("itb_kvget_check: %s: batch of %u (out residue %u, per_lane %d): request %u: got (%d, %u, %u, %u), "
                   "want (%d, %u, %u, %u)\n", what, nreq, oshift, per_lane, r, err[r], nr[r], depth[r], len[r],
                   want[r].err, want[r].nr, want[r].depth, want[r].len);
            failures++;
            return;
        }
        at += want[r].len;
    }
    if (first[nreq] != total || (room && memcmp(O.at, all.data(), room) != 0)) {
        printf("itb_kvget_check: %s: batch of %u (out residue %u, per_lane %d, cap %llu of %llu): records differ\n", what,
               nreq, oshift, per_lane, (unsigned long long)cap, (unsigned long long)total);
        failures++;
    }
}

}  // namespace

int main()
{
    const uint32_t kFull = 11904 + 512 * 1024;
    std::vector<uint8_t> img(kFull);
    static const uint32_t vlens[] = {0, 1, 11, 12, 13, 27, 28, 29, 43, 44, 319, 320, 321};
    static const uint32_t klens[] = {0, 1, 3, 4, 5, 7, 8, 9, 16, 17, 255, 256, 320};
    for (int round = 0; round < 40; round++) {
        for (auto& b : img)
            b = (uint8_t)rnd();
        const uint32_t adepth = 1 + rnd() % 10, n_ites = 1 + rnd() % 64;
        const uint32_t n_cut = round % 4 == 0 ? rnd() % 600 : 0;
        const uint32_t n = 11904 + 512 * n_ites - (n_cut < 512 * n_ites ? n_cut : 0);
        for (uint32_t o = 0; o < 2048; o++) {
            const bool wild = rnd() % 16 == 0;
            put_slot(img, o, wild ? rnd() % 32768 : rnd() % n_ites, wild ? rnd() % 32768 : rnd() % 2048, rnd() % 4);
        }
        for (uint32_t nr = 0; nr < n_ites; nr++) {
            uint8_t* e = &img[11904 + 512 * nr];
            const uint32_t fl = (rd32(e + 24) & ~0xC000u) | (rnd() % 8 ? (rnd() % 2 ? 0x8000u : 0x4000u) : 0u);
            const uint32_t vl = vlens[rnd() % 13], kl = klens[rnd() % 13];
            memcpy(e + 24, &fl, 4);
            memcpy(e + 28, &vl, 4);
            memcpy(e + 40, &kl, 4);
        }
        std::vector<uint8_t> keys;
        std::vector<pom_kvget_req> reqs;
        std::vector<uint32_t> target;
        for (uint32_t t = 0; t < 150; t++) {
            pom_kvget_req q;
            memset(&q, 0, sizeof q);
            const uint32_t nr = rnd() % n_ites;
            const uint8_t* e = &img[11904 + 512 * nr];
            q.key = rnd() % 4 ? rd64(e + 32) : rnd();
            static const uint32_t flags[] = {0x40000010, 0x40000010, 0x40000050, 0x50, 0x10, 0, 0x40000011, 0x40};
            q.flag = flags[rnd() % 8];
            q.kvflag = (rnd() % 2 ? 0x4000u : 0x8000u) | (uint32_t)(rnd() % 7) | (rnd() % 32 == 0 ? 0x1000u : 0u);
            q.sklen = rnd() % 4 ? rd32(e + 40) : klens[rnd() % 13];
            if (rnd() % 32 == 0)
                q.sklen = 321 + (uint32_t)(rnd() % 1000);
            q.skey_off = (uint32_t)keys.size();
            if (q.sklen <= 320) {
                keys.insert(keys.end(), e + 44, e + 44 + q.sklen);
                if (q.sklen && rnd() % 4 == 0)
                    keys[keys.size() - 1 - rnd() % q.sklen] ^= 0x40;
            }
            q.itb = rnd() % 16 == 0 ? (uint32_t)(1 + rnd() % 3) : 0;
            q.reserved = (uint32_t)rnd();
            reqs.push_back(q);
            target.push_back(nr);
        }
        // the home slot of every other request leads to its ITE
        for (uint32_t t = 0; t < reqs.size(); t += 2)
            put_slot(img, (uint32_t)reqs[t].key & ((1u << adepth) - 1u), target[t], rnd() % 2048, 1 + rnd() % 3);
        // string keys outside the blob, by one byte and by far; an empty one at the blob's end
        pom_kvget_req q = reqs[0];
        q.itb = 0;
        q.flag = 0x40000010;
        q.kvflag = 0x4000;
        q.sklen = 9;
        q.skey_off = (uint32_t)keys.size() - 8;
        reqs.push_back(q);
        q.skey_off = 0xFFFFFFFFu;
        reqs.push_back(q);
        q.sklen = 0;
        q.skey_off = (uint32_t)keys.size();
        reqs.push_back(q);
        q.sklen = 321;                  // matches nothing, and the blob is not read
        q.skey_off = 0xFFFFFFFFu;
        reqs.push_back(q);
        for (uint32_t cnt : {1u, 2u, 63u, 64u, 65u, 129u, (uint32_t)reqs.size()}) {
            std::vector<pom_kvget_req> some(reqs.end() - cnt, reqs.end());
            for (int per_lane = 0; per_lane < 2; per_lane++) {
                check_batch(img, n, adepth, some, keys, round % 16, round % 8, 0, per_lane, 8, "random");
                check_batch(img, n, adepth, some, keys, round % 16, (round + 3) % 8, 1 + round % 15, per_lane, 8, "random");
                check_batch(img, n, adepth, some, keys, (round + 5) % 16, 1, 8, per_lane, 1 + round % 7, "capped");
                check_batch(img, n, adepth, some, keys, 0, 0, round % 16, per_lane, 0, "cap 0");
            }
        }
    }
    // directed: payloads that end inside the index table, right behind it, inside an ITE
    for (auto& b : img)
        b = (uint8_t)rnd();
    for (uint32_t o = 0; o < 2048; o++)
        put_slot(img, o, o % 8, (o + 1) % 2048, 2);         // one cycle through every slot
    std::vector<uint8_t> keys(8, 0x11);
    pom_kvget_req q;
    memset(&q, 0, sizeof q);
    q.flag = 0x40000010;
    q.kvflag = 0x4000;
    q.sklen = 8;
    for (uint32_t n : {0u, 3712u, 11903u, 11904u, 11904u + 511u, 11904u + 512u, 11904u + 8u * 512u - 1u, 11904u + 8u * 512u})
        for (uint32_t shift : {0u, 1u, 8u, 15u}) {
            q.key = shift;
            check_batch(img, n, 10, {q}, keys, shift, shift % 8, 0, 0, 8, "cut payload, cyclic table");
        }
    // the cases must have reached every outcome
    if (hits < 100 || misses < 100 || loops < 1 || cuts < 10 || refused < 50 || toolong < 1 || capped < 50) {
        printf("itb_kvget_check: thin coverage: %d hits, %d misses, %d loops, %d cut, %d refused, %d too long, %d capped\n",
               hits, misses, loops, cuts, refused, toolong, capped);
        failures++;
    }
    if (failures) {
        printf("itb_kvget_check: %d failures\n", failures);
        return 1;
    }
    printf("itb_kvget_check: ok (%d hits, %d misses, %d loops, %d cut, %d refused, %d too long, %d capped)\n", hits, misses,
           loops, cuts, refused, toolong, capped);
    return 0;
}
#endif
