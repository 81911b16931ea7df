// itb_keys_host.cc -- pomegranate_amd/csrc/itb_keys.h on the CPU (never part
// of the product library).
//   libitb_keys_host.so  itb_keys_host(): itb_keys_one over one payload
//                        (itb_keys_host_batch(): over many);
//                        itb_keys_wave_host(): the count kernel's rounds and
//                        the emit kernel's with the header's copy plan
//                        (itb_keys_granule), the 64 lanes one after another
//                        (tests/test_kvlist.py compares both with its oracle)
//   itb_keys_check       (-DITB_KEYS_CHECK) both against a second, naive walk
//                        written below, over directed and seeded random
//                        payloads.  Every payload, every needle and every
//                        output is a heap block of exactly its length at the
//                        residue under test, so a sanitizer build sees any
//                        load at or past a payload's or the needle's end and
//                        any store outside the output.
#include <assert.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "itb_keys.h"

// linear: the failure-table search, else the plain one.
extern "C" int itb_keys_host(const uint8_t* payload, uint32_t n, uint32_t adepth, uint32_t op, const uint8_t* needle,
                             uint32_t needle_len, uint8_t* out, uint64_t cap, uint32_t* live, uint32_t* dnum,
                             uint32_t* bytes, uint32_t* keybytes, uint64_t* mask, int linear)
{
    return linear ? itb_keys_one<true>(payload, n, adepth, op, needle, needle_len, out, cap, live, dnum, bytes, keybytes, mask)
                  : itb_keys_one<false>(payload, n, adepth, op, needle, needle_len, out, cap, live, dnum, bytes, keybytes, mask);
}

// itb_keys_one over `count` payloads, records packed in payload order:
// first[b] = the byte offset of payload b's records, first[count] the total;
// out NULL: counts alone (scripts/kvlist_rate.py: the host walk of its
// decode-and-copy-back path).
extern "C" int itb_keys_host_batch(const uint8_t* const* payload, const uint32_t* n, const uint8_t* adepth,
                                   size_t count, uint32_t op, const uint8_t* needle, uint32_t needle_len,
                                   uint8_t* out, uint64_t cap, uint64_t* first, uint32_t* dnum)
{
    uint64_t at = 0;
    int worst = 0;
    if (!out)
        cap = 0;
    for (size_t b = 0; b < count; b++) {
        uint32_t live, bytes, keybytes;
        first[b] = at;
        const int err = itb_keys_one<true>(payload[b], n[b], adepth[b], op, needle, needle_len,
                                           out + (at < cap ? at : cap), at < cap ? cap - at : 0, &live, &dnum[b],
                                           &bytes, &keybytes, nullptr);
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

// What itb_keys.hip does for one ITB: the count kernel's needle staging,
// rounds and words (mask[16] included), then the emit kernel's rounds off the
// mask, writing out[at, min(at + bytes, out_cap)).
extern "C" int itb_keys_wave_host(const uint8_t* p, uint32_t n, uint32_t adepth, uint32_t op, const uint8_t* needle,
                                  uint32_t needle_len, uint8_t* out, uint64_t at, uint64_t out_cap, uint32_t* live,
                                  uint32_t* dnum, uint32_t* bytes, uint32_t* keybytes, uint64_t* mask, int linear)
{
    *live = *dnum = *bytes = *keybytes = 0;
    for (uint32_t r = 0; r < POM_KV_MASK_WORDS; r++)
        mask[r] = 0;
    uint8_t s_needle[POM_KV_NEEDLE_MAX + 1], s_fail[POM_KV_NEEDLE_MAX + 1];
    uint32_t m = 0;
    if (op >= POM_KV_OP_GREP) {
        for (uint32_t t = 0; t < needle_len; t++)
            s_needle[t] = needle[t];
        m = itb_keys_needle_len(s_needle, needle_len);
        if (linear)
            itb_keys_failure(s_needle, m, s_fail);
    }
    int32_t e = itb_scan_precheck(n, adepth);
    if (e == 0)
        e = itb_scan_live(p, n, adepth, live);
    if (e != 0)
        return e;
    const uint32_t rounds = itb_scan_rounds(adepth);
    uint32_t nd = 0, nb = 0, nk = 0;
    bool bad_key = false, bad_name = false;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t w = itb_scan_word(p, r, adepth);
        for (uint32_t lane = 0; lane < 64; lane++) {
            if (!((w >> lane) & 1u))
                continue;
            const uint32_t nr = 64u * r + lane;
            const itb_keys_entry k = itb_keys_load<false>(p, nr);
            bad_key |= k.bad == POM_KV_E_KEY;
            bad_name |= k.bad == POM_RD_E_NAME;
            if (k.bad)
                continue;
            nk += k.keylen;
            const bool emits = linear ? itb_keys_emits<true>(p, nr, k, op, s_needle, m, s_fail)
                                      : itb_keys_emits<false>(p, nr, k, op, s_needle, m, s_fail);
            if (emits) {
                nd++;
                nb += 4u + k.keylen;
                mask[r] |= 1ull << lane;
            }
        }
    }
    if (bad_key || bad_name) {
        for (uint32_t r = 0; r < POM_KV_MASK_WORDS; r++)
            mask[r] = 0;
        return bad_key ? POM_KV_E_KEY : POM_RD_E_NAME;
    }
    *dnum = nd;
    *bytes = nb;
    *keybytes = nk;
    if (nd == 0 || out_cap == 0)
        return 0;
    const HostOut mem;
    const uint64_t cap_end = (uint64_t)(uintptr_t)out + out_cap;
    for (uint32_t r = 0; r < rounds && at < out_cap; r++) {
        const uint64_t mm = mask[r] & itb_scan_word(p, r, adepth);
        uint64_t w0[64], w1[64], w2[64];
        uint32_t start[64], nr[64], meta[64], cnt = 0, span = 0;
        uint8_t hlen[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            if (!((mm >> lane) & 1u))
                continue;
            const itb_keys_entry k = itb_keys_load<true>(p, 64u * r + lane);
            w0[cnt] = k.head.w0;
            w1[cnt] = k.head.w1;
            w2[cnt] = k.head.w2;
            hlen[cnt] = (uint8_t)k.head.len;
            start[cnt] = span;
            nr[cnt] = 64u * r + lane;
            meta[cnt] = itb_keys_meta(k);
            span += k.head.len + k.memlen;
            cnt++;
        }
        if (cnt == 0)
            continue;
        const uint64_t dst = (uint64_t)(uintptr_t)out + at;
        const itb_keys_round R{w0, w1, w2, start, nr, meta, hlen, cnt, span, p, dst,
                               dst + span < cap_end ? dst + span : cap_end};
        const uint32_t granules = itb_keys_granules(R);
        for (uint32_t g = 0; g < granules; g++)
            itb_keys_granule(mem, R, g);
        at += span;
    }
    return 0;
}

#ifdef ITB_KEYS_CHECK
namespace {

struct Result {
    int err;
    uint32_t live, dnum, keybytes;
    uint64_t mask[16];
    std::vector<uint8_t> bytes;
};

// mds/itb.c:2483-2532 with __readdir_filter bit by bit, with the rules of
// pom_kvlist.h for what the reference leaves undefined.
Result naive(const uint8_t* p, uint32_t n, uint32_t adepth, uint32_t op, const uint8_t* needle, uint32_t needle_len)
{
    Result R{0, 0, 0, 0, {}, {}};
    if (adepth < 1 || adepth > 10) {
        R.err = -22;
        return R;
    }
    if (n < 3712) {
        R.err = -4097;
        return R;
    }
    std::string nd;
    for (uint32_t i = 0; i < needle_len && needle[i]; i++)
        nd.push_back((char)needle[i]);
    bool cut = false, longname = false, longkey = false;
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
        uint32_t flags, klen, namelen;
        int64_t key;
        memcpy(&flags, ite + 24, 4);
        memcpy(&key, ite + 32, 8);
        memcpy(&klen, ite + 40, 4);
        memcpy(&namelen, ite + 20, 4);
        std::string k, hay;
        bool filtered = false;
        if (flags & 0x8000) {
            char buf[128];
            snprintf(buf, 127, "%ld", (long)key);
            k = buf;
            for (uint32_t i = 44; i < 364 && ite[i]; i++)
                hay.push_back((char)ite[i]);
            filtered = true;
        } else if (flags & 0x4000) {
            if (klen > 320) {
                longkey = true;
                continue;
            }
            k.assign((const char*)ite + 44, klen);
            for (uint32_t i = 44 + klen; i < 364 && ite[i]; i++)
                hay.push_back((char)ite[i]);
            filtered = true;
        } else {
            if (namelen > 256) {
                longname = true;
                continue;
            }
            k.assign((const char*)ite + 104, namelen);
        }
        R.keybytes += (uint32_t)k.size();
        if (op >= 2 && filtered && hay.find(nd) == std::string::npos)
            continue;
        R.dnum++;
        R.mask[nr / 64] |= 1ull << (nr % 64);
        const uint32_t len = (uint32_t)k.size();
        for (int i = 0; i < 4; i++)
            R.bytes.push_back((uint8_t)(len >> 8 * i));
        R.bytes.insert(R.bytes.end(), k.begin(), k.end());
    }
    if (cut || longname || longkey) {
        R.err = cut ? -4097 : longkey ? -4101 : -4099;
        R.dnum = R.keybytes = 0;
        memset(R.mask, 0, sizeof R.mask);
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
// outputs at residue `oshift`, whole and under a few caps; the needle in a
// block of its own at residue shift % 8
void check(const std::vector<uint8_t>& image, uint32_t n, uint32_t adepth, uint32_t shift, uint32_t oshift,
           uint32_t op, const std::string& needle, const char* what)
{
    uint8_t* exact = static_cast<uint8_t*>(malloc(n + shift + (n + shift == 0)));
    uint8_t* base = exact + shift;
    if (n)
        memcpy(base, image.data(), n);
    const uint32_t nshift = shift % 8, nlen = (uint32_t)needle.size();
    uint8_t* nexact = static_cast<uint8_t*>(malloc(nlen + nshift + (nlen + nshift == 0)));
    uint8_t* nd = nexact + nshift;
    memcpy(nd, needle.data(), nlen);
    const Result want = naive(base, n, adepth, op, nd, nlen);
    const uint64_t total = want.bytes.size();
    std::vector<uint64_t> caps = {total, 0, 1, 3, 4, 5, 15, 16, 17, total ? total - 1 : 0, total / 2, total / 3 + 7};
    for (uint64_t cap : caps) {
        if (cap > total)
            continue;
        for (int form = 0; form < 4; form++) {
            const int wave = form & 1, linear = form >> 1;
            uint8_t* oexact = static_cast<uint8_t*>(malloc(cap + oshift + (cap + oshift == 0)));
            uint8_t* out = oexact + oshift;
            memset(oexact, 0xA5, cap + oshift);
            uint32_t live = 77, dnum = 77, bytes = 77, keybytes = 77;
            uint64_t mask[16];
            memset(mask, 0x77, sizeof mask);
            const int err = wave ? itb_keys_wave_host(base, n, adepth, op, nd, nlen, out, 0, cap, &live, &dnum, &bytes,
                                                      &keybytes, mask, linear)
                                 : itb_keys_host(base, n, adepth, op, nd, nlen, out, cap, &live, &dnum, &bytes,
                                                 &keybytes, mask, linear);
            bool ok = err == want.err && dnum == want.dnum && bytes == total && keybytes == want.keybytes &&
                      live == (want.err == -22 || n < 3712 ? 0u : want.live) &&
                      memcmp(mask, want.mask, sizeof mask) == 0 &&
                      (cap == 0 || memcmp(out, want.bytes.data(), cap) == 0);
            for (uint32_t i = 0; i < oshift; i++)
                ok = ok && oexact[i] == 0xA5;
            if (!ok) {
                failures++;
                fprintf(stderr, "%s (%s, %s): n=%u adepth=%u shift=%u oshift=%u op=%u needle=%u cap=%llu: err %d/%d "
                        "live %u/%u dnum %u/%u bytes %u/%llu keybytes %u/%u\n", what, wave ? "wave" : "one",
                        linear ? "linear" : "plain", n, adepth, shift, oshift, op, nlen, (unsigned long long)cap, err,
                        want.err, live, want.live, dnum, want.dnum, bytes, (unsigned long long)total, keybytes,
                        want.keybytes);
            }
            free(oexact);
        }
    }
    free(nexact);
    free(exact);
}

void put32(std::vector<uint8_t>& img, uint32_t nr, uint32_t off, uint32_t v)
{
    memcpy(img.data() + 11904 + 512 * nr + off, &v, 4);
}

void put64(std::vector<uint8_t>& img, uint32_t nr, uint32_t off, uint64_t v)
{
    memcpy(img.data() + 11904 + 512 * nr + off, &v, 8);
}

const uint32_t kKlens[] = {0, 1, 3, 4, 5, 11, 12, 13, 255, 256, 319, 320, 24, 40};
const uint32_t kNamelens[] = {0, 1, 15, 16, 17, 255, 256, 7, 33};

// random non-zero bytes everywhere, values over a four-letter alphabet with a
// terminator somewhere (or none); the three kinds mixed
std::vector<uint8_t> random_image(uint32_t density, bool bad = false)
{
    std::vector<uint8_t> img(11904 + 512 * 1024);
    for (auto& b : img)
        b = (uint8_t)(1 + rnd() % 255);
    for (uint32_t i = 0; i < 128; i++) {
        uint8_t v = 0;
        for (int k = 0; k < 8; k++)
            v |= (rnd() % 100 < density) << k;
        img[3584 + i] = v;
    }
    for (uint32_t nr = 0; nr < 1024; nr++) {
        uint8_t* ite = img.data() + 11904 + 512 * nr;
        for (uint32_t i = 44; i < 364; i++)
            ite[i] = (uint8_t)("abAB"[rnd() % 4]);
        if (rnd() % 4)
            ite[44 + rnd() % 320] = 0;
        const uint32_t kind = (uint32_t)(rnd() % 4);
        uint32_t flags = (uint32_t)rnd() & ~0xC000u;
        flags |= kind == 0 ? 0x8000u : kind == 1 ? 0xC000u : kind == 2 ? 0x4000u : 0u;
        put32(img, nr, 24, flags);
        static const uint64_t keys[] = {0, 9, 10, ~0ull, 1ull << 63, ~0ull >> 1, 999999999ull, 1000000000ull,
                                        999999999999999999ull, 1000000000000000000ull};
        put64(img, nr, 32, rnd() % 2 ? keys[rnd() % 10] : rnd() >> (rnd() % 64));
        put32(img, nr, 40, kind == 2 || rnd() % 2 ? kKlens[rnd() % 14] : 1000u + (uint32_t)rnd());
        put32(img, nr, 20, kind == 3 || rnd() % 2 ? kNamelens[rnd() % 9] : 300u + (uint32_t)rnd() % 100000);
        if (bad && rnd() % 300 == 0)
            put32(img, nr, 40, 321 + (uint32_t)(rnd() % 2) * (1u << 20));
        if (bad && rnd() % 300 == 0)
            put32(img, nr, 20, 257);
    }
    return img;
}

void set_bits(std::vector<uint8_t>& img, std::initializer_list<uint32_t> bits)
{
    memset(img.data() + 3584, 0, 128);
    for (uint32_t nr : bits)
        img[3584 + nr / 8] |= 1u << (nr % 8);
}

void set_value(std::vector<uint8_t>& img, uint32_t nr, uint32_t flags, uint32_t klen, const std::string& value)
{
    put32(img, nr, 24, flags);
    put32(img, nr, 40, klen);
    memcpy(img.data() + 11904 + 512 * nr + 44, value.data(), value.size());
}

}  // namespace

int main()
{
    std::vector<uint8_t> img = random_image(50);
    const uint32_t full = (uint32_t)img.size();
    const std::string needles[] = {"", "a", "ab", "abAB", "bbbbbbbb", "aabbaabba", std::string("ab\0cd", 5),
                                   std::string("\0ab", 3), std::string(255, 'a'), "aBaB" + std::string(12, 'b')};
    // adepth with bits above the limit; every payload residue against a moving output residue
    for (uint32_t adepth = 0; adepth <= 12; adepth++)
        for (uint32_t shift = 0; shift < 16; shift++)
            check(img, full, adepth, shift, (5 * shift + adepth) % 16, shift % 4, needles[(shift + adepth) % 10], "adepth");
    // every output residue at one aligned and one odd payload
    for (uint32_t oshift = 0; oshift < 16; oshift++) {
        check(img, 11904 + 512 * 128, 7, 0, oshift, 0, "", "output residue");
        check(img, 11904 + 512 * 128, 7, 3, oshift, 2, "ab", "output residue");
    }
    // cuts around the bitmap, the first ITE, and one byte short of a live ITE's end
    set_bits(img, {0, 5, 63, 64, 200});
    for (uint32_t n : {0u, 1u, 3583u, 3711u, 3712u, 11903u, 11904u, 11904u + 511u, 11904u + 512u,
                       11904u + 512u * 201u - 1u, 11904u + 512u * 201u, 11904u + 512u * 201u + 1u})
        for (uint32_t shift : {0u, 1u, 7u, 8u, 15u})
            check(img, n, 10, shift, shift ^ 9u, 2, "a", "cut");
    // the grep's edges on one STR and one NORMAL entry: matches that end at ITE
    // byte 363, that would need byte 364, behind a terminator, inside the key
    for (uint32_t klen : {0u, 1u, 3u, 4u, 5u, 11u, 12u, 13u, 255u, 256u, 319u, 320u, 321u, 1u << 20})
        for (const std::string& nd : {std::string("xyz"), std::string("x"), std::string(9, 'x'), std::string("")}) {
            set_bits(img, {3, 4, 5});
            const uint32_t m = (uint32_t)nd.size();
            std::string v(320, 'q');
            if (m) {
                v.replace(320 - m, m, nd);                               // ends exactly at byte 363
                if (klen + m <= 320 && klen >= 1)
                    v.replace(klen - 1, m, nd);                          // straddles 44 + klen
            }
            set_value(img, 3, 0x4000, klen, v);
            std::string u(320, 'q');
            if (m > 1)
                u.replace(321 - m, m - 1, nd.substr(0, m - 1));          // would need byte 364 ...
            set_value(img, 4, 0x8000, klen, u);
            if (m)
                img[11904 + 512 * 4 + 364] = (uint8_t)nd[m - 1];          // ... which holds the needle's last byte
            std::string t(320, 'q');
            t[7] = 0;
            if (m)
                t.replace(8, m, nd);                                     // wholly behind a zero byte
            set_value(img, 5, 0xC000, klen, t);
            check(img, full, 10, klen % 16, m % 16, 2, nd, "grep edges");
            check(img, full, 10, (klen + 3) % 16, 1, 3, nd, "grep edges");
        }
    // both errors in one ITB: POM_KV_E_KEY wins, whichever comes first
    set_bits(img, {1, 2, 3});
    set_value(img, 1, 0, 0, "");
    put32(img, 1, 20, 257);
    set_value(img, 2, 0x4000, 321, "");
    set_value(img, 3, 0x8000, 0, "");
    check(img, full, 10, 0, 0, 0, "", "both errors");
    check(img, full, 10, 5, 3, 2, "zz", "both errors");
    set_bits(img, {1, 3});
    check(img, full, 10, 5, 3, 2, "zz", "name error");
    // the restart case, bytes around the terminator, the adversarial value
    set_bits(img, {0, 1, 2});
    set_value(img, 0, 0x8000, 0, std::string("aaab\0", 5));
    set_value(img, 1, 0x8000, 0, std::string("\x01\x7F\x80\xFF\0\x80\x01", 7));
    set_value(img, 2, 0x8000, 0, std::string(320, 'a'));
    for (const std::string& nd : {std::string("aab"), std::string("\x7F\x80"), std::string("\x80\xFF"),
                                  std::string("\xFF\x80"), std::string("\xFF"), std::string("\x80\x01"),
                                  std::string(159, 'a') + "b", std::string(160, 'a')})
        check(img, full, 10, 2, 9, 2, nd, "haystacks");
    // empty, full, single bits, alternating
    img = random_image(50);
    set_bits(img, {});
    check(img, full, 10, 3, 0, 0, "", "empty");
    check(img, 3712, 10, 3, 0, 2, "a", "empty, bitmap only");
    memset(img.data() + 3584, 0xFF, 128);
    check(img, full, 10, 5, 11, 0, "", "full");
    check(img, full, 10, 5, 11, 2, "abA", "full");
    check(img, full - 1, 10, 5, 11, 0, "", "full, one byte short");
    for (uint32_t nr : {0u, 63u, 64u, 1023u}) {
        set_bits(img, {nr});
        check(img, full, 10, nr % 16, 3, 0, "", "single bit");
        check(img, 11904 + 512 * (nr + 1), 10, nr % 16, 3, 2, "b", "single bit, payload ends with its ITE");
        check(img, 11904 + 512 * (nr + 1) - 1, 10, nr % 16, 3, 0, "", "single bit, one byte short");
    }
    memset(img.data() + 3584, 0x55, 128);
    check(img, full, 10, 9, 2, 1, "", "alternating");
    memset(img.data() + 3584, 0xAA, 128);
    check(img, full, 10, 9, 2, 3, "Ab", "alternating");
    // the largest listing: 1,024 STR entries with 320-byte keys; and every decimal length
    memset(img.data() + 3584, 0xFF, 128);
    for (uint32_t nr = 0; nr < 1024; nr++) {
        put32(img, nr, 24, 0x4000);
        put32(img, nr, 40, 320);
    }
    check(img, full, 10, 0, 0, 0, "", "maximum");
    check(img, full, 10, 13, 6, 2, "", "maximum");
    uint64_t pw = 1;
    for (uint32_t nr = 0; nr < 1024; nr++) {
        put32(img, nr, 24, 0x8000);
        const uint64_t v = nr % 4 < 2 ? pw : pw - 1;
        put64(img, nr, 32, nr % 2 ? 0ull - v : v);
        if (nr % 4 == 3)
            pw = pw > ~0ull / 10 ? 1 : pw * 10;
    }
    put64(img, 1000, 32, 1ull << 63);
    put64(img, 1001, 32, ~0ull >> 1);
    put64(img, 1002, 32, ~0ull);
    check(img, full, 10, 4, 7, 0, "", "decimal");
    // seeded random ITBs: density, adepth, length, residues, op and needle all vary
    for (uint32_t t = 0; t < 200; t++) {
        std::vector<uint8_t> r = random_image((uint32_t)(rnd() % 101), t % 3 == 0);
        const uint32_t adepth = 1 + (uint32_t)(rnd() % 10);
        const uint32_t ites = (uint32_t)(rnd() % 1025);
        uint32_t n = 11904 + 512 * ites;
        if (rnd() % 4 == 0)
            n -= (uint32_t)(rnd() % 600);
        check(r, n, adepth, (uint32_t)(rnd() % 16), (uint32_t)(rnd() % 16), (uint32_t)(rnd() % 4), needles[rnd() % 10],
              "random");
    }
    if (failures) {
        fprintf(stderr, "itb_keys_check: %d FAILED\n", failures);
        return 1;
    }
    printf("itb_keys_check: ok\n");
    return 0;
}
#endif
