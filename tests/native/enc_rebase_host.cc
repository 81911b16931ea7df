// enc_rebase_host.cc -- pomegranate_amd/csrc/lzo1x_enc_rebase.h on the CPU
// (never part of the product library).
//   libenc_rebase_host.so  enc_rebase_{top,due,target,pair,live8}_host(): the
//                          header's functions one by one;
//                          enc_rebase_sweep_host(): the encoder's window walk
//                          (ip from 4 in steps, a re-base wherever one is
//                          due) over a range of block sizes, with what
//                          tests/test_enc_rebase.py asserts counted up
//   enc_rebase_check       (-DENC_REBASE_CHECK) the same walk over a model
//                          dictionary of real u16 entries in a heap block of
//                          exactly its size: every entry the reference could
//                          still accept survives a re-base exactly, every
//                          cleared one lay more than M4_MAX_OFFSET back, and
//                          the bitmap bytes say which are left
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "lzo1x_enc_rebase.h"

namespace {

uint64_t xorshift(uint64_t& s)
{
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

// The step from one window to the next: mode 0 a fixed step `param`; mode 1
// random steps of 1..64 (seed `param`); mode 2 the cycle 1, 2, .., 70 (a step
// past 64 is a match running out of its window).
struct Stepper {
    uint32_t mode, param, k;
    uint64_t s;
    Stepper(uint32_t mode_, uint32_t param_)
        : mode(mode_), param(param_), k(0), s(0x9E3779B97F4A7C15ull ^ ((uint64_t)param_ << 17))
    {
    }
    uint32_t next()
    {
        if (mode == 0)
            return param;
        if (mode == 1)
            return 1 + (uint32_t)(xorshift(s) % 64);
        k = k % 70 + 1;
        return k;
    }
};

}  // namespace

extern "C" {

struct enc_rebase_sweep {
    uint64_t windows;           // windows walked
    uint64_t rebases;           // re-bases in all
    uint64_t bad_fit;           // windows whose highest storable position did not fit after the decision
    uint64_t bad_target;        // re-bases with nb > ip - 0xC000, nb < base, or a position below the base
    uint32_t n_first_rebased;   // the smallest block size that re-based (0: none did)
    uint32_t min_gap;           // the smallest distance between two re-bases of a block (0xFFFFFFFF: none)
    uint32_t last_window_top;   // of the last block: the highest storable position of its last window
    uint32_t last_rebases;      // of the last block: its re-bases
};

uint32_t enc_rebase_top_host(uint32_t ip, uint32_t ip_end) { return enc_rebase_top(ip, ip_end); }
int enc_rebase_due_host(uint32_t ip, uint32_t ip_end, uint32_t base) { return enc_rebase_due(ip, ip_end, base); }
uint32_t enc_rebase_target_host(uint32_t ip) { return enc_rebase_target(ip); }
uint32_t enc_rebase_pair_host(uint32_t pair, uint32_t delta) { return enc_rebase_pair(pair, delta); }
uint32_t enc_rebase_live8_host(const uint32_t* pairs) { return enc_rebase_live8(pairs); }

// Blocks of n_lo, n_lo + n_step, .. <= n_hi bytes (n >= 14), each walked as
// parse_wave walks it; at the first window at or past jump_at the step is
// jump_len instead (0: no such jump).
void enc_rebase_sweep_host(uint32_t n_lo, uint32_t n_hi, uint32_t n_step, uint32_t mode, uint32_t param,
                           uint32_t jump_at, uint32_t jump_len, enc_rebase_sweep* r)
{
    memset(r, 0, sizeof *r);
    r->min_gap = 0xFFFFFFFFu;
    for (uint64_t n64 = n_lo; n64 <= n_hi; n64 += n_step) {
        const uint32_t n = (uint32_t)n64, ip_end = n - 13;
        Stepper st(mode, param);
        uint32_t base = 0, rebases = 0, last_at = 0, top = 0;
        bool jumped = jump_len == 0;
        for (uint32_t ip = 4; ip < ip_end;) {
            if (enc_rebase_due(ip, ip_end, base)) {
                const uint32_t nb = enc_rebase_target(ip);
                if (ip < ENC_REBASE_BACK || nb > ip - ENC_REBASE_BACK || nb < base)
                    r->bad_target++;
                if (rebases && ip - last_at < r->min_gap)
                    r->min_gap = ip - last_at;
                last_at = ip;
                base = nb;
                rebases++;
            }
            top = enc_rebase_top(ip, ip_end);
            if (ip < base)
                r->bad_target++;
            if ((uint64_t)top - base + 1 > ENC_REBASE_VMAX || top >= ip_end || top < ip)
                r->bad_fit++;
            r->windows++;
            uint32_t step = st.next();
            if (!jumped && ip >= jump_at) {
                step = jump_len;
                jumped = true;
            }
            if (step >= ip_end - ip)
                break;
            ip += step;
        }
        r->rebases += rebases;
        if (rebases && !r->n_first_rebased)
            r->n_first_rebased = n;
        r->last_window_top = top;
        r->last_rebases = rebases;
    }
}

}  // extern "C"

#ifdef ENC_REBASE_CHECK
namespace {

constexpr uint32_t kSlots = 1u << 14;
constexpr uint32_t kM4MaxOffset = 0xBFFF;
int failures = 0;

void fail(const char* what, uint32_t n, uint32_t ip, uint32_t slot)
{
    if (failures++ < 20)
        fprintf(stderr, "enc_rebase_check: %s (n %u, ip %u, slot %u)\n", what, n, ip, slot);
}

// One block: every window stores a few of its positions in pseudo-random
// slots; truth[] keeps the positions themselves.  occ is the written-slots
// bitmap as the device keeps it, refreshed at every re-base.
void model_block(uint32_t n, uint32_t mode, uint32_t param, uint32_t jump_at, uint32_t jump_len)
{
    uint16_t* dict = static_cast<uint16_t*>(malloc(kSlots * sizeof(uint16_t)));
    uint32_t* truth = static_cast<uint32_t*>(calloc(kSlots, sizeof(uint32_t)));
    uint8_t* occ = static_cast<uint8_t*>(calloc(kSlots / 8, 1));
    uint64_t s = 0xD1B54A32D192ED03ull + n;
    for (uint32_t i = 0; i < kSlots; i++)
        dict[i] = (uint16_t)xorshift(s);                 // an earlier block's garbage
    const uint32_t ip_end = n - 13;
    Stepper st(mode, param);
    uint32_t base = 0;
    bool jumped = jump_len == 0;
    for (uint32_t ip = 4; ip < ip_end;) {
        if (enc_rebase_due(ip, ip_end, base)) {
            const uint32_t nb = enc_rebase_target(ip), delta = nb - base;
            for (uint32_t c = 0; c < kSlots / 8; c++) {
                if (!occ[c])
                    continue;                            // (neither loaded nor stored)
                uint32_t w[4];
                memcpy(w, dict + 8 * c, 16);
                for (int i = 0; i < 4; i++)
                    w[i] = enc_rebase_pair(w[i], delta);
                memcpy(dict + 8 * c, w, 16);
                occ[c] = (uint8_t)(enc_rebase_live8(w) & occ[c]);
            }
            base = nb;
            for (uint32_t slot = 0; slot < kSlots; slot++) {
                const bool written = (occ[slot >> 3] >> (slot & 7)) & 1;
                const uint32_t e = written ? dict[slot] : 0u;
                const uint32_t pos = truth[slot];            // 0: never written (positions are >= 4)
                if (pos && ip - pos <= kM4MaxOffset) {
                    if (!e || base + e - 1 != pos)
                        fail("an entry within M4_MAX_OFFSET did not survive exactly", n, ip, slot);
                } else if (e && (!pos || base + e - 1 != pos))
                    fail("a surviving entry is not the slot's last position", n, ip, slot);
                if (written && !dict[slot])
                    fail("a cleared entry kept its bitmap bit", n, ip, slot);
            }
        }
        const uint32_t top = enc_rebase_top(ip, ip_end);
        for (uint32_t p = ip; p <= top; p += 1 + (uint32_t)(xorshift(s) % 5)) {
            const uint32_t slot = (uint32_t)(xorshift(s) % kSlots);
            const uint32_t v = p - base + 1;
            if (v == 0 || v > ENC_REBASE_VMAX)
                fail("a stored value does not fit", n, ip, slot);
            dict[slot] = (uint16_t)v;
            truth[slot] = p;
            occ[slot >> 3] |= (uint8_t)(1u << (slot & 7));
        }
        uint32_t step = st.next();
        if (!jumped && ip >= jump_at) {
            step = jump_len;
            jumped = true;
        }
        if (step >= ip_end - ip)
            break;
        ip += step;
    }
    free(dict);
    free(truth);
    free(occ);
}

}  // namespace

int main()
{
    // the packed pairs against per-entry arithmetic, at the edges of delta
    for (uint32_t delta : {0u, 1u, 2u, 0x3FFFu, 0x7FFFu, 0x8000u, 0xFFFEu, 0xFFFFu, 0x10000u, 0x12345u, 0xFFFFFFFFu})
        for (uint32_t a : {0u, 1u, 2u, 0x3FFFu, 0x4000u, 0x7FFFu, 0x8000u, 0xFFFEu, 0xFFFFu})
            for (uint32_t b : {0u, 1u, 0x8000u, 0xFFFFu}) {
                const uint32_t got = enc_rebase_pair(a | b << 16, delta);
                const uint32_t wa = a > delta ? a - delta : 0, wb = b > delta ? b - delta : 0;
                if (got != (wa | wb << 16))
                    fail("enc_rebase_pair", delta, a, b);
            }
    for (uint32_t m = 0; m < 256; m++) {
        uint32_t w[4];
        for (int i = 0; i < 4; i++)
            w[i] = ((m >> (2 * i)) & 1 ? 0x0001u + m : 0u) | ((m >> (2 * i + 1)) & 1 ? 0x80000000u >> (m & 15) : 0u);
        if (enc_rebase_live8(w) != m)
            fail("enc_rebase_live8", m, 0, 0);
    }
    // the model dictionary: sizes around the first re-base, long blocks, all step modes, a long jump
    for (uint32_t n : {65535u, 65548u, 65549u, 65550u, 65600u, 81920u, 131072u, 200000u, 600000u})
        for (uint32_t mode = 0; mode < 3; mode++)
            model_block(n, mode, mode == 0 ? 64 : 7, 0, 0);
    model_block(200000, 0, 1, 0, 0);
    model_block(300000, 1, 3, 70000, 100000);            // one jump past every entry
    model_block(300000, 2, 0, 66000, 0xC000);
    model_block(300000, 2, 0, 66000, 0xBFFF);
    enc_rebase_sweep r;
    enc_rebase_sweep_host(14, 65548, 1, 2, 0, 0, 0, &r);
    if (r.rebases || r.bad_fit || r.bad_target)
        fail("a block of up to 65,548 bytes re-based or overflowed", 0, 0, 0);
    if (failures) {
        fprintf(stderr, "enc_rebase_check: %d FAILED\n", failures);
        return 1;
    }
    printf("enc_rebase_check: ok\n");
    return 0;
}
#endif
