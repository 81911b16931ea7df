// itb_rules_host.cc -- pomegranate_amd/csrc/itb_rules.h on the CPU, alone: the
// finish of an ITB compress and of an ITB decompress over the table of
// tests/test_gpu_record_rules.py (payload sizes, ties between the compressed and
// the original length, every tmp_cap edge), with no GPU call and nothing loaded
// into Python.  Every buffer is a heap block of exactly its stated capacity, so
// in a sanitizer build a byte past a capacity is a report; the results are
// compared with a restatement of mds/itb.c:2923-2944 and :2966-2979 written
// here.
//   itb_rules_check          the header's functions
//   itb_rules_check_parent   (-DITB_RULES_PARENT, `make -f itb_rules.mk parent`)
//                            the compress finish as it stood before tmp_cap was
//                            honoured: header and stream copied unchecked.  It
//                            is there to show that this program sees the
//                            overrun; no test runs it.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "itb_rules.h"

namespace {

const size_t H = POM_ITBH_SIZE;
const size_t kItbFull = H + POM_ITB_PAYLOAD_MAX;

size_t worst(size_t n) { return n + n / 16 + 64 + 3; }

int failures = 0;

#ifdef ITB_RULES_PARENT
void finish_compress(uint8_t* in, uint8_t* tmp, size_t, const uint8_t* z, size_t slen, size_t dlen, int st,
                     uint8_t** oi, int* err)
{
    *oi = in;
    *err = itb_rules_rd32(in + POM_ITBH_LEN_OFF) >= H ? 0 : -EINVAL;
    if (*err)
        return;
    memcpy(tmp, in, H);
    if (st != 0) {
        *err = st;
        return;
    }
    if (dlen >= slen)
        return;
    if (z != tmp + H)
        memcpy(tmp + H, z, dlen);
    itb_rules_wr32(tmp + POM_ITBH_ZLEN_OFF, itb_rules_rd32(tmp + POM_ITBH_LEN_OFF));
    itb_rules_wr32(tmp + POM_ITBH_LEN_OFF, (uint32_t)(H + dlen));
    itb_rules_wr16(tmp + POM_ITBH_ALGO_OFF, POM_COMPR_LZO);
    *oi = tmp;
}
#else
void finish_compress(uint8_t* in, uint8_t* tmp, size_t tmp_cap, const uint8_t* z, size_t slen, size_t dlen, int st,
                     uint8_t** oi, int* err)
{
    itb_rules_finish_compress(in, tmp, tmp_cap, z, slen, dlen, st, oi, err);
}
#endif

void fail(const char* what, uint32_t hlen, size_t dlen, size_t tmp_cap, int st)
{
    failures++;
    fprintf(stderr, "compress: h.len %u, stream %zu, tmp_cap %zu, status %d: %s\n", hlen, dlen, tmp_cap, st, what);
}

// One record of h.len bytes whose payload "compressed" to dlen bytes with the
// encoder's code st, finished into a tmp of exactly tmp_cap bytes.
void check_compress(uint32_t hlen, size_t dlen, size_t tmp_cap, int st)
{
    const size_t slen = hlen >= H ? hlen - H : 0;
    const size_t in_size = hlen >= H ? hlen : H;
    uint8_t* in = static_cast<uint8_t*>(malloc(in_size));
    uint8_t* keep = static_cast<uint8_t*>(malloc(in_size));
    uint8_t* tmp = static_cast<uint8_t*>(malloc(tmp_cap));
    for (size_t i = 0; i < in_size; i++)
        in[i] = (uint8_t)(i * 131 + 7);
    itb_rules_wr32(in + POM_ITBH_LEN_OFF, hlen);
    itb_rules_wr32(in + POM_ITBH_ZLEN_OFF, 0);
    itb_rules_wr16(in + POM_ITBH_ALGO_OFF, POM_COMPR_NONE);
    memcpy(keep, in, in_size);
    if (tmp_cap)
        memset(tmp, 0xA5, tmp_cap);
    // the stream: where itb_wb_init has the encoder write it
    const int direct = itb_rules_direct(tmp_cap, worst(slen));
    if (direct != (tmp_cap >= H + worst(slen)))
        fail("itb_rules_direct", hlen, dlen, tmp_cap, st);
    uint8_t* aside = direct ? nullptr : static_cast<uint8_t*>(malloc(worst(slen)));
    uint8_t* z = direct ? tmp + H : aside;
    for (size_t i = 0; i < dlen; i++)
        z[i] = (uint8_t)(i * 29 + 3);

    uint8_t* oi = nullptr;
    int err = 12345;
    finish_compress(in, tmp, tmp_cap, z, slen, dlen, st, &oi, &err);

    // mds/itb.c:2923-2944, and the capacity rule of pom_itb.h
    const int want_err = hlen < H ? -EINVAL : st;
    const bool compressed = want_err == 0 && dlen < slen && H + dlen <= tmp_cap;
    if (err != want_err)
        fail("err", hlen, dlen, tmp_cap, st);
    if (oi != (compressed ? tmp : in))
        fail(compressed ? "kept, expected compressed" : "compressed, expected kept", hlen, dlen, tmp_cap, st);
    if (memcmp(in, keep, in_size) != 0)
        fail("in[] changed", hlen, dlen, tmp_cap, st);
    if (tmp_cap < H || hlen < H) {
        for (size_t i = 0; i < tmp_cap && (tmp_cap < H || !direct || i < H); i++)
            if (tmp[i] != 0xA5) {
                fail("tmp[] written", hlen, dlen, tmp_cap, st);
                break;
            }
    } else if (compressed) {
        uint8_t hdr[POM_ITBH_SIZE];
        memcpy(hdr, keep, H);
        itb_rules_wr32(hdr + POM_ITBH_ZLEN_OFF, hlen);
        itb_rules_wr32(hdr + POM_ITBH_LEN_OFF, (uint32_t)(H + dlen));
        itb_rules_wr16(hdr + POM_ITBH_ALGO_OFF, POM_COMPR_LZO);
        if (memcmp(tmp, hdr, H) != 0)
            fail("compressed header", hlen, dlen, tmp_cap, st);
        for (size_t i = 0; i < dlen; i++)
            if (tmp[H + i] != (uint8_t)(i * 29 + 3)) {
                fail("compressed payload", hlen, dlen, tmp_cap, st);
                break;
            }
        if (!direct)
            for (size_t i = H + dlen; i < tmp_cap; i++)
                if (tmp[i] != 0xA5) {
                    fail("tmp[] written past the record", hlen, dlen, tmp_cap, st);
                    break;
                }
    } else {
        if (memcmp(tmp, keep, H) != 0)
            fail("kept: header copy", hlen, dlen, tmp_cap, st);
        if (!direct)
            for (size_t i = H; i < tmp_cap; i++)
                if (tmp[i] != 0xA5) {
                    fail("kept: tmp[] written past the header", hlen, dlen, tmp_cap, st);
                    break;
                }
    }
    free(aside);
    free(tmp);
    free(keep);
    free(in);
}

void check_decompress(int st, size_t produced, uint32_t zlen)
{
    uint8_t* hdr = static_cast<uint8_t*>(malloc(H));
    uint8_t keep[POM_ITBH_SIZE];
    for (size_t i = 0; i < H; i++)
        hdr[i] = (uint8_t)(i * 37 + 11);
    itb_rules_wr32(hdr + POM_ITBH_LEN_OFF, 264 + 99);
    itb_rules_wr32(hdr + POM_ITBH_ZLEN_OFF, zlen);
    itb_rules_wr16(hdr + POM_ITBH_ALGO_OFF, POM_COMPR_LZO);
    memcpy(keep, hdr, H);
    for (int with_ok = 0; with_ok < 2; with_ok++) {
        memcpy(hdr, keep, H);
        int err = 12345, ok = 12345;
        const uint32_t len = itb_rules_finish_decompress(hdr, st, produced, &err, with_ok ? &ok : nullptr);
        itb_rules_wr32(keep + POM_ITBH_LEN_OFF, (uint32_t)(H + produced));
        itb_rules_wr16(keep + POM_ITBH_ALGO_OFF, POM_COMPR_NONE);
        const int want_ok = st == 0 && (uint64_t)produced + H == zlen;
        if (err != st || len != H + produced || (with_ok && ok != want_ok) || memcmp(hdr, keep, H) != 0) {
            failures++;
            fprintf(stderr, "decompress: status %d, produced %zu, zlen %u: err %d, len %u, len_ok %d\n", st, produced,
                    zlen, err, len, ok);
        }
    }
    free(hdr);
}

}  // namespace

int main()
{
    // the payload sizes of the family: the encoder's n <= 13 branch, the first
    // sizes that parse, the tie sizes and a one-ITE ITB
    for (size_t slen : {(size_t)0, (size_t)1, (size_t)13, (size_t)14, (size_t)15, (size_t)40, (size_t)300,
                        (size_t)1000, (size_t)12416}) {
        const uint32_t hlen = (uint32_t)(H + slen);
        // the stream against the payload: +1, 0, -1, -2, a third of it, nothing
        for (long d : {1L, 0L, -1L, -2L, -(long)(slen - slen / 3), -(long)slen}) {
            if ((long)slen + d < 0)
                continue;
            const size_t dlen = (size_t)((long)slen + d);
            for (size_t tmp_cap : {(size_t)0, (size_t)1, (size_t)263, (size_t)264, H + dlen - 1, H + dlen,
                                   (size_t)hlen - 1, (size_t)hlen, H + worst(slen) - 1, H + worst(slen), kItbFull})
                for (int st : {0, -1})
                    check_compress(hlen, dlen, tmp_cap, st);
        }
    }
    // h.len below the header size: -EINVAL, tmp untouched
    for (uint32_t hlen : {0u, 100u, 263u})
        for (size_t tmp_cap : {(size_t)0, (size_t)263, (size_t)264, kItbFull})
            check_compress(hlen, 0, tmp_cap, 0);
    // the decompress finish: every decoder code, the length check at its edges
    for (int st : {0, -4, -5, -6, -7, -8})
        for (size_t produced : {(size_t)0, (size_t)1, (size_t)40, (size_t)12416, (size_t)POM_ITB_PAYLOAD_MAX})
            for (long dz : {-1L, 0L, 1L})
                check_decompress(st, produced, (uint32_t)((long)(H + produced) + dz));
    check_decompress(0, 0, 0);
    if (failures) {
        fprintf(stderr, "itb_rules_check: %d FAILED\n", failures);
        return 1;
    }
    printf("itb_rules_check: ok\n");
    return 0;
}
