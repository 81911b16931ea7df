// lzo1x_enc_rebase.h -- when the encoder's u16 dictionary is re-based, and to
// where (lzo1x_encode_fast.hip, parse_wave), stated once as plain C++ for the
// device and for tests/native/enc_rebase_host.cc on the CPU.
//
// A dictionary entry is v = position - base + 1 (0 = empty), 16 bits.  The
// window at ip stores the positions of its path lanes: ip (lane 0 always
// probes) through min(ip + 63, ip_end - 1), ip_end = n - 13 being the first
// position the reference no longer probes (lib/minilzo.c:2929).  A re-base is
// due exactly when the highest of them would not fit: a block of up to
// 65,548 bytes (ip_end - 1 = n - 14 <= 65,534) never re-bases.
//
// The new base is ip - (M4_MAX_OFFSET + 1).  Every entry below it lies more
// than M4_MAX_OFFSET behind this window's and every later probe, so the
// reference rejects it too (lib/minilzo.c:2878-2883) and clearing it leaves
// the parse as it was; any lower base would be as exact, this one puts the
// next re-base furthest away (0xFFFF - 0xC000 - 63 = 16,320 bytes at least).
// When a re-base is due, ip + 63 - base >= 0xFFFF, so the target is above
// the old base and above 0, and the window's own values are at most
// 0xC000 + 64.
#ifndef POM_LZO1X_ENC_REBASE_H
#define POM_LZO1X_ENC_REBASE_H

#include <stdint.h>

#ifdef __HIPCC__
#define ENC_REBASE_FN __device__ __forceinline__
#else
#define ENC_REBASE_FN static inline
#endif

#define ENC_REBASE_WINDOW 64u                     /* positions per window (the wave) */
#define ENC_REBASE_VMAX 0xFFFFu                   /* the largest entry */
#define ENC_REBASE_BACK 0xC000u                   /* M4_MAX_OFFSET + 1 */

/* The highest position the window at ip can store (ip < ip_end). */
ENC_REBASE_FN uint32_t enc_rebase_top(uint32_t ip, uint32_t ip_end)
{
    const uint32_t last = ip + (ENC_REBASE_WINDOW - 1);
    return last < ip_end - 1 ? last : ip_end - 1;
}

/* Must the dictionary be re-based before the window at ip (base <= ip < ip_end)? */
ENC_REBASE_FN int enc_rebase_due(uint32_t ip, uint32_t ip_end, uint32_t base)
{
    return enc_rebase_top(ip, ip_end) - base + 1 > ENC_REBASE_VMAX;
}

/* The new base for a re-base due at ip. */
ENC_REBASE_FN uint32_t enc_rebase_target(uint32_t ip)
{
    return ip - ENC_REBASE_BACK;
}

/* One packed pair of entries moved down by delta = new base - old base: an
 * entry at or below delta (a position below the new base, or empty) becomes 0. */
ENC_REBASE_FN uint32_t enc_rebase_pair(uint32_t pair, uint32_t delta)
{
    const uint32_t lo = pair & 0xFFFFu, hi = pair >> 16;
    const uint32_t nlo = lo > delta ? lo - delta : 0u;
    const uint32_t nhi = hi > delta ? hi - delta : 0u;
    return nlo | (nhi << 16);
}

/* The bitmap byte of 8 re-based entries (4 packed pairs): bit i set when
 * entry i is not 0. */
ENC_REBASE_FN uint32_t enc_rebase_live8(const uint32_t pairs[4])
{
    uint32_t m = 0;
    for (int i = 0; i < 4; i++) {
        m |= (pairs[i] & 0xFFFFu ? 1u : 0u) << (2 * i);
        m |= (pairs[i] >> 16 ? 1u : 0u) << (2 * i + 1);
    }
    return m;
}

#endif
