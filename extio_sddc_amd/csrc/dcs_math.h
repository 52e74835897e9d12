// dcs_math.h — the channel DCS decoder's arithmetic (sddc_ddc.h, sddc_ddc_channel_dcs_*), shared word for
// word by the device kernels (ddc_channel_dcs.hip) and the CPU backend (cpu/r2iq_cpu.cpp), as tone_math.h
// is for the tone detector, whose gate (squelch_step) it uses.
//
// A digital code squelch is a 23-bit Golay (23, 12) codeword sent over and over at 134.4 bit/s as NRZ below
// the audio.  The decoder takes the sign of a real sense stream, sorts the signs of a window of W blocks of
// B = kDcsBlock = 256 samples (anchored to the stream position) into sub-bins of an eighth of a bit, forms
// the 23 bit sums at each of the 8 timing phases, keeps the phase with the widest eye, and matches the
// word against a table of codewords over all 23 rotations.  After the one sign test per sample everything
// is an integer: sums of -1, 0 and +1, shifts, popcounts and comparisons, so the results do not depend on
// the order of any sum, and numpy reproduces them (tools/channel_dcs_model.py).
//
//   sample n      of a window (n = p - 256 W j, 0 <= n < 256 W <= 65536): s = dcs_sign (+1 if x > 0, -1 if
//                 x < 0, else 0; a NaN is 0; S16 is the code's own sign); m = dcs_subbin(w, n) = (w n) >> 29,
//                 the product in 64 bits (w <= 2^29, so it is below 2^45); S[m] += s for m < kDcsSubBins = 192.
//   window        c[t][b] = S[8 b + t] + .. + S[8 b + t + 7] (dcs_bit_sum), t = 0..7, b = 0..22: the sum of s
//                 over floor((w n - t 2^29) / 2^32) = b.  Q[t] = the sum over b of |c[t][b]| (at most 256 W
//                 = 2^16).  dcs_best_phase: the largest Q, the lowest t on a tie.  dcs_word: bit b = (c[t][b] >
//                 0), complemented in 23 bits if the channel inverts.
//   match         dcs_distance(word, cw) = the minimum over r = 0..22 of popcount(word xor dcs_rot(cw, r));
//                 dcs_key(d, i) = d << 8 | i orders the candidates: the lowest d, then the lowest i
//                 (kDcsNoKey: no candidate, d reads kDcsNoMatch = 24).
//   flags         good = 256 Q[t] >= eye N[t] (both at most 2^24), u = good && d <= e_open, v = good && d <=
//                 e_close (dcs_flags).  N[t] = the number of n < 256 W with t <= m(n) < t + 184 (dcs_count, at
//                 set time).
//   gate          squelch_step(u, v, A, H) once per completed window, as in the tone detector.
//
// The generator polynomial of dcs_codeword is g = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1 = 0xC75: the word
// is (parity << 12) | 0x800 | code with parity = (d x^11) mod g over GF(2), d = 0x800 | code; code 023
// (octal) gives 0x763813.
#pragma once

#include <stdint.h>

#include "squelch_math.h"

#if defined(__HIPCC__)
#define SDDC_DCS_FN __host__ __device__ __forceinline__
#else
#define SDDC_DCS_FN inline
#endif

namespace sddc {
namespace dcs {

constexpr int kDcsBlock = squelch::kSquelchBlock;   // SDDC_DDC_DCS_BLOCK
constexpr int kDcsMaxWindow = 256;                  // SDDC_DDC_DCS_MAX_WINDOW
constexpr int kDcsMaxCodes = 128;                   // SDDC_DDC_DCS_MAX_CODES
constexpr int kDcsMaxErrors = 3;                    // SDDC_DDC_DCS_MAX_ERRORS
constexpr int kDcsMaxEye = 256;                     // SDDC_DDC_DCS_MAX_EYE
constexpr int kDcsMaxAttack = squelch::kSquelchMaxAttack, kDcsMaxHang = squelch::kSquelchMaxHang;
constexpr int kDcsAny = -1, kDcsOff = -2;           // SDDC_DDC_DCS_ANY, _OFF
constexpr int kDcsBits = 23, kDcsPhases = 8, kDcsSubBins = 192, kDcsSpan = 184;
constexpr uint32_t kDcsMaxWord = 1u << 29, kDcsWordMask = 0x7fffffu;
constexpr uint32_t kDcsNoMatch = 24, kDcsNoKey = (kDcsNoMatch << 8) | 0xffu;

SDDC_DCS_FN int dcs_sign(float x) { return (x > 0.f ? 1 : 0) - (x < 0.f ? 1 : 0); }
SDDC_DCS_FN int dcs_sign_s16(int v) { return (v > 0 ? 1 : 0) - (v < 0 ? 1 : 0); }

SDDC_DCS_FN uint32_t dcs_subbin(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * (uint64_t)n) >> 29); }

SDDC_DCS_FN int dcs_popcount(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// c[t][b] from the window's sub-bin sums
SDDC_DCS_FN int dcs_bit_sum(const int *S, int t, int b)
{
    int c = 0;
    for (int i = 0; i < 8; i++) c += S[8 * b + t + i];
    return c;
}

SDDC_DCS_FN uint32_t dcs_abs(int c) { return (uint32_t)(c < 0 ? -c : c); }

// one step of the ascending scan over t: the largest Q, the lowest t on a tie (*best < 0: none yet)
SDDC_DCS_FN void dcs_best_phase(int t, uint32_t Q, int *best, uint32_t *Qbest)
{
    const bool take = *best < 0 || Q > *Qbest;
    *best = take ? t : *best;
    *Qbest = take ? Q : *Qbest;
}

// cw rotated by r = 0..22 in 23 bits
SDDC_DCS_FN uint32_t dcs_rot(uint32_t cw, int r) { return ((cw << r) | (cw >> (kDcsBits - r))) & kDcsWordMask; }

SDDC_DCS_FN uint32_t dcs_distance(uint32_t word, uint32_t cw)
{
    uint32_t d = kDcsNoMatch;
    for (int r = 0; r < kDcsBits; r++) {
        const uint32_t e = (uint32_t)dcs_popcount(word ^ dcs_rot(cw, r));
        d = e < d ? e : d;
    }
    return d;
}

SDDC_DCS_FN uint32_t dcs_key(uint32_t d, int i) { return (d << 8) | (uint32_t)i; }

// whether table entry i is a candidate of a channel whose code setting is `code`
SDDC_DCS_FN bool dcs_candidate(int code, int i, int ncodes) { return code == kDcsAny ? i < ncodes : i == code; }

SDDC_DCS_FN void dcs_flags(uint32_t Q, uint32_t N, uint32_t d, uint32_t eye, uint32_t e_open, uint32_t e_close, bool *u, bool *v)
{
    const bool good = 256u * Q >= eye * N;
    *u = good && d <= e_open;
    *v = good && d <= e_close;
}

// (host) the whole window on its sub-bin sums: Q, t, the word, the best candidate (-1: none) and its d
inline void dcs_window(const int *S, const uint32_t *cws, int ncodes, int code, int invert, uint32_t *Q, int *t, int *best, uint32_t *d)
{
    int tb = -1;
    uint32_t Qb = 0;
    for (int tt = 0; tt < kDcsPhases; tt++) {
        uint32_t q = 0;
        for (int b = 0; b < kDcsBits; b++) q += dcs_abs(dcs_bit_sum(S, tt, b));
        dcs_best_phase(tt, q, &tb, &Qb);
    }
    uint32_t word = 0;
    for (int b = 0; b < kDcsBits; b++) word |= (dcs_bit_sum(S, tb, b) > 0 ? 1u : 0u) << b;
    if (invert) word ^= kDcsWordMask;
    uint32_t key = kDcsNoKey;
    for (int i = 0; i < ncodes; i++) {
        if (!dcs_candidate(code, i, ncodes)) continue;
        const uint32_t k = dcs_key(dcs_distance(word, cws[i]), i);
        key = k < key ? k : key;
    }
    *Q = Qb;
    *t = tb;
    *best = key == kDcsNoKey ? -1 : (int)(key & 0xffu);
    *d = key >> 8;
}

// (host) N[t], t = 0..7: the samples of a window of W blocks that a word at phase t holds
inline void dcs_count(uint32_t w, int W, uint32_t *N)
{
    for (int t = 0; t < kDcsPhases; t++) N[t] = 0;
    for (uint32_t n = 0; n < (uint32_t)(kDcsBlock * W); n++) {
        const uint32_t m = dcs_subbin(w, n);
        for (int t = 0; t < kDcsPhases; t++) N[t] += m >= (uint32_t)t && m < (uint32_t)(t + kDcsSpan) ? 1u : 0u;
    }
}

// (host) the 23-bit codeword of the three octal digits code = 0..511
inline uint32_t dcs_codeword(uint32_t code)
{
    const uint32_t d = 0x800u | code;
    uint32_t rem = d << 11;   // d x^11, degree at most 22
    for (int bit = 22; bit >= 11; bit--)
        if ((rem >> bit) & 1u) rem ^= 0xC75u << (bit - 11);
    return (rem << 12) | d;
}

}  // namespace dcs
}  // namespace sddc
