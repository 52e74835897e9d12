// tone_math.h — the channel tone detector's arithmetic (sddc_ddc.h, sddc_ddc_channel_tone_*), shared word
// for word by the device kernels (ddc_channel_tone.hip) and the CPU backend (cpu/r2iq_cpu.cpp), as
// squelch_math.h is for the squelch, whose gate it uses (squelch_step), with the blanker's block tree
// (blank_tree, blank_power, blank_finite) and the demodulator's phase word (demod_sincos_word).
//
// A bank of single-bin DFTs (Goertzel filters) per channel over a real sense stream, in blocks of B =
// kToneBlock = 256 samples and windows of W blocks, both anchored to the stream position, and a gate on
// the channel's audio that opens when the strongest tone of the channel's mask holds enough of the
// window's energy.  Everything is a fixed sequence of float operations that IEEE 754 rounds correctly (*,
// +, explicit fmaf, comparisons and selects) and of integer operations; the device side includes this
// under `#pragma clang fp contract(off)`, the CPU backend and the runtime are built with
// -ffp-contract=off, and numpy reproduces the bits (tools/channel_tone_model.py).
//
//   sample        x (S16: (float)v), q = x * x.  A sample with !blank_finite(q) enters every sum as x = 0,
//                 q = 0 and marks its window bad.
//   block k       (samples 256 k .. 256 k + 255 of the stream) for tone t with the phase word w_t (2^-32
//                 cycles per sample): (c_i, s_i) = demod_sincos_word(w_t * i) (uint32 product, i = 0..255),
//                 a_i = x_i * c_i, b_i = x_i * s_i, Ck = blank_tree(a), Sk = blank_tree(b); (cr, sr) =
//                 demod_sincos_word(w_t * (uint32)(256 k)); tone_rotate: Re_k = fmaf(Ck, cr, -(Sk * sr)),
//                 Im_k = fmaf(Ck, sr, Sk * cr); p_k = blank_tree(q).
//   window j      (blocks j W .. j W + W - 1) Zr, Zi, E: the left folds from +0 in block order, Z = Z + Re_k
//                 and so on.  P_t = blank_power(Zr, Zi).  tone_best: the ascending scan of the mask's
//                 tones, replaced only on a strict >: the lowest index that no other tone exceeds (-1 and P
//                 = 0 for an empty mask).  tone_flags: u = !bad && E > Emin && P_best > To * E, v the same
//                 with Tc; To = (float)((double)rho_open * 256 W), Tc likewise, Emin = (float)((double)
//                 e_min * 256 W) (tone_scale, at set time).
//   gate          squelch_step(u, v, A, H) once per completed window, all zero on a new stream; the gate
//                 after window j applies to window j + 1 (no look-ahead, no fade).  A mask of 0 is bypass:
//                 always open.
//   audio         a sample of an open window passes (the stored F32 word, so a NaN keeps its payload; S16
//                 codes survive (float) and demod_s16), a closed one is +0.
//
// Range of the bit-exact guarantee: samples that are 0 or of magnitude in [2^-40, 2^40], rho >= 2^-28,
// e_min 0 or in [2^-80, 2^80].  A phasor component is 0 or at least 2^-30 in magnitude (the smallest
// nonzero |z| is 2^-29, times pi / 4) and at most 1 + 2^-22, so a product a_i is 0 or in [2^-70, 2^41] and
// a multiple of 2^-93; sums of such values are multiples of 2^-93 too, so every tree value is 0 or at
// least 2^-93 and at most 2^49; Sk * sr and Sk * cr are 0 or at least 2^-123; |Re_k|, |Im_k| <= 2^50 and
// the folds stay below 2^59, P below 2^119.  q is 0 or in [2^-80, 2^80], p_k and E are 0 or in [2^-80,
// 2^96]; To is in [2^-20, 2^16], so To * E is 0 or in [2^-100, 2^112].  Nothing overflows.  The one value
// that can be subnormal is a fold that cancels (an fmaf whose two terms of at least 2^-123 agree to
// their last bits, or P of a |Z| below 2^-63): such a P is below 2^-125 and so below every To * E > 0
// that it is compared with, whether a backend keeps the subnormal or flushes it, so no decision depends
// on it (gfx950 as hipcc builds it and x86 both keep subnormals, so d_level and d_powers agree there
// too).  Outside the range both sides perform the same operations; no value is a reason for a memory
// fault.
//
// Accuracy against the float64 evaluation of the same definition on the same float32 samples, words and
// scaled thresholds (cos and sin of the exact phase 2 pi (w i mod 2^32) / 2^32), u = 2^-24, X = the sum of
// |x_i| over the window (X <= sqrt(256 W E)):
//   a_i           |a_i - x_i cos| <= |x_i| (4 u + u (1 + 4 u)): demod_sincos_word's 4 u and one rounding.
//   Ck, Sk        8 tree levels on top: |Ck - Ck64| <= (5.01 + 8.01) u X_k <= 13.1 u X_k (X_k: the block's).
//   Re_k, Im_k    both block sums' errors (2 * 13.1 u), the rotation's phasor error on |Ck|, |Sk| <= X_k
//                 (2 * 4 u), the product's rounding (u) and the fmaf's (2 u, its value is at most |Ck| +
//                 |Sk|): |Re_k - Re_k64| <= 38 u X_k.
//   Zr, Zi        W - 1 additions that round, |Re_k64| <= X_k: |Zr - Zr64| <= (38 + W) u X =: eps X.
//   P_t           |Zr^2 - Zr64^2| <= eps X (2 |Zr64| + eps X), the same for Zi, |Zr64| + |Zi64| <= sqrt(2
//                 P64), three roundings in blank_power:
//                     |P_t - P_t64| <= tone_bound_p = 1.01 (2 sqrt(2) eps X sqrt(P64) + 2 eps^2 X^2 + 3 u P64).
//   E             one rounding in q, 8 tree levels, W - 1 fold additions, all terms >= 0:
//                     |E - E64| <= 1.01 (W + 8) u E64.
//   To * E        one more rounding: |To * E - (To * E)64| <= tone_bound_te = 1.01 (W + 9) u To E64.
// u_j or v_j can differ from the float64 evaluation only where |P64 - T E64| <= tone_bound_p +
// tone_bound_te or |E64 - Emin| <= 1.01 (W + 8) u E64, which tests/test_channel_tone_cpu.py checks; these
// are derived figures, not measured ones.
#pragma once

#include <stdint.h>

#include "blanker_math.h"
#include "demod_math.h"
#include "squelch_math.h"

#if defined(__HIPCC__)
#define SDDC_TONE_FN __host__ __device__ __forceinline__
#else
#define SDDC_TONE_FN inline
#endif

namespace sddc {
namespace tone {

constexpr int kToneBlock = blank::kBlankBlock;   // SDDC_DDC_TONE_BLOCK
constexpr int kToneMaxTones = 64;                // SDDC_DDC_TONE_MAX_TONES
constexpr int kToneMaxWindow = 256;              // SDDC_DDC_TONE_MAX_WINDOW
constexpr int kToneMaxAttack = squelch::kSquelchMaxAttack, kToneMaxHang = squelch::kSquelchMaxHang;

// the phasor of sample i of a block, and of block k's start (pos256 = (uint32)(256 k))
SDDC_TONE_FN void tone_phasor(uint32_t w, uint32_t i, float *c, float *s) { demod::demod_sincos_word(w * i, c, s); }

SDDC_TONE_FN void tone_rotate(float Ck, float Sk, float cr, float sr, float *re, float *im)
{
    *re = demod::fma_(Ck, cr, -(Sk * sr));
    *im = demod::fma_(Ck, sr, Sk * cr);
}

// one step of the ascending scan: tone t with the power P against the best so far (*best < 0: none)
SDDC_TONE_FN void tone_best(int t, float P, int *best, float *Pbest)
{
    const bool take = *best < 0 || P > *Pbest;
    *best = take ? t : *best;
    *Pbest = take ? P : *Pbest;
}

SDDC_TONE_FN void tone_flags(float P, float E, bool bad, float To, float Tc, float Emin, bool *u, bool *v)
{
    const bool live = !bad && E > Emin;
    *u = live && P > To * E;
    *v = live && P > Tc * E;
}

// (host) (float)((double)x * 256 W)
inline float tone_scale(float x, int W) { return (float)((double)x * 256.0 * (double)W); }

}  // namespace tone
}  // namespace sddc
