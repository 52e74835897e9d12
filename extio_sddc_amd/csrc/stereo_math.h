// stereo_math.h — the channel stereo decoder's arithmetic (sddc_ddc.h, sddc_ddc_channel_stereo_*), shared
// word for word by the device kernels (ddc_channel_stereo.hip) and the CPU backend (cpu/r2iq_cpu.cpp).  It
// adds three things to what it reuses: the pilot's phase from a window's single-bin DFT, the 38 kHz carrier
// of a sample, and the matrix.  The pilot measurement is the tone detector's (tone_math.h: tone_phasor,
// tone_rotate, tone_flags, tone_scale) with the blanker's tree and power (blank_tree, blank_power,
// blank_finite), the carrier is the demodulator's phase word (demod_sincos_word), the stereo / mono decision
// is the squelch's gate (squelch_step).
//
// The input is the stereo multiplex (MPX) of a broadcast FM station as the FM discriminator delivers it:
// L + R up to 15 kHz, a pilot at 19 kHz, L - R double-sideband around a suppressed carrier at 38 kHz whose
// phase is twice the pilot's (ITU-R BS.450: for a pilot sin(psi) the carrier is sin(2 psi)).  Everything is a
// fixed sequence of float operations that IEEE 754 rounds correctly (*, +, -, explicit fmaf, one sqrt, two
// divisions, comparisons and selects) and of integer operations; the device side includes this under
// `#pragma clang fp contract(off)`, the CPU backend and the runtime are built with -ffp-contract=off, and
// numpy reproduces the bits (tools/channel_stereo_model.py).  B = kStereoBlock = 256.
//
//   per handle    the pilot's phase word w (2^-32 cycles per sample, not 0), w2 = 2 w mod 2^32, a window of W
//                 blocks, an attack A and a hang H in windows.
//   per channel   a mode (kStereoMono: both outputs are the input; kStereoAuto), To, Tc, Emin (tone_scale of
//                 rho_open, rho_close, e_min) and g2 = 2 g (stereo_g2, at set time), g the separation gain.
//   sample        x (S16: (float)v), q = x * x.  A sample with !blank_finite(q) enters the sums as x = 0, q =
//                 0 and marks its window bad: the tone detector's rule.
//   block k       Re_k, Im_k, p_k: the tone detector's block sums for the single tone w.
//   window j      Zr, Zi, E: the tone detector's folds; P = blank_power(Zr, Zi); (u, v) = tone_flags(P, E, bad,
//                 To, Tc, Emin).  So (P, E) are the tone detector's d_level for the table {w} and the same W.
//   pilot phase   for x_i = sin(phi_i + alpha), phi_i = 2 pi w i / 2^32, the sum Z = sum x_i e^{j phi_i} is
//                 (N / 2) (sin alpha + j cos alpha).  Where v holds, stereo_phase: n = sqrt_(P), vr = Zi / n, vi
//                 = Zr / n (the unit vector e^{j alpha}), qr = fma_(vr, vr, -(vi * vi)), qi = (2 * vr) * vi (its
//                 square e^{2 j alpha}).  Where v does not hold, q stays.  A new stream has q = (1, 0).
//   gate          squelch_step(u, v, A, H) once per completed window, all zero on a new stream.  The gate and
//                 the q after window j apply to window j + 1: no look-ahead and no delay.
//   carrier       block k of an open window, sample i of the block: (tc_i, ts_i) = tone_phasor(w2, i); (rc, rs)
//                 = tone_phasor(w2, (uint32)(256 k)); (rr, ri) = tone_rotate(qr, qi, rc, rs); stereo_sub: sub_i
//                 = fma_(tc_i, ri, ts_i * rr), which is sin(2 (phi + alpha)) at the sample.
//   outputs       open window of a kStereoAuto channel: stereo_lr: d = (g2 * x) * sub, L = x + d, R = x - d (x
//                 as read, a non-finite one included); S16 outputs through demod_s16.  Otherwise L = R = the
//                 input sample by the tone detector's pass rule (the stored F32 word, so a NaN keeps its
//                 payload; S16 codes survive (float) and demod_s16).
//
// With MPX = (L + R) / 2 + ((L - R) / 2) sin(2 psi) + pilot and g = 1: x + 2 x sin(2 psi) = L + terms at 19,
// 38 and 76 kHz and L, R images around them, all above 23 kHz; x - 2 x sin(2 psi) = R likewise.  The 15 kHz
// low-pass that removes them commutes with the matrix and is the audio resampler's, after this stage.
//
// Range of the bit-exact guarantee: the tone detector's (samples 0 or of magnitude in [2^-40, 2^40], rho >=
// 2^-28, e_min 0 or in [2^-80, 2^80]) and g 0 or in [2^-40, 2^40].  tone_math.h shows that no decision depends
// on a subnormal or an overflow.  stereo_phase runs only where v holds: P > Tc * E and E > Emin >= 0, so Tc *
// E is at least 2^-100 and P is a normal number in (2^-100, 2^119): P = 0 is excluded, n = sqrt_(P) is in
// (2^-50, 2^60) and no division is by zero.  P = Zr^2 (1 + d1) + Zi^2 (1 + d2) to one more rounding and n to
// another, so |Zr| / n and |Zi| / n are at most 1 + 3 u: vr and vi are 0 or of magnitude at most 1 + 3.02 u,
// and the larger of them is at least 0.707.  The smaller one can be anything down to a subnormal or 0 (a
// fold that cancels); it decides nothing, and gfx950 as hipcc builds it and x86 both keep subnormals and
// round the division correctly, so q agrees there too.  |qr|, |qi| <= 1 + 2^-20.  The carrier's values are at
// most 1 + 2^-19 in magnitude; g2 * x is 0 or in [2^-79, 2^81], d and the outputs are below 2^82.  A product
// ts * rr or (g2 * x) * sub next to a zero of the carrier can be subnormal; it is a value of the output, not
// of a decision.
//
// Accuracy against the float64 evaluation of the same definition (cos and sin of the exact phases, exact
// sqrt and /) on the same float32 samples, words and scaled thresholds, u = 2^-24, in two parts:
//   1. q          tone_math.h: |Zr - Zr64|, |Zi - Zi64| <= eps X, eps = (38 + W) u, X the sum of |x_i| over the
//                 window, so |Z - Z64| <= sqrt(2) eps X as vectors; n64 = |Z64| = sqrt(P64), r = sqrt(2) eps X /
//                 n64.  For unit vectors |a / |a| - b / |b|| <= 2 |a - b| / (|a| + |b|) <= r / (1 - r / 2).  The
//                 float32 (vr, vi) is the unit vector of the float32 Z to 3.02 u per component (P's three
//                 roundings halve under the root, the root's and the division's).  So
//                     |v - v64| <= dv = r / (1 - r / 2) + 3.02 u,
//                 |v^2 - v64^2| = |v - v64| |v + v64| <= dv (2 + dv), and qr and qi add two roundings of
//                 values of at most 1 + 2^-20:
//                     |qr - qr64|, |qi - qi64| <= stereo_bound_q = dv (2 + dv) + 2.02 u.
//                 P64 > about rho_close X^2 (X <= sqrt(256 W E)), so r <= sqrt(2) eps / sqrt(rho_close): 2e-4
//                 at W = 8 and rho_close = 0.002.  A q that is held has the bound of the window that set it.
//   2. L, R       given the same float32 q, x and g2.  demod_sincos_word: 4 u per component.  rr and ri: the
//                 block phasor's error on |qr| + |qi| <= sqrt(2) (1 + 2^-20) (4 sqrt(2) u), the product's
//                 rounding (u) and the fmaf's (1.01 u): 7.7 u.  sub: the sample phasor's error on |rr| + |ri|
//                 (4 sqrt(2) u), rr's and ri's error on |tc| + |ts| (7.7 sqrt(2) u), the product's rounding and
//                 the fmaf's (2.01 u): |sub - sub64| <= 18.6 u.  d: the two products' roundings on |sub| <= 1 +
//                 2^-19 (2.01 u): |d - d64| <= 20.7 u |g2 x|.  L and R: one more rounding of a value of at most
//                 |x| + 1.0001 |g2 x|:
//                     |L - L64|, |R - R64| <= stereo_bound_lr = 1.01 u (|x| + 22 |g2 x|).
// The decisions u_j, v_j differ from the float64 evaluation only inside tone_math.h's bounds.  These are
// derived figures, not measured ones; tests/test_channel_stereo_cpu.py asserts them.
#pragma once

#include <stdint.h>

#include "tone_math.h"

#if defined(__HIPCC__)
#define SDDC_STEREO_FN __host__ __device__ __forceinline__
#else
#define SDDC_STEREO_FN inline
#endif

namespace sddc {
namespace stereo {

constexpr int kStereoBlock = tone::kToneBlock;           // SDDC_DDC_STEREO_BLOCK
constexpr int kStereoMaxWindow = tone::kToneMaxWindow;   // SDDC_DDC_STEREO_MAX_WINDOW
constexpr int kStereoMaxAttack = tone::kToneMaxAttack, kStereoMaxHang = tone::kToneMaxHang;
constexpr int kStereoMono = 0, kStereoAuto = 1;          // SDDC_DDC_STEREO_MONO, _AUTO

// q = the square of the pilot's unit phase vector, from a window's Z and P = blank_power(Zr, Zi) > 0
SDDC_STEREO_FN void stereo_phase(float Zr, float Zi, float P, float *qr, float *qi)
{
    const float n = demod::sqrt_(P);
    const float vr = Zi / n, vi = Zr / n;
    *qr = demod::fma_(vr, vr, -(vi * vi));
    *qi = (2.f * vr) * vi;
}

// the carrier's phasor at the start of the block at pos256 = (uint32)(256 k), turned by q
SDDC_STEREO_FN void stereo_block(float qr, float qi, uint32_t w2, uint32_t pos256, float *rr, float *ri)
{
    float rc, rs;
    tone::tone_phasor(w2, pos256, &rc, &rs);
    tone::tone_rotate(qr, qi, rc, rs, rr, ri);
}

// the carrier at a sample whose phasor within the block is (tc, ts)
SDDC_STEREO_FN float stereo_sub(float tc, float ts, float rr, float ri) { return demod::fma_(tc, ri, ts * rr); }

SDDC_STEREO_FN void stereo_lr(float x, float g2, float sub, float *L, float *R)
{
    const float d = (g2 * x) * sub;
    *L = x + d;
    *R = x - d;
}

// (host) 2 g: exact
inline float stereo_g2(float g) { return 2.f * g; }

}  // namespace stereo
}  // namespace sddc
