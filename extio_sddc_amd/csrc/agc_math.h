// agc_math.h — the channel AGC's arithmetic (sddc_ddc.h, sddc_ddc_channel_agc_*), shared word for word
// by the device kernels (ddc_channel_agc.hip) and the CPU backend (cpu/r2iq_cpu.cpp), as demod_math.h
// is for the demodulator and audio_iir_math.h for the audio filter.
//
// A fast-attack, exponential-release peak AGC.  A channel has three float parameters: T, the target
// peak level (T == 0: the channel is bypassed), d, the release factor per sample (0 <= d < 1), and F,
// the envelope floor (the largest gain is T / F).  Everything here is a fixed sequence of float
// operations that IEEE 754 rounds correctly: *, /, comparisons and fabsf, no libm, no fminf / fmaxf.
// The device side includes this under `#pragma clang fp contract(off)`, the CPU backend and the runtime
// are built with -ffp-contract=off, so both sides produce the same bits (the division is the
// correctly rounded one on both; gfx950 code keeps float subnormals and the CPU backend sets no
// FTZ / DAZ).
//
//   agc_abs       the magnitude of a sample: a = |x|, a NaN gives 0, an infinity FLT_MAX.
//   agc_env       one envelope step: t = d * e; e = (a > t) ? a : t.
//   agc_out       the output of a sample from the running envelope R after its step:
//                 den = (R > F) ? R : F; g = T / den; y = g * x.  A bypassed channel: y = x as it is.
//   agc_boundary  the block transition: t = dB * E; E = (Z > t) ? Z : t.
//   agc_block_decay  (host) dB = float(d^B): eight squarings of (double)d with plain uncontracted *,
//                 then one rounding to float.  For a small d it underflows to 0, which is valid: the
//                 envelope of an earlier block then does not reach the next one.
//
// The stream (the definition that both backends compute): per channel the entry envelope E of the
// current block, the running envelope R, the running envelope from a zero start Zr and a position n,
// all zero at a set or reset.  Per sample: a = agc_abs(x); R = agc_env(a, d, R); Zr = agc_env(a, d, Zr);
// y[n] = agc_out(T, F, R, x); n++; when n is a multiple of B = kAgcBlock: E = agc_boundary(dB, E, Zr),
// R = E, Zr = 0.  In exact arithmetic this is e[n] = max(|x[n]|, d e[n-1]), y = T x / max(e, F): the
// maps e -> max(m, k e) compose associatively, as affine maps do, so a block of samples collapses to
// the pair (Zr, d^B).  A block's outputs depend on the stream before it through E alone, which is
// what lets the device run the blocks of a call in parallel.  The envelope runs for bypassed channels
// too: it is their signal meter.
//
// Since den >= |x| (R >= a after its step), |y| <= T (1 + 2 u), u = 2^-24: one rounding of the
// quotient and one of the product.  With T <= 32767 / (1 + 2 u) the stage cannot clip an S16 output.
//
// Accuracy against the float64 plain recurrence on the same float32 parameters and samples.  Every
// candidate |x[t]| d^(n - t) of the maximum reaches R through at most B - 1 rounded multiplies in the
// zero-start pass of its own block, one multiply by dB per later boundary (one rounding, plus dB's
// own rounding) and at most B multiplies in n's block.  max is monotone, so with K(n) = ceil((n + 1) / B)
//     |y[n] - y64[n]| <= 1.01 (2 B + 2 K(n) + 2) u |y64[n]|        (F32 out; S16 adds 1/2 and the clamp)
// (the last 2: the quotient and the product; the 1.01 covers the second order), while no envelope on
// the deciding path is subnormal, which F >= 2^-60 ensures for den.  tools/channel_agc_model.py
// evaluates it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SDDC_AGC_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define SDDC_AGC_FN inline
#endif

namespace sddc {
namespace agc {

constexpr int kAgcBlock = 256;   // SDDC_DDC_AGC_BLOCK
constexpr int kAgcParams = 4;    // floats per channel as the backends read them: T, d, F, dB
constexpr float kAgcFltMax = 3.40282346638528859812e+38f;

SDDC_AGC_FN float agc_abs(float x)
{
    if (!(x == x)) return 0.f;
    const float a = __builtin_fabsf(x);
    return a > kAgcFltMax ? kAgcFltMax : a;
}

SDDC_AGC_FN float agc_env(float a, float d, float e)
{
    const float t = d * e;
    return a > t ? a : t;
}

SDDC_AGC_FN float agc_out(float T, float F, float R, float x)
{
    if (T == 0.f) return x;
    const float den = R > F ? R : F;
    const float g = T / den;
    return g * x;
}

SDDC_AGC_FN float agc_boundary(float dB, float E, float Z)
{
    const float t = dB * E;
    return Z > t ? Z : t;
}

// (host) float(d^256).  Compiled with contraction off: every product is one rounded double operation.
inline float agc_block_decay(float d)
{
    double p = (double)d;
    for (int i = 0; i < 8; i++) p = p * p;
    return (float)p;
}

}  // namespace agc
}  // namespace sddc
