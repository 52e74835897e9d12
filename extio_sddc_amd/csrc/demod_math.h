// demod_math.h — the channel demodulator's arithmetic (sddc_ddc.h, sddc_ddc_channel_demodulate_*), shared
// word for word by the device kernel (ddc_channel_demod.hip) and the CPU backend (cpu/r2iq_cpu.cpp).
//
// Everything here is a fixed sequence of float operations that IEEE 754 rounds correctly: explicit
// fmaf, +, -, *, /, sqrtf, comparisons, and integer operations on the phase word.  There is no libm
// or OCML transcendental and no min / max / rint call (their treatment of NaN and the rounding
// mode differ between the two sides).  The device side includes this under `#pragma clang fp
// contract(off)`, the CPU backend is built with -ffp-contract=off, and hipcc's divide and sqrtf for
// gfx950 are the correctly rounded ones, so both sides produce the same bits for inputs whose
// components are 0 or of magnitude in [2^-40, 2^40] (no subnormal intermediate).
//
// Accuracy (tests/test_channel_demod_cpu.py sweeps both against float64):
//   demod_angle       at most 4 ulp of the result (<= 8 u |theta|, u = 2^-24)
//   demod_sincos_word absolute error at most 4 u per component, the rounding of the phase included
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SDDC_DEMOD_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define SDDC_DEMOD_FN inline
#endif

namespace sddc {

// one channel of the demodulator, as the device and the CPU backend read it
struct ChDemChannel {
    int mode;         // SDDC_DDC_DEMOD_AM / _FM / _BFO
    float gain;
    uint32_t word;    // BFO phase increment per sample, in 2^-32 cycles
    uint32_t pad;
};

namespace demod {

#if defined(__HIP_DEVICE_COMPILE__)
SDDC_DEMOD_FN float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
SDDC_DEMOD_FN float sqrt_(float a) { return __builtin_sqrtf(a); }
#else
SDDC_DEMOD_FN float fma_(float a, float b, float c) { return std::fmaf(a, b, c); }
SDDC_DEMOD_FN float sqrt_(float a) { return std::sqrt(a); }
#endif

// The angle of (re, im) in (-pi, pi], with angle(0, 0) = +0: t = min / max of the magnitudes,
// atan(t) = t P(t^2) with P of degree 8 (relative error of the real polynomial 1.7e-8 on [0, 1]),
// then the reflections about pi/4, pi/2 and 0; pi/2 and pi are carried as float + float.
SDDC_DEMOD_FN float demod_angle(float im, float re)
{
    const float ax = re < 0.f ? 0.f - re : re, ay = im < 0.f ? 0.f - im : im;
    const bool steep = ay > ax;
    const float mx = steep ? ay : ax, mn = steep ? ax : ay;
    if (mx == 0.f) return 0.f;
    const float t = mn / mx, s = t * t;
    float p = 0x1.7a54bp-9f;
    p = fma_(p, s, -0x1.09ad72p-6f);
    p = fma_(p, s, 0x1.5fb326p-5f);
    p = fma_(p, s, -0x1.34376ep-4f);
    p = fma_(p, s, 0x1.b44026p-4f);
    p = fma_(p, s, -0x1.22f12p-3f);
    p = fma_(p, s, 0x1.997492p-3f);
    p = fma_(p, s, -0x1.5554b2p-2f);
    float r = fma_(t * s, p, t);                                   // t + t^3 (P - 1) / t^2
    if (steep) r = (0x1.921fb6p+0f - r) + -0x1.777a5cp-25f;        // pi/2 - r
    if (re < 0.f) r = (0x1.921fb6p+1f - r) + -0x1.777a5cp-24f;     // pi - r
    return im < 0.f ? 0.f - r : r;
}

// cos and sin of 2 pi w / 2^32.  k = the nearest quarter cycle, z = (w - k 2^30) / 2^29 in [-1, 1):
// sin(pi z / 4) = z S(z^2) and cos(pi z / 4) = C(z^2) are the Taylor polynomials to z^9 and z^10 with
// pi / 4 folded into the coefficients (remainders 1.8e-9 and 1.1e-10), then the quarter turns.  z = 0
// gives exactly (1, 0), so every quarter cycle is exact, with +0 for the zero.
SDDC_DEMOD_FN void demod_sincos_word(uint32_t w, float *c, float *s)
{
    const uint32_t k = (w + 0x20000000u) >> 30;
    const int32_t r = (int32_t)(w - (k << 30));
    const float z = (float)r * 0x1p-29f, q = z * z;
    float sp = 0x1.507834p-22f;              // (pi/4)^9 / 9!
    sp = fma_(sp, q, -0x1.32d2ccp-15f);      // -(pi/4)^7 / 7!
    sp = fma_(sp, q, 0x1.466bc6p-9f);       // (pi/4)^5 / 5!
    sp = fma_(sp, q, -0x1.4abbcep-4f);      // -(pi/4)^3 / 3!
    sp = fma_(sp, q, 0x1.921fb6p-1f);       // pi/4
    float cp = -0x1.a6d1f2p-26f;             // -(pi/4)^10 / 10!
    cp = fma_(cp, q, 0x1.e1f506p-19f);       // (pi/4)^8 / 8!
    cp = fma_(cp, q, -0x1.55d3c8p-12f);      // -(pi/4)^6 / 6!
    cp = fma_(cp, q, 0x1.03c1f0p-6f);        // (pi/4)^4 / 4!
    cp = fma_(cp, q, -0x1.3bd3ccp-2f);       // -(pi/4)^2 / 2!
    cp = fma_(cp, q, 1.f);
    sp = sp * z;
    switch (k & 3u) {
    case 0: *c = cp; *s = sp; break;
    case 1: *c = 0.f - sp; *s = cp; break;
    case 2: *c = 0.f - cp; *s = 0.f - sp; break;
    default: *c = sp; *s = 0.f - cp; break;
    }
}

// the three per-sample formulas on sample values (I, Q), the previous sample (Ip, Qp) and the gain g
SDDC_DEMOD_FN float demod_power(float I, float Q) { return fma_(I, I, Q * Q); }
SDDC_DEMOD_FN float demod_am(float I, float Q, float g) { return g * sqrt_(fma_(I, I, Q * Q)); }
SDDC_DEMOD_FN float demod_fm(float I, float Q, float Ip, float Qp, float g)
{
    const float re = fma_(I, Ip, Q * Qp), im = fma_(Q, Ip, -(I * Qp));
    return g * demod_angle(im, re);
}
SDDC_DEMOD_FN float demod_bfo(float I, float Q, uint32_t word, float g)
{
    float c, s;
    demod_sincos_word(word, &c, &s);
    return g * fma_(I, c, -(Q * s));
}

// SDDC_DDC_AUDIO_S16: round to nearest even, clamp to [-32768, 32767], NaN becomes 0.  After the
// clamp |y| <= 2^15, where adding and subtracting 1.5 x 2^23 rounds to an integer exactly.
SDDC_DEMOD_FN int16_t demod_s16(float y)
{
    if (!(y == y)) return 0;
    y = y < -32768.f ? -32768.f : (y > 32767.f ? 32767.f : y);
    const float t = (y + 12582912.f) - 12582912.f;
    return (int16_t)(int)t;
}

}  // namespace demod
}  // namespace sddc
