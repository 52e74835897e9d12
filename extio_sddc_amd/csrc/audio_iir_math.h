// audio_iir_math.h — the channel audio filter's arithmetic (sddc_ddc.h, sddc_ddc_channel_audio_filter_*),
// shared word for word by the device kernels (ddc_channel_audio.hip) and the CPU backend
// (cpu/r2iq_cpu.cpp), as demod_math.h is for the demodulator.
//
// A channel's filter is a cascade of S = 1..4 biquad sections in transposed direct form II, section k
// five floats (b0, b1, b2, a1, a2) with a0 = 1 and two state floats (s1, s2).  Everything here is a
// fixed sequence of float operations that IEEE 754 rounds correctly: explicit fmaf and *, no libm.
// The device side includes this under `#pragma clang fp contract(off)`, the CPU backend and the
// runtime are built with -ffp-contract=off, so both sides produce the same bits.
//
//   audio_step    one sample through the cascade: for k = 0 .. S - 1
//                     y  = fmaf(b0, x, s1)
//                     s1 = fmaf(-a1, y, fmaf(b1, x, s2))
//                     s2 = fmaf(-a2, y, b2 * x)
//                     x  = y
//                 and the last y is the output.
//   audio_adv     the block transition: out_i = Z_i, then for j = 0 .. 2S - 1 in order
//                 out_i = fmaf(M_ij, E_j, out_i).
//   audio_block_matrix  (host) M = float(A^B), A the 2S x 2S matrix of one zero-input step in exact
//                 arithmetic on the float coefficients: B zero-input steps of the recurrence above in
//                 double on each unit vector, every fmaf(a, b, c) written a * b + c with plain * and +.
//
// The stream (the definition that both backends compute): per channel three state vectors E (the
// entry state of the current block), R (the running state) and Zr (the running zero-state state) and
// a position n, all zero at a set or reset.  Per sample: y[n] = audio_step(x, R); audio_step(x, Zr)
// with its output dropped; n++; when n is a multiple of B = kAudioBlock: E = audio_adv(E, Zr), R = E,
// Zr = 0.  In exact arithmetic this is the plain recurrence; a block's outputs depend on the stream
// before it through E alone, which is what lets the device run the blocks of a call in parallel.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SDDC_AUDIO_FN __host__ __device__ __forceinline__
#define SDDC_AUDIO_UNROLL _Pragma("unroll")
#else
#include <cmath>
#define SDDC_AUDIO_FN inline
#define SDDC_AUDIO_UNROLL
#endif

namespace sddc {
namespace audio {

constexpr int kAudioBlock = 256;     // SDDC_DDC_AUDIO_BLOCK
constexpr int kAudioMaxSections = 4;

#if defined(__HIP_DEVICE_COMPILE__)
SDDC_AUDIO_FN float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
#else
SDDC_AUDIO_FN float fma_(float a, float b, float c) { return std::fmaf(a, b, c); }
#endif

// one sample through S sections: coef [S][5], state s [2S] = (s1, s2) per section
template <int S> SDDC_AUDIO_FN float audio_step(const float *coef, float *s, float x)
{
SDDC_AUDIO_UNROLL
    for (int k = 0; k < S; k++) {
        const float b0 = coef[5 * k], b1 = coef[5 * k + 1], b2 = coef[5 * k + 2], a1 = coef[5 * k + 3], a2 = coef[5 * k + 4];
        const float y = fma_(b0, x, s[2 * k]);
        s[2 * k] = fma_(-a1, y, fma_(b1, x, s[2 * k + 1]));
        s[2 * k + 1] = fma_(-a2, y, b2 * x);
        x = y;
    }
    return x;
}

// out = M E + Z, row i accumulated from Z_i over j = 0 .. 2S - 1 in order; M is [2S][2S] row-major.
// out may not alias E.
template <int S> SDDC_AUDIO_FN void audio_adv(const float *M, const float *E, const float *Z, float *out)
{
SDDC_AUDIO_UNROLL
    for (int i = 0; i < 2 * S; i++) {
        float acc = Z[i];
SDDC_AUDIO_UNROLL
        for (int j = 0; j < 2 * S; j++) acc = fma_(M[i * 2 * S + j], E[j], acc);
        out[i] = acc;
    }
}

// (host) M [2S][2S] row-major of the channel whose sections are coef [S][5].  Compiled with
// contraction off: every product and sum below is one rounded double operation.
inline void audio_block_matrix(const float *coef, int S, float *M)
{
    const int n = 2 * S;
    for (int col = 0; col < n; col++) {
        double s[2 * kAudioMaxSections] = {};
        s[col] = 1.0;
        for (int step = 0; step < kAudioBlock; step++) {
            double x = 0.0;
            for (int k = 0; k < S; k++) {
                const double b0 = coef[5 * k], b1 = coef[5 * k + 1], b2 = coef[5 * k + 2], a1 = coef[5 * k + 3],
                             a2 = coef[5 * k + 4];
                const double y = b0 * x + s[2 * k];
                const double inner = b1 * x + s[2 * k + 1];
                s[2 * k] = (-a1) * y + inner;
                const double last = b2 * x;
                s[2 * k + 1] = (-a2) * y + last;
                x = y;
            }
        }
        for (int i = 0; i < n; i++) M[i * n + col] = (float)s[i];
    }
}

}  // namespace audio
}  // namespace sddc
