// audio_resample_math.h — the channel audio resampler's arithmetic (sddc_ddc.h,
// sddc_ddc_channel_audio_resample_*), shared by the device kernel (ddc_channel_audio_resample.hip), the
// CPU backend (cpu/r2iq_cpu.cpp) and the runtime's position bookkeeping (ddc_runtime.cpp).
//
// An output is one fixed sequence of correctly rounded float operations on sample values:
//   a[j mod 4] = fmaf(g_p[j], x[s - j], a[j mod 4])   for j = 0 .. K - 1,   y = (a0 + a1) + (a2 + a3)
// with g_p[j] = h[p + jL] (zero beyond ntaps) and x[i] = 0 before the stream's first sample.  Both
// backends run exactly this: ars_step is the one operation of the loop, ars_sum the closing adds, and
// ars_dot the whole sequence on a contiguous history (the CPU backend's loop; the device kernel walks
// its LDS tile with ars_step in the same order).  Nothing here is contracted: the multiply-adds are
// explicit fmaf, the closing adds have no product next to them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SDDC_ARS_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define SDDC_ARS_FN inline
#endif

namespace sddc {
namespace ars {

#if defined(__HIP_DEVICE_COMPILE__)
SDDC_ARS_FN float ars_step(float g, float x, float a) { return __builtin_fmaf(g, x, a); }
#else
SDDC_ARS_FN float ars_step(float g, float x, float a) { return std::fmaf(g, x, a); }
#endif

SDDC_ARS_FN float ars_sum(const float a[4]) { return (a[0] + a[1]) + (a[2] + a[3]); }

// SDDC_DDC_AUDIO_S16 input: the code as a float, no scale
SDDC_ARS_FN float ars_value(int16_t v) { return (float)v; }

// g: the K taps of the output's phase; x: the output's newest sample x[s], with x[-j] = x[s - j]
SDDC_ARS_FN float ars_dot(const float *g, const float *x, int K)
{
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < K; j++) a[j & 3] = ars_step(g[j], x[-j], a[j & 3]);
    return ars_sum(a);
}

// The host-ordered taps g[p][j] = h[p + jL], K = ceil(ntaps / L) per phase, zero-padded.
inline void ars_order_taps(const float *h, int ntaps, int L, float *g)
{
    const int K = (ntaps + L - 1) / L;
    for (int p = 0; p < L; p++)
        for (int j = 0; j < K; j++) g[p * K + j] = p + j * L < ntaps ? h[p + j * L] : 0.f;
}

// The stream position in reduced form.  With N samples consumed and m0 = ceil(N L / M) outputs
// produced, e = m0 M - N L (0 <= e < M) is all a call needs: its output k has s L + p = e + k M, s
// counted from the call's first sample.
inline int ars_position(int L, int M, uint64_t pos)
{
    const int r = (int)((pos % (uint64_t)M) * (uint64_t)L % (uint64_t)M);
    return r ? M - r : 0;
}
// outputs of nsamp <= 2^40 samples at the reduced position e: the k >= 0 with e + k M < nsamp L
inline uint64_t ars_count(int L, int M, int e, uint64_t nsamp)
{
    const uint64_t span = nsamp * (uint64_t)L;
    return span > (uint64_t)e ? (span - (uint64_t)e + (uint64_t)M - 1) / (uint64_t)M : 0;
}
// the position after that call
inline int ars_advance(int L, int M, int e, uint64_t nsamp, uint64_t nout)
{
    return (int)((int64_t)e + (int64_t)nout * M - (int64_t)nsamp * L);
}

}  // namespace ars
}  // namespace sddc
