// blanker_math.h — the channel noise blanker's arithmetic (sddc_ddc.h, sddc_ddc_channel_blank_*), shared
// word for word by the device kernels (ddc_channel_blank.hip) and the CPU backend (cpu/r2iq_cpu.cpp), as
// agc_math.h is for the AGC.
//
// A feed-forward impulse blanker on a channel's IQ stream, defined in blocks of B = kBlankBlock = 256
// samples anchored to the stream position.  Everything here is a fixed sequence of float operations
// that IEEE 754 rounds correctly: *, +, comparisons and selects, no libm, no fmaf, no fminf / fmaxf.
// The device side includes this under `#pragma clang fp contract(off)`, the CPU backend and the runtime
// are built with -ffp-contract=off, so both sides produce the same bits, and numpy's float32 operations
// reproduce them (tools/channel_blanker_model.py).
//
//   blank_power      q = (I * I) + (Q * Q), three roundings.
//   blank_finite     q <= FLT_MAX; a NaN or an infinite q is "non-finite": always a hit of a channel that
//                    is not bypassed, and it enters the block power as 0.
//   block power p_k  the balanced pairwise tree over the block's 256 values in sample order: level 0
//                    adds (q[0] + q[1]), (q[2] + q[3]), ..., eight levels (blank_tree on an array; the
//                    kernel does the lower six levels across lanes and the upper two in a lane, the same
//                    additions: a + b and b + a are the same float).
//   blank_reference  P_k of the n = min(k, M) block powers before block k, w[0] = p_{k-n} ... w[n-1] =
//                    p_{k-1}.  MEAN: S = (..((w[0] + w[1]) + w[2]) ..) + w[n-1], P = S * rn[n], rn[n] =
//                    (float)(1.0 / n) (a table of constants).  MEDIAN: the value of rank (n - 1) / 2
//                    (0-based, ascending), found by comparisons alone.  n == 0: no finite sample hits.
//   blank_threshold  t = thr * P; t_k = (t > qmin) ? t : qmin, with thr = (float)((double)k2 / 256.0)
//                    made at set time (blank_thr).  thr == 0: the channel is bypassed, a pure delay.
//   blank_hit        !finite || (n > 0 && q > t_k).
//
// The stream (the definition that both backends compute), per channel, with the guard g: blank[i] is
// true if a hit[j] exists with |j - i| <= g, j >= 0; the output y[n] is (+0, +0) for n < g and otherwise
// blank[n - g] ? (+0, +0) : x[n - g], the stored sample bit for bit.  y[n] needs hits up to j = n only,
// so the stage is causal with a delay of g.  With L[n] the index of the last hit at or before n, blank[n
// - g] is L[n] >= n - 2 g: of the last 2 g hit flags only the most recent set one matters, which is how
// both backends keep them.
//
// Range of the bit-exact guarantee: components that are 0 or of magnitude in [2^-40, 2^40], k2 <= 2^40,
// qmin <= 2^80.  Then I * I and Q * Q are 0 or in [2^-80, 2^80], q is 0 or in [2^-80, 2^81], a block
// power is 0 or in [2^-80, 2^89], S (at most 16 terms) below 2^93, P likewise, thr in [2^-8, 2^32] and
// t below 2^125 and, where P > 0, at least 2^-88: nothing overflows, and nothing on the deciding path is
// subnormal (the smallest normal float is 2^-126), so backends that flush subnormals and backends that
// keep them agree.  Outside the range the operations are still the same on both sides; what the header
// promises there is only that no out-of-range value is a reason for a memory fault.
//
// Accuracy against the float64 evaluation of the same definition on the same float32 samples: q carries
// 3 roundings (relative 2 u each at most, u = 2^-24; the products are exact in float64's view up to
// u), a block power 8 more on top of each q, the MEAN M - 1 additions and one multiply, the threshold
// thr's own rounding and one multiply: the hit flag can differ only where |q64 - t64| <= 1.01 (8 + M + 5)
// u t64, which tests/test_channel_blanker_cpu.py checks.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SDDC_BLANK_FN __host__ __device__ __forceinline__
#else
#define SDDC_BLANK_FN inline
#endif

namespace sddc {
namespace blank {

constexpr int kBlankBlock = 256;       // SDDC_DDC_BLANKER_BLOCK
constexpr int kBlankMaxGuard = 64;     // SDDC_DDC_BLANKER_MAX_GUARD
constexpr int kBlankMaxRef = 16;       // SDDC_DDC_BLANKER_MAX_REF_BLOCKS
constexpr int kBlankMean = 0, kBlankMedian = 1;
constexpr float kBlankFltMax = 3.40282346638528859812e+38f;

SDDC_BLANK_FN float blank_power(float i, float q)
{
    const float a = i * i, b = q * q;
    return a + b;
}

SDDC_BLANK_FN bool blank_finite(float q) { return q <= kBlankFltMax; }

// rn[n] = (float)(1.0 / n), n = 1..16
SDDC_BLANK_FN float blank_rn(int n)
{
    static constexpr float rn[kBlankMaxRef + 1] = {
        0.f,
        (float)(1.0 / 1.0),  (float)(1.0 / 2.0),  (float)(1.0 / 3.0),  (float)(1.0 / 4.0),
        (float)(1.0 / 5.0),  (float)(1.0 / 6.0),  (float)(1.0 / 7.0),  (float)(1.0 / 8.0),
        (float)(1.0 / 9.0),  (float)(1.0 / 10.0), (float)(1.0 / 11.0), (float)(1.0 / 12.0),
        (float)(1.0 / 13.0), (float)(1.0 / 14.0), (float)(1.0 / 15.0), (float)(1.0 / 16.0)};
    return rn[n];
}

// The block power of q[0..255] (non-finite values already replaced by 0); q is overwritten.
inline float blank_tree(float *q)
{
    for (int len = kBlankBlock; len > 1; len >>= 1)
        for (int i = 0; i < len / 2; i++) q[i] = q[2 * i] + q[2 * i + 1];
    return q[0];
}

// P_k of w[0..n-1], 1 <= n <= 16, oldest first.
inline float blank_reference(const float *w, int n, int mode)
{
    if (mode == kBlankMean) {
        float S = w[0];
        for (int b = 1; b < n; b++) S = S + w[b];
        return S * blank_rn(n);
    }
    const int r = (n - 1) / 2;
    float P = w[0];
    for (int a = 0; a < n; a++) {
        int rank = 0;
        for (int b = 0; b < n; b++) rank += (w[b] < w[a] || (w[b] == w[a] && b < a)) ? 1 : 0;
        P = rank == r ? w[a] : P;
    }
    return P;
}

SDDC_BLANK_FN float blank_threshold(float thr, float P, float qmin)
{
    const float t = thr * P;
    return t > qmin ? t : qmin;
}

// n: the number of reference blocks (0 in block 0 of a stream); the channel is not bypassed
SDDC_BLANK_FN bool blank_hit(float q, float t, int n) { return !blank_finite(q) || (n > 0 && q > t); }

// (host) thr = (float)((double)k2 / 256.0)
inline float blank_thr(float k2) { return (float)((double)k2 / 256.0); }

}  // namespace blank
}  // namespace sddc
