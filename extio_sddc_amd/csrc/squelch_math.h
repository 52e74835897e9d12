// squelch_math.h — the channel squelch's arithmetic (sddc_ddc.h, sddc_ddc_channel_squelch_*), shared word
// for word by the device kernels (ddc_channel_squelch.hip) and the CPU backend (cpu/r2iq_cpu.cpp), as
// blanker_math.h is for the noise blanker, whose block power it uses (blank_power, blank_finite,
// blank_tree).
//
// A gate on a channel's audio, driven by the level of a sense stream, defined in blocks of B =
// kSquelchBlock = 256 samples anchored to the stream position.  Everything here is a fixed sequence of
// float operations that IEEE 754 rounds correctly (*, +, comparisons and selects) and of integer
// operations.  The device side includes this under `#pragma clang fp contract(off)`, the CPU backend and
// the runtime are built with -ffp-contract=off, so both sides produce the same bits, and numpy's float32
// operations reproduce them (tools/channel_squelch_model.py).
//
//   squelch_q_real   q = x * x, one rounding (a real sense stream; S16 read as (float)v).
//   blank_power      q = (I * I) + (Q * Q), three roundings (a complex sense stream).
//   block level p_k  blank_tree over the block's 256 q values in sample order; a q that is not
//                    blank_finite enters as 0 and marks the block bad.
//   squelch_flags    LEVEL: u = p > To, v = p > Tc (Tc <= To); NOISE: u = p < To, v = p < Tc (Tc >= To);
//                    a bad block has u = v = false.  To and Tc are 256 times the mean-square thresholds of
//                    the set call (squelch_scale: exact, a power of two).
//   squelch_step     after block k: r = u ? min(r + 1, A) : 0; n = v ? 0 : min(n + 1, H + 1);
//                    open = open ? (n <= H) : (r >= A).  All zero on a new stream.
//   squelch_kind     from G_k (open after block k - 1), G_{k-1} and the fade flag: how block k's samples
//                    are weighted: kZero (w = 0), kPass (w = 1), kUp (w = (i + 1) / 256), kDown (w =
//                    (255 - i) / 256).  OFF is kPass and MUTE is kZero from sample 0.
//   squelch_weight   the weight of sample i of a kUp / kDown block: an integer below 2^8 times 2^-8, exact.
//   squelch_apply    kPass: x; kZero: +0; else x * w, one rounding.  (The F32 to F32 path passes the stored
//                    word on kPass instead, so a NaN keeps its payload; S16 codes survive (float) and
//                    demod_s16 unchanged.)
//
// Range of the bit-exact guarantee: the blanker's.  Components that are 0 or of magnitude in [2^-40,
// 2^40]: q is 0 or in [2^-80, 2^81], a block level 0 or in [2^-80, 2^89]; thresholds finite, >= 0 and
// <= 2^80, so 256 T <= 2^88: nothing overflows and nothing on the deciding path is subnormal.  x * w
// with |x| >= 2^-40 and w >= 2^-8 is normal too.  Outside the range the operations are the same on both
// sides; no value is a reason for a memory fault.
//
// Accuracy against the float64 evaluation of the same definition on the same float32 samples: q carries
// at most 3 roundings and the tree 8 more, each of relative size u = 2^-24, the comparison none (256 T
// is exact): u_k or v_k can differ only where |p64 - T| <= 1.01 * 11 u T, which
// tests/test_channel_squelch_cpu.py checks.
#pragma once

#include <stdint.h>

#include "blanker_math.h"

#if defined(__HIPCC__)
#define SDDC_SQ_FN __host__ __device__ __forceinline__
#else
#define SDDC_SQ_FN inline
#endif

namespace sddc {
namespace squelch {

constexpr int kSquelchBlock = blank::kBlankBlock;   // SDDC_DDC_SQUELCH_BLOCK
constexpr int kSquelchOff = 0, kSquelchLevel = 1, kSquelchNoise = 2, kSquelchMute = 3;   // SDDC_DDC_SQUELCH_*
constexpr int kSenseSelf = 0, kSenseF32 = 1, kSenseS16 = 2, kSenseCF32 = 3, kSenseCS16 = 4;   // .._SENSE_*
constexpr int kSquelchMaxAttack = 255, kSquelchMaxHang = 65535;
constexpr int kZero = 0, kPass = 1, kUp = 2, kDown = 3;

SDDC_SQ_FN float squelch_q_real(float x) { return x * x; }

// (host) 256 T: exact for T <= 2^80
inline float squelch_scale(float T) { return T * 256.f; }

SDDC_SQ_FN void squelch_flags(float p, bool bad, int mode, float To, float Tc, bool *u, bool *v)
{
    const bool noise = mode == kSquelchNoise;
    const bool a = noise ? p < To : p > To, b = noise ? p < Tc : p > Tc;
    *u = !bad && a;
    *v = !bad && b;
}

SDDC_SQ_FN void squelch_step(bool u, bool v, uint32_t A, uint32_t H, uint32_t *r, uint32_t *n, uint32_t *open)
{
    const uint32_t r1 = *r + 1 < A ? *r + 1 : A, n1 = *n + 1 < H + 1 ? *n + 1 : H + 1;
    *r = u ? r1 : 0u;
    *n = v ? 0u : n1;
    *open = *open ? (*n <= H ? 1u : 0u) : (*r >= A ? 1u : 0u);
}

// g: G_k, gp: G_{k-1} (0 or 1)
SDDC_SQ_FN int squelch_kind(int mode, uint32_t g, uint32_t gp, int fade)
{
    if (mode == kSquelchOff) return kPass;
    if (mode == kSquelchMute) return kZero;
    if (!fade || g == gp) return g ? kPass : kZero;
    return g ? kUp : kDown;
}

// kind is kUp or kDown, 0 <= i < 256
SDDC_SQ_FN float squelch_weight(int kind, int i)
{
    return (float)(kind == kUp ? i + 1 : 255 - i) * 0.00390625f;
}

SDDC_SQ_FN float squelch_apply(int kind, int i, float x)
{
    if (kind == kPass) return x;
    if (kind == kZero) return 0.f;
    return x * squelch_weight(kind, i);
}

}  // namespace squelch
}  // namespace sddc
