// split_coeffs.h — the (P, r) coefficients of the split x filter of one bin, in double, rounded
// once: the one place both table-build kernels (build_fs_tables_kernel, ddc_fs.hip;
// build_split_filter_kernel, ddc_persistent.hip) take them from.  Plain C++ that also compiles
// without hipcc (tests/harness/split_coeffs_harness.cpp prints the table on the host,
// tests/test_split_coeffs_harness.py holds every bin to the per-bin bar).
//
//   P = Hh (1 - i W),  Q = Hh (1 + i W),  W = e^{-2 pi i b / 8192},  r = Q / (i P)
//
// W is NOT read from the float post8192 table: with |W_f|^2 != 1 the ratio Q / (i P) is no longer
// real, and the real part the kernels keep is off by a relative (|W_f|^2 - 1) / (|1 - i W_f| |1 + i W_f|),
// which grows like 1 / |b - 2048| (1e-5 at bins 2045..2051, above the project's bar before any
// float32 arithmetic).  Nor are 1 -+ i W formed by subtraction.  With phi = pi (2048 - b) / 4096,
// i W = e^{i phi}, and with (c, s) = (cos, sin)(phi / 2):
//   1 - i W = -2 i s e^{i phi / 2} = 2 s (s - i c),   1 + i W = 2 c e^{i phi / 2} = 2 c (c + i s),
//   r = c / s = cot(pi / 4 - pi b / 8192)
// so every factor is a product of exactly rounded values of sin and cos of the exact argument
// (2048 - b) / 8192 (in half turns): no cancellation at any bin, r exactly real before its one
// rounding.  r is infinite at b = 2048 (s = 0, P = 0); the two kernels keep that entry differently:
//   kSplitQ0:  p = Q, r = 0          (the d = 0 frame kernel's wave-0 path, F = Q conj Z)
//   kSplit2p64: p = Q / (i 2^64), r = 2^64   (split_pr as it stands: exact power-of-two scalings)
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define SDDC_HD __host__ __device__
#else
#define SDDC_HD
#endif

namespace sddc {

enum SplitMid { kSplitQ0 = 0, kSplit2p64 = 1 };

struct SplitCoeffs {
    float px, py;   // P
    float r;
};

// (hr, hi): Hh of the bin's inverse input; bin in [0, 4096)
SDDC_HD inline SplitCoeffs split_pr_coeffs(double hr, double hi, int bin, SplitMid mid)
{
    double s, c;
    const double a = (double)(2048 - bin) / 8192.0;   // phi / 2 in half turns, exact
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(a, &s, &c);
#else
    s = std::sin(3.14159265358979323846 * a);
    c = std::cos(3.14159265358979323846 * a);
#endif
    SplitCoeffs o;
    if (bin == 2048) {   // s = 0, c = 1: Q = 2 Hh
        const double q0 = 2.0 * hr, q1 = 2.0 * hi;
        if (mid == kSplitQ0) {
            o.px = (float)q0;
            o.py = (float)q1;
            o.r = 0.f;
        } else {
            constexpr double k = 0x1p-64;
            o.px = (float)(q1 * k);   // -i Q 2^-64
            o.py = (float)(-q0 * k);
            o.r = 0x1p64f;
        }
        return o;
    }
    const double pr = 2.0 * s * s, pi = -2.0 * s * c;   // 1 - i W
    o.px = (float)(hr * pr - hi * pi);
    o.py = (float)(hr * pi + hi * pr);
    o.r = (float)(c / s);
    return o;
}

}  // namespace sddc
