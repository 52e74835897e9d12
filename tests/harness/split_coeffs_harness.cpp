// split_coeffs_harness — the build kernels' (P, r) coefficient code (extio_sddc_amd/csrc/split_coeffs.h)
// compiled for the host: prints "bin p.x p.y r" for the 4096 bins with Hh = 1, floats with 9
// significant digits (exact round trip).  argv[1]: "q0" (the d = 0 frame kernel's bin-2048
// entry, default) or "2p64" (the persistent kernel's).  tests/test_split_coeffs_harness.py
// compares it with numpy in longdouble.
#include <cstdio>
#include <cstring>

#include "split_coeffs.h"

int main(int argc, char **argv)
{
    sddc::SplitMid mid = sddc::kSplitQ0;
    if (argc > 1) {
        if (!std::strcmp(argv[1], "2p64")) mid = sddc::kSplit2p64;
        else if (std::strcmp(argv[1], "q0")) {
            std::fprintf(stderr, "usage: %s [q0|2p64]\n", argv[0]);
            return 2;
        }
    }
    for (int b = 0; b < 4096; b++) {
        const sddc::SplitCoeffs c = sddc::split_pr_coeffs(1.0, 0.0, b, mid);
        std::printf("%d %.9g %.9g %.9g\n", b, (double)c.px, (double)c.py, (double)c.r);
    }
    return 0;
}
