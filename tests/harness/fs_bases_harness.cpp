// The d = 0 kernel's packed LDS lane bases (extio_sddc_amd/csrc/fs_bases.h) evaluated on the host
// for all 256 threads (tests/test_fs_packed_bases.py): one line per thread t,
//   t c  row pair col wc wt twf twi  t16 t4 tt lane
// each value as the kernel unpacks it from the four packed words, for the LDS byte addresses
// lds0, twl0, wtab0 given on the command line.
#include <cstdio>
#include <cstdlib>

#define __constant__ static const   // the permutation table as a host array
#include "ddc_fs_perm.h"
#include "fs_bases.h"

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s lds0 twl0 wtab0\n", argv[0]);
        return 2;
    }
    const uint32_t lds0 = (uint32_t)std::strtoul(argv[1], nullptr, 0), twl0 = (uint32_t)std::strtoul(argv[2], nullptr, 0),
                   wtab0 = (uint32_t)std::strtoul(argv[3], nullptr, 0);
    for (int t = 0; t < 256; t++) {
        const int c = kFsPerm[t];
        const sddc::FsBases b = sddc::fs_bases_pack(t, c, lds0, twl0, wtab0);
        std::printf("%d %d  %u %u %u %u %u %u %u  %u %u %u %u\n", t, c, sddc::fs_lo(b.p[0]), sddc::fs_hi(b.p[0]),
                    sddc::fs_lo(b.p[1]), sddc::fs_hi(b.p[1]), sddc::fs_lo(b.p[2]), sddc::fs_hi(b.p[2]),
                    sddc::fs_lo(b.p[3]), sddc::fs_t16(b.p[3]), sddc::fs_t4(b.p[3]),
                    sddc::fs_t(b.p[3]), sddc::fs_lane(b.p[3]));
    }
    return 0;
}
