// fs_shares.h — the d = 0 kernel's per-workgroup frame split as a cumulative-share table in the
// kernel arguments (plain C++: shared by the kernel, the runtime and the controller,
// fs_split_controller.hpp).
//
// Workgroup v of G takes the frames [fs_share_start(ns, G, v), fs_share_start(ns, G, v + 1)) of
// the ns frames of a launch: a(v) = ns P[v] >> 15 for v < G, a(G) = ns, with P[v] in 0..32768 the
// 15-bit fixed-point share of the frames in front of workgroup v, non-decreasing.  So the ranges
// are monotone and cover [0, ns) exactly once whatever the table holds (a table that is not
// monotone is a host bug: fs_shares_valid), empty ranges included.  For ns <= 32768 every integer
// boundary A is representable (P = ceil(32768 A / ns) gives a = A: ns P < 32768 A + ns); above, the
// boundaries fall on a grid of ns / 32768 frames.  2 KB of the 4 KB kernel argument limit.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SDDC_HD __host__ __device__
#else
#define SDDC_HD
#endif

namespace sddc {

constexpr int kFsShareMaxG = 1024;   // workgroups a table covers (4 x 256 CUs)
constexpr int kFsShareBits = 15;
constexpr unsigned kFsShareOne = 1u << kFsShareBits;

struct FsShares {
    uint32_t p[kFsShareMaxG / 2];   // P[v]: 16 bits each, v even in the low half
};

SDDC_HD inline unsigned fs_share_get(const FsShares &t, int v) { return (t.p[v >> 1] >> (16 * (v & 1))) & 0xffffu; }
inline void fs_share_set(FsShares &t, int v, unsigned pv)
{
    const int sh = 16 * (v & 1);
    t.p[v >> 1] = (t.p[v >> 1] & ~(0xffffu << sh)) | ((pv & 0xffffu) << sh);
}

// first frame of workgroup v (v >= G: ns)
SDDC_HD inline int fs_share_start(int ns, int G, int v, const FsShares &t)
{
    if (v >= G) return ns;
    return (int)(((long long)ns * (long long)fs_share_get(t, v)) >> kFsShareBits);
}

// the table entry of boundary A (frames in front of the workgroup) of ns frames
inline unsigned fs_share_of(long long A, int ns)
{
    if (ns <= 0 || A <= 0) return 0u;
    if (A >= ns) return kFsShareOne;
    return (unsigned)((A * (long long)kFsShareOne + ns - 1) / ns);
}

inline bool fs_shares_valid(const FsShares &t, int G)
{
    if (G < 1 || G > kFsShareMaxG) return false;
    unsigned last = 0u;
    for (int v = 0; v < G; v++) {
        const unsigned pv = fs_share_get(t, v);
        if (pv < last || pv > kFsShareOne) return false;
        last = pv;
    }
    return true;
}

}  // namespace sddc
