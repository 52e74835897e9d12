// fs_bases.h — the d = 0 fused-split kernel's LDS layout helpers and its frame-invariant lane
// addresses, packed two to a register (plain C++: shared by the kernel, ddc_fs.hip, and the host
// harness tests/harness/fs_bases_harness.cpp).
//
// Every LDS access of the frame loop is one lane base plus a per-register immediate, and the
// bases depend on the thread index t and its F2 column c = kFsPerm[t] only: they never change
// during a launch.  Held unpacked they would cost seven VGPRs at 128, so the loop used to
// re-derive each one from t and c in every pass (about 45 VALU per wave and frame, three of them
// quarter-rate multiplies).  Every base is a byte address below 65 536 (the workgroup's LDS is
// 40 852 bytes), so two share one register and a use costs one v_and_b32 or v_lshrrev_b32:
//   p[0] = row   | pair << 16     the F0 / I2 row of t,        the F1 / I1 pair lane of t
//   p[1] = col   | wc << 16       the F2 / I0 column of c,     the twiddle base W^c
//   p[2] = wt    | twf << 16      the twiddle base W^t,        F1's table column fs_pair_col(t)
//   p[3] = twi   | (16 t) << 16   I1's table column fs_pair_row(t), the thread's P-table offset
// 16 t is the byte offset of the lane's 16-byte P pair; 4 t (the input load offset), t and the
// lane number are shifts of the same half, so the loop needs no other copy of t.
#pragma once

#include <stdint.h>

#ifndef SDDC_HD
#if defined(__HIPCC__)
#define SDDC_HD __host__ __device__
#else
#define SDDC_HD
#endif
#endif

namespace sddc {

// fs_slot(t, 0): the F0 / I2 row of thread t
SDDC_HD inline int fs_row_slot(int t) { return 272 * (t >> 4) + (t >= 128) + 34 * ((t & 15) >> 1) + (t & 1); }
// fs_pair_lane: F1's and I1's thread t takes row u = 2 (t >> 5) + (t & 1) of each 16-row block,
// column j = (t >> 1) & 15: its base slot fs_slot(u, j) = 34 (t >> 5) + (t & 31) = t + 2 (t >> 5)
// (the block's 272 r + [r >= 8] is the immediate)
SDDC_HD inline int fs_pair_row(int t) { return 2 * (t >> 5) + (t & 1); }
SDDC_HD inline int fs_pair_col(int t) { return (t >> 1) & 15; }
SDDC_HD inline int fs_pair_slot(int t) { return t + 2 * (t >> 5); }
// F2 reads / I0 stores of column c = 16 h + cl: rows 16 h + r, column cl at
// 272 h + [h >= 8] + 2 cl (+ the immediate 34 (r >> 1) + (r & 1))
SDDC_HD inline int fs_col_slot(int c) { return 272 * (c >> 4) + (c >= 128) + 2 * (c & 15); }
// the twiddle bases W^j (j < 256) sit at j + [j >= 128], W^{4j} kFsTw later
SDDC_HD inline int fs_tw_slot(int j) { return j + (j >= 128); }

constexpr int kFsLds = 4352;        // float2 slots of the exchange buffer
constexpr int kFsTw = 256 + 1;      // float2 slots of one twiddle-base table
constexpr int kFsTwl = 15 * 16;     // float2 slots of the F1 / I1 twiddle table

struct FsBases {
    uint32_t p[4];
};

// lds0, twl0, wtab0: the byte addresses of the exchange buffer, the F1 / I1 table and the twiddle
// bases in the workgroup's LDS
SDDC_HD inline FsBases fs_bases_pack(int t, int c, uint32_t lds0, uint32_t twl0, uint32_t wtab0)
{
    FsBases b;
    b.p[0] = (lds0 + 8u * (uint32_t)fs_row_slot(t)) | (lds0 + 8u * (uint32_t)fs_pair_slot(t)) << 16;
    b.p[1] = (lds0 + 8u * (uint32_t)fs_col_slot(c)) | (wtab0 + 8u * (uint32_t)fs_tw_slot(c)) << 16;
    b.p[2] = (wtab0 + 8u * (uint32_t)fs_tw_slot(t)) | (twl0 + 8u * (uint32_t)fs_pair_col(t)) << 16;
    b.p[3] = (twl0 + 8u * (uint32_t)fs_pair_row(t)) | (16u * (uint32_t)t) << 16;
    return b;
}

// the halves of one packed word
SDDC_HD inline uint32_t fs_lo(uint32_t w) { return w & 0xffffu; }
SDDC_HD inline uint32_t fs_hi(uint32_t w) { return w >> 16; }
// of p[3]: the byte offsets 16 t and 4 t, the thread index and the lane number
SDDC_HD inline uint32_t fs_t16(uint32_t w) { return w >> 16; }
SDDC_HD inline uint32_t fs_t4(uint32_t w) { return w >> 18; }
SDDC_HD inline uint32_t fs_t(uint32_t w) { return w >> 20; }
SDDC_HD inline uint32_t fs_lane(uint32_t w) { return (w >> 20) & 63u; }

}  // namespace sddc
