// channel_stage.hpp — what the streaming channel kernels share (ddc_channel_decimate.hip,
// ddc_channel_resample.hip): the sample formats, the launch and the pitch of the LDS layout, and the
// description of the stage both kernels begin a tile with.
//
// The stage.  A 256-thread workgroup brings one tile's sample values of one channel stream to LDS
// and keeps the stream's tail for the next call.  A tile needs P consecutive sample values of
// channel c, from index s0 of the call on; s0 < 0 reaches into earlier calls, whose last H values
// per channel the handle keeps on the device (the tail).
//   tail     positions [0, pg) of the tile (pg = -s0 when s0 < 0) come from tail_in, 8 bytes per lane.
//   call     positions [pg, P) come from the call's buffer in aligned 16-byte loads (consecutive
//            lanes consecutive addresses).  A thread issues all its loads of the tile before it uses
//            the first, so a workgroup has its whole tile in flight.  The vectors that straddle the
//            tile's ends are read sample by sample, so nothing outside the stream is touched.  CS16
//            is unpacked with integer ops and scaled by 1 / cs16_scale.
//   store    position p goes to LDS as float2 at the kernel's polyphase transposition,
//            (p mod m) pitch + p div m, whose pitch polyphase_pitch() below has chosen.
//   new tail stream sample i of the call's last H goes to tail_out, written by the tile that owns it
//            (a tile owns its positions from H on; the first tile of a channel also the H before,
//            i.e. the samples of earlier calls), read from tail_in: two buffers that the host swaps
//            per call, so no workgroup reads a tail another one is writing.
// A sample value is the same float whether it comes from the tail or from the call's buffer, so
// the kernels' sums do not depend on the call's cut of the stream.
//
// The stage's text stands in both kernels, line for line alike but for the names (R / M, L / H,
// rmagic / mmagic).  As one __forceinline__ template here it computes the same bits, but the
// compiler then allocates and schedules both kernels differently, and on an MI355X the CF32
// decimator lost 2 - 4.5 % in two rows of tools/channel_decimate_bench.py (the CS16 rows gained
// 2 - 10 %; profiles/channel_stream/).  A fix to the stage is made in both files.
#pragma once

#include <hip/hip_runtime.h>

#include "ddc_kernels.h"

namespace sddc {
namespace chstage {

constexpr int NT = 256;

// one LDS read per instruction (ddc_frame_common.hpp XRD: the compiler's ds_read2 pairs cost 8
// LDS cycles against 2 for a ds_read_b64)
#define CDC_RD(dst, expr) do { dst = (expr); asm volatile("" ::: "memory"); } while (0)

template <bool CS16> struct Fmt;
template <> struct Fmt<false> {
    using Sample = float2;   // (I, Q) floats
    using Vec = float4;      // 2 samples
    static constexpr int V = 2;
};
template <> struct Fmt<true> {
    using Sample = int;      // (I, Q) int16 in one dword, I in the low half
    using Vec = int4;        // 4 samples
    static constexpr int V = 4;
};

__device__ __forceinline__ float2 to_value(float2 x, float) { return x; }
__device__ __forceinline__ float2 to_value(int x, float inv_s)
{
    return make_float2((float)(int)(short)(x & 0xffff) * inv_s, (float)(x >> 16) * inv_s);
}

// One workgroup per item of the call (a.nitems), or full residency with a loop; max_wgs > 0 caps the grid.
template <class Kernel, class Args>
hipError_t launch_stage(const KernelTables &t, Kernel kern, const void *d_iq, float *d_out, const float *d_taps,
                        const float2 *d_tail_in, float2 *d_tail_out, const Args &a, int max_wgs, int device,
                        hipStream_t s)
{
    int occ = 0, cus = 0;
    hipError_t e = launch_geometry(t.lc, reinterpret_cast<const void *>(kern), NT, device, &occ, &cus);
    if (e != hipSuccess) return e;
    long long grid = a.nitems;
    if (grid > (long long)cus * occ) grid = (long long)cus * occ;
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), 0, s, d_iq, d_out, d_taps, d_tail_in, d_tail_out, a);
    return hipGetLastError();
}

// The pitch of a polyphase transposition by `mod` whose rows need `need` slots.  The stage's stores:
// lane l of a 16-lane group holds samples V l + e (V = 2 CF32, 4 CS16) and stores e with one
// ds_write_b64, banked on the float2 index mod 16.  The pitch in [need, max_pitch] with the fewest
// extra LDS cycles (*store_conflicts; tools/channel_decimate_banks.py), the smallest of equals.
inline int polyphase_pitch(int mod, int need, int max_pitch, int V, int *store_conflicts)
{
    int best = -1, best_pitch = 0;
    for (int pitch = need; pitch <= max_pitch; pitch++) {
        int cost = 0;
        for (int e = 0; e < V; e++)
            for (int g0 = 0; g0 < 64; g0 += 16) {
                int cnt[16] = {}, worst = 0;
                for (int l = g0; l < g0 + 16; l++) {
                    const int p = V * l + e, k = ((p % mod) * pitch + p / mod) & 15;
                    if (++cnt[k] > worst) worst = cnt[k];
                }
                cost += worst - 1;
            }
        if (best < 0 || cost < best) {
            best = cost;
            best_pitch = pitch;
        }
    }
    *store_conflicts = best;
    return best_pitch;
}

}  // namespace chstage
}  // namespace sddc
