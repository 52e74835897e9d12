// ddc_channel_demod.hip — the channel demodulator for gfx950 (sddc_ddc_channel_demodulate_device):
// AM, FM (quadrature discriminator) or BFO (product detector) audio from every channel stream of the
// DDC's output, CF32 or CS16 in, F32 or S16 out, streaming (each channel's last sample value and the
// stream position live in the handle), and optionally each channel's mean power over the call.
//
// Work item: one (channel, tile) of kChDemTile samples, taken by a 256-thread workgroup.  The mode,
// the gain and the BFO word of an item are workgroup-uniform (one 16-byte scalar load), the mode a
// scalar branch.  There is no reuse, so nothing but the power passes through LDS:
//   loads    the tile's samples in aligned 16-byte loads (V = 2 CF32 or 4 CS16 samples), vector kv =
//            tid + 256 k at position kv V - al of the tile (al = the first sample's offset within
//            its 16-byte line): consecutive lanes read consecutive addresses, and a thread issues
//            every load of the tile before it uses the first.  The vectors across the tile's ends
//            are read sample by sample, so nothing outside the stream is touched.
//   previous FM only.  The sample before a thread's first comes from the lane below (one cross-lane
//            move of the raw sample); lane 0 of a wave reads it from the call's buffer (one 8- or
//            4-byte load per vector, issued with the others); the sample before the tile's first is
//            read by thread 0 from the call's buffer, or from the handle's last-sample buffer when
//            the tile starts the call.  A sample value is the same float on every one of these
//            paths (to_value of the same bits), which is what makes the result cut-invariant.
//   last     the thread that holds the call's last sample of a channel writes its value to the
//            other last-sample buffer (the host swaps the two per call, so no workgroup reads what
//            another one writes).
//   stores   a thread's V outputs in one store where they are whole and the address is aligned to
//            V outputs (16 bytes for CS16 in / F32 out, 8 or 4 bytes otherwise: the outputs follow
//            the loads' sample groups, so loads and stores are both fully coalesced), else one by
//            one: 4-byte stores for F32, 2-byte stores for S16.  Plain stores: nontemporal ones measured
//            no faster.
//   power    (d_power given) each sample's fmaf(I, I, Q Q) goes to LDS at its position in the tile
//            (zeros past the tile's end); thread t adds positions t, t + 256, .. in that order, the
//            wave adds its 64 sums in an xor butterfly (32, 16, .. 1: every lane forms the same
//            sums), thread 0 adds the four waves as (0 + 1) + (2 + 3) and stores the tile's partial.
//            channel_power_finish_kernel then adds a channel's partials (thread t tiles t, t + 256,
//            .. in order, then a binary tree over the 256 threads) and scales by 1 / nsamp.  The
//            order depends on nsamp alone: not on the alignment, the grid or the other channels,
//            and there are no atomics.  Without d_power the kernel instance has no LDS and no barrier.
//
// Determinism: an output is demod_math.h's fixed sequence of float operations on its own sample
// values (FM: and the one before); the BFO phase is the exact 32-bit product w (pos + i).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "channel_stage.hpp"
#include "ddc_kernels.h"

// demod_math.h and every float operation below: no contraction (the CPU backend computes the same bits)
#pragma clang fp contract(off)
#include "demod_math.h"

namespace sddc {
namespace {

using namespace chstage;

constexpr int T = kChDemTile;
static_assert(T % NT == 0 && T <= 8192, "whole rounds of the power sum; small tests");

struct Args {
    long long nsamp, tiles, nitems;   // per channel: samples, tiles; items of the call
    size_t in_stride, out_stride;     // components (float or int16) / output samples per channel
    unsigned pos;                     // the stream position of the call's first sample mod 2^32
    float inv_s;                      // CS16: 1 / cs16_scale
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
template <bool S16, int V> struct OutVec;
template <> struct OutVec<false, 2> { using type = f32x2; };
template <> struct OutVec<false, 4> { using type = f32x4; };
template <> struct OutVec<true, 2> { using type = s16x2; };
template <> struct OutVec<true, 4> { using type = s16x4; };

// Outputs e = lo .. hi - 1 of a thread's V, output 0 at address o (never dereferenced when lo > 0).
template <bool S16, int V> __device__ __forceinline__ void store_group(char *o, const float (&y)[V], int lo, int hi)
{
    using E = std::conditional_t<S16, short, float>;
    using OV = typename OutVec<S16, V>::type;
    E v[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        if constexpr (S16) v[e] = demod::demod_s16(y[e]);
        else v[e] = y[e];
    }
    if (lo == 0 && hi == V && ((uintptr_t)o & (sizeof(OV) - 1)) == 0) {
        OV x;
#pragma unroll
        for (int e = 0; e < V; e++) x[e] = v[e];
        *reinterpret_cast<OV *>(o) = x;
    } else {
#pragma unroll
        for (int e = 0; e < V; e++)
            if (e >= lo && e < hi) reinterpret_cast<E *>(o)[e] = v[e];
    }
}

__device__ __forceinline__ int lane_below(int x) { return __shfl_up(x, 1); }
__device__ __forceinline__ float2 lane_below(float2 x) { return make_float2(__shfl_up(x.x, 1), __shfl_up(x.y, 1)); }

template <bool CS16, bool S16, bool POWER>
__global__ __launch_bounds__(NT) void channel_demod_kernel(const void *__restrict__ iq, void *__restrict__ out,
                                                           const ChDemChannel *__restrict__ chan,
                                                           const float2 *__restrict__ last_in,
                                                           float2 *__restrict__ last_out, float *__restrict__ partial,
                                                           const Args a)
{
    using F = Fmt<CS16>;
    using Sample = typename F::Sample;
    using Vec = typename F::Vec;
    constexpr int V = F::V;
    constexpr int KV = (T / V + 1 + NT - 1) / NT;   // vectors that hold a sample of a tile: T / V + 1 at most
    constexpr int ES = S16 ? 2 : 4;                 // bytes per output sample
    __shared__ float pw[POWER ? T : 1];
    __shared__ float wsum[NT / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63;

    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {   // workgroup-uniform
        const long long c = item / a.tiles, t = item - c * a.tiles, s0 = t * T;
        const int tn = (int)(a.nsamp - s0 < T ? a.nsamp - s0 : T);
        const ChDemChannel ch = chan[c];
        const float g = ch.gain;
        // sample s0 of the channel, al samples past a 16-byte line; vector kv starts at position kv V - al
        const char *gp = static_cast<const char *>(iq) + (size_t)c * a.in_stride * (sizeof(Sample) / 2) +
                         (size_t)s0 * sizeof(Sample);
        const int al = (int)(((uintptr_t)gp / sizeof(Sample)) % V);
        const int nv = (tn + al + V - 1) / V;   // vectors that hold a sample of the tile: <= KV NT
        const bool fm = ch.mode == 1;           // SDDC_DDC_DEMOD_FM
        auto sample_at = [&](int p) { return *reinterpret_cast<const Sample *>(gp + (long long)p * (int)sizeof(Sample)); };

        // every load of the tile, then the first use
        Sample raw[KV][V], below[KV];
        float2 halo = make_float2(0.f, 0.f);
#pragma unroll
        for (int k = 0; k < KV; k++) {
            const int kv = tid + k * NT, e0 = kv * V - al;
#pragma unroll
            for (int e = 0; e < V; e++) raw[k][e] = Sample{};
            below[k] = Sample{};
            if (kv >= nv) continue;
            if (e0 >= 0 && e0 + V <= tn) {
                const Vec x = *reinterpret_cast<const Vec *>(gp + (long long)e0 * (int)sizeof(Sample));
                if constexpr (CS16) {
                    raw[k][0] = x.x;
                    raw[k][1] = x.y;
                    raw[k][2] = x.z;
                    raw[k][3] = x.w;
                } else {
                    raw[k][0] = make_float2(x.x, x.y);
                    raw[k][1] = make_float2(x.z, x.w);
                }
            } else {   // a vector across an end of the tile: the samples inside, one by one
#pragma unroll
                for (int e = 0; e < V; e++)
                    if (e0 + e >= 0 && e0 + e < tn) raw[k][e] = sample_at(e0 + e);
            }
            if (fm && lane == 0 && kv > 0) below[k] = sample_at(e0 - 1);   // 0 <= e0 - 1 < tn
        }
        if (fm && tid == 0) halo = s0 > 0 ? to_value(sample_at(-1), a.inv_s) : last_in[c];

        auto body = [&](auto mode_c) {
            constexpr int MODE = decltype(mode_c)::value;
#pragma unroll
            for (int k = 0; k < KV; k++) {
                const int kv = tid + k * NT, e0 = kv * V - al;
                float2 pv = make_float2(0.f, 0.f);
                if constexpr (MODE == 1) {   // all lanes: the move is outside the test of kv
                    Sample b = lane_below(raw[k][V - 1]);
                    if (lane == 0) b = below[k];
                    pv = to_value(b, a.inv_s);
                }
                if (kv >= nv) continue;
                float2 v[V];
                float y[V];
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const int p = e0 + e;
                    v[e] = to_value(raw[k][e], a.inv_s);
                    if constexpr (MODE == 0) {
                        y[e] = demod::demod_am(v[e].x, v[e].y, g);
                    } else if constexpr (MODE == 1) {
                        float2 q = e == 0 ? pv : v[e > 0 ? e - 1 : 0];
                        if (p == 0) q = halo;   // thread 0 alone holds position 0
                        y[e] = demod::demod_fm(v[e].x, v[e].y, q.x, q.y, g);
                    } else {
                        y[e] = demod::demod_bfo(v[e].x, v[e].y, ch.word * (a.pos + (unsigned)(s0 + p)), g);
                    }
                    if (p >= 0 && p < tn) {
                        if constexpr (POWER) pw[p] = demod::demod_power(v[e].x, v[e].y);
                        if (s0 + p == a.nsamp - 1) last_out[c] = v[e];
                    }
                }
                char *o = static_cast<char *>(out) + ((long long)c * (long long)a.out_stride + s0 + e0) * ES;
                store_group<S16, V>(o, y, e0 < 0 ? -e0 : 0, tn - e0 < V ? tn - e0 : V);
            }
        };
        if (ch.mode == 0) body(std::integral_constant<int, 0>());
        else if (ch.mode == 1) body(std::integral_constant<int, 1>());
        else body(std::integral_constant<int, 2>());

        if constexpr (POWER) {
            for (int p = tn + tid; p < T; p += NT) pw[p] = 0.f;
            __syncthreads();
            float acc = pw[tid];
#pragma unroll
            for (int j = 1; j < T / NT; j++) acc += pw[tid + j * NT];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
            if (lane == 0) wsum[tid >> 6] = acc;
            __syncthreads();   // also: every read of pw is done before the next item's writes
            if (tid == 0) partial[c * a.tiles + t] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        }
    }
}

// P_c = (the sum of channel c's tile partials) x inv_n: thread t adds tiles t, t + 256, .. in order,
// then a binary tree over the threads; one workgroup per channel.
__global__ __launch_bounds__(NT) void channel_power_finish_kernel(const float *__restrict__ partial, long long tiles,
                                                                  float inv_n, float *__restrict__ power)
{
    __shared__ float sm[NT];
    const int tid = (int)threadIdx.x;
    const long long c = blockIdx.x;
    float acc = 0.f;
    for (long long j = tid; j < tiles; j += NT) acc += partial[c * tiles + j];
    sm[tid] = acc;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) sm[tid] += sm[tid + s];
        __syncthreads();
    }
    if (tid == 0) power[c] = sm[0] * inv_n;
}

using Kernel = void (*)(const void *, void *, const ChDemChannel *, const float2 *, float2 *, float *, const Args);
template <bool CS16, bool S16> Kernel pick(bool power)
{
    return power ? channel_demod_kernel<CS16, S16, true> : channel_demod_kernel<CS16, S16, false>;
}

}  // namespace

hipError_t launch_channel_demod(const KernelTables &t, const void *d_iq, int cs16, float cs16_scale, int nch,
                                size_t nsamp, size_t in_stride, const ChDemChannel *d_chan, uint32_t pos,
                                const float2 *d_last_in, float2 *d_last_out, void *d_out, int s16, size_t out_stride,
                                float *d_power, float *d_partial, int max_wgs, int device, hipStream_t s)
{
    if (!d_iq || !d_out || !d_chan || !d_last_in || !d_last_out || nch < 1 || nsamp == 0 ||
        nsamp > ((size_t)1 << 40) || (d_power && !d_partial))
        return hipErrorInvalidValue;
    Args a;
    a.nsamp = (long long)nsamp;
    a.tiles = (long long)channel_demod_tiles(nsamp);
    a.nitems = a.tiles * nch;
    a.in_stride = nch > 1 ? in_stride : 0;
    a.out_stride = nch > 1 ? out_stride : 0;
    a.pos = pos;
    a.inv_s = cs16 ? (float)(1.0 / (double)cs16_scale) : 1.f;
    const bool power = d_power != nullptr;
    const Kernel kern = cs16 ? (s16 ? pick<true, true>(power) : pick<true, false>(power))
                             : (s16 ? pick<false, true>(power) : pick<false, false>(power));
    int occ = 0, cus = 0;
    hipError_t e = launch_geometry(t.lc, reinterpret_cast<const void *>(kern), NT, device, &occ, &cus);
    if (e != hipSuccess) return e;
    long long grid = a.nitems;
    if (grid > (long long)cus * occ) grid = (long long)cus * occ;
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), 0, s, d_iq, d_out, d_chan, d_last_in, d_last_out, d_partial, a);
    e = hipGetLastError();
    if (e != hipSuccess || !power) return e;
    hipLaunchKernelGGL(channel_power_finish_kernel, dim3((unsigned)nch), dim3(NT), 0, s, d_partial, a.tiles,
                       (float)(1.0 / (double)nsamp), d_power);
    return hipGetLastError();
}

}  // namespace sddc
