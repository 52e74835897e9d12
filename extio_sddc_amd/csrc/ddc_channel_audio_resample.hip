// ddc_channel_audio_resample.hip — the channel audio resampler for gfx950
// (sddc_ddc_channel_audio_resample_device): the channel resampler's rational L/M polyphase FIR on REAL
// streams, F32 or S16 in, F32 or S16 out, streaming (the last K - 1 sample values of each channel live
// on the device as floats, K = ceil(ntaps / L); the stream position lives on the host as e < M).
//
//   y_c[m] = sum_{j < K} h[p + jL] x_c[s - j]       mM = sL + p, 0 <= p < L, h[k] = 0 for k >= ntaps
//
// The decomposition is ddc_channel_resample.hip's: output k = a L + b of the call has e + k M =
// (a M + o_b) L + p_b, so for a fixed b the outputs over a are an integer decimator by M with the tap
// set g_p[j] = h[p + jL] and the sample offset o_b.  A work item is one (channel, tile) of `ta`
// consecutive a, taken by a 256-thread workgroup; the tile's sample values go to LDS transposed
// polyphase by M (position s at (s mod M) pitch + s div M), the tails are double-buffered and swapped
// by the host, and a call without an output still moves them.  Every sample of [old tail | call] is
// owned by exactly one tile, and a tile writes those of its own samples that are among the stream's last
// K - 1 to the new tail: mostly the last tile, but also an earlier one whose range reaches past
// nsamp - (K - 1), and the first tile for what a short call keeps of the old tail.
//
// What real samples change.
//   slots    An LDS slot is one float, 4 bytes: a tile holds twice the samples of the IQ resampler's,
//            so ta goes up to 1024, and a small M needs so little of it that a second instance of the
//            kernel with half the LDS (32 KiB) runs five workgroups per CU instead of two.
//   loads    A 16-byte load carries 4 F32 or 8 S16 samples.  A channel's base is aligned to one sample
//            only, so each item finds its own offset `al` to the 16-byte grid; the vectors that
//            straddle an end of the tile's samples are read sample by sample.
//   stores   One ds_write_b32 per sample (banked mod 32 in two 32-lane halves): lane l of a half
//            holds samples V l + e and stores e; channel_audio_resample_pitch() picks the pitch.
//   reads    One ds_read_b32 per tap, served in the halves {0-31} and {32-63}, each conflict-free on
//            32 consecutive slots whatever the row.  A row holds consecutive a, so the unit of work
//            is (b, 64 consecutive a) for one WAVE: both halves share b, and with it the tap set, the
//            row and the column of every tap.  The taps come through scalar loads and feed the fma as
//            a scalar operand, the walk through the rows (down one per tap, wrapping to the previous
//            column) is three scalar instructions, and a lane spends one add and one fma per tap.
//   outputs  F32: one 4-byte store per lane.  S16: with L = 1 consecutive lanes hold consecutive
//            outputs, and a lane whose address is 4-byte aligned stores its neighbour's value with its
//            own; the stream's odd first and last samples, a wave's edges and every L > 1 (the lanes'
//            outputs are L apart) take single 2-byte stores.
//
// Determinism: an output is audio_resample_math.h's fixed sequence on sample values that are the same
// floats whether they come from the tail or from the call's buffer.  The order depends on (p, j, K)
// alone, there are no atomics, and the CPU backend runs the same sequence: the same bits.
//
// Barriers: two per round of the item loop, outside every condition (ddc_channel_decimate.hip).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "audio_resample_math.h"
#include "channel_stage.hpp"
#include "ddc_kernels.h"
#include "demod_math.h"

namespace sddc {
namespace {

using chstage::NT;

constexpr int NW = NT / 64;

struct Args {
    long long nsamp, nout, na, tiles, nitems;   // per channel: samples, outputs, values of a, tiles; items of the call
    size_t in_stride, out_stride;               // samples per channel
    int L, M, K, e;                             // factors, taps per phase, the call's position
    int ta, pitch;                              // values of a per tile, the rows' pitch
    unsigned mmagic;                            // ceil(2^32 / M): s div M = umulhi(s, mmagic) for s < 2^16; 0: M = 1
};

template <bool S16> struct Fmt;
template <> struct Fmt<false> {
    using Sample = float;
    using Vec = float4;
    static constexpr int V = 4;
};
template <> struct Fmt<true> {
    using Sample = int16_t;
    using Vec = int4;
    static constexpr int V = 8;
};

__device__ __forceinline__ float to_value(float x) { return x; }
__device__ __forceinline__ float to_value(int16_t x) { return ars::ars_value(x); }

// s div M for s < 2^16 (M = 1 has no 32-bit magic: mmagic = 0 stands for it)
__device__ __forceinline__ unsigned div_m(unsigned s, unsigned mmagic) { return mmagic ? __umulhi(s, mmagic) : s; }

// The compiler may not start a block's fmas before its reads are issued: eight values at a time pass
// through an empty asm, which waits for their reads and holds the fmas behind it.
__device__ __forceinline__ void pin8(float *u)
{
    asm volatile("" : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]), "+v"(u[6]), "+v"(u[7]));
}

// One wave unit's sums.  col: the lane's column of the unit's rows (its a within the tile); g: the
// unit's tap set (wave-uniform, K floats); off: the slot of column 0 for tap 0, wave-uniform.  Tap j
// adds to partial sum j mod 4 by one fma.  From tap to tap the position steps down one row, and from
// row 0 (off < pitch: a column index is below the pitch) to row M - 1 of the column before: a scalar
// compare, select and add.
__device__ __forceinline__ float fir(const float *col, const float *__restrict__ g, int off, int K, int M, int pitch)
{
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int wrap = (M - 1) * pitch - 1, down = -pitch;
    int j = 0;
    // blocks of 16, then one of 8: every read of a block is issued before its first fma (a wave waits
    // once per block for its scalar and LDS loads, so the block's size sets the taps per wait)
    auto block = [&](auto nt) {
        constexpr int N = decltype(nt)::value;
        float h[N], u[N];
#pragma unroll
        for (int t = 0; t < N; t++) h[t] = g[j + t];
#pragma unroll
        for (int t = 0; t < N; t++) {
            CDC_RD(u[t], col[off]);
            off += off < pitch ? wrap : down;
        }
#pragma unroll
        for (int t = 0; t < N; t += 8) pin8(u + t);
#pragma unroll
        for (int t = 0; t < N; t++) acc[t & 3] = ars::ars_step(h[t], u[t], acc[t & 3]);
        j += N;
    };
    while (j + 16 <= K) block(std::integral_constant<int, 16>());
    if (j + 8 <= K) block(std::integral_constant<int, 8>());
    // the last K mod 8 taps (j is a multiple of 8: tap j + t adds to sum t mod 4)
#pragma unroll
    for (int t = 0; t < 7; t++) {
        if (j + t < K) {
            float u;
            CDC_RD(u, col[off]);
            off += off < pitch ? wrap : down;
            acc[t & 3] = ars::ars_step(g[j + t], u, acc[t & 3]);
        }
    }
    return ars::ars_sum(acc);
}

template <bool IN16, bool OUT16, int LDS>
__global__ __launch_bounds__(NT) void channel_audio_resample_kernel(const void *__restrict__ in, float *__restrict__ out,
                                                                    const float *__restrict__ taps,
                                                                    const float2 *__restrict__ tail_in2,
                                                                    float2 *__restrict__ tail_out2, const Args a)
{
    using F = Fmt<IN16>;
    using Sample = typename F::Sample;
    constexpr int V = F::V;
    // every vector of the largest tile in registers at once: LDS / V + 1 vectors at most
    constexpr int KV = (LDS / V + 2 + NT - 1) / NT;
    __shared__ float lds[LDS + 128];
    const float *tail_in = reinterpret_cast<const float *>(tail_in2);
    float *tail_out = reinterpret_cast<float *>(tail_out2);
    const int tid = (int)threadIdx.x;
    const int M = a.M, L = a.L, K = a.K, H = K - 1, pitch = a.pitch;

    // the same trip count in every workgroup
    const int rounds = (int)((a.nitems + gridDim.x - 1) / gridDim.x);
    for (int round = 0; round < rounds; round++) {
        const long long item = (long long)round * gridDim.x + blockIdx.x;
        const bool ok = item < a.nitems;   // workgroup-uniform
        long long c = 0, a0 = 0;
        int an = 0;
        __syncthreads();   // the previous round's reads are done
        if (ok) {
            c = item / a.tiles;
            const long long t = item - c * a.tiles;
            a0 = t * a.ta;
            an = (int)(a.na - a0 < a.ta ? a.na - a0 : a.ta);   // 0: a call without an output
            // The tile's samples by position p = i - s0 < P, i the index within the call (negative:
            // earlier calls): [0, pg) come from the tail, [pg, P) from the call's buffer; the tile
            // owns [pown, P), and position ptail is the first sample of the new tail (below 0 when
            // the new tail begins before this tile: every owned position is then part of it; at
            // least P when it begins behind it).  The last tile runs to the call's end (fewer than M
            // samples past its last a: one more column).
            const long long s0 = a0 * M - H;
            const long long end = t == a.tiles - 1 ? a.nsamp : (a0 + an) * M;
            const int P = (int)(end - s0);
            const int pg = s0 < 0 ? (int)-s0 : 0;
            const int pown = t == 0 ? 0 : H;
            const long long dt = a.nsamp - H - s0;
            const int ptail = dt > P ? P : (int)dt;
            const bool tails = ptail < P;              // workgroup-uniform
            auto put = [&](int p, float v) {
                const unsigned q = div_m((unsigned)p, a.mmagic);
                lds[((unsigned)p - q * (unsigned)M) * (unsigned)pitch + q] = v;
                if (tails && p >= pown && p >= ptail) tail_out[c * H + (p - ptail)] = v;
            };
            for (int p = tid; p < pg; p += NT) put(p, tail_in[c * H + (H - pg) + p]);
            // position pg is sample max(s0, 0) of the channel, al samples past a 16-byte line
            const char *gp = static_cast<const char *>(in) +
                             ((size_t)c * a.in_stride + (size_t)(s0 > 0 ? s0 : 0)) * sizeof(Sample);
            const int al = (int)(((uintptr_t)gp / sizeof(Sample)) % V);
            const int nv = (P - pg + al + V - 1) / V;   // vectors that hold a sample of the tile: <= KV NT
            typename F::Vec w[KV];
            // the whole vectors first, all in flight together; vector kv starts at position pg - al + kv V
#pragma unroll
            for (int k = 0; k < KV; k++) {
                const int kv = tid + k * NT, e0 = kv * V - al;
                if (kv < nv && e0 >= 0 && pg + e0 + V <= P)
                    w[k] = *reinterpret_cast<const typename F::Vec *>(gp + (long long)e0 * (int)sizeof(Sample));
            }
#pragma unroll
            for (int k = 0; k < KV; k++) {
                const int kv = tid + k * NT, e0 = kv * V - al;
                if (kv >= nv) continue;
                if (e0 >= 0 && pg + e0 + V <= P) {
                    const int p = pg + e0;
                    if constexpr (IN16) {
                        const int d[4] = {w[k].x, w[k].y, w[k].z, w[k].w};
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            put(p + 2 * i, to_value((int16_t)(d[i] & 0xffff)));
                            put(p + 2 * i + 1, to_value((int16_t)(d[i] >> 16)));
                        }
                    } else {
                        put(p, w[k].x);
                        put(p + 1, w[k].y);
                        put(p + 2, w[k].z);
                        put(p + 3, w[k].w);
                    }
                } else {   // a vector across an end of the tile's samples: the samples inside, one by one
#pragma unroll
                    for (int e = 0; e < V; e++)
                        if (e0 + e >= 0 && pg + e0 + e < P)
                            put(pg + e0 + e, to_value(*reinterpret_cast<const Sample *>(gp + (long long)(e0 + e) * (int)sizeof(Sample))));
                }
            }
        }
        __syncthreads();
        if (ok && an > 0) {   // no barrier below this point
            // units: (b, the hf-th 64 of the tile's a) for b < L, hf < nh; a wave takes one at a time
            const int nh = (an + 63) >> 6, units = L * nh;
            const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int lane = tid & 63;
            for (int u = wave; u < units; u += NW) {
                const int b = u / nh, hf = u - b * nh;   // wave-uniform, like all of the unit but ar
                const int tb = a.e + b * M, o = tb / L;
                const float *g = taps + (tb - o * L) * K;
                const int ar = (hf << 6) + lane;           // the lane's a within the tile
                const long long k = (a0 + ar) * L + b;     // its output of the call
                const bool live = ar < an && k < a.nout;
                // tap 0 of column 0: position o + K - 1 (a lane without an output computes on a = 0)
                const unsigned s = (unsigned)(o + H), q = div_m(s, a.mmagic);
                const int row = (int)(s - q * (unsigned)M);
                const float y = fir(lds + (live ? ar : 0), g, row * pitch + (int)q, K, M, pitch);
                if constexpr (!OUT16) {
                    if (live) out[(size_t)c * a.out_stride + (size_t)k] = y;
                } else {
                    int16_t *d = reinterpret_cast<int16_t *>(out) + (size_t)c * a.out_stride + (size_t)k;
                    const int16_t v = demod::demod_s16(y);
                    if (L == 1) {
                        // consecutive lanes, consecutive outputs, and the live lanes are the wave's first
                        const unsigned mine = (uint16_t)v;
                        const unsigned next = (unsigned)__shfl_down((int)mine, 1);
                        const bool pair = __shfl_down((int)live, 1) != 0 && lane < 63;
                        const bool even = ((uintptr_t)d & 2) == 0;
                        if (live) {
                            if (even && pair) *reinterpret_cast<unsigned *>(d) = mine | (next << 16);
                            else if (even || lane == 0) *d = v;   // an odd address past lane 0: stored by the lane before
                        }
                    } else if (live) {
                        *d = v;
                    }
                }
            }
        }
    }
}

template <bool IN16, bool OUT16>
hipError_t launch_sized(const KernelTables &t, int lds, const void *d_in, float *d_out, const float *d_taps,
                        const float2 *tail_in, float2 *tail_out, const Args &a, int max_wgs, int device, hipStream_t s)
{
    return lds == kChArsLdsSmall
               ? chstage::launch_stage(t, channel_audio_resample_kernel<IN16, OUT16, kChArsLdsSmall>, d_in, d_out, d_taps,
                                       tail_in, tail_out, a, max_wgs, device, s)
               : chstage::launch_stage(t, channel_audio_resample_kernel<IN16, OUT16, kChArsLds>, d_in, d_out, d_taps,
                                       tail_in, tail_out, a, max_wgs, device, s);
}

}  // namespace

int channel_audio_resample_pitch(int mod, int need, int max_pitch, int V, int *store_conflicts)
{
    int best = -1, best_pitch = 0;
    for (int pitch = need; pitch <= max_pitch; pitch++) {
        int cost = 0;
        for (int e = 0; e < V; e++) {
            int cycles = 0;   // LDS-array cycles of store e: the worst bank's addresses, per half
            for (int g0 = 0; g0 < 64; g0 += 32) {
                int cnt[32] = {}, worst = 0;
                for (int l = g0; l < g0 + 32; l++) {
                    const int p = V * l + e, k = ((p % mod) * pitch + p / mod) & 31;
                    if (++cnt[k] > worst) worst = cnt[k];
                }
                cycles += worst;
            }
            if (cycles > 4) cost += cycles - 4;   // the instruction's own 4 cycles hide 2-way in both halves
        }
        if (best < 0 || cost < best) {
            best = cost;
            best_pitch = pitch;
        }
    }
    *store_conflicts = best;
    return best_pitch;
}

ChArsLayout channel_audio_resample_layout(int L, int M, int ntaps, int in_s16)
{
    ChArsLayout g;
    g.K = (ntaps + L - 1) / L;
    // columns beside the tile's own: the halo's, and one for the last tile's samples past its last a
    const int hcols = (g.K - 1 + M - 1) / M + 1;
    auto fit = [&](int lds) {
        const int ta = lds / M - hcols - 1;   // one column spare
        return ta > kChArsMaxA ? kChArsMaxA : ta;
    };
    g.lds = fit(kChArsLdsSmall) >= kChArsSmallMinA ? kChArsLdsSmall : kChArsLds;
    g.ta = fit(g.lds);
    if (g.ta < 1) return g;
    const int need = g.ta + hcols, room = g.lds / M;
    const int top = need + kChArsPitchPad < room ? need + kChArsPitchPad : room;
    g.pitch = channel_audio_resample_pitch(M, need, top, in_s16 ? 8 : 4, &g.store_conflicts);
    return g;
}

hipError_t launch_channel_audio_resample(const KernelTables &t, const void *d_in, int in_s16, int nch, size_t nsamp,
                                         size_t in_stride, const float *d_taps, int ntaps, int L, int M, int e,
                                         size_t nout, const float *d_tail_in, float *d_tail_out, void *d_out,
                                         int out_s16, size_t out_stride, int max_wgs, int device, hipStream_t s)
{
    if (!d_in || !d_out || !d_taps || nch < 1 || ntaps < 1 || ntaps > kChResMaxTaps || L < 1 || L > kChResMaxUp || M < 1 ||
        M > kChResMaxDown || e < 0 || e >= M || nsamp == 0 || nsamp > ((size_t)1 << 40))
        return hipErrorInvalidValue;
    const ChArsLayout g = channel_audio_resample_layout(L, M, ntaps, in_s16);
    if (g.K > kChResMaxK || g.ta < 1 || (long long)g.pitch * M > g.lds) return hipErrorInvalidValue;
    if (g.K > 1 && (!d_tail_in || !d_tail_out)) return hipErrorInvalidValue;
    // the count of the ABI (sddc_ddc_resample_count), so every output's samples are in the call
    if ((uint64_t)nout != ars::ars_count(L, M, e, nsamp)) return hipErrorInvalidValue;
    if (nout == 0 && g.K == 1) return hipSuccess;   // nothing to store, no tail to move
    Args a;
    a.nsamp = (long long)nsamp;
    a.nout = (long long)nout;
    a.na = (a.nout + L - 1) / L;
    a.tiles = (a.na + g.ta - 1) / g.ta;
    if (a.tiles < 1) a.tiles = 1;   // the item that moves the tail
    a.nitems = a.tiles * nch;
    a.in_stride = nch > 1 ? in_stride : 0;
    a.out_stride = nch > 1 ? out_stride : 0;
    a.L = L;
    a.M = M;
    a.K = g.K;
    a.e = e;
    a.ta = g.ta;
    a.pitch = g.pitch;
    a.mmagic = M == 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)M - 1) / (unsigned)M);
    const float2 *ti = reinterpret_cast<const float2 *>(d_tail_in);
    float2 *to = reinterpret_cast<float2 *>(d_tail_out);
    float *o = static_cast<float *>(d_out);
    if (in_s16)
        return out_s16 ? launch_sized<true, true>(t, g.lds, d_in, o, d_taps, ti, to, a, max_wgs, device, s)
                       : launch_sized<true, false>(t, g.lds, d_in, o, d_taps, ti, to, a, max_wgs, device, s);
    return out_s16 ? launch_sized<false, true>(t, g.lds, d_in, o, d_taps, ti, to, a, max_wgs, device, s)
                   : launch_sized<false, false>(t, g.lds, d_in, o, d_taps, ti, to, a, max_wgs, device, s);
}

}  // namespace sddc
