// ddc_channel_resample.hip — the channel resampler for gfx950 (sddc_ddc_channel_resample_device): a
// rational L/M polyphase FIR with real taps on every channel stream of the DDC's output, CF32 or
// CS16 in, CF32 out, streaming (the last K - 1 sample values of each channel live on the device,
// K = ceil(ntaps / L); the stream position lives on the host, reduced to one number e < M).
//
//   u_c[iL] = x_c[i], 0 elsewhere;   v_c[n] = sum_k h[k] u_c[n - k];   y_c[m] = v_c[mM]
//   y_c[m] = sum_{j < K} h[p + jL] x_c[s - j]       mM = sL + p, 0 <= p < L, h[k] = 0 for k >= ntaps
//
// The position.  With N samples consumed and m0 = ceil(N L / M) outputs produced, e = m0 M - N L
// (0 <= e < M) is all a call needs: its output k = 0, 1, .. has s L + p = e + k M with s counted from
// the call's first sample.  Write k = a L + b (0 <= b < L): e + k M = (a M + o_b) L + p_b with
// o_b = (e + b M) div L < M and p_b = (e + b M) mod L, so for a fixed b the outputs over a are an
// integer decimator by M with the tap set g_p[j] = h[p + jL] and the sample offset o_b.
//
// Work item: one (channel, tile) of `ta` consecutive a (ta L outputs), taken by a 256-thread workgroup:
//   stage    the tile's ta M + K - 1 sample values (the last tile: up to the call's end) go to LDS as
//            float2 and the stream's last K - 1 to the handle's tail, as channel_stage.hpp describes.
//            Sample position s of the tile is stored polyphase-transposed by M at
//            (s mod M) pitch + s div M, so that
//   compute  the 32 lanes of a half wave hold one b and 32 consecutive a, and read consecutive
//            float2 for every tap: ds_read_b64 is served in the lane groups {0-31} and {32-63}, each
//            conflict-free on 64 consecutive dwords whatever the row.  The unit of work is such a
//            (b, 32 a) half; a wave takes two units at a time (two b when ta <= 32, two a-halves of
//            one b otherwise), so both tap sets of a wave are wave-uniform: they come through scalar
//            loads from the host-ordered copy g[p][j] (K floats per phase, zero-padded) and a lane
//            picks its half's with one select.  Tap j of lane (a, b) reads position
//            a M + o_b + K - 1 - j: the row steps down by one per tap and wraps to the previous
//            column.  Sixteen reads are issued before the first fma.
// The samples past the call's last output belong to the last tile, which so writes them to the new
// tail.  A call without an output (M > L, a short call) still has one item, which only moves the tail.
//
// Determinism: an output is the fixed sequence
//   a[j mod 4] = fma(g_p[j], x[s - j], a[j mod 4])   for j = 0, 1, .. K - 1;   y = (a0 + a1) + (a2 + a3)
// on sample values that are the same floats whether they come from the tail or from the call's
// buffer.  The order depends on (p, j, K) alone: not on the tile, the grid, the stream, the other
// channels, the call's cut of the stream or the position, and there are no atomics.
//
// Barriers: two per round of the item loop, outside every condition (ddc_channel_decimate.hip).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "channel_stage.hpp"
#include "ddc_kernels.h"

namespace sddc {
namespace {

using namespace chstage;

constexpr int NW = NT / 64;

struct Args {
    long long nsamp, nout, na, tiles, nitems;   // per channel: samples, outputs, values of a, tiles; items of the call
    size_t in_stride, out_stride;               // components (float or int16) / floats per channel
    int L, M, K, e;                             // factors, taps per phase, the call's position
    int ta, pitch;                              // values of a per tile, the rows' pitch
    unsigned mmagic;                            // ceil(2^32 / M): s div M = umulhi(s, mmagic) for s < 2^16; 0: M = 1
    float inv_s;                                // CS16: 1 / cs16_scale
};

// s div M for s < 2^16 (M = 1 has no 32-bit magic: mmagic = 0 stands for it)
__device__ __forceinline__ unsigned div_m(unsigned s, unsigned mmagic) { return mmagic ? __umulhi(s, mmagic) : s; }

// The sums of one wave's two units.  glo / ghi: the tap sets of the lower and the upper half
// (wave-uniform pointers, K floats each); `upper`: the lane's half; row / addr: the lane's position
// for tap 0 (row = position mod M, addr = its LDS slot).  Tap j adds to partial sum j mod 4 by one
// fma; the four sums are added as (0 + 1) + (2 + 3).
__device__ __forceinline__ float2 fir(const float2 *lds, const float *__restrict__ glo, const float *__restrict__ ghi,
                                      bool upper, int row, int addr, int K, int M, int pitch)
{
    float2 acc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = make_float2(0.f, 0.f);
    const int wrap = M * pitch - 1;   // from row 0 to row M - 1 of the previous column
    int j = 0;
    // blocks of 16, then one of 8: every load of a block is issued before its first fma (a wave
    // waits once per block for its scalar and LDS loads, so the block's size sets the taps per wait)
    auto block = [&](auto nt) {
        constexpr int N = decltype(nt)::value;
        float hl[N], hh[N];
        float2 u[N];
#pragma unroll
        for (int t = 0; t < N; t++) {
            hl[t] = glo[j + t];
            hh[t] = ghi[j + t];
        }
#pragma unroll
        for (int t = 0; t < N; t++) {
            CDC_RD(u[t], lds[addr]);
            addr -= pitch;
            if (--row < 0) {
                row += M;
                addr += wrap;
            }
        }
#pragma unroll
        for (int t = 0; t < N; t++) {
            const float h = upper ? hh[t] : hl[t];
            acc[t & 3].x = fmaf(h, u[t].x, acc[t & 3].x);
            acc[t & 3].y = fmaf(h, u[t].y, acc[t & 3].y);
        }
        j += N;
    };
    while (j + 16 <= K) block(std::integral_constant<int, 16>());
    if (j + 8 <= K) block(std::integral_constant<int, 8>());
    // the last K mod 8 taps (j is a multiple of 8: tap j + t adds to sum t mod 4)
#pragma unroll
    for (int t = 0; t < 7; t++) {
        if (j + t < K) {
            const float h = upper ? ghi[j + t] : glo[j + t];
            float2 u;
            CDC_RD(u, lds[addr]);
            addr -= pitch;
            if (--row < 0) {
                row += M;
                addr += wrap;
            }
            acc[t & 3].x = fmaf(h, u.x, acc[t & 3].x);
            acc[t & 3].y = fmaf(h, u.y, acc[t & 3].y);
        }
    }
    return make_float2((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y));
}

template <bool CS16>
__global__ __launch_bounds__(NT) void channel_resample_kernel(const void *__restrict__ iq, float *__restrict__ out,
                                                              const float *__restrict__ taps,
                                                              const float2 *__restrict__ tail_in,
                                                              float2 *__restrict__ tail_out, const Args a)
{
    using F = Fmt<CS16>;
    using Sample = typename F::Sample;
    constexpr int V = F::V;
    // every vector of the largest tile in registers at once: kChResLds / V + 1 vectors at most
    constexpr int KV = (kChResLds / V + 2 + NT - 1) / NT;
    __shared__ float2 lds[kChResLds + 64];
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
            // owns [pown, P), and position ptail is the first sample of the new tail.  The last
            // tile runs to the call's end (fewer than M samples past its last a: one more column).
            const long long s0 = a0 * M - H;
            const long long end = t == a.tiles - 1 ? a.nsamp : (a0 + an) * M;
            const int P = (int)(end - s0);
            const int pg = s0 < 0 ? (int)-s0 : 0;
            const int pown = t == 0 ? 0 : H;
            const long long dt = a.nsamp - H - s0;
            const int ptail = dt > P ? P : (int)dt;   // >= -H
            const bool tails = ptail < P;              // workgroup-uniform
            auto put = [&](int p, float2 v) {
                const unsigned q = div_m((unsigned)p, a.mmagic);
                lds[((unsigned)p - q * (unsigned)M) * (unsigned)pitch + q] = v;
                if (tails && p >= pown && p >= ptail) tail_out[c * H + (p - ptail)] = v;
            };
            for (int p = tid; p < pg; p += NT) put(p, tail_in[c * H + (H - pg) + p]);
            // position pg is sample max(s0, 0) of the channel, al samples past a 16-byte line
            const char *gp = static_cast<const char *>(iq) + (size_t)c * a.in_stride * (sizeof(Sample) / 2) +
                             (size_t)(s0 > 0 ? s0 : 0) * sizeof(Sample);
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
                    if constexpr (CS16) {
                        put(pg + e0, to_value(w[k].x, a.inv_s));
                        put(pg + e0 + 1, to_value(w[k].y, a.inv_s));
                        put(pg + e0 + 2, to_value(w[k].z, a.inv_s));
                        put(pg + e0 + 3, to_value(w[k].w, a.inv_s));
                    } else {
                        put(pg + e0, make_float2(w[k].x, w[k].y));
                        put(pg + e0 + 1, make_float2(w[k].z, w[k].w));
                    }
                } else {   // a vector across an end of the tile's samples: the samples inside, one by one
#pragma unroll
                    for (int e = 0; e < V; e++)
                        if (e0 + e >= 0 && pg + e0 + e < P)
                            put(pg + e0 + e, to_value(*reinterpret_cast<const Sample *>(gp + (long long)(e0 + e) * (int)sizeof(Sample)),
                                                      a.inv_s));
                }
            }
        }
        __syncthreads();
        if (ok && an > 0) {   // no barrier below this point
            // units: (b, half hf of the tile's a) for b < L, hf < nh; a wave takes units 2 i, 2 i + 1
            const int nh = (an + 31) >> 5, units = L * nh;
            const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const bool upper = (tid & 32) != 0;
            const int lane = tid & 31;
            float2 *dst = reinterpret_cast<float2 *>(out + (size_t)c * a.out_stride);
            for (int u0 = 2 * wave; u0 < units; u0 += 2 * NW) {
                const int u1 = u0 + 1 < units ? u0 + 1 : u0;   // an odd count: the upper half idles on unit u0
                const int blo = u0 / nh, bhi = u1 / nh;        // wave-uniform
                const int tlo = a.e + blo * M, thi = a.e + bhi * M;
                const int olo = tlo / L, ohi = thi / L;
                const float *glo = taps + (tlo - olo * L) * K, *ghi = taps + (thi - ohi * L) * K;
                const int u = upper ? u1 : u0, b = upper ? bhi : blo, o = upper ? ohi : olo;
                const int ar = ((u - b * nh) << 5) + lane;     // the lane's a within the tile
                const long long k = (a0 + ar) * L + b;         // its output of the call
                const bool live = ar < an && k < a.nout && (!upper || u0 + 1 < units);
                // tap 0's position: a M + o + K - 1 (a lane without an output computes on a = 0)
                const int s = (live ? ar : 0) * M + o + H;
                const unsigned q = div_m((unsigned)s, a.mmagic);
                const int row = (int)((unsigned)s - q * (unsigned)M);
                const float2 y = fir(lds, glo, ghi, upper, row, row * pitch + (int)q, K, M, pitch);
                if (live) dst[k] = y;
            }
        }
    }
}

}  // namespace

ChResLayout channel_resample_layout(int L, int M, int ntaps, int cs16)
{
    ChResLayout g;
    g.K = (ntaps + L - 1) / L;
    // columns beside the tile's own: the halo's, and one for the last tile's samples past its last a
    const int hcols = (g.K - 1 + M - 1) / M + 1;
    const int room = kChResLds / M;   // columns the LDS holds
    g.ta = room - hcols - 1;          // one column spare: the search below always has an odd pitch to take
    if (g.ta > kChResMaxA) g.ta = kChResMaxA;
    if (g.ta < 1) return g;
    const int need = g.ta + hcols;
    // a pitch that the LDS holds
    const int top = need + kChResPitchPad < room ? need + kChResPitchPad : room;
    g.pitch = polyphase_pitch(M, need, top, cs16 ? 4 : 2, &g.store_conflicts);
    return g;
}

void channel_resample_order_taps(const float *h, int ntaps, int L, float *g)
{
    const int K = (ntaps + L - 1) / L;
    for (int p = 0; p < L; p++)
        for (int j = 0; j < K; j++) g[p * K + j] = p + j * L < ntaps ? h[p + j * L] : 0.f;
}

hipError_t launch_channel_resample(const KernelTables &t, const void *d_iq, int cs16, float cs16_scale, int nch,
                                   size_t nsamp, size_t in_stride, const float *d_taps, int ntaps, int L, int M,
                                   int e, size_t nout, const float2 *d_tail_in, float2 *d_tail_out, float *d_out,
                                   size_t out_stride, int max_wgs, int device, hipStream_t s)
{
    if (!d_iq || !d_out || !d_taps || nch < 1 || ntaps < 1 || ntaps > kChResMaxTaps || L < 1 || L > kChResMaxUp || M < 1 ||
        M > kChResMaxDown || e < 0 || e >= M || nsamp == 0 || nsamp > ((size_t)1 << 40))
        return hipErrorInvalidValue;
    const ChResLayout g = channel_resample_layout(L, M, ntaps, cs16);
    if (g.K > kChResMaxK || g.ta < 1 || (long long)g.pitch * M > kChResLds) return hipErrorInvalidValue;
    if (g.K > 1 && (!d_tail_in || !d_tail_out)) return hipErrorInvalidValue;
    // the count of the ABI (sddc_ddc_resample_count), so every output's samples are in the call
    const long long want = (long long)nsamp * L > e ? ((long long)nsamp * L - e + M - 1) / M : 0;
    if ((long long)nout != want) return hipErrorInvalidValue;
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
    a.inv_s = cs16 ? (float)(1.0 / (double)cs16_scale) : 1.f;
    return cs16 ? launch_stage(t, channel_resample_kernel<true>, d_iq, d_out, d_taps, d_tail_in, d_tail_out, a, max_wgs, device, s)
                : launch_stage(t, channel_resample_kernel<false>, d_iq, d_out, d_taps, d_tail_in, d_tail_out, a, max_wgs, device, s);
}

}  // namespace sddc
