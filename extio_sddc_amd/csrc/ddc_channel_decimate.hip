// ddc_channel_decimate.hip — the channel decimator for gfx950 (sddc_ddc_channel_decimate_device): an
// integer-factor decimating FIR with real taps on every channel stream of the DDC's output, CF32 or
// CS16 in, CF32 out, streaming (the last ntaps - 1 sample values of each channel live on the device).
//
//   v_c[i] = sum_{j < ntaps} h[j] x_c[i - j]      i = stream index since the last reset
//   y_c[m] = v_c[m R]
//
// Work item: one (channel, tile) of `tile` <= kChDecTile outputs, taken by a 256-thread workgroup:
//   stage    the tile's tile R + ntaps - 1 sample values go to LDS as float2 and the stream's last
//            ntaps - 1 to the handle's tail, as channel_stage.hpp describes (at most 10 16-byte
//            loads per thread).  Sample p of the tile is stored polyphase-transposed at
//            (p mod R) pitch + p div R, so that
//   compute  output o reads tap j's sample (o R + L - j, L = ntaps - 1) at
//            ((L - j) mod R) pitch + (L - j) div R + o: the lanes of a wave read consecutive float2
//            for every tap (ds_read_b64, conflict-free for any pitch).  The taps are walked phase by
//            phase, so a phase's samples sit at immediate offsets of one address; eight reads per
//            output are issued before the first fma.  A thread owns outputs tid and tid + 256 (a
//            tile of more than 256 outputs) and shares each tap between them; the tap index is
//            uniform, so the taps come through scalar loads, eight per trip, from a copy the host
//            has put in the walk's order.
//
// Determinism: with k = L - j = q R + r, an output is the fixed sequence
//   a[q mod 4] = fma(h[j], x[mR - j], a[q mod 4])  for r = 0 .. R - 1, q = 0, 1, ..   y = (a0 + a1) + (a2 + a3)
// on sample values that are the same floats whether they come from the tail or from the call's
// buffer.  The order depends on the tap index, R and ntaps alone: not on the tile, the grid, the
// call's cut of the stream or the other channels, and there are no atomics.
//
// Barriers: two per round of the item loop, outside every condition.  The loop runs
// ceil(items / grid) rounds in every workgroup; a workgroup whose item is past the end stages and
// stores nothing; a wave without an output of the tile skips the sums (they hold no barrier), and a
// thread of the other waves whose output is past the tile's end computes on output 0's samples and
// stores nothing.
#include <hip/hip_runtime.h>

#include "channel_stage.hpp"
#include "ddc_kernels.h"

namespace sddc {
namespace {

using namespace chstage;

struct Args {
    long long nsamp, nout, tiles, nitems;   // per channel: samples, outputs, tiles; items of the call
    size_t in_stride, out_stride;           // components (float or int16) / floats per channel
    int R, ntaps, tile, pitch;
    unsigned rmagic;                        // ceil(2^32 / R): p div R = umulhi(p, rmagic) for p < 2^16
    float inv_s;                            // CS16: 1 / cs16_scale
};

// The sums of outputs tid (and tid + NT for NO = 2) of a staged tile.  The taps arrive in the
// kernel's order (channel_decimate_order_taps): phase r = 0 .. min(R, ntaps) - 1 of the tile's rows,
// and within it row q = 0 .. (L - r) / R, tap h[L - (q R + r)] on the sample at r pitch + q + o, so
// a phase's reads sit at immediate offsets of one address and its taps are consecutive floats.
// Tap (r, q) adds to partial sum q mod 4 by one fma; the four sums are added as (0 + 1) + (2 + 3).
template <int NO>
__device__ __forceinline__ void fir(const float2 *lds, const float *__restrict__ g, int tid, int tn, int R, int L,
                                    int pitch, float2 *dst)
{
    const float2 *x = lds + (tid < tn ? tid : 0);   // the second output: NT slots on
    float2 acc[NO][4];
#pragma unroll
    for (int i = 0; i < NO; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[i][k] = make_float2(0.f, 0.f);
    const int Q = L / R, rlong = L % R, nph = L + 1 < R ? L + 1 : R;   // uniform
    for (int r = 0; r < nph; r++) {
        const float2 *xr = x + r * pitch;
        const int cnt = Q + (r <= rlong ? 1 : 0);
        int q = 0;
        for (; q + 8 <= cnt; q += 8) {
            float h[8];
            float2 u[NO][8];
#pragma unroll
            for (int e = 0; e < 8; e++) h[e] = g[e];
#pragma unroll
            for (int e = 0; e < 8; e++)
#pragma unroll
                for (int i = 0; i < NO; i++) CDC_RD(u[i][e], xr[q + e + i * NT]);
#pragma unroll
            for (int e = 0; e < 8; e++)
#pragma unroll
                for (int i = 0; i < NO; i++) {
                    acc[i][e & 3].x = fmaf(h[e], u[i][e].x, acc[i][e & 3].x);
                    acc[i][e & 3].y = fmaf(h[e], u[i][e].y, acc[i][e & 3].y);
                }
            g += 8;
        }
        // the phase's last cnt mod 8 rows (q is a multiple of 8: row q + e adds to sum e mod 4)
#pragma unroll
        for (int e = 0; e < 7; e++) {
            if (q + e < cnt) {
                const float h = g[e];
#pragma unroll
                for (int i = 0; i < NO; i++) {
                    float2 u;
                    CDC_RD(u, xr[q + e + i * NT]);
                    acc[i][e & 3].x = fmaf(h, u.x, acc[i][e & 3].x);
                    acc[i][e & 3].y = fmaf(h, u.y, acc[i][e & 3].y);
                }
            }
        }
        g += cnt - q;
    }
    // 8 bytes per lane, consecutive lanes consecutive samples
#pragma unroll
    for (int i = 0; i < NO; i++)
        if (tid + i * NT < tn)
            dst[tid + i * NT] = make_float2((acc[i][0].x + acc[i][1].x) + (acc[i][2].x + acc[i][3].x),
                                            (acc[i][0].y + acc[i][1].y) + (acc[i][2].y + acc[i][3].y));
}

template <bool CS16>
__global__ __launch_bounds__(NT) void channel_decimate_kernel(const void *__restrict__ iq, float *__restrict__ out,
                                                              const float *__restrict__ taps,
                                                              const float2 *__restrict__ tail_in,
                                                              float2 *__restrict__ tail_out, const Args a)
{
    using F = Fmt<CS16>;
    using Sample = typename F::Sample;
    constexpr int V = F::V;
    // every vector of the largest tile in registers at once: kChDecLds / V + 1 vectors at most
    constexpr int KV = (kChDecLds / V + 2 + NT - 1) / NT;
    // + NT slots: the second output's read of a thread whose first output is the tile's last
    __shared__ float2 lds[kChDecLds + NT];
    const int tid = (int)threadIdx.x;
    const int R = a.R, L = a.ntaps - 1, pitch = a.pitch;

    // the same trip count in every workgroup
    const int rounds = (int)((a.nitems + gridDim.x - 1) / gridDim.x);
    for (int round = 0; round < rounds; round++) {
        const long long item = (long long)round * gridDim.x + blockIdx.x;
        const bool ok = item < a.nitems;   // workgroup-uniform
        long long c = 0, m0 = 0;
        int tn = 0;
        __syncthreads();   // the previous round's reads are done
        if (ok) {
            c = item / a.tiles;
            const long long t = item - c * a.tiles;
            m0 = t * a.tile;
            tn = (int)(a.nout - m0 < a.tile ? a.nout - m0 : a.tile);
            // The tile's samples by position p = i - s0 < P, i the index within the call (negative:
            // earlier calls): [0, pg) come from the tail, [pg, P) from the call's buffer; the tile
            // owns [pown, P), and position ptail is the first sample of the new tail.
            const long long s0 = m0 * R - L;
            const int P = tn * R + L;
            const int pg = s0 < 0 ? (int)-s0 : 0;
            const int pown = t == 0 ? 0 : L;
            const long long dt = a.nsamp - L - s0;
            const int ptail = dt > P ? P : (int)dt;   // >= -L
            const bool tails = ptail < P;              // workgroup-uniform
            auto put = [&](int p, float2 v) {
                const unsigned q = __umulhi((unsigned)p, a.rmagic);
                lds[((unsigned)p - q * (unsigned)R) * (unsigned)pitch + q] = v;
                if (tails && p >= pown && p >= ptail) tail_out[c * L + (p - ptail)] = v;
            };
            for (int p = tid; p < pg; p += NT) put(p, tail_in[c * L + (L - pg) + p]);
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
        // a wave without an output of the tile has nothing to add (no barrier below this point)
        if (ok && (tid & ~63) < tn) {
            float2 *dst = reinterpret_cast<float2 *>(out + (size_t)c * a.out_stride) + m0;
            if (a.tile > NT) fir<2>(lds, taps, tid, tn, R, L, pitch, dst);
            else fir<1>(lds, taps, tid, tn, R, L, pitch, dst);
        }
    }
}

}  // namespace

ChDecLayout channel_decimate_layout(int R, int ntaps, int cs16)
{
    ChDecLayout g;
    const int hrows = (ntaps - 1 + R - 1) / R;   // rows of the halo
    g.tile = kChDecLds / R - kChDecPitchPad - hrows;
    if (g.tile > kChDecTile) g.tile = kChDecTile;
    if (g.tile > 64) g.tile &= ~63;   // whole waves
    const int need = g.tile + hrows;
    g.pitch = polyphase_pitch(R, need, need + kChDecPitchPad, cs16 ? 4 : 2, &g.store_conflicts);
    return g;
}

void channel_decimate_order_taps(const float *h, int ntaps, int R, float *g)
{
    const int L = ntaps - 1;
    for (int r = 0; r < R && r <= L; r++)
        for (int k = r; k <= L; k += R) *g++ = h[L - k];
}

hipError_t launch_channel_decimate(const KernelTables &t, const void *d_iq, int cs16, float cs16_scale, int nch,
                                   size_t nsamp, size_t in_stride, const float *d_taps, int ntaps, int R,
                                   const float2 *d_tail_in, float2 *d_tail_out, float *d_out, size_t out_stride,
                                   int max_wgs, int device, hipStream_t s)
{
    if (!d_iq || !d_out || !d_taps || nch < 1 || ntaps < 1 || ntaps > kChDecMaxTaps || R < 2 || R > kChDecMaxFactor ||
        nsamp == 0 || nsamp % (size_t)R != 0 || nsamp > ((size_t)1 << 40) || (ntaps > 1 && (!d_tail_in || !d_tail_out)))
        return hipErrorInvalidValue;
    const ChDecLayout g = channel_decimate_layout(R, ntaps, cs16);
    if (g.tile < 1 || (long long)g.pitch * R > kChDecLds) return hipErrorInvalidValue;
    Args a;
    a.nsamp = (long long)nsamp;
    a.nout = a.nsamp / R;
    a.tiles = (a.nout + g.tile - 1) / g.tile;
    a.nitems = a.tiles * nch;
    a.in_stride = nch > 1 ? in_stride : 0;
    a.out_stride = nch > 1 ? out_stride : 0;
    a.R = R;
    a.ntaps = ntaps;
    a.tile = g.tile;
    a.pitch = g.pitch;
    a.rmagic = (unsigned)((0x100000000ULL + (unsigned)R - 1) / (unsigned)R);
    a.inv_s = cs16 ? (float)(1.0 / (double)cs16_scale) : 1.f;
    return cs16 ? launch_stage(t, channel_decimate_kernel<true>, d_iq, d_out, d_taps, d_tail_in, d_tail_out, a, max_wgs, device, s)
                : launch_stage(t, channel_decimate_kernel<false>, d_iq, d_out, d_taps, d_tail_in, d_tail_out, a, max_wgs, device, s);
}

}  // namespace sddc
