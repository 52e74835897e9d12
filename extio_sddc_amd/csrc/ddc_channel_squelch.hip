// ddc_channel_squelch.hip — the channel squelch for gfx950 (sddc_ddc_channel_squelch_device): a gate per
// channel on real audio streams, F32 or S16 in and out, driven by the block level of a sense stream (the
// audio itself, a second real buffer, or the complex buffer the demodulator read), streaming (each
// channel's state machine, last level and unfinished block live in the handle), in the block form that
// squelch_math.h defines.
//
// A launch covers the stream blocks (B = 256 samples, anchored to the stream position) that hold one of
// its samples; u is a sample's index counted from the start of the first of them, so the launch's samples
// are hb <= u < end, nblocks blocks of which the first nc are complete at its end.  Three launches on the
// caller's stream, all reading the handle's state as it was before the call:
//   levels   channel_squelch_levels_kernel: a wave owns a run of consecutive blocks of one channel.  Lane l
//            holds samples 4 l .. 4 l + 3 of a block, one 16-byte load (8 bytes of S16, two loads of CF32)
//            where the base, the stride and the position allow, else four loads; q per sample, the lower
//            two tree levels in the lane and the upper six as xor-shuffles of one value (the definition's
//            tree: the same additions as ddc_channel_blank.hip's, which keeps four values per lane through
//            the shuffles; measured: DESIGN.md §4.18), the next block's samples loaded before the current
//            block's arithmetic.  A complete block's level goes into words[c][k] (the sign bit marks a bad
//            block: a level is never negative), the unfinished block's q values and bad flag into the
//            other state buffer.  The sense stream is read once.
//   gates    channel_squelch_gates_kernel: a wave per channel walks the channel's blocks in stream order, 64
//            per step and four steps per load: a lane per block for the comparisons, two ballots, then the
//            state machine on the ballots in scalar registers.  A step that cannot move the gate (closed
//            and no u-block, or open and every block a v-block) is closed-form bit arithmetic; any other
//            step is a serial walk over its 64 bits.  It replaces words[c][k] by how block k is weighted
//            (squelch_kind: zero, pass, fade up, fade down) and writes the rest of the next state, d_open,
//            d_count and d_level.  Nothing here touches the streams.
//   outputs  channel_squelch_outputs_kernel: a wave per run of blocks again.  A block of kind zero is
//            written as +0 without a read; the others are read once and written once, four consecutive
//            samples per lane (16 bytes of F32) where the bases, the strides and the position allow, else
//            lane l takes samples l, l + 64, l + 128, l + 192.
// With the sense kind SELF the audio is therefore read twice in all (once for levels, once for outputs,
// less the closed blocks).  The host swaps the two state buffers per launch, so no wave reads what another
// one writes.  Nothing outside the streams is read or written.
//
// Determinism: every value is squelch_math.h's fixed sequence of operations; the grid, the run length, the
// stream and the other channels decide only which wave does it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ddc_kernels.h"

#pragma clang fp contract(off)
#include "demod_math.h"
#include "squelch_math.h"

namespace sddc {
namespace {

using namespace squelch;

constexpr int B = kSquelchBlock;
constexpr int W = 64;    // threads per workgroup: one wave
constexpr int WR = 8;    // blocks per wave of the levels and the outputs kernels
// a channel's state, in 32-bit words
constexpr int R_OFF = 0, N_OFF = 1, OPEN_OFF = 2, GPREV_OFF = 3, BAD_OFF = 4, LEVEL_OFF = 5;
constexpr int Q_OFF = 8;   // the unfinished block's q values
static_assert(Q_OFF + B == kSquelchStateWords, "state layout");
constexpr uint32_t kBadBit = 0x80000000u;

struct Args {
    int hb, end;        // the launch's samples are hb <= u < end
    int nblocks, nc;    // blocks that hold samples of the launch; blocks complete at its end
    int nch, nruns;     // nruns: runs of WR blocks per channel
    int attack, hang, fade;
    int accumulate;     // d_count holds the earlier launches of the same call
    long long in_stride, out_stride, sense_stride;   // samples (sense: real or complex samples) per channel
};

// the sense stream's sample types: a real float, a real int16, a float pair, an int16 pair
enum { S_F32 = 0, S_S16 = 1, S_CF32 = 2, S_CS16 = 3 };
template <int S> struct SenseT;
template <> struct SenseT<S_F32> { using T = float; };
template <> struct SenseT<S_S16> { using T = short; };
template <> struct SenseT<S_CF32> { using T = float2; };
template <> struct SenseT<S_CS16> { using T = uint32_t; };

template <int S> __device__ __forceinline__ float sense_q(typename SenseT<S>::T r)
{
    if constexpr (S == S_F32) return squelch_q_real(r);
    else if constexpr (S == S_S16) return squelch_q_real((float)r);
    else if constexpr (S == S_CF32) return blank::blank_power(r.x, r.y);
    else return blank::blank_power((float)(short)(r & 0xffffu), (float)(short)(r >> 16));
}

// samples u0 .. u0 + 3 of a stream whose sample 0 is at p, with the widest aligned loads
template <int S> __device__ __forceinline__ void load_quad(const typename SenseT<S>::T *__restrict__ p, typename SenseT<S>::T (&d)[4])
{
    if constexpr (S == S_F32) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else if constexpr (S == S_S16) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        d[0] = (short)(v.x & 0xffffu), d[1] = (short)(v.x >> 16), d[2] = (short)(v.y & 0xffffu), d[3] = (short)(v.y >> 16);
    } else if constexpr (S == S_CF32) {
        const float4 v = reinterpret_cast<const float4 *>(p)[0], w = reinterpret_cast<const float4 *>(p)[1];
        d[0] = make_float2(v.x, v.y), d[1] = make_float2(v.z, v.w), d[2] = make_float2(w.x, w.y), d[3] = make_float2(w.z, w.w);
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
}

// words: [nch][nblocks].  state: [nch][kSquelchStateWords].  VEC: every quad 4 l .. 4 l + 3 of a block is
// aligned to its load.
template <int S, bool VEC>
__global__ __launch_bounds__(W) void channel_squelch_levels_kernel(const void *__restrict__ sense_, uint32_t *__restrict__ words,
                                                                   const uint32_t *__restrict__ state_in,
                                                                   uint32_t *__restrict__ state_out, const Args a)
{
    using T = typename SenseT<S>::T;
    const int lane = (int)threadIdx.x;
    const long long nitems = (long long)a.nch * a.nruns;
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.nruns), r = (int)(item - (long long)c * a.nruns);
        const int ka = r * WR, kb = ka + WR < a.nblocks ? ka + WR : a.nblocks;
        // sample u of the launch's blocks is in[u]; only hb <= u < end is touched
        const T *__restrict__ in = static_cast<const T *>(sense_) + c * a.sense_stride - a.hb;
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kSquelchStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kSquelchStateWords;
        auto load_block = [&](int kk, T (&dst)[4]) {
            const int u0 = kk * B + 4 * lane;
            if (VEC && u0 >= a.hb && u0 + 4 <= a.end) {
                load_quad<S>(in + u0, dst);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    dst[j] = T{};
                    if (u0 + j >= a.hb && u0 + j < a.end) dst[j] = in[u0 + j];
                }
            }
        };
        T nxt[4];
        load_block(ka, nxt);
        for (int kk = ka; kk < kb; kk++) {
            T raw[4];
#pragma unroll
            for (int j = 0; j < 4; j++) raw[j] = nxt[j];
            if (kk + 1 < kb) load_block(kk + 1, nxt);
            float s[4];
            bool bad = false;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = kk * B + 4 * lane + j;
                const bool valid = u >= a.hb && u < a.end;
                const float q = sense_q<S>(raw[j]);
                const bool fin = blank::blank_finite(q);
                s[j] = fin ? q : 0.f;
                bad = bad || (valid && !fin);
                if (!valid) s[j] = u < a.hb ? __uint_as_float(st_in[Q_OFF + u]) : 0.f;   // u < hb: block 0, u < B
            }
            unsigned long long anybad = __ballot(bad);
            if (kk == 0 && a.hb > 0 && st_in[BAD_OFF]) anybad = 1;
            if (kk >= a.nc) {   // the unfinished block: its q values are the next call's
#pragma unroll
                for (int j = 0; j < 4; j++) st_out[Q_OFF + 4 * lane + j] = __float_as_uint(s[j]);
                if (lane == 0) st_out[BAD_OFF] = anybad ? 1u : 0u;
            } else {
                float p = (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
                for (int m = 1; m < W; m <<= 1) p = p + __shfl_xor(p, m);
                if (lane == 0) words[(size_t)c * a.nblocks + kk] = (__float_as_uint(p) & ~kBadBit) | (anybad ? kBadBit : 0u);
            }
        }
    }
}

// modes: [nch]; thr: [nch] (256 To, 256 Tc).  open, count, level: null or [nch].
__global__ __launch_bounds__(W) void channel_squelch_gates_kernel(uint32_t *__restrict__ words, const int *__restrict__ modes,
                                                                  const float2 *__restrict__ thr,
                                                                  const uint32_t *__restrict__ state_in,
                                                                  uint32_t *__restrict__ state_out, uint32_t *__restrict__ d_open,
                                                                  uint32_t *__restrict__ d_count, float *__restrict__ d_level,
                                                                  const Args a)
{
    constexpr int NS = 4;   // steps per load
    const int lane = (int)threadIdx.x;
    const uint32_t A = (uint32_t)a.attack, H = (uint32_t)a.hang;
    auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };   // wave-uniform: scalar registers
    for (int c = (int)blockIdx.x; c < a.nch; c += (int)gridDim.x) {
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kSquelchStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kSquelchStateWords;
        uint32_t *__restrict__ w = words + (size_t)c * a.nblocks;
        const int mode = (int)uni((uint32_t)modes[c]);
        const float2 t = thr[c];
        const bool gated = mode == kSquelchLevel || mode == kSquelchNoise;
        uint32_t r = uni(st_in[R_OFF]), n = uni(st_in[N_OFF]), open = uni(st_in[OPEN_OFF]), gprev = uni(st_in[GPREV_OFF]);
        uint32_t level = uni(st_in[LEVEL_OFF]);
        uint32_t before = gprev;   // the gate of the block before the step's first one
        uint32_t cnt = 0;
        for (int kq = 0; kq < a.nblocks; kq += NS * W) {
            uint32_t word[NS];
#pragma unroll
            for (int q = 0; q < NS; q++) word[q] = kq + q * W + lane < a.nc ? w[kq + q * W + lane] : 0u;
#pragma unroll
            for (int q = 0; q < NS; q++) {
                const int k0 = kq + q * W, k = k0 + lane;
                if (k0 >= a.nblocks) break;
                const int m = a.nblocks - k0 < W ? a.nblocks - k0 : W;             // blocks of this step
                const int mc = a.nc - k0 < 0 ? 0 : (a.nc - k0 < W ? a.nc - k0 : W);   // the complete ones among them
                const unsigned long long mm = ~0ull >> (W - m), cm = mc ? ~0ull >> (W - mc) : 0ull;
                bool u, v;
                squelch_flags(__uint_as_float(word[q] & ~kBadBit), (word[q] & kBadBit) != 0, mode, t.x, t.y, &u, &v);
                const unsigned long long U = __ballot(u) & cm, V = __ballot(v) & cm;
                unsigned long long G = 0;
                if (!gated) {
                    G = mode == kSquelchOff ? ~0ull : 0ull;
                } else if (!open && U == 0) {
                    // stays closed: r = 0, n counts the blocks since the last v-block
                    if (mc) {
                        const uint32_t since = V ? (uint32_t)(mc - 1 - (63 - __builtin_clzll(V))) : n + (uint32_t)mc;
                        n = since < H + 1 ? since : H + 1;
                        r = 0;
                        gprev = 0;
                    }
                } else if (open && V == cm) {
                    // stays open: n = 0, r counts the u-blocks since the last block that is none
                    G = mm;
                    if (mc) {
                        const unsigned long long Z = ~U & cm;
                        const uint32_t run = Z ? (uint32_t)(mc - 1 - (63 - __builtin_clzll(Z))) : r + (uint32_t)mc;
                        r = run < A ? run : A;
                        n = 0;
                        gprev = 1;
                    }
                } else {
                    for (int j = 0; j < m; j++) {
                        const uint32_t g = open;
                        G |= (unsigned long long)g << j;
                        if (j < mc) {
                            gprev = g;
                            squelch_step((U >> j) & 1, (V >> j) & 1, A, H, &r, &n, &open);
                        }
                    }
                }
                if (mc > 0) level = uni((uint32_t)__shfl((int)word[q], mc - 1)) & ~kBadBit;
                const uint32_t g = (uint32_t)(G >> lane) & 1u;
                const uint32_t gp = lane ? (uint32_t)(G >> (lane - 1)) & 1u : before;
                before = (uint32_t)(G >> (m - 1)) & 1u;
                if (k < a.nblocks) {
                    w[k] = (uint32_t)squelch_kind(mode, g, gp, a.fade);
                    const int lo = k * B > a.hb ? k * B : a.hb, hi = (k + 1) * B < a.end ? (k + 1) * B : a.end;
                    cnt += g ? (uint32_t)(hi - lo) : 0u;
                }
            }
        }
#pragma unroll
        for (int m = 1; m < W; m <<= 1) cnt += __shfl_xor(cnt, m);
        if (lane == 0) {
            st_out[R_OFF] = r;
            st_out[N_OFF] = n;
            st_out[OPEN_OFF] = open;
            st_out[GPREV_OFF] = gprev;
            st_out[LEVEL_OFF] = level;
            if (d_open) d_open[c] = mode == kSquelchOff ? 1u : (gated ? open : 0u);
            if (d_count) d_count[c] = (a.accumulate ? d_count[c] : 0u) + cnt;
            if (d_level) d_level[c] = __uint_as_float(level);
        }
    }
}

template <bool IN16> struct InQ;    // four consecutive input samples
template <> struct InQ<false> { using T = uint4; };
template <> struct InQ<true> { using T = uint2; };

// sample i of a block of `kind` (not kZero) from the stored input word (F32 bits, or a sign-extended code)
template <bool IN16, bool OUT16> __device__ __forceinline__ uint32_t gate_sample(int kind, int i, uint32_t raw)
{
    const float x = IN16 ? (float)(int)raw : __uint_as_float(raw);
    if constexpr (OUT16) return (uint32_t)(uint16_t)demod::demod_s16(squelch_apply(kind, i, x));
    else if constexpr (!IN16) return kind == kPass ? raw : __float_as_uint(squelch_apply(kind, i, x));   // a NaN keeps its payload
    else return __float_as_uint(squelch_apply(kind, i, x));
}

template <bool IN16, bool OUT16, bool VEC>
__global__ __launch_bounds__(W) void channel_squelch_outputs_kernel(const void *__restrict__ in_, void *__restrict__ out_,
                                                                    const uint32_t *__restrict__ words, const Args a)
{
    using I = std::conditional_t<IN16, short, uint32_t>;
    using O = std::conditional_t<OUT16, unsigned short, uint32_t>;
    using IQ = typename InQ<IN16>::T;
    using OQ = typename InQ<OUT16>::T;
    const int lane = (int)threadIdx.x;
    const long long nitems = (long long)a.nch * a.nruns;
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.nruns), r = (int)(item - (long long)c * a.nruns);
        const int ka = r * WR, kb = ka + WR < a.nblocks ? ka + WR : a.nblocks;
        // sample u of the launch's blocks is in[u] / out[u]; only hb <= u < end is touched
        const I *__restrict__ in = static_cast<const I *>(in_) + c * a.in_stride - a.hb;
        O *__restrict__ out = static_cast<O *>(out_) + c * a.out_stride - a.hb;
        for (int kk = ka; kk < kb; kk++) {
            const int kind = (int)words[(size_t)c * a.nblocks + kk];
            if constexpr (VEC) {
                const int i0 = 4 * lane, u0 = kk * B + i0;
                if (u0 >= a.hb && u0 + 4 <= a.end) {
                    uint32_t y[4] = {0u, 0u, 0u, 0u};
                    if (kind != kZero) {
                        const IQ v = *reinterpret_cast<const IQ *>(in + u0);
                        uint32_t x[4];
                        if constexpr (IN16) {
                            x[0] = (uint32_t)(int)(short)(v.x & 0xffffu);
                            x[1] = (uint32_t)((int)v.x >> 16);
                            x[2] = (uint32_t)(int)(short)(v.y & 0xffffu);
                            x[3] = (uint32_t)((int)v.y >> 16);
                        } else {
                            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
                        }
#pragma unroll
                        for (int q = 0; q < 4; q++) y[q] = gate_sample<IN16, OUT16>(kind, i0 + q, x[q]);
                    }
                    OQ o;
                    if constexpr (OUT16) {
                        o.x = y[0] | (y[1] << 16);
                        o.y = y[2] | (y[3] << 16);
                    } else {
                        o.x = y[0], o.y = y[1], o.z = y[2], o.w = y[3];
                    }
                    *reinterpret_cast<OQ *>(out + u0) = o;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int u = u0 + q;
                        if (u >= a.hb && u < a.end)
                            out[u] = (O)(kind == kZero ? 0u : gate_sample<IN16, OUT16>(kind, i0 + q, (uint32_t)(int)in[u]));
                    }
                }
            } else {
                uint32_t x[4] = {0u, 0u, 0u, 0u};
                if (kind != kZero) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int u = kk * B + W * j + lane;
                        if (u >= a.hb && u < a.end) x[j] = (uint32_t)(int)in[u];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int u = kk * B + W * j + lane;
                    if (u >= a.hb && u < a.end) out[u] = (O)(kind == kZero ? 0u : gate_sample<IN16, OUT16>(kind, W * j + lane, x[j]));
                }
            }
        }
    }
}

hipError_t grid_of(const KernelTables &t, const void *kern, long long items, int max_wgs, int device, unsigned *grid)
{
    int occ = 0, cus = 0;
    const hipError_t e = launch_geometry(t.lc, kern, W, device, &occ, &cus);
    if (e != hipSuccess) return e;
    long long g = items;
    if (g > (long long)cus * occ) g = (long long)cus * occ;
    if (max_wgs > 0 && g > max_wgs) g = max_wgs;
    *grid = (unsigned)(g < 1 ? 1 : g);
    return hipSuccess;
}

template <int S, bool VEC>
hipError_t launch_levels_v(const KernelTables &t, const void *d_sense, uint32_t *d_words, const uint32_t *st_in, uint32_t *st_out,
                           const Args &a, int max_wgs, int device, hipStream_t s)
{
    const auto k = channel_squelch_levels_kernel<S, VEC>;
    unsigned grid = 0;
    const hipError_t e = grid_of(t, reinterpret_cast<const void *>(k), (long long)a.nch * a.nruns, max_wgs, device, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(W), 0, s, d_sense, d_words, st_in, st_out, a);
    return hipGetLastError();
}

// size: the bytes of a sense sample; quads are aligned to min(16, 4 size) bytes
template <int S>
hipError_t launch_levels(const KernelTables &t, const void *d_sense, uint32_t *d_words, const uint32_t *st_in, uint32_t *st_out,
                         const Args &a, int max_wgs, int device, hipStream_t s)
{
    const uintptr_t size = sizeof(typename SenseT<S>::T), align = 4 * size < 16 ? 4 * size : 16;
    const bool vec = (((uintptr_t)d_sense - (uintptr_t)a.hb * size) % align) == 0 && ((uintptr_t)a.sense_stride * size) % align == 0;
    return vec ? launch_levels_v<S, true>(t, d_sense, d_words, st_in, st_out, a, max_wgs, device, s)
               : launch_levels_v<S, false>(t, d_sense, d_words, st_in, st_out, a, max_wgs, device, s);
}

template <bool IN16, bool OUT16, bool VEC>
hipError_t launch_outputs(const KernelTables &t, const void *d_in, void *d_out, const uint32_t *d_words, const Args &a,
                          int max_wgs, int device, hipStream_t s)
{
    const auto k = channel_squelch_outputs_kernel<IN16, OUT16, VEC>;
    unsigned grid = 0;
    const hipError_t e = grid_of(t, reinterpret_cast<const void *>(k), (long long)a.nch * a.nruns, max_wgs, device, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(W), 0, s, d_in, d_out, d_words, a);
    return hipGetLastError();
}

template <bool IN16, bool OUT16>
hipError_t launch_outputs_v(bool vec, const KernelTables &t, const void *d_in, void *d_out, const uint32_t *d_words,
                            const Args &a, int max_wgs, int device, hipStream_t s)
{
    return vec ? launch_outputs<IN16, OUT16, true>(t, d_in, d_out, d_words, a, max_wgs, device, s)
               : launch_outputs<IN16, OUT16, false>(t, d_in, d_out, d_words, a, max_wgs, device, s);
}

}  // namespace

hipError_t launch_channel_squelch(const KernelTables &t, const void *d_audio, int in_s16, const void *d_sense, int sense_kind,
                                  int nch, size_t nsamp, size_t in_stride, size_t sense_stride, uint64_t pos,
                                  const int *d_modes, const float *d_thr, int attack, int hang, int fade,
                                  const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_words, void *d_out,
                                  int out_s16, size_t out_stride, uint32_t *d_open, uint32_t *d_count, float *d_level,
                                  int accumulate, int max_wgs, int device, hipStream_t s)
{
    if (!d_audio || !d_out || !d_modes || !d_thr || !d_state_in || !d_state_out || !d_words || nch < 1 || nsamp == 0 ||
        nsamp > kSquelchMaxLaunch || attack < 1 || attack > kSquelchMaxAttack || hang < 0 || hang > kSquelchMaxHang ||
        sense_kind < kSenseSelf || sense_kind > kSenseCS16 || (sense_kind != kSenseSelf && !d_sense))
        return hipErrorInvalidValue;
    Args a;
    a.hb = (int)(pos % (uint64_t)B);
    a.end = a.hb + (int)nsamp;
    a.nblocks = (a.end + B - 1) / B;
    a.nc = a.end / B;
    a.nch = nch;
    a.nruns = (a.nblocks + WR - 1) / WR;
    a.attack = attack;
    a.hang = hang;
    a.fade = fade ? 1 : 0;
    a.accumulate = accumulate ? 1 : 0;
    a.in_stride = nch > 1 ? (long long)in_stride : 0;
    a.out_stride = nch > 1 ? (long long)out_stride : 0;
    const bool cplx = sense_kind == kSenseCF32 || sense_kind == kSenseCS16;
    a.sense_stride = nch > 1 ? (long long)(sense_kind == kSenseSelf ? in_stride : cplx ? sense_stride / 2 : sense_stride) : 0;

    hipError_t e;
    switch (sense_kind) {
    case kSenseSelf:
        e = in_s16 ? launch_levels<S_S16>(t, d_audio, d_words, d_state_in, d_state_out, a, max_wgs, device, s)
                   : launch_levels<S_F32>(t, d_audio, d_words, d_state_in, d_state_out, a, max_wgs, device, s);
        break;
    case kSenseF32: e = launch_levels<S_F32>(t, d_sense, d_words, d_state_in, d_state_out, a, max_wgs, device, s); break;
    case kSenseS16: e = launch_levels<S_S16>(t, d_sense, d_words, d_state_in, d_state_out, a, max_wgs, device, s); break;
    case kSenseCF32: e = launch_levels<S_CF32>(t, d_sense, d_words, d_state_in, d_state_out, a, max_wgs, device, s); break;
    default: e = launch_levels<S_CS16>(t, d_sense, d_words, d_state_in, d_state_out, a, max_wgs, device, s); break;
    }
    if (e != hipSuccess) return e;

    unsigned grid = 0;
    const auto gates = channel_squelch_gates_kernel;
    if ((e = grid_of(t, reinterpret_cast<const void *>(gates), nch, max_wgs, device, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(gates, dim3(grid), dim3(W), 0, s, d_words, d_modes, reinterpret_cast<const float2 *>(d_thr), d_state_in,
                       d_state_out, d_open, d_count, d_level, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    // four consecutive samples per lane where every quad of a block is aligned on both sides
    const uintptr_t is = in_s16 ? 2 : 4, os = out_s16 ? 2 : 4;
    const bool vec = (((uintptr_t)d_audio - (uintptr_t)a.hb * is) % (4 * is)) == 0 &&
                     (((uintptr_t)d_out - (uintptr_t)a.hb * os) % (4 * os)) == 0 && a.in_stride % 4 == 0 && a.out_stride % 4 == 0;
    if (in_s16)
        return out_s16 ? launch_outputs_v<true, true>(vec, t, d_audio, d_out, d_words, a, max_wgs, device, s)
                       : launch_outputs_v<true, false>(vec, t, d_audio, d_out, d_words, a, max_wgs, device, s);
    return out_s16 ? launch_outputs_v<false, true>(vec, t, d_audio, d_out, d_words, a, max_wgs, device, s)
                   : launch_outputs_v<false, false>(vec, t, d_audio, d_out, d_words, a, max_wgs, device, s);
}

}  // namespace sddc
