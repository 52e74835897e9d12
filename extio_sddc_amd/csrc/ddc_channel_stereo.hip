// ddc_channel_stereo.hip — the channel stereo decoder for gfx950 (sddc_ddc_channel_stereo_device): the
// pilot's single-bin DFT per channel over a real MPX stream (F32 or S16), the stereo / mono gate, and the
// matrix L = x + d, R = x - d with d = (2 g x) sin(2 psi) into two output streams (F32 or S16), streaming (each
// channel's gate, carrier phase, last results, unfinished window and unfinished block live in the handle), in
// the block and window form that stereo_math.h defines.
//
// A launch covers the stream blocks (B = 256 samples, anchored to the stream position) that hold one of its
// samples; u is a sample's index counted from the start of the first of them, so the launch's samples are hs
// <= u < end (hs < B), in nblk blocks of which the first nfull are complete at its end; the first block is
// block kw0 of its window.  Three launches on the caller's stream, all reading the handle's state as it was
// before the call:
//   windows  channel_stereo_windows_kernel: a wave owns a run of kRunBlocks blocks of one channel.  Lane l
//            holds samples 4 l .. 4 l + 3 of a block, one 16-byte load (8 bytes of S16) where the base, the
//            stride and the position allow, else four loads; its four pilot phasors depend on the lane alone
//            and are computed once per wave.  Per block 12 multiplies, three sums (two tree levels in the
//            lane, six xor-shuffle steps across lanes: blank_tree's additions) and the block rotation, which
//            is wave-uniform.  Lane 0 writes (Re_k, Im_k, p_k, bad) to the scratch.  The wave that meets the
//            launch's first block takes the samples before hs from the state's stored block; the one that
//            meets an unfinished last block writes the next state's.  No LDS.
//   gates    channel_stereo_gates_kernel: a lane per channel walks the channel's blocks in stream order:
//            the folds, and at a window's end the flags, the phase (one sqrt, two divisions) and squelch_step.
//            It writes (stereo, qr, qi) of every window that holds a sample to the scratch, the rest of the
//            next state, d_stereo, d_count, d_level and d_phase.
//   outputs  channel_stereo_outputs_kernel, the hot path: a wave owns WR blocks of one channel, a lane four
//            samples of each; the lane's four carrier phasors of w2 depend on the lane alone and live in
//            registers.  Per block of an open window one wave-uniform phasor and rotation, per sample one fma,
//            three multiplies, an add and a subtract; 16-byte loads and stores where the three bases, the
//            strides and the position allow (VEC), else a sample per lane and step.  A block of a closed window
//            or of a MONO channel is copied.
// The host swaps the two state buffers per launch set, so no wave reads what another one writes.  Nothing
// outside the streams is read or written.
//
// Determinism: every value is stereo_math.h's fixed sequence of operations; the grid, the run length, the
// stream and the other channels decide only which wave does it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ddc_kernels.h"

#pragma clang fp contract(off)
#include "stereo_math.h"

namespace sddc {
namespace {

using namespace stereo;

constexpr int B = kStereoBlock;
constexpr int WV = 64;           // threads per workgroup: one wave
constexpr int kRunBlocks = 32;   // blocks per wave of the windows kernel
constexpr int WR = 8;            // blocks per wave of the outputs kernel
// a channel's state, in 32-bit words (cpu::R2iq::StereoChannel)
constexpr int R_OFF = 0, N_OFF = 1, OPEN_OFF = 2, QR_OFF = 3, QI_OFF = 4, PLAST_OFF = 5, ELAST_OFF = 6;
constexpr int ZR_OFF = 7, ZI_OFF = 8, E_OFF = 9, BAD_OFF = 10;
constexpr int X_OFF = 12;   // the unfinished block's samples
static_assert(X_OFF + B == kStereoStateWords, "state layout");
static_assert(4 * WV == B, "a lane holds four samples of a block");

struct Args {
    int hs, end;          // the launch's samples are hs <= u < end
    int W, kw0;           // blocks per window; the first block's index in its window
    int nblk, nfull;      // blocks that hold samples of the launch; the ones complete at its end
    int nwin;             // windows that hold one of these blocks
    int nch, nruns;       // nruns: runs of kRunBlocks blocks per channel (windows kernel)
    int oruns;            // runs of WR blocks per channel (outputs kernel)
    int attack, hang;
    int accumulate;       // d_count holds the earlier launches of the same call
    uint32_t pos256;      // the stream position of u = 0, modulo 2^32 (a multiple of 256)
    uint32_t w, w2;       // the pilot's phase word and the carrier's
    long long in_stride, out_stride;   // samples per channel
};

template <bool S16> struct SampleT { using T = std::conditional_t<S16, short, float>; };

template <bool S16> __device__ __forceinline__ void load_quad(const typename SampleT<S16>::T *__restrict__ p, float (&d)[4])
{
    if constexpr (!S16) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        d[0] = (float)(short)(v.x & 0xffffu), d[1] = (float)(short)(v.x >> 16);
        d[2] = (float)(short)(v.y & 0xffffu), d[3] = (float)(short)(v.y >> 16);
    }
}

__device__ __forceinline__ float wave_tree(float p)
{
#pragma unroll
    for (int m = 1; m < WV; m <<= 1) p = p + __shfl_xor(p, m);
    return p;
}

// scratch: [nch][nblk][4] block words, then [nch][nwin][4] window words.  state: [nch][kStereoStateWords].
// VEC: every quad 4 l .. 4 l + 3 of a block is aligned to its load.
template <bool S16, bool VEC>
__global__ __launch_bounds__(WV) void channel_stereo_windows_kernel(const void *__restrict__ in_, uint32_t *__restrict__ scratch,
                                                                    const uint32_t *__restrict__ state_in,
                                                                    uint32_t *__restrict__ state_out, const Args a)
{
    using T = typename SampleT<S16>::T;
    const int lane = (int)threadIdx.x;
    float pc[4], ps[4];
#pragma unroll
    for (int q = 0; q < 4; q++) tone::tone_phasor(a.w, (uint32_t)(4 * lane + q), &pc[q], &ps[q]);
    const long long nitems = (long long)a.nch * a.nruns;
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.nruns), r = (int)(item - (long long)c * a.nruns);
        const int ka = r * kRunBlocks, kb = ka + kRunBlocks < a.nblk ? ka + kRunBlocks : a.nblk;
        // sample u of the launch's blocks is in[u]; only hs <= u < end is touched
        const T *__restrict__ in = static_cast<const T *>(in_) + c * a.in_stride - a.hs;
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kStereoStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kStereoStateWords;
        for (int kk = ka; kk < kb; kk++) {
            const int u0 = kk * B + 4 * lane;
            float x[4];
            if (VEC && u0 >= a.hs && u0 + 4 <= a.end) {
                load_quad<S16>(in + u0, x);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int u = u0 + j;
                    x[j] = 0.f;
                    if (u >= a.hs && u < a.end) x[j] = (float)in[u];
                    else if (u < a.hs) x[j] = __uint_as_float(st_in[X_OFF + u]);   // kk = 0: the stored block
                }
            }
            bool bad = false;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool fin = blank::blank_finite(x[j] * x[j]);
                x[j] = fin ? x[j] : 0.f;
                bad = bad || !fin;
            }
            const uint32_t anybad = __ballot(bad) ? 1u : 0u;
            uint4 wd = make_uint4(0u, 0u, 0u, anybad);
            if (kk < a.nfull) {
                const float q0 = x[0] * x[0], q1 = x[1] * x[1], q2 = x[2] * x[2], q3 = x[3] * x[3];
                const float a0 = x[0] * pc[0], a1 = x[1] * pc[1], a2 = x[2] * pc[2], a3 = x[3] * pc[3];
                const float b0 = x[0] * ps[0], b1 = x[1] * ps[1], b2 = x[2] * ps[2], b3 = x[3] * ps[3];
                const float pk = wave_tree((q0 + q1) + (q2 + q3));
                const float Ck = wave_tree((a0 + a1) + (a2 + a3)), Sk = wave_tree((b0 + b1) + (b2 + b3));
                float cr, sr, re, im;
                tone::tone_phasor(a.w, a.pos256 + (uint32_t)kk * (uint32_t)B, &cr, &sr);   // wave-uniform
                tone::tone_rotate(Ck, Sk, cr, sr, &re, &im);
                wd.x = __float_as_uint(re), wd.y = __float_as_uint(im), wd.z = __float_as_uint(pk);
            } else {   // the stream ends inside this block: its samples are the next call's
#pragma unroll
                for (int q = 0; q < 4; q++) st_out[X_OFF + 4 * lane + q] = __float_as_uint(x[q]);
            }
            if (lane == 0) *reinterpret_cast<uint4 *>(scratch + ((size_t)c * a.nblk + kk) * 4) = wd;
        }
    }
}

// modes: [nch]; thr: [nch][4] (To, Tc, Emin, g2).  d_stereo, d_count: null or [nch]; d_level, d_phase: null or
// [nch][2].
__global__ __launch_bounds__(WV) void channel_stereo_gates_kernel(uint32_t *__restrict__ scratch, const uint32_t *__restrict__ modes,
                                                                  const float *__restrict__ thr, const uint32_t *__restrict__ state_in,
                                                                  uint32_t *__restrict__ state_out, uint32_t *__restrict__ d_stereo,
                                                                  uint32_t *__restrict__ d_count, float *__restrict__ d_level,
                                                                  float *__restrict__ d_phase, const Args a)
{
    const uint32_t A = (uint32_t)a.attack, H = (uint32_t)a.hang;
    const int WB = a.W * B;   // samples per window
    for (int c = (int)(blockIdx.x * WV + threadIdx.x); c < a.nch; c += (int)gridDim.x * WV) {
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kStereoStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kStereoStateWords;
        const uint4 *__restrict__ blk = reinterpret_cast<const uint4 *>(scratch) + (size_t)c * a.nblk;
        uint4 *__restrict__ win = reinterpret_cast<uint4 *>(scratch) + (size_t)a.nch * a.nblk + (size_t)c * a.nwin;
        const bool autom = modes[c] == (uint32_t)kStereoAuto;
        const float To = thr[4 * c], Tc = thr[4 * c + 1], Emin = thr[4 * c + 2];
        uint32_t r = st_in[R_OFF], n = st_in[N_OFF], open = st_in[OPEN_OFF];
        float qr = __uint_as_float(st_in[QR_OFF]), qi = __uint_as_float(st_in[QI_OFF]);
        float plast = __uint_as_float(st_in[PLAST_OFF]), elast = __uint_as_float(st_in[ELAST_OFF]);
        float zr = __uint_as_float(st_in[ZR_OFF]), zi = __uint_as_float(st_in[ZI_OFF]), E = __uint_as_float(st_in[E_OFF]);
        uint32_t bad = st_in[BAD_OFF];
        uint32_t cnt = 0;
        int kw = a.kw0, jj = 0;
        // window jj of the launch takes the gate and the phase in force; its samples of the launch are counted
        auto emit = [&]() {
            const uint32_t g = autom ? open : 0u;
            win[jj] = make_uint4(g, __float_as_uint(qr), __float_as_uint(qi), 0u);
            const int lo = (jj * a.W - a.kw0) * B, hi = lo + WB;
            const int l2 = lo > a.hs ? lo : a.hs, h2 = hi < a.end ? hi : a.end;
            cnt += g ? (uint32_t)(h2 - l2) : 0u;
        };
        emit();
        for (int kk = 0; kk < a.nfull; kk++) {
            const uint4 wd = blk[kk];
            zr = zr + __uint_as_float(wd.x);
            zi = zi + __uint_as_float(wd.y);
            E = E + __uint_as_float(wd.z);
            bad |= wd.w;
            if (++kw < a.W) continue;
            kw = 0;
            const float P = blank::blank_power(zr, zi);
            bool u, v;
            tone::tone_flags(P, E, bad != 0, To, Tc, Emin, &u, &v);
            if (v) stereo_phase(zr, zi, P, &qr, &qi);
            squelch::squelch_step(u, v, A, H, &r, &n, &open);
            plast = P, elast = E;
            zr = zi = E = 0.f;
            bad = 0;
            if (++jj < a.nwin) emit();
        }
        if (a.nblk > a.nfull) bad |= blk[a.nfull].w;
        st_out[R_OFF] = r;
        st_out[N_OFF] = n;
        st_out[OPEN_OFF] = open;
        st_out[QR_OFF] = __float_as_uint(qr);
        st_out[QI_OFF] = __float_as_uint(qi);
        st_out[PLAST_OFF] = __float_as_uint(plast);
        st_out[ELAST_OFF] = __float_as_uint(elast);
        st_out[ZR_OFF] = __float_as_uint(zr);
        st_out[ZI_OFF] = __float_as_uint(zi);
        st_out[E_OFF] = __float_as_uint(E);
        st_out[BAD_OFF] = bad;
        st_out[BAD_OFF + 1] = 0u;
        if (d_stereo) d_stereo[c] = autom ? open : 0u;
        if (d_count) d_count[c] = (a.accumulate ? d_count[c] : 0u) + cnt;
        if (d_level) d_level[2 * c] = plast, d_level[2 * c + 1] = elast;
        if (d_phase) d_phase[2 * c] = qr, d_phase[2 * c + 1] = qi;
    }
}

template <bool S16> struct Quad;    // four consecutive samples
template <> struct Quad<false> { using T = uint4; };
template <> struct Quad<true> { using T = uint2; };

// the float value of a stored input word (F32 bits, or a sign-extended code)
template <bool IN16> __device__ __forceinline__ float value_of(uint32_t raw)
{
    if constexpr (IN16) return (float)(int)raw;
    else return __uint_as_float(raw);
}

// a passed sample from the stored input word
template <bool IN16, bool OUT16> __device__ __forceinline__ uint32_t pass_sample(uint32_t raw)
{
    if constexpr (OUT16) return (uint32_t)(uint16_t)demod::demod_s16(value_of<IN16>(raw));
    else if constexpr (!IN16) return raw;   // a NaN keeps its payload
    else return __float_as_uint((float)(int)raw);
}

template <bool OUT16> __device__ __forceinline__ uint32_t out_word(float y)
{
    if constexpr (OUT16) return (uint32_t)(uint16_t)demod::demod_s16(y);
    else return __float_as_uint(y);
}

// win: the scratch's window words [nch][nwin][4]; thr: [nch][4]
template <bool IN16, bool OUT16, bool VEC>
__global__ __launch_bounds__(WV) void channel_stereo_outputs_kernel(const void *__restrict__ in_, void *__restrict__ left_,
                                                                    void *__restrict__ right_, const uint4 *__restrict__ win,
                                                                    const float *__restrict__ thr, const Args a)
{
    using I = std::conditional_t<IN16, short, uint32_t>;
    using O = std::conditional_t<OUT16, unsigned short, uint32_t>;
    using IQ = typename Quad<IN16>::T;
    using OQ = typename Quad<OUT16>::T;
    const int lane = (int)threadIdx.x;
    // the lane's samples of a block: 4 l + q (VEC), 64 q + l (a sample per lane and step)
    float tc[4], ts[4];
#pragma unroll
    for (int q = 0; q < 4; q++) tone::tone_phasor(a.w2, (uint32_t)(VEC ? 4 * lane + q : WV * q + lane), &tc[q], &ts[q]);
    const long long nitems = (long long)a.nch * a.oruns;
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.oruns), r = (int)(item - (long long)c * a.oruns);
        const int ka = r * WR, kb = ka + WR < a.nblk ? ka + WR : a.nblk;
        // sample u of the launch's blocks is in[u] / left[u] / right[u]; only hs <= u < end is touched
        const I *__restrict__ in = static_cast<const I *>(in_) + c * a.in_stride - a.hs;
        O *__restrict__ left = static_cast<O *>(left_) + c * a.out_stride - a.hs;
        O *__restrict__ right = static_cast<O *>(right_) + c * a.out_stride - a.hs;
        const float g2 = thr[4 * c + 3];
        for (int kk = ka; kk < kb; kk++) {
            const uint4 wd = win[(size_t)c * a.nwin + (a.kw0 + kk) / a.W];
            const bool open = wd.x != 0;
            float rr = 0.f, ri = 0.f;
            if (open)   // wave-uniform
                stereo_block(__uint_as_float(wd.y), __uint_as_float(wd.z), a.w2, a.pos256 + (uint32_t)kk * (uint32_t)B, &rr, &ri);
            // the two output words of the stored input word raw, sample q of the lane
            auto sample = [&](uint32_t raw, int q, uint32_t *yl, uint32_t *yr) {
                if (open) {
                    float L, R;
                    stereo_lr(value_of<IN16>(raw), g2, stereo_sub(tc[q], ts[q], rr, ri), &L, &R);
                    *yl = out_word<OUT16>(L), *yr = out_word<OUT16>(R);
                } else {
                    *yl = *yr = pass_sample<IN16, OUT16>(raw);
                }
            };
            if constexpr (VEC) {
                const int u0 = kk * B + 4 * lane;
                if (u0 >= a.hs && u0 + 4 <= a.end) {
                    const IQ v = *reinterpret_cast<const IQ *>(in + u0);
                    uint32_t x[4], yl[4], yr[4];
                    if constexpr (IN16) {
                        x[0] = (uint32_t)(int)(short)(v.x & 0xffffu);
                        x[1] = (uint32_t)((int)v.x >> 16);
                        x[2] = (uint32_t)(int)(short)(v.y & 0xffffu);
                        x[3] = (uint32_t)((int)v.y >> 16);
                    } else {
                        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) sample(x[q], q, &yl[q], &yr[q]);
                    OQ ol, orr;
                    if constexpr (OUT16) {
                        ol.x = yl[0] | (yl[1] << 16), ol.y = yl[2] | (yl[3] << 16);
                        orr.x = yr[0] | (yr[1] << 16), orr.y = yr[2] | (yr[3] << 16);
                    } else {
                        ol.x = yl[0], ol.y = yl[1], ol.z = yl[2], ol.w = yl[3];
                        orr.x = yr[0], orr.y = yr[1], orr.z = yr[2], orr.w = yr[3];
                    }
                    *reinterpret_cast<OQ *>(left + u0) = ol;
                    *reinterpret_cast<OQ *>(right + u0) = orr;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int u = u0 + q;
                        if (u >= a.hs && u < a.end) {
                            uint32_t yl, yr;
                            sample((uint32_t)(int)in[u], q, &yl, &yr);
                            left[u] = (O)yl, right[u] = (O)yr;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int u = kk * B + WV * q + lane;
                    if (u >= a.hs && u < a.end) {
                        uint32_t yl, yr;
                        sample((uint32_t)(int)in[u], q, &yl, &yr);
                        left[u] = (O)yl, right[u] = (O)yr;
                    }
                }
            }
        }
    }
}

hipError_t grid_of(const KernelTables &t, const void *kern, long long items, int max_wgs, int device, unsigned *grid)
{
    int occ = 0, cus = 0;
    const hipError_t e = launch_geometry(t.lc, kern, WV, device, &occ, &cus);
    if (e != hipSuccess) return e;
    long long g = items;
    if (g > (long long)cus * occ) g = (long long)cus * occ;
    if (max_wgs > 0 && g > max_wgs) g = max_wgs;
    *grid = (unsigned)(g < 1 ? 1 : g);
    return hipSuccess;
}

template <bool S16, bool VEC>
hipError_t launch_windows(const KernelTables &t, const void *d_in, uint32_t *d_scratch, const uint32_t *st_in, uint32_t *st_out,
                          const Args &a, int max_wgs, int device, hipStream_t s)
{
    const auto k = channel_stereo_windows_kernel<S16, VEC>;
    unsigned grid = 0;
    const hipError_t e = grid_of(t, reinterpret_cast<const void *>(k), (long long)a.nch * a.nruns, max_wgs, device, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(WV), 0, s, d_in, d_scratch, st_in, st_out, a);
    return hipGetLastError();
}

template <bool IN16, bool OUT16, bool VEC>
hipError_t launch_outputs(const KernelTables &t, const void *d_in, void *d_left, void *d_right, const uint4 *d_win, const float *d_thr,
                          const Args &a, int max_wgs, int device, hipStream_t s)
{
    const auto k = channel_stereo_outputs_kernel<IN16, OUT16, VEC>;
    unsigned grid = 0;
    const hipError_t e = grid_of(t, reinterpret_cast<const void *>(k), (long long)a.nch * a.oruns, max_wgs, device, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(WV), 0, s, d_in, d_left, d_right, d_win, d_thr, a);
    return hipGetLastError();
}

template <bool IN16, bool OUT16>
hipError_t launch_outputs_v(bool vec, const KernelTables &t, const void *d_in, void *d_left, void *d_right, const uint4 *d_win,
                            const float *d_thr, const Args &a, int max_wgs, int device, hipStream_t s)
{
    return vec ? launch_outputs<IN16, OUT16, true>(t, d_in, d_left, d_right, d_win, d_thr, a, max_wgs, device, s)
               : launch_outputs<IN16, OUT16, false>(t, d_in, d_left, d_right, d_win, d_thr, a, max_wgs, device, s);
}

}  // namespace

hipError_t launch_channel_stereo(const KernelTables &t, const void *d_in, int in_s16, int nch, size_t nsamp, size_t in_stride,
                                 uint64_t pos, uint32_t word, const uint32_t *d_modes, const float *d_thr, int window, int attack,
                                 int hang, const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_scratch, void *d_left,
                                 void *d_right, int out_s16, size_t out_stride, uint32_t *d_stereo, uint32_t *d_count,
                                 float *d_level, float *d_phase, int accumulate, int max_wgs, int device, hipStream_t s)
{
    if (!d_in || !d_modes || !d_thr || !d_state_in || !d_state_out || !d_scratch || !d_left || !d_right || nch < 1 || nsamp == 0 ||
        nsamp > kStereoMaxLaunch || word == 0 || window < 1 || window > kStereoMaxWindow || attack < 1 || attack > kStereoMaxAttack ||
        hang < 0 || hang > kStereoMaxHang)
        return hipErrorInvalidValue;
    Args a;
    a.hs = (int)(pos % (uint64_t)B);
    a.end = a.hs + (int)nsamp;
    a.W = window;
    a.kw0 = (int)((pos / (uint64_t)B) % (uint64_t)window);
    a.nblk = (a.end + B - 1) / B;
    a.nfull = a.end / B;
    a.nwin = (a.kw0 + a.nblk + window - 1) / window;
    a.nch = nch;
    a.nruns = (a.nblk + kRunBlocks - 1) / kRunBlocks;
    a.oruns = (a.nblk + WR - 1) / WR;
    a.attack = attack;
    a.hang = hang;
    a.accumulate = accumulate ? 1 : 0;
    a.pos256 = (uint32_t)(pos - (uint64_t)a.hs);
    a.w = word;
    a.w2 = word * 2u;
    a.in_stride = nch > 1 ? (long long)in_stride : 0;
    a.out_stride = nch > 1 ? (long long)out_stride : 0;

    // four consecutive samples per lane where every quad of a block is aligned to its load
    const uintptr_t is = in_s16 ? 2 : 4, os = out_s16 ? 2 : 4;
    const bool ivec = (((uintptr_t)d_in - (uintptr_t)a.hs * is) % (4 * is)) == 0 && a.in_stride % 4 == 0;
    hipError_t e;
    if (in_s16)
        e = ivec ? launch_windows<true, true>(t, d_in, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s)
                 : launch_windows<true, false>(t, d_in, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s);
    else
        e = ivec ? launch_windows<false, true>(t, d_in, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s)
                 : launch_windows<false, false>(t, d_in, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s);
    if (e != hipSuccess) return e;

    unsigned grid = 0;
    const auto gates = channel_stereo_gates_kernel;
    if ((e = grid_of(t, reinterpret_cast<const void *>(gates), (nch + WV - 1) / WV, max_wgs, device, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(gates, dim3(grid), dim3(WV), 0, s, d_scratch, d_modes, d_thr, d_state_in, d_state_out, d_stereo, d_count, d_level,
                       d_phase, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    const uint4 *d_win = reinterpret_cast<const uint4 *>(d_scratch) + (size_t)nch * a.nblk;
    const bool vec = ivec && (((uintptr_t)d_left - (uintptr_t)a.hs * os) % (4 * os)) == 0 &&
                     (((uintptr_t)d_right - (uintptr_t)a.hs * os) % (4 * os)) == 0 && a.out_stride % 4 == 0;
    if (in_s16)
        return out_s16 ? launch_outputs_v<true, true>(vec, t, d_in, d_left, d_right, d_win, d_thr, a, max_wgs, device, s)
                       : launch_outputs_v<true, false>(vec, t, d_in, d_left, d_right, d_win, d_thr, a, max_wgs, device, s);
    return out_s16 ? launch_outputs_v<false, true>(vec, t, d_in, d_left, d_right, d_win, d_thr, a, max_wgs, device, s)
                   : launch_outputs_v<false, false>(vec, t, d_in, d_left, d_right, d_win, d_thr, a, max_wgs, device, s);
}

}  // namespace sddc
