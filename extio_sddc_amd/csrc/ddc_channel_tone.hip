// ddc_channel_tone.hip — the channel tone detector for gfx950 (sddc_ddc_channel_tone_device): a bank of
// single-bin DFTs per channel over a real sense stream (F32 or S16) and a gate on the channel's audio (F32
// or S16 in and out, optional), streaming (each channel's gate, last results, unfinished window and
// unfinished block live in the handle), in the block and window form that tone_math.h defines.
//
// A launch covers the stream windows (W blocks of B = 256 samples, anchored to the stream position) that
// hold one of its samples; u is a sample's index counted from the start of the first of them, so the
// launch's samples are hs <= u < end, in nwin windows of which the first nwc are complete at its end.
// Three launches on the caller's stream, all reading the handle's state as it was before the call:
//   windows  channel_tone_windows_kernel: a wave owns a run of whole windows of one channel.  Lane l holds
//            samples 4 l .. 4 l + 3 of a block, one 16-byte load (8 bytes of S16) where the base, the stride
//            and the position allow, else four loads.  kRun blocks are loaded into registers at a time;
//            the mask's tones are then taken in chunks of kChunk (8 and 8; 4 and 4 where no mask has more
//            than four tones): the lane's four phasors per tone (they depend on the tone and the lane
//            alone: computed once per wave when the mask fits one chunk, else once per chunk and kRun
//            blocks), 8 multiplies and two 6-step xor-shuffle trees per tone and block, then the block
//            rotation and the fold, which are wave-uniform: lane t keeps tone t's Zr and Zi, so 64 tones
//            cost two registers.  The stream is read once whatever the mask.
//            At a window's end the wave scans the mask's tones for the best one and writes four words to
//            the scratch: P_best, E, the tone, the bad flag.  The wave that owns the launch's first window
//            starts from the state's sums and stored block; the one that owns the last writes the next
//            state's; the one that owns the last complete window writes every P_t (state and d_powers).
//   gates    channel_tone_gates_kernel: a wave per channel walks the channel's windows in stream order, 64
//            per step: a lane per window for the comparisons, two ballots, then squelch_step on the
//            ballots in scalar registers, with the closed-form steps of the squelch's gates kernel.  It
//            replaces a window's first scratch word by its gate (1 pass, 0 zero) and writes the rest of
//            the next state, d_tone, d_open, d_count and d_level.
//   outputs  channel_tone_outputs_kernel (only with audio): the squelch's outputs kernel at window
//            granularity; a closed window is written as +0 without a read.
// The host swaps the two state buffers per launch set, so no wave reads what another one writes.  Nothing
// outside the streams is read or written.
//
// Determinism: every value is tone_math.h's fixed sequence of operations; the grid, the run length, the
// chunking, the stream and the other channels decide only which wave does it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ddc_kernels.h"

#pragma clang fp contract(off)
#include "tone_math.h"

namespace sddc {
namespace {

using namespace tone;

constexpr int B = kToneBlock;
constexpr int WV = 64;       // threads per workgroup: one wave
// The windows kernel's shape, chosen by measurement: kRun blocks held in registers at a
// time and kChunk tones whose phasors are held in registers at a time.  Masks of at most kSmallChunk tones on
// every channel take the small shape (fewer registers, more waves in flight: the stream's read is what
// bounds them), the others the large one.
constexpr int kRunLarge = 8, kChunkLarge = 8, kRunSmall = 4, kSmallChunk = 4;
constexpr int WR = 8;            // blocks per wave of the outputs kernel
constexpr int kRunBlocks = 32;   // a wave of the windows kernel owns whole windows of about this many blocks
// a channel's state, in 32-bit words
constexpr int R_OFF = 0, N_OFF = 1, OPEN_OFF = 2, TONE_OFF = 3 /* tone + 1 */, PBEST_OFF = 4, ELAST_OFF = 5;
constexpr int E_OFF = 6, BAD_OFF = 7, ZR_OFF = 8, ZI_OFF = ZR_OFF + kToneMaxTones, POW_OFF = ZI_OFF + kToneMaxTones;
constexpr int X_OFF = POW_OFF + kToneMaxTones;   // the unfinished block's samples
static_assert(X_OFF + B == kToneStateWords, "state layout");
static_assert(kToneMaxTones == WV, "lane t keeps tone t's sums");

struct Args {
    int hs, end;          // the launch's samples are hs <= u < end
    int W;                // blocks per window
    int nwin, nwc;        // windows that hold samples of the launch; windows complete at its end
    int nch, nruns, wrun; // nruns: runs of wrun windows per channel (windows kernel)
    int oruns;            // runs of WR blocks per channel (outputs kernel)
    int attack, hang, ntones;
    int accumulate;       // d_count holds the earlier launches of the same call
    uint32_t pos256;      // the stream position of u = 0, modulo 2^32 (a multiple of 256)
    long long sense_stride, in_stride, out_stride;   // samples per channel
};

template <bool S16> struct SenseT { using T = std::conditional_t<S16, short, float>; };

template <bool S16> __device__ __forceinline__ void load_quad(const typename SenseT<S16>::T *__restrict__ p, float (&d)[4])
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

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// scratch: [nch][nwin][4].  state: [nch][kToneStateWords].  VEC: every quad 4 l .. 4 l + 3 of a block is aligned
// to its load.
template <bool S16, bool VEC, int kRun, int kChunk>
__global__ __launch_bounds__(WV) void channel_tone_windows_kernel(const void *__restrict__ sense_, const uint32_t *__restrict__ tones,
                                                                  const uint64_t *__restrict__ masks, uint32_t *__restrict__ scratch,
                                                                  const uint32_t *__restrict__ state_in,
                                                                  uint32_t *__restrict__ state_out, float *__restrict__ d_powers,
                                                                  const Args a)
{
    using T = typename SenseT<S16>::T;
    const int lane = (int)threadIdx.x;
    const long long nitems = (long long)a.nch * a.nruns;
    const int nblocks = (a.end + B - 1) / B, nfull = a.end / B;   // blocks that hold a sample; complete ones
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.nruns), r = (int)(item - (long long)c * a.nruns);
        const int ja = r * a.wrun, jb = ja + a.wrun < a.nwin ? ja + a.wrun : a.nwin;
        // sample u of the launch's windows is in[u]; only hs <= u < end is touched
        const T *__restrict__ in = static_cast<const T *>(sense_) + c * a.sense_stride - a.hs;
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kToneStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kToneStateWords;
        const uint64_t mw = masks[c];
        const uint64_t mask = ((uint64_t)uni((uint32_t)(mw >> 32)) << 32) | uni((uint32_t)mw);
        const bool one_chunk = __builtin_popcountll(mask) <= kChunk;
        // block kk's samples of this lane, non-finite ones as 0; returns whether one of them was non-finite
        auto load_block = [&](int kk, float (&x)[4]) -> bool {
            const int u0 = kk * B + 4 * lane;
            if (VEC && u0 >= a.hs && u0 + 4 <= a.end) {
                load_quad<S16>(in + u0, x);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int u = u0 + j;
                    x[j] = 0.f;
                    if (u >= a.hs && u < a.end) x[j] = (float)in[u];
                    else if (u < a.hs && u >= a.hs / B * B) x[j] = __uint_as_float(st_in[X_OFF + u - a.hs / B * B]);
                }
            }
            bool bad = false;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool fin = blank::blank_finite(x[j] * x[j]);
                x[j] = fin ? x[j] : 0.f;
                bad = bad || !fin;
            }
            return bad;
        };
        float pc[kChunk][4], ps[kChunk][4];
        int tix[kChunk];
        bool have = false;   // pc, ps and tix hold the mask's only chunk
        for (int j = ja; j < jb; j++) {
            float zr = 0.f, zi = 0.f, E = 0.f;
            bool bad = false;
            int kfirst = j * a.W;
            if (j == 0) {   // the window the stream was in: its sums so far, and where its new samples begin
                kfirst = a.hs / B;
                zr = __uint_as_float(st_in[ZR_OFF + lane]);
                zi = __uint_as_float(st_in[ZI_OFF + lane]);
                E = __uint_as_float(uni(st_in[E_OFF]));
                bad = uni(st_in[BAD_OFF]) != 0;
            }
            const int kend = (j + 1) * a.W < nfull ? (j + 1) * a.W : nfull;   // the window's complete blocks end here
            for (int ks = kfirst; ks < kend; ks += kRun) {
                const int nb = kend - ks < kRun ? kend - ks : kRun;
                float x[kRun][4];
#pragma unroll
                for (int b = 0; b < kRun; b++) {
                    if (b < nb) {
                        bad = load_block(ks + b, x[b]) || bad;
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; q++) x[b][q] = 0.f;
                    }
                }
#pragma unroll
                for (int b = 0; b < kRun; b++) {
                    if (b < nb) {
                        const float q0 = x[b][0] * x[b][0], q1 = x[b][1] * x[b][1], q2 = x[b][2] * x[b][2], q3 = x[b][3] * x[b][3];
                        E = E + wave_tree((q0 + q1) + (q2 + q3));
                    }
                }
                uint64_t mrem = mask;
                while (mrem) {
                    if (!have) {
#pragma unroll
                        for (int t = 0; t < kChunk; t++) {
                            tix[t] = -1;
                            if (mrem) {
                                tix[t] = __builtin_ctzll(mrem);
                                mrem &= mrem - 1;
                                const uint32_t w = tones[tix[t]];
#pragma unroll
                                for (int q = 0; q < 4; q++) tone_phasor(w, (uint32_t)(4 * lane + q), &pc[t][q], &ps[t][q]);
                            }
                        }
                        have = one_chunk;
                    } else {
                        mrem = 0;
                    }
#pragma unroll
                    for (int b = 0; b < kRun; b++) {
                        if (b < nb) {
                            const uint32_t p256 = a.pos256 + (uint32_t)(ks + b) * (uint32_t)B;
#pragma unroll
                            for (int t = 0; t < kChunk; t++) {
                                if (tix[t] >= 0) {
                                    const float a0 = x[b][0] * pc[t][0], a1 = x[b][1] * pc[t][1], a2 = x[b][2] * pc[t][2],
                                                a3 = x[b][3] * pc[t][3];
                                    const float b0 = x[b][0] * ps[t][0], b1 = x[b][1] * ps[t][1], b2 = x[b][2] * ps[t][2],
                                                b3 = x[b][3] * ps[t][3];
                                    const float Ck = wave_tree((a0 + a1) + (a2 + a3)), Sk = wave_tree((b0 + b1) + (b2 + b3));
                                    float cr, sr, re, im;
                                    tone_phasor(tones[tix[t]], p256, &cr, &sr);   // wave-uniform
                                    tone_rotate(Ck, Sk, cr, sr, &re, &im);
                                    const bool mine = lane == tix[t];
                                    zr = mine ? zr + re : zr;
                                    zi = mine ? zi + im : zi;
                                }
                            }
                        }
                    }
                }
            }
            unsigned long long anybad = __ballot(bad);
            if (j == a.nwin - 1 && nblocks > nfull) {   // the stream ends inside a block: its samples are the next call's
                float xp[4];
                anybad |= __ballot(load_block(nfull, xp));
#pragma unroll
                for (int q = 0; q < 4; q++) st_out[X_OFF + 4 * lane + q] = __float_as_uint(xp[q]);
            }
            const bool complete = j < a.nwc;
            if (complete) {
                const float P = (mask >> lane) & 1 ? blank::blank_power(zr, zi) : 0.f;
                int best = -1;
                float Pbest = 0.f;
                for (uint64_t mm = mask; mm; mm &= mm - 1) {
                    const int t = __builtin_ctzll(mm);
                    tone_best(t, __shfl(P, t), &best, &Pbest);
                }
                if (lane == 0) {
                    uint4 wd;
                    wd.x = __float_as_uint(Pbest), wd.y = __float_as_uint(E), wd.z = (uint32_t)(best + 1), wd.w = anybad ? 1u : 0u;
                    *reinterpret_cast<uint4 *>(scratch + ((size_t)c * a.nwin + j) * 4) = wd;
                }
                if (j == a.nwc - 1) {
                    st_out[POW_OFF + lane] = __float_as_uint(P);
                    if (d_powers && lane < a.ntones) d_powers[(size_t)c * a.ntones + lane] = P;
                }
            } else if (a.nwc == 0) {   // no window completes in this launch: the last results stay
                const uint32_t P = st_in[POW_OFF + lane];
                st_out[POW_OFF + lane] = P;
                if (d_powers && lane < a.ntones) d_powers[(size_t)c * a.ntones + lane] = __uint_as_float(P);
            }
            if (j == a.nwin - 1) {
                st_out[ZR_OFF + lane] = complete ? 0u : __float_as_uint(zr);
                st_out[ZI_OFF + lane] = complete ? 0u : __float_as_uint(zi);
                if (lane == 0) {
                    st_out[E_OFF] = complete ? 0u : __float_as_uint(E);
                    st_out[BAD_OFF] = !complete && anybad ? 1u : 0u;
                }
            }
        }
    }
}

// masks: [nch]; thr: [nch][3] (To, Tc, Emin).  d_tone, d_open, d_count: null or [nch]; d_level: null or [nch][2].
__global__ __launch_bounds__(WV) void channel_tone_gates_kernel(uint32_t *__restrict__ scratch, const uint64_t *__restrict__ masks,
                                                                const float *__restrict__ thr, const uint32_t *__restrict__ state_in,
                                                                uint32_t *__restrict__ state_out, int *__restrict__ d_tone,
                                                                uint32_t *__restrict__ d_open, uint32_t *__restrict__ d_count,
                                                                float *__restrict__ d_level, const Args a)
{
    const int lane = (int)threadIdx.x;
    const uint32_t A = (uint32_t)a.attack, H = (uint32_t)a.hang;
    const int WB = a.W * B;   // samples per window
    for (int c = (int)blockIdx.x; c < a.nch; c += (int)gridDim.x) {
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kToneStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kToneStateWords;
        uint4 *__restrict__ w = reinterpret_cast<uint4 *>(scratch) + (size_t)c * a.nwin;
        const bool gated = masks[c] != 0;
        const float To = thr[3 * c], Tc = thr[3 * c + 1], Emin = thr[3 * c + 2];
        uint32_t r = uni(st_in[R_OFF]), n = uni(st_in[N_OFF]), open = uni(st_in[OPEN_OFF]);
        uint32_t tone1 = uni(st_in[TONE_OFF]), pbest = uni(st_in[PBEST_OFF]), elast = uni(st_in[ELAST_OFF]);
        uint32_t cnt = 0;
        for (int k0 = 0; k0 < a.nwin; k0 += WV) {
            const int k = k0 + lane;
            const int m = a.nwin - k0 < WV ? a.nwin - k0 : WV;                    // windows of this step
            const int mc = a.nwc - k0 < 0 ? 0 : (a.nwc - k0 < WV ? a.nwc - k0 : WV);   // the complete ones among them
            const unsigned long long mm = ~0ull >> (WV - m), cm = mc ? ~0ull >> (WV - mc) : 0ull;
            uint4 wd = make_uint4(0u, 0u, 0u, 0u);
            if (k < a.nwc) wd = w[k];
            bool u, v;
            tone_flags(__uint_as_float(wd.x), __uint_as_float(wd.y), wd.w != 0, To, Tc, Emin, &u, &v);
            const unsigned long long U = __ballot(u) & cm, V = __ballot(v) & cm;
            unsigned long long G = 0;
            if (!gated) {
                G = ~0ull;
            } else if (!open && U == 0) {
                // stays closed: r = 0, n counts the windows since the last v-window
                if (mc) {
                    const uint32_t since = V ? (uint32_t)(mc - 1 - (63 - __builtin_clzll(V))) : n + (uint32_t)mc;
                    n = since < H + 1 ? since : H + 1;
                    r = 0;
                }
            } else if (open && V == cm) {
                // stays open: n = 0, r counts the u-windows since the last window that is none
                G = mm;
                if (mc) {
                    const unsigned long long Z = ~U & cm;
                    const uint32_t run = Z ? (uint32_t)(mc - 1 - (63 - __builtin_clzll(Z))) : r + (uint32_t)mc;
                    r = run < A ? run : A;
                    n = 0;
                }
            } else {
                for (int j = 0; j < m; j++) {
                    G |= (unsigned long long)open << j;
                    if (j < mc) squelch::squelch_step((U >> j) & 1, (V >> j) & 1, A, H, &r, &n, &open);
                }
            }
            if (mc > 0) {   // the last complete window so far
                const bool vl = (V >> (mc - 1)) & 1;
                tone1 = vl ? uni((uint32_t)__shfl((int)wd.z, mc - 1)) : 0u;
                pbest = uni((uint32_t)__shfl((int)wd.x, mc - 1));
                elast = uni((uint32_t)__shfl((int)wd.y, mc - 1));
            }
            const uint32_t g = (uint32_t)(G >> lane) & 1u;
            if (k < a.nwin) {
                scratch[((size_t)c * a.nwin + k) * 4] = g;
                const int lo = k * WB > a.hs ? k * WB : a.hs, hi = (k + 1) * WB < a.end ? (k + 1) * WB : a.end;
                cnt += g ? (uint32_t)(hi - lo) : 0u;
            }
        }
#pragma unroll
        for (int m = 1; m < WV; m <<= 1) cnt += __shfl_xor(cnt, m);
        if (lane == 0) {
            st_out[R_OFF] = r;
            st_out[N_OFF] = n;
            st_out[OPEN_OFF] = open;
            st_out[TONE_OFF] = tone1;
            st_out[PBEST_OFF] = pbest;
            st_out[ELAST_OFF] = elast;
            if (d_tone) d_tone[c] = (int)tone1 - 1;
            if (d_open) d_open[c] = gated ? open : 1u;
            if (d_count) d_count[c] = (a.accumulate ? d_count[c] : 0u) + cnt;
            if (d_level) d_level[2 * c] = __uint_as_float(pbest), d_level[2 * c + 1] = __uint_as_float(elast);
        }
    }
}

template <bool IN16> struct InQ;    // four consecutive samples
template <> struct InQ<false> { using T = uint4; };
template <> struct InQ<true> { using T = uint2; };

// a passed sample from the stored input word (F32 bits, or a sign-extended code)
template <bool IN16, bool OUT16> __device__ __forceinline__ uint32_t pass_sample(uint32_t raw)
{
    if constexpr (OUT16) return (uint32_t)(uint16_t)demod::demod_s16(IN16 ? (float)(int)raw : __uint_as_float(raw));
    else if constexpr (!IN16) return raw;   // a NaN keeps its payload
    else return __float_as_uint((float)(int)raw);
}

template <bool IN16, bool OUT16, bool VEC>
__global__ __launch_bounds__(WV) void channel_tone_outputs_kernel(const void *__restrict__ in_, void *__restrict__ out_,
                                                                  const uint32_t *__restrict__ scratch, const Args a)
{
    using I = std::conditional_t<IN16, short, uint32_t>;
    using O = std::conditional_t<OUT16, unsigned short, uint32_t>;
    using IQ = typename InQ<IN16>::T;
    using OQ = typename InQ<OUT16>::T;
    const int lane = (int)threadIdx.x;
    const long long nitems = (long long)a.nch * a.oruns;
    const int kb0 = a.hs / B, nblocks = (a.end + B - 1) / B;   // the blocks that hold a sample are kb0 <= kk < nblocks
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.oruns), r = (int)(item - (long long)c * a.oruns);
        const int ka = kb0 + r * WR, kb = ka + WR < nblocks ? ka + WR : nblocks;
        // sample u of the launch's windows is in[u] / out[u]; only hs <= u < end is touched
        const I *__restrict__ in = static_cast<const I *>(in_) + c * a.in_stride - a.hs;
        O *__restrict__ out = static_cast<O *>(out_) + c * a.out_stride - a.hs;
        for (int kk = ka; kk < kb; kk++) {
            const bool pass = scratch[((size_t)c * a.nwin + kk / a.W) * 4] != 0;
            if constexpr (VEC) {
                const int u0 = kk * B + 4 * lane;
                if (u0 >= a.hs && u0 + 4 <= a.end) {
                    uint32_t y[4] = {0u, 0u, 0u, 0u};
                    if (pass) {
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
                        for (int q = 0; q < 4; q++) y[q] = pass_sample<IN16, OUT16>(x[q]);
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
                        if (u >= a.hs && u < a.end) out[u] = (O)(pass ? pass_sample<IN16, OUT16>((uint32_t)(int)in[u]) : 0u);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int u = kk * B + WV * j + lane;
                    if (u >= a.hs && u < a.end) out[u] = (O)(pass ? pass_sample<IN16, OUT16>((uint32_t)(int)in[u]) : 0u);
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

template <bool S16, bool VEC, int kRun, int kChunk>
hipError_t launch_windows_k(const KernelTables &t, const void *d_sense, const uint32_t *d_tones, const uint64_t *d_masks,
                            uint32_t *d_scratch, const uint32_t *st_in, uint32_t *st_out, float *d_powers, const Args &a, int max_wgs,
                            int device, hipStream_t s)
{
    const auto k = channel_tone_windows_kernel<S16, VEC, kRun, kChunk>;
    unsigned grid = 0;
    const hipError_t e = grid_of(t, reinterpret_cast<const void *>(k), (long long)a.nch * a.nruns, max_wgs, device, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(WV), 0, s, d_sense, d_tones, d_masks, d_scratch, st_in, st_out, d_powers, a);
    return hipGetLastError();
}

template <bool S16, bool VEC>
hipError_t launch_windows(bool small, const KernelTables &t, const void *d_sense, const uint32_t *d_tones, const uint64_t *d_masks,
                          uint32_t *d_scratch, const uint32_t *st_in, uint32_t *st_out, float *d_powers, const Args &a, int max_wgs,
                          int device, hipStream_t s)
{
    return small ? launch_windows_k<S16, VEC, kRunSmall, kSmallChunk>(t, d_sense, d_tones, d_masks, d_scratch, st_in, st_out, d_powers,
                                                                      a, max_wgs, device, s)
                 : launch_windows_k<S16, VEC, kRunLarge, kChunkLarge>(t, d_sense, d_tones, d_masks, d_scratch, st_in, st_out, d_powers,
                                                                      a, max_wgs, device, s);
}

template <bool IN16, bool OUT16, bool VEC>
hipError_t launch_outputs(const KernelTables &t, const void *d_in, void *d_out, const uint32_t *d_scratch, const Args &a,
                          int max_wgs, int device, hipStream_t s)
{
    const auto k = channel_tone_outputs_kernel<IN16, OUT16, VEC>;
    unsigned grid = 0;
    const hipError_t e = grid_of(t, reinterpret_cast<const void *>(k), (long long)a.nch * a.oruns, max_wgs, device, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(WV), 0, s, d_in, d_out, d_scratch, a);
    return hipGetLastError();
}

template <bool IN16, bool OUT16>
hipError_t launch_outputs_v(bool vec, const KernelTables &t, const void *d_in, void *d_out, const uint32_t *d_scratch,
                            const Args &a, int max_wgs, int device, hipStream_t s)
{
    return vec ? launch_outputs<IN16, OUT16, true>(t, d_in, d_out, d_scratch, a, max_wgs, device, s)
               : launch_outputs<IN16, OUT16, false>(t, d_in, d_out, d_scratch, a, max_wgs, device, s);
}

}  // namespace

hipError_t launch_channel_tone(const KernelTables &t, const void *d_sense, int sense_s16, size_t sense_stride, const void *d_audio,
                               int in_s16, int nch, size_t nsamp, size_t in_stride, uint64_t pos, const uint32_t *d_tones,
                               int ntones, const uint64_t *d_masks, int max_mask_tones, const float *d_thr, int window, int attack,
                               int hang, const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_scratch, void *d_out, int out_s16,
                               size_t out_stride, int *d_tone, uint32_t *d_open, uint32_t *d_count, float *d_level,
                               float *d_powers, int accumulate, int max_wgs, int device, hipStream_t s)
{
    if (!d_sense || !d_tones || !d_masks || !d_thr || !d_state_in || !d_state_out || !d_scratch || nch < 1 || nsamp == 0 ||
        nsamp > kToneMaxLaunch || ntones < 1 || ntones > kToneMaxTones || window < 1 || window > kToneMaxWindow || attack < 1 ||
        attack > kToneMaxAttack || hang < 0 || hang > kToneMaxHang || (d_audio && !d_out))
        return hipErrorInvalidValue;
    const uint64_t WB = (uint64_t)window * B;
    Args a;
    a.hs = (int)(pos % WB);
    a.end = a.hs + (int)nsamp;
    a.W = window;
    a.nwin = (int)(((uint64_t)a.end + WB - 1) / WB);
    a.nwc = (int)((uint64_t)a.end / WB);
    a.nch = nch;
    a.wrun = window >= kRunBlocks ? 1 : kRunBlocks / window;
    a.nruns = (a.nwin + a.wrun - 1) / a.wrun;
    a.oruns = ((a.end + B - 1) / B - a.hs / B + WR - 1) / WR;
    a.attack = attack;
    a.hang = hang;
    a.ntones = ntones;
    a.accumulate = accumulate ? 1 : 0;
    a.pos256 = (uint32_t)(pos - (uint64_t)a.hs);
    a.sense_stride = nch > 1 ? (long long)sense_stride : 0;
    a.in_stride = nch > 1 ? (long long)in_stride : 0;
    a.out_stride = nch > 1 ? (long long)out_stride : 0;

    // four consecutive samples per lane where every quad of a block is aligned to its load
    const uintptr_t ss = sense_s16 ? 2 : 4;
    const bool svec = (((uintptr_t)d_sense - (uintptr_t)(a.hs % B) * ss) % (4 * ss)) == 0 && a.sense_stride % 4 == 0;
    const bool small = max_mask_tones <= kSmallChunk;
    hipError_t e;
    if (sense_s16)
        e = svec ? launch_windows<true, true>(small, t, d_sense, d_tones, d_masks, d_scratch, d_state_in, d_state_out, d_powers, a, max_wgs, device, s)
                 : launch_windows<true, false>(small, t, d_sense, d_tones, d_masks, d_scratch, d_state_in, d_state_out, d_powers, a, max_wgs, device, s);
    else
        e = svec ? launch_windows<false, true>(small, t, d_sense, d_tones, d_masks, d_scratch, d_state_in, d_state_out, d_powers, a, max_wgs, device, s)
                 : launch_windows<false, false>(small, t, d_sense, d_tones, d_masks, d_scratch, d_state_in, d_state_out, d_powers, a, max_wgs, device, s);
    if (e != hipSuccess) return e;

    unsigned grid = 0;
    const auto gates = channel_tone_gates_kernel;
    if ((e = grid_of(t, reinterpret_cast<const void *>(gates), nch, max_wgs, device, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(gates, dim3(grid), dim3(WV), 0, s, d_scratch, d_masks, d_thr, d_state_in, d_state_out, d_tone, d_open, d_count,
                       d_level, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!d_audio) return hipSuccess;

    const uintptr_t is = in_s16 ? 2 : 4, os = out_s16 ? 2 : 4;
    const bool vec = (((uintptr_t)d_audio - (uintptr_t)(a.hs % B) * is) % (4 * is)) == 0 &&
                     (((uintptr_t)d_out - (uintptr_t)(a.hs % B) * os) % (4 * os)) == 0 && a.in_stride % 4 == 0 && a.out_stride % 4 == 0;
    if (in_s16)
        return out_s16 ? launch_outputs_v<true, true>(vec, t, d_audio, d_out, d_scratch, a, max_wgs, device, s)
                       : launch_outputs_v<true, false>(vec, t, d_audio, d_out, d_scratch, a, max_wgs, device, s);
    return out_s16 ? launch_outputs_v<false, true>(vec, t, d_audio, d_out, d_scratch, a, max_wgs, device, s)
                   : launch_outputs_v<false, false>(vec, t, d_audio, d_out, d_scratch, a, max_wgs, device, s);
}

}  // namespace sddc
