// ddc_channel_dcs.hip — the channel DCS decoder for gfx950 (sddc_ddc_channel_dcs_device): the signs of a
// real sense stream (F32 or S16) sorted into eighth-of-a-bit sub-bins per window, the 8 x 23 bit sums, the
// best timing phase, the match of its word against a table of codewords over all rotations, and a gate on
// the channel's audio (F32 or S16 in and out, optional), streaming (each channel's gate, last results and
// unfinished window's sub-bin sums live in the handle), in the window form that dcs_math.h defines.
//
// A launch covers the stream windows (W blocks of B = 256 samples, anchored to the stream position) that
// hold one of its samples; u is a sample's index counted from the start of the first of them, so the
// launch's samples are hs <= u < end, in nwin windows of which the first nwc are complete at its end.
// Three launches on the caller's stream, all reading the handle's state as it was before the call, as in
// ddc_channel_tone.hip:
//   windows  channel_dcs_windows_kernel: a wave owns a run of whole windows of one channel and keeps the
//            window's 192 sub-bin sums in LDS.  Lane l holds samples 4 l .. 4 l + 3 of a block, one 16-byte
//            load (8 bytes of S16) where the base, the stride and the position allow, else four loads; kRun
//            blocks are loaded at a time.  The lane folds the signs of its consecutive samples that share a
//            sub-bin in a register and adds each such sum to the LDS with one integer atomic: integer sums
//            are order-free, so the result does not depend on which lane or wave adds first.  At a window's
//            end lanes 0..22 form the bit sums by sliding over the sub-bins, six xor-shuffle steps give the 8
//            Q, a ballot the word, lanes i and i + 64 take the candidates i and i + 64 of the table, and a
//            wave minimum of the (d, i) key names the best.  Four words go to the scratch: the flags u and
//            v, Q, the packed (code + 1, d, t), and 0.  The wave that owns the launch's first window starts
//            from the state's sums; the one that owns the last writes the next state's.
//   gates    channel_dcs_gates_kernel: the tone detector's gates kernel on those records: a wave per
//            channel, 64 windows per step, squelch_step on ballots with the closed-form steps.  It replaces
//            a window's first scratch word by its gate and writes the rest of the next state, d_code,
//            d_open, d_count and d_info.
//   outputs  channel_dcs_outputs_kernel (only with audio): the tone detector's outputs kernel; a closed
//            window is written as +0 without a read.
// The host swaps the two state buffers per launch set, so no wave reads what another one writes.  Nothing
// outside the streams is read or written.
//
// Determinism: every value is an integer function of the signs; the grid, the run length, the stream and the
// other channels decide only which wave computes it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ddc_kernels.h"

#pragma clang fp contract(off)
#include "dcs_math.h"
#include "demod_math.h"

namespace sddc {
namespace {

using namespace dcs;

constexpr int B = kDcsBlock;
constexpr int WV = 64;           // threads per workgroup: one wave
constexpr int kRun = 4;          // blocks loaded into registers at a time (windows kernel)
constexpr int WR = 8;            // blocks per wave of the outputs kernel
constexpr int kRunBlocks = 32;   // a wave of the windows kernel owns whole windows of about this many blocks
// a channel's state, in 32-bit words
constexpr int R_OFF = 0, N_OFF = 1, OPEN_OFF = 2, CODE_OFF = 3 /* code + 1 */, Q_OFF = 4, NT_OFF = 5, D_OFF = 6, T_OFF = 7;
constexpr int S_OFF = 8;         // the unfinished window's sub-bin sums
static_assert(S_OFF + kDcsSubBins == kDcsStateWords, "state layout");
static_assert(kDcsMaxCodes == 2 * WV, "lanes i and i + 64 take the candidates");

struct Args {
    int hs, end;          // the launch's samples are hs <= u < end
    int W;                // blocks per window
    int nwin, nwc;        // windows that hold samples of the launch; windows complete at its end
    int nch, nruns, wrun; // nruns: runs of wrun windows per channel (windows kernel)
    int oruns;            // runs of WR blocks per channel (outputs kernel)
    int attack, hang, ncodes;
    int accumulate;       // d_count holds the earlier launches of the same call
    uint32_t word;        // the bit phase word
    uint32_t e_open, e_close;
    uint32_t N[kDcsPhases];
    long long sense_stride, in_stride, out_stride;   // samples per channel
};

template <bool S16> struct SenseT { using T = std::conditional_t<S16, short, float>; };

// four consecutive samples as their signs
template <bool S16> __device__ __forceinline__ void load_quad(const typename SenseT<S16>::T *__restrict__ p, int (&s)[4])
{
    if constexpr (!S16) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        s[0] = dcs_sign(v.x), s[1] = dcs_sign(v.y), s[2] = dcs_sign(v.z), s[3] = dcs_sign(v.w);
    } else {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        s[0] = dcs_sign_s16((int)(short)(v.x & 0xffffu)), s[1] = dcs_sign_s16((int)v.x >> 16);
        s[2] = dcs_sign_s16((int)(short)(v.y & 0xffffu)), s[3] = dcs_sign_s16((int)v.y >> 16);
    }
}

template <bool S16> __device__ __forceinline__ int load_one(const typename SenseT<S16>::T *__restrict__ p)
{
    if constexpr (!S16) return dcs_sign(*p);
    else return dcs_sign_s16((int)*p);
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < WV; m <<= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < WV; m <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
        v = o < v ? o : v;
    }
    return v;
}

// scratch: [nch][nwin][4].  state: [nch][kDcsStateWords].  params: [nch][3] = (code, invert, eye).  VEC: every
// quad 4 l .. 4 l + 3 of a block is aligned to its load.  BALLOT: the sub-bin sums by ballots and popcounts instead
// of LDS atomics (the other order-free route; slower as measured, kept selectable: DESIGN.md §4.20).
template <bool S16, bool VEC, bool BALLOT>
__global__ __launch_bounds__(WV) void channel_dcs_windows_kernel(const void *__restrict__ sense_, const uint32_t *__restrict__ cws,
                                                                 const int *__restrict__ params, uint32_t *__restrict__ scratch,
                                                                 const uint32_t *__restrict__ state_in,
                                                                 uint32_t *__restrict__ state_out, const Args a)
{
    using T = typename SenseT<S16>::T;
    __shared__ int S[kDcsSubBins + kDcsPhases];   // the tail stays 0: lanes past the 23 bits read it
    const int lane = (int)threadIdx.x;
    const long long nitems = (long long)a.nch * a.nruns;
    const int WB = a.W * B;
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.nruns), r = (int)(item - (long long)c * a.nruns);
        const int ja = r * a.wrun, jb = ja + a.wrun < a.nwin ? ja + a.wrun : a.nwin;
        // sample u of the launch's windows is in[u]; only hs <= u < end is touched
        const T *__restrict__ in = static_cast<const T *>(sense_) + c * a.sense_stride - a.hs;
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kDcsStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kDcsStateWords;
        const int code = (int)uni((uint32_t)params[3 * c]), invert = (int)uni((uint32_t)params[3 * c + 1]);
        const uint32_t eye = uni((uint32_t)params[3 * c + 2]);
        for (int j = ja; j < jb; j++) {
            __syncthreads();   // the window before is read out
            // the window the stream was in starts from its sums so far
            for (int m = lane; m < kDcsSubBins + kDcsPhases; m += WV) S[m] = j == 0 && m < kDcsSubBins ? (int)st_in[S_OFF + m] : 0;
            __syncthreads();
            const int u_lo = j * WB > a.hs ? j * WB : a.hs, u_hi = (j + 1) * WB < a.end ? (j + 1) * WB : a.end;
            const int kfirst = u_lo / B, kend = (u_hi + B - 1) / B;   // the blocks that hold one of its samples
            for (int ks = kfirst; ks < kend; ks += kRun) {
                int s[kRun][4];
#pragma unroll
                for (int b = 0; b < kRun; b++) {
                    const int u0 = (ks + b) * B + 4 * lane;
                    if (VEC && u0 >= u_lo && u0 + 4 <= u_hi) {
                        load_quad<S16>(in + u0, s[b]);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int u = u0 + q;
                            s[b][q] = 0;
                            if (u >= u_lo && u < u_hi) s[b][q] = load_one<S16>(in + u);
                        }
                    }
                }
#pragma unroll
                for (int b = 0; b < kRun; b++) {
                    if constexpr (BALLOT) {
                        // wave-uniform: the block's sub-bins one after the other; a ballot of the lanes whose
                        // sample q lies in it masks the ballots of the positive and of the negative signs
                        const uint32_t nb0 = (uint32_t)((ks + b) * B - j * WB);
                        unsigned long long P[4], Ng[4];
                        uint32_t mq[4];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            P[q] = __ballot(s[b][q] > 0);
                            Ng[q] = __ballot(s[b][q] < 0);
                            mq[q] = dcs_subbin(a.word, nb0 + (uint32_t)(4 * lane + q));
                        }
                        if ((P[0] | P[1] | P[2] | P[3] | Ng[0] | Ng[1] | Ng[2] | Ng[3]) == 0) continue;
                        const uint32_t m_lo = dcs_subbin(a.word, nb0), m_hi = dcs_subbin(a.word, nb0 + (uint32_t)(B - 1));
                        for (uint32_t m = m_lo; m <= m_hi && m < (uint32_t)kDcsSubBins; m++) {
                            int sum = 0;
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                const unsigned long long in_m = __ballot(mq[q] == m);
                                sum += __builtin_popcountll(P[q] & in_m) - __builtin_popcountll(Ng[q] & in_m);
                            }
                            if (lane == 0 && sum != 0) S[m] += sum;
                        }
                        continue;
                    }
                    // the lane's samples in sample order: consecutive ones of one sub-bin fold into one add
                    const uint32_t n0 = (uint32_t)((ks + b) * B + 4 * lane - j * WB);
                    uint64_t ph = (uint64_t)a.word * (uint64_t)n0;   // dcs_subbin(w, n0 + q) = (w n0 + q w) >> 29
                    uint32_t mcur = (uint32_t)(ph >> 29);
                    int acc = s[b][0];
#pragma unroll
                    for (int q = 1; q < 4; q++) {
                        ph += a.word;
                        const uint32_t m = (uint32_t)(ph >> 29);
                        if (m != mcur) {
                            if (acc != 0 && mcur < (uint32_t)kDcsSubBins) atomicAdd(&S[mcur], acc);
                            mcur = m;
                            acc = 0;
                        }
                        acc += s[b][q];
                    }
                    if (acc != 0 && mcur < (uint32_t)kDcsSubBins) atomicAdd(&S[mcur], acc);
                }
            }
            __syncthreads();
            const bool complete = j < a.nwc;
            if (complete) {
                // lane b < 23: c[t][b], t = 0..7, sliding over the sub-bins; the other lanes hold zeros
                const int bb = lane < kDcsBits ? lane : kDcsBits;   // 8 * 23 + 7 + 8 < the array's length
                int cs[kDcsPhases];
                cs[0] = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) cs[0] += S[8 * bb + i];
#pragma unroll
                for (int t = 1; t < kDcsPhases; t++) cs[t] = cs[t - 1] - S[8 * bb + t - 1] + S[8 * bb + t + 7];
                int tb = -1;
                uint32_t Qb = 0;
#pragma unroll
                for (int t = 0; t < kDcsPhases; t++) {
                    if (lane >= kDcsBits) cs[t] = 0;
                    dcs_best_phase(t, wave_sum(dcs_abs(cs[t])), &tb, &Qb);
                }
                int cb = cs[0];
#pragma unroll
                for (int t = 1; t < kDcsPhases; t++) cb = t == tb ? cs[t] : cb;
                uint32_t word = (uint32_t)__ballot(cb > 0) & kDcsWordMask;
                if (invert) word ^= kDcsWordMask;
                uint32_t key = kDcsNoKey;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int i = lane + h * WV;
                    if (i < a.ncodes && dcs_candidate(code, i, a.ncodes)) {
                        const uint32_t k = dcs_key(dcs_distance(word, cws[i]), i);
                        key = k < key ? k : key;
                    }
                }
                key = wave_min(key);
                const uint32_t d = key >> 8, best1 = key == kDcsNoKey ? 0u : (key & 0xffu) + 1u;
                bool fu, fv;
                dcs_flags(Qb, a.N[tb], d, eye, a.e_open, a.e_close, &fu, &fv);
                if (lane == 0) {
                    uint4 wd;
                    wd.x = (fu ? 1u : 0u) | (fv ? 2u : 0u), wd.y = Qb, wd.z = best1 | (d << 8) | ((uint32_t)tb << 16), wd.w = 0u;
                    *reinterpret_cast<uint4 *>(scratch + ((size_t)c * a.nwin + j) * 4) = wd;
                }
            }
            if (j == a.nwin - 1)
                for (int m = lane; m < kDcsSubBins; m += WV) st_out[S_OFF + m] = complete ? 0u : (uint32_t)S[m];
        }
    }
}

// params: [nch][3].  d_code, d_open, d_count: null or [nch]; d_info: null or [nch][4].
__global__ __launch_bounds__(WV) void channel_dcs_gates_kernel(uint32_t *__restrict__ scratch, const int *__restrict__ params,
                                                               const uint32_t *__restrict__ state_in, uint32_t *__restrict__ state_out,
                                                               int *__restrict__ d_code, uint32_t *__restrict__ d_open,
                                                               uint32_t *__restrict__ d_count, uint32_t *__restrict__ d_info, const Args a)
{
    const int lane = (int)threadIdx.x;
    const uint32_t A = (uint32_t)a.attack, H = (uint32_t)a.hang;
    const int WB = a.W * B;   // samples per window
    for (int c = (int)blockIdx.x; c < a.nch; c += (int)gridDim.x) {
        const uint32_t *__restrict__ st_in = state_in + (size_t)c * kDcsStateWords;
        uint32_t *__restrict__ st_out = state_out + (size_t)c * kDcsStateWords;
        uint4 *__restrict__ w = reinterpret_cast<uint4 *>(scratch) + (size_t)c * a.nwin;
        const bool gated = params[3 * c] != kDcsOff;
        uint32_t r = uni(st_in[R_OFF]), n = uni(st_in[N_OFF]), open = uni(st_in[OPEN_OFF]);
        uint32_t code1 = uni(st_in[CODE_OFF]), ql = uni(st_in[Q_OFF]), nl = uni(st_in[NT_OFF]), dl = uni(st_in[D_OFF]),
                 tl = uni(st_in[T_OFF]);
        uint32_t cnt = 0;
        for (int k0 = 0; k0 < a.nwin; k0 += WV) {
            const int k = k0 + lane;
            const int m = a.nwin - k0 < WV ? a.nwin - k0 : WV;                    // windows of this step
            const int mc = a.nwc - k0 < 0 ? 0 : (a.nwc - k0 < WV ? a.nwc - k0 : WV);   // the complete ones among them
            const unsigned long long mm = ~0ull >> (WV - m), cm = mc ? ~0ull >> (WV - mc) : 0ull;
            uint4 wd = make_uint4(0u, 0u, 0u, 0u);
            if (k < a.nwc) wd = w[k];
            const unsigned long long U = __ballot((wd.x & 1u) != 0) & cm, V = __ballot((wd.x & 2u) != 0) & cm;
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
                const uint32_t z = uni((uint32_t)__shfl((int)wd.z, mc - 1));
                code1 = vl ? (z & 0xffu) : 0u;
                ql = uni((uint32_t)__shfl((int)wd.y, mc - 1));
                dl = (z >> 8) & 0xffu;
                tl = z >> 16;
                nl = a.N[tl & 7u];
            }
            const uint32_t g = (uint32_t)(G >> lane) & 1u;
            if (k < a.nwin) {
                scratch[((size_t)c * a.nwin + k) * 4] = g;
                const int lo = k * WB > a.hs ? k * WB : a.hs, hi = (k + 1) * WB < a.end ? (k + 1) * WB : a.end;
                cnt += g ? (uint32_t)(hi - lo) : 0u;
            }
        }
        cnt = wave_sum(cnt);
        if (lane == 0) {
            st_out[R_OFF] = r;
            st_out[N_OFF] = n;
            st_out[OPEN_OFF] = open;
            st_out[CODE_OFF] = code1;
            st_out[Q_OFF] = ql;
            st_out[NT_OFF] = nl;
            st_out[D_OFF] = dl;
            st_out[T_OFF] = tl;
            if (d_code) d_code[c] = (int)code1 - 1;
            if (d_open) d_open[c] = gated ? open : 1u;
            if (d_count) d_count[c] = (a.accumulate ? d_count[c] : 0u) + cnt;
            if (d_info) {
                uint32_t *__restrict__ o = d_info + 4 * (size_t)c;   // aligned to a word, no more
                o[0] = ql, o[1] = nl, o[2] = dl, o[3] = tl;
            }
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
__global__ __launch_bounds__(WV) void channel_dcs_outputs_kernel(const void *__restrict__ in_, void *__restrict__ out_,
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

template <bool S16, bool VEC, bool BALLOT>
hipError_t launch_windows_k(const KernelTables &t, const void *d_sense, const uint32_t *d_cws, const int *d_params, uint32_t *d_scratch,
                            const uint32_t *st_in, uint32_t *st_out, const Args &a, int max_wgs, int device, hipStream_t s)
{
    const auto k = channel_dcs_windows_kernel<S16, VEC, BALLOT>;
    unsigned grid = 0;
    const hipError_t e = grid_of(t, reinterpret_cast<const void *>(k), (long long)a.nch * a.nruns, max_wgs, device, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(WV), 0, s, d_sense, d_cws, d_params, d_scratch, st_in, st_out, a);
    return hipGetLastError();
}

template <bool S16, bool VEC>
hipError_t launch_windows(bool ballot, const KernelTables &t, const void *d_sense, const uint32_t *d_cws, const int *d_params,
                          uint32_t *d_scratch, const uint32_t *st_in, uint32_t *st_out, const Args &a, int max_wgs, int device,
                          hipStream_t s)
{
    return ballot ? launch_windows_k<S16, VEC, true>(t, d_sense, d_cws, d_params, d_scratch, st_in, st_out, a, max_wgs, device, s)
                  : launch_windows_k<S16, VEC, false>(t, d_sense, d_cws, d_params, d_scratch, st_in, st_out, a, max_wgs, device, s);
}

template <bool IN16, bool OUT16, bool VEC>
hipError_t launch_outputs(const KernelTables &t, const void *d_in, void *d_out, const uint32_t *d_scratch, const Args &a,
                          int max_wgs, int device, hipStream_t s)
{
    const auto k = channel_dcs_outputs_kernel<IN16, OUT16, VEC>;
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

hipError_t launch_channel_dcs(const KernelTables &t, const void *d_sense, int sense_s16, size_t sense_stride, const void *d_audio,
                              int in_s16, int nch, size_t nsamp, size_t in_stride, uint64_t pos, const uint32_t *d_cws, int ncodes,
                              const int *d_params, uint32_t word, const uint32_t *counts, int window, int e_open, int e_close,
                              int attack, int hang, const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_scratch,
                              void *d_out, int out_s16, size_t out_stride, int *d_code, uint32_t *d_open, uint32_t *d_count,
                              uint32_t *d_info, int accumulate, int ballot, int max_wgs, int device, hipStream_t s)
{
    if (!d_sense || !d_cws || !d_params || !counts || !d_state_in || !d_state_out || !d_scratch || nch < 1 || nsamp == 0 ||
        nsamp > kDcsMaxLaunch || ncodes < 1 || ncodes > kDcsMaxCodes || window < 1 || window > kDcsMaxWindow || word < 1 ||
        word > kDcsMaxWord || e_open < 0 || e_open > e_close || e_close > kDcsMaxErrors || attack < 1 || attack > kDcsMaxAttack ||
        hang < 0 || hang > kDcsMaxHang || (d_audio && !d_out))
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
    a.ncodes = ncodes;
    a.accumulate = accumulate ? 1 : 0;
    a.word = word;
    a.e_open = (uint32_t)e_open;
    a.e_close = (uint32_t)e_close;
    for (int i = 0; i < kDcsPhases; i++) a.N[i] = counts[i];
    a.sense_stride = nch > 1 ? (long long)sense_stride : 0;
    a.in_stride = nch > 1 ? (long long)in_stride : 0;
    a.out_stride = nch > 1 ? (long long)out_stride : 0;

    // four consecutive samples per lane where every quad of a block is aligned to its load
    const uintptr_t ss = sense_s16 ? 2 : 4;
    const bool svec = (((uintptr_t)d_sense - (uintptr_t)(a.hs % B) * ss) % (4 * ss)) == 0 && a.sense_stride % 4 == 0;
    hipError_t e;
    if (sense_s16)
        e = svec ? launch_windows<true, true>(ballot != 0, t, d_sense, d_cws, d_params, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s)
                 : launch_windows<true, false>(ballot != 0, t, d_sense, d_cws, d_params, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s);
    else
        e = svec ? launch_windows<false, true>(ballot != 0, t, d_sense, d_cws, d_params, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s)
                 : launch_windows<false, false>(ballot != 0, t, d_sense, d_cws, d_params, d_scratch, d_state_in, d_state_out, a, max_wgs, device, s);
    if (e != hipSuccess) return e;

    unsigned grid = 0;
    const auto gates = channel_dcs_gates_kernel;
    if ((e = grid_of(t, reinterpret_cast<const void *>(gates), nch, max_wgs, device, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(gates, dim3(grid), dim3(WV), 0, s, d_scratch, d_params, d_state_in, d_state_out, d_code, d_open, d_count, d_info,
                       a);
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
