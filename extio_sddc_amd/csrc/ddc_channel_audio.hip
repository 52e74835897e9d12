// ddc_channel_audio.hip — the channel audio filter for gfx950 (sddc_ddc_channel_audio_filter_device): a
// cascade of S = 1..4 biquad sections per channel on real audio streams, F32 or S16 in and out,
// streaming (each channel's three state vectors live in the handle), in the block form that
// audio_iir_math.h defines, so that a call's full blocks of B = 256 samples run in parallel.
//
// A run of a call is cut at the stream's block boundaries into a head (the samples that finish the
// block an earlier call began, or the whole run when it ends inside that block), nblk full blocks and
// a tail.  Three launches on the caller's stream:
//   ends     channel_audio_block_kernel<.., false>: one lane per (channel, full block).  The lane runs
//            the zero-state recurrence over its block and writes the end state Z_k into its scratch
//            slot of 2S floats.
//   scan     channel_audio_scan_kernel: one lane per channel, in stream order (the slots of the next
//            64 / 2S blocks are loaded while the current ones are advanced).  The head from the
//            handle's R and Zr, with its outputs, and E = adv(E, Zr) if it completes the block; then
//            per full block the slot's Z_k is replaced by the entry state E_k and E = adv(E, Z_k);
//            then the tail from R = E, Zr = 0 with its outputs; and (E, R, Zr) go to the other state
//            buffer (the host swaps the two per run, so no lane reads what another one writes).
//   outputs  channel_audio_block_kernel<.., true>: one lane per (channel, full block) again.  The
//            lane runs the recurrence from E_k and produces the block's B outputs.
// The lanes of a wave hold 64 consecutive (channel, block) items, whose samples lie B apart in
// memory, so no lane walks global memory itself: a workgroup is one wave, and the wave moves chunks
// of CH = 32 samples of its 64 rows through LDS.  Rows r and r + 1 of a chunk are loaded by the two
// 32-lane halves with consecutive lanes on consecutive samples (128 bytes per row and chunk, any
// alignment, F32 or S16), the next chunk's loads are issued before the current chunk is computed,
// a lane reads its own row at pitch CH + 1 (bank (lane + i) mod 32: no conflict within a half, one
// ds_read_b32 each, CDC_RD keeps the compiler from pairing them), overwrites it with its outputs,
// and the rows go back to memory the way they came.  Nothing outside the streams is read or written.
//
// Determinism: an output is audio_iir_math.h's fixed sequence of float operations on the definition's
// state; the grid, the run length, the stream and the other channels decide only which lane does it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "channel_stage.hpp"
#include "ddc_kernels.h"

// audio_iir_math.h, demod_s16 and every float operation below: no contraction
#pragma clang fp contract(off)
#include "audio_iir_math.h"
#include "demod_math.h"

namespace sddc {
namespace {

using namespace audio;

constexpr int B = kAudioBlock;
constexpr int W = 64;            // threads per workgroup: one wave
constexpr int CH = 32;           // samples of a row per chunk
constexpr int PITCH = CH + 1;
static_assert(B % CH == 0 && W == 2 * CH, "whole chunks; two rows per load instruction");

struct Args {
    long long head, nblk, tail;       // samples, full blocks, samples of this run per channel
    long long nitems;                 // nch * nblk
    long long in_stride, out_stride;  // samples per channel
    int nch;
    int head_completes;               // the head ends at a block boundary
};

template <bool IN16> using InT = std::conditional_t<IN16, short, float>;
template <bool OUT16> using OutT = std::conditional_t<OUT16, short, float>;

template <bool OUT16> __device__ __forceinline__ OutT<OUT16> to_out(float y)
{
    if constexpr (OUT16) return demod::demod_s16(y);
    else return y;
}

// One lane per (channel, full block): item = c * nblk + k.  OUTPUT false: Z_k from a zero state into
// scratch[(k * nch + c) * 2S ..]; OUTPUT true: the block's outputs from the E_k that the scan left there.
template <int S, bool IN16, bool OUT16, bool OUTPUT>
__global__ __launch_bounds__(W) void channel_audio_block_kernel(const void *__restrict__ in_, void *__restrict__ out_,
                                                                const float *__restrict__ coef,
                                                                float *__restrict__ scratch, const Args a)
{
    using I = InT<IN16>;
    using O = OutT<OUT16>;
    const I *__restrict__ in = static_cast<const I *>(in_);
    O *__restrict__ out = static_cast<O *>(out_);
    __shared__ float tile[W * PITCH];
    __shared__ long long row_in[W], row_out[W];   // a row's first sample in `in` / `out`; -1: no such item
    const int lane = (int)threadIdx.x, half = lane >> 5, j = lane & 31;
    const long long ngroups = (a.nitems + W - 1) / W;

    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long item = grp * W + lane;
        const bool active = item < a.nitems;
        const long long c = active ? item / a.nblk : 0, k = active ? item - c * a.nblk : 0;
        __syncthreads();   // the previous group's reads of the rows are done
        row_in[lane] = active ? c * a.in_stride + a.head + k * B : -1;
        row_out[lane] = active ? c * a.out_stride + a.head + k * B : -1;
        float cf[5 * S], st[2 * S];
#pragma unroll
        for (int q = 0; q < 5 * S; q++) cf[q] = active ? coef[c * (5 * S) + q] : 0.f;
        float *slot = scratch + (k * a.nch + c) * (2 * S);
#pragma unroll
        for (int q = 0; q < 2 * S; q++) st[q] = (OUTPUT && active) ? slot[q] : 0.f;
        __syncthreads();

        I raw[CH];
        auto load_chunk = [&](int ch) {
#pragma unroll
            for (int rr = 0; rr < CH; rr++) {
                const long long base = row_in[2 * rr + half];
                raw[rr] = I(0);
                if (base >= 0) raw[rr] = in[base + ch * CH + j];
            }
        };
        load_chunk(0);
        for (int ch = 0; ch < B / CH; ch++) {
#pragma unroll
            for (int rr = 0; rr < CH; rr++) tile[(2 * rr + half) * PITCH + j] = (float)raw[rr];
            __syncthreads();
            if (ch + 1 < B / CH) load_chunk(ch + 1);   // in flight while this chunk is computed
#pragma unroll
            for (int i = 0; i < CH; i++) {
                float x;
                CDC_RD(x, tile[lane * PITCH + i]);
                const float y = audio_step<S>(cf, st, x);
                if constexpr (OUTPUT) tile[lane * PITCH + i] = y;
            }
            if constexpr (OUTPUT) {
                __syncthreads();
#pragma unroll
                for (int rr = 0; rr < CH; rr++) {
                    const long long base = row_out[2 * rr + half];
                    if (base >= 0) out[base + ch * CH + j] = to_out<OUT16>(tile[(2 * rr + half) * PITCH + j]);
                }
            }
            __syncthreads();   // the tile is free for the next chunk
        }
        if constexpr (!OUTPUT) {
            if (active) {
#pragma unroll
                for (int q = 0; q < 2 * S; q++) slot[q] = st[q];
            }
        }
    }
}

// One lane per channel, the stream order of the run (see the head of the file).  state: [nch][3][2S]
// floats E, R, Zr.
template <int S, bool IN16, bool OUT16>
__global__ __launch_bounds__(W) void channel_audio_scan_kernel(const void *__restrict__ in_, void *__restrict__ out_,
                                                               const float *__restrict__ coef,
                                                               const float *__restrict__ mat,
                                                               const float *__restrict__ state_in,
                                                               float *__restrict__ state_out,
                                                               float *__restrict__ scratch, const Args a)
{
    using I = InT<IN16>;
    using O = OutT<OUT16>;
    constexpr int N = 2 * S;
    constexpr int U = 8;        // samples of the head and the tail whose loads are issued together
    constexpr int UB = 64 / N;  // scratch slots per register buffer
    for (long long c = (long long)blockIdx.x * W + threadIdx.x; c < a.nch; c += (long long)gridDim.x * W) {
        const I *__restrict__ in = static_cast<const I *>(in_) + c * a.in_stride;
        O *__restrict__ out = static_cast<O *>(out_) + c * a.out_stride;
        float cf[5 * S], M[N * N], E[N], R[N], Zr[N];
#pragma unroll
        for (int q = 0; q < 5 * S; q++) cf[q] = coef[c * (5 * S) + q];
#pragma unroll
        for (int q = 0; q < N * N; q++) M[q] = mat[c * (N * N) + q];
#pragma unroll
        for (int q = 0; q < N; q++) {
            E[q] = state_in[c * 3 * N + q];
            R[q] = state_in[c * 3 * N + N + q];
            Zr[q] = state_in[c * 3 * N + 2 * N + q];
        }
        // n samples from index i0 on through R and Zr, with their outputs
        auto run = [&](long long i0, long long n) {
            for (long long i = 0; i < n; i += U) {
                I x[U];
#pragma unroll
                for (int e = 0; e < U; e++) x[e] = i + e < n ? in[i0 + i + e] : I(0);
#pragma unroll
                for (int e = 0; e < U; e++)
                    if (i + e < n) {
                        const float y = audio_step<S>(cf, R, (float)x[e]);
                        (void)audio_step<S>(cf, Zr, (float)x[e]);
                        out[i0 + i + e] = to_out<OUT16>(y);
                    }
            }
        };
        auto restart = [&](const float *Z) {   // E = adv(E, Z), R = E, Zr = 0
            float nE[N];
            audio_adv<S>(M, E, Z, nE);
#pragma unroll
            for (int q = 0; q < N; q++) {
                E[q] = nE[q];
                R[q] = nE[q];
                Zr[q] = 0.f;
            }
        };
        run(0, a.head);
        if (a.head_completes) restart(Zr);
        // The full blocks, UB at a time from two register buffers: the loads of the next UB slots are
        // issued before the current UB are advanced (16 waves at most run this kernel, so nothing
        // else hides the latency of a slot).  A slot's address is a wave-uniform base plus the
        // lane's channel offset; past the run's last block the last slot is loaded again and unused.
        const int nb = (int)a.nblk;   // at most 2^20 per run
        if (nb > 0) {
            float2 *const lane_slots = reinterpret_cast<float2 *>(scratch + c * N);
            const size_t pitch = (size_t)a.nch * S;   // float2 between the slots of consecutive blocks
            float ZA[UB][N], ZB[UB][N];
            auto fetch = [&](float (&Z)[UB][N], int k) {
#pragma unroll
                for (int e = 0; e < UB; e++) {
                    const float2 *sl = lane_slots + (size_t)(k + e < nb ? k + e : nb - 1) * pitch;
#pragma unroll
                    for (int q = 0; q < S; q++) {
                        const float2 v = sl[q];
                        Z[e][2 * q] = v.x;
                        Z[e][2 * q + 1] = v.y;
                    }
                }
            };
            auto advance = [&](const float (&Z)[UB][N], int k) {
#pragma unroll
                for (int e = 0; e < UB; e++)
                    if (k + e < nb) {
                        float2 *sl = lane_slots + (size_t)(k + e) * pitch;
                        float nE[N];
#pragma unroll
                        for (int q = 0; q < S; q++) sl[q] = make_float2(E[2 * q], E[2 * q + 1]);
                        audio_adv<S>(M, E, Z[e], nE);
#pragma unroll
                        for (int q = 0; q < N; q++) E[q] = nE[q];
                    }
            };
            fetch(ZA, 0);
            for (int k = 0; k < nb; k += 2 * UB) {
                fetch(ZB, k + UB);
                advance(ZA, k);
                fetch(ZA, k + 2 * UB);
                advance(ZB, k + UB);
            }
#pragma unroll
            for (int q = 0; q < N; q++) {
                R[q] = E[q];
                Zr[q] = 0.f;
            }
        }
        run(a.head + a.nblk * B, a.tail);
#pragma unroll
        for (int q = 0; q < N; q++) {
            state_out[c * 3 * N + q] = E[q];
            state_out[c * 3 * N + N + q] = R[q];
            state_out[c * 3 * N + 2 * N + q] = Zr[q];
        }
    }
}

template <int S, bool IN16, bool OUT16>
hipError_t launch_run(const KernelTables &t, const void *d_in, void *d_out, const float *d_coef, const float *d_mat,
                      const float *d_state_in, float *d_state_out, float *d_scratch, const Args &a, int max_wgs,
                      int device, hipStream_t s)
{
    const auto ends = channel_audio_block_kernel<S, IN16, OUT16, false>;
    const auto outs = channel_audio_block_kernel<S, IN16, OUT16, true>;
    const auto scan = channel_audio_scan_kernel<S, IN16, OUT16>;
    auto grid_of = [&](const void *kern, long long groups, unsigned *grid) {
        int occ = 0, cus = 0;
        const hipError_t e = launch_geometry(t.lc, kern, W, device, &occ, &cus);
        if (e != hipSuccess) return e;
        long long g = groups;
        if (g > (long long)cus * occ) g = (long long)cus * occ;
        if (max_wgs > 0 && g > max_wgs) g = max_wgs;
        *grid = (unsigned)g;
        return hipSuccess;
    };
    const long long bgroups = (a.nitems + W - 1) / W;
    unsigned grid = 0;
    hipError_t e;
    if (a.nblk > 0) {
        if ((e = grid_of(reinterpret_cast<const void *>(ends), bgroups, &grid)) != hipSuccess) return e;
        hipLaunchKernelGGL(ends, dim3(grid), dim3(W), 0, s, d_in, d_out, d_coef, d_scratch, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = grid_of(reinterpret_cast<const void *>(scan), (a.nch + W - 1) / W, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(scan, dim3(grid), dim3(W), 0, s, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.nblk > 0) {
        if ((e = grid_of(reinterpret_cast<const void *>(outs), bgroups, &grid)) != hipSuccess) return e;
        hipLaunchKernelGGL(outs, dim3(grid), dim3(W), 0, s, d_in, d_out, d_coef, d_scratch, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int S>
hipError_t launch_fmt(int in16, int out16, const KernelTables &t, const void *d_in, void *d_out, const float *d_coef,
                      const float *d_mat, const float *d_state_in, float *d_state_out, float *d_scratch, const Args &a,
                      int max_wgs, int device, hipStream_t s)
{
    if (in16)
        return out16 ? launch_run<S, true, true>(t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s)
                     : launch_run<S, true, false>(t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s);
    return out16 ? launch_run<S, false, true>(t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s)
                 : launch_run<S, false, false>(t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s);
}

}  // namespace

hipError_t launch_channel_audio(const KernelTables &t, const void *d_in, int in_s16, int nch, int nsec, size_t nsamp,
                                size_t in_stride, unsigned block_pos, const float *d_coef, const float *d_mat,
                                const float *d_state_in, float *d_state_out, float *d_scratch, void *d_out, int out_s16,
                                size_t out_stride, int max_wgs, int device, hipStream_t s)
{
    if (!d_in || !d_out || !d_coef || !d_mat || !d_state_in || !d_state_out || nch < 1 || nsec < 1 ||
        nsec > audio::kAudioMaxSections || nsamp == 0 || nsamp > ((size_t)1 << 40) || block_pos >= (unsigned)B)
        return hipErrorInvalidValue;
    Args a;
    const long long n = (long long)nsamp, to_edge = (B - (long long)block_pos) % B;
    a.head = to_edge < n ? to_edge : n;
    a.head_completes = a.head > 0 && a.head == to_edge;
    a.nblk = (n - a.head) / B;
    a.tail = n - a.head - a.nblk * B;
    a.nitems = a.nblk * nch;
    a.in_stride = nch > 1 ? (long long)in_stride : 0;
    a.out_stride = nch > 1 ? (long long)out_stride : 0;
    a.nch = nch;
    if (a.nblk > 0 && !d_scratch) return hipErrorInvalidValue;
    switch (nsec) {
    case 1: return launch_fmt<1>(in_s16, out_s16, t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s);
    case 2: return launch_fmt<2>(in_s16, out_s16, t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s);
    case 3: return launch_fmt<3>(in_s16, out_s16, t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s);
    default: return launch_fmt<4>(in_s16, out_s16, t, d_in, d_out, d_coef, d_mat, d_state_in, d_state_out, d_scratch, a, max_wgs, device, s);
    }
}

}  // namespace sddc
