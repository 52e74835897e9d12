// ddc_channel_agc.hip — the channel AGC for gfx950 (sddc_ddc_channel_agc_device): a fast-attack,
// exponential-release peak AGC per channel on real audio streams, F32 or S16 in and out, streaming
// (each channel's three envelopes live in the handle), in the max-plus block form that agc_math.h
// defines, so that a call's full blocks of B = 256 samples run in parallel.
//
// A run of a call is cut at the stream's block boundaries into a head (the samples that finish the
// block an earlier call began, or the whole run when it ends inside that block), nblk full blocks and
// a tail.  Three launches on the caller's stream:
//   ends     channel_agc_block_kernel<.., false>: one lane per (channel, full block).  The lane runs
//            the envelope from a zero start over its block and writes the end value Z_k into its
//            scratch slot of one float.
//   scan     channel_agc_scan_kernel: one lane per channel, in stream order (the slots of the next 32
//            blocks are loaded while the current ones are advanced).  The head from the handle's R
//            and Zr, with its outputs, and E = max(Zr, dB E) if it completes the block; then per full
//            block the slot's Z_k is replaced by the entry envelope E_k and E = max(Z_k, dB E): two
//            dependent operations; then the tail from R = E, Zr = 0 with its outputs; R goes to d_env
//            and (E, R, Zr) to the other state buffer (the host swaps the two per run, so no lane
//            reads what another one writes).
//   outputs  channel_agc_block_kernel<.., true>: one lane per (channel, full block) again.  The lane
//            runs the envelope from E_k and produces the block's B outputs.
// The lanes of a wave hold 64 consecutive (channel, block) items, whose samples lie B apart in
// memory, so no lane walks global memory itself: a workgroup is one wave, and the wave moves chunks
// of CH = 32 samples of its 64 rows through LDS.  Rows r and r + 1 of a chunk are loaded by the two
// 32-lane halves with consecutive lanes on consecutive samples (128 bytes per row and chunk, any
// alignment, F32 or S16), the next chunk's loads are issued before the current chunk is computed,
// a lane reads its own row at pitch CH + 1 (bank (lane + i) mod 32: no conflict within a half, one
// ds_read_b32 each, CDC_RD keeps the compiler from pairing them), overwrites it with its outputs,
// and the rows go back to memory the way they came.  Nothing outside the streams is read or written.
// (This row staging is ddc_channel_audio.hip's, line for line; sharing it is left to a later change,
// as it was for the decimator and the resampler.)
//
// Determinism: an output is agc_math.h's fixed sequence of float operations on the definition's
// state; the grid, the run length, the stream and the other channels decide only which lane does it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "channel_stage.hpp"
#include "ddc_kernels.h"

// agc_math.h, demod_s16 and every float operation below: no contraction
#pragma clang fp contract(off)
#include "agc_math.h"
#include "demod_math.h"

namespace sddc {
namespace {

using namespace agc;

constexpr int B = kAgcBlock;
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

// One lane per (channel, full block): item = c * nblk + k.  OUTPUT false: Z_k from a zero start into
// scratch[k * nch + c]; OUTPUT true: the block's outputs from the E_k that the scan left there.
// par: [nch] (T, d, F, dB).
template <bool IN16, bool OUT16, bool OUTPUT>
__global__ __launch_bounds__(W) void channel_agc_block_kernel(const void *__restrict__ in_, void *__restrict__ out_,
                                                              const float4 *__restrict__ par,
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
        const float4 p = active ? par[c] : make_float4(0.f, 0.f, 1.f, 0.f);
        const float T = p.x, d = p.y, F = p.z;
        float *slot = scratch + (k * a.nch + c);
        float e = (OUTPUT && active) ? *slot : 0.f;
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
            // the row's chunk into registers first: a tile write between two reads would make each read
            // wait for the division before it
            float xs[CH];
#pragma unroll
            for (int i = 0; i < CH; i++) CDC_RD(xs[i], tile[lane * PITCH + i]);
#pragma unroll
            for (int i = 0; i < CH; i++) {
                e = agc_env(agc_abs(xs[i]), d, e);
                if constexpr (OUTPUT) tile[lane * PITCH + i] = agc_out(T, F, e, xs[i]);
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
            if (active) *slot = e;
        }
    }
}

// One lane per channel, the stream order of the run (see the head of the file).  state: [nch][3]
// floats E, R, Zr.  env: null, or [nch] floats that receive R after the run's last sample.
template <bool IN16, bool OUT16>
__global__ __launch_bounds__(W) void channel_agc_scan_kernel(const void *__restrict__ in_, void *__restrict__ out_,
                                                             const float4 *__restrict__ par,
                                                             const float *__restrict__ state_in,
                                                             float *__restrict__ state_out,
                                                             float *__restrict__ scratch, float *__restrict__ env,
                                                             const Args a)
{
    using I = InT<IN16>;
    using O = OutT<OUT16>;
    constexpr int U = 8;     // samples of the head and the tail whose loads are issued together
    constexpr int UB = 32;   // scratch slots per register buffer
    for (long long c = (long long)blockIdx.x * W + threadIdx.x; c < a.nch; c += (long long)gridDim.x * W) {
        const I *__restrict__ in = static_cast<const I *>(in_) + c * a.in_stride;
        O *__restrict__ out = static_cast<O *>(out_) + c * a.out_stride;
        const float4 p = par[c];
        const float T = p.x, d = p.y, F = p.z, dB = p.w;
        float E = state_in[c * 3], R = state_in[c * 3 + 1], Zr = state_in[c * 3 + 2];
        // n samples from index i0 on through R and Zr, with their outputs
        auto run = [&](long long i0, long long n) {
            for (long long i = 0; i < n; i += U) {
                I x[U];
#pragma unroll
                for (int q = 0; q < U; q++) x[q] = i + q < n ? in[i0 + i + q] : I(0);
#pragma unroll
                for (int q = 0; q < U; q++)
                    if (i + q < n) {
                        const float xf = (float)x[q], m = agc_abs(xf);
                        R = agc_env(m, d, R);
                        Zr = agc_env(m, d, Zr);
                        out[i0 + i + q] = to_out<OUT16>(agc_out(T, F, R, xf));
                    }
            }
        };
        run(0, a.head);
        if (a.head_completes) {
            E = agc_boundary(dB, E, Zr);
            R = E;
            Zr = 0.f;
        }
        // The full blocks, UB at a time from two register buffers: the loads of the next UB slots are
        // issued before the current UB are advanced (16 waves at most run this kernel, so nothing
        // else hides the latency of a slot).  Consecutive lanes hold consecutive floats of a block's
        // slots; past the run's last block the last slot is loaded again and unused.
        const int nb = (int)a.nblk;   // at most 2^20 per run
        if (nb > 0) {
            float *const lane_slots = scratch + c;
            const size_t pitch = (size_t)a.nch;   // floats between the slots of consecutive blocks
            float ZA[UB], ZB[UB];
            auto fetch = [&](float (&Z)[UB], int k) {
#pragma unroll
                for (int q = 0; q < UB; q++) Z[q] = lane_slots[(size_t)(k + q < nb ? k + q : nb - 1) * pitch];
            };
            auto advance = [&](const float (&Z)[UB], int k) {
#pragma unroll
                for (int q = 0; q < UB; q++)
                    if (k + q < nb) {
                        lane_slots[(size_t)(k + q) * pitch] = E;
                        E = agc_boundary(dB, E, Z[q]);
                    }
            };
            fetch(ZA, 0);
            for (int k = 0; k < nb; k += 2 * UB) {
                fetch(ZB, k + UB);
                advance(ZA, k);
                fetch(ZA, k + 2 * UB);
                advance(ZB, k + UB);
            }
            R = E;
            Zr = 0.f;
        }
        run(a.head + a.nblk * B, a.tail);
        if (env) env[c] = R;
        state_out[c * 3] = E;
        state_out[c * 3 + 1] = R;
        state_out[c * 3 + 2] = Zr;
    }
}

template <bool IN16, bool OUT16>
hipError_t launch_run(const KernelTables &t, const void *d_in, void *d_out, const float4 *d_par, const float *d_state_in,
                      float *d_state_out, float *d_scratch, float *d_env, const Args &a, int max_wgs, int device,
                      hipStream_t s)
{
    const auto ends = channel_agc_block_kernel<IN16, OUT16, false>;
    const auto outs = channel_agc_block_kernel<IN16, OUT16, true>;
    const auto scan = channel_agc_scan_kernel<IN16, OUT16>;
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
        hipLaunchKernelGGL(ends, dim3(grid), dim3(W), 0, s, d_in, d_out, d_par, d_scratch, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = grid_of(reinterpret_cast<const void *>(scan), (a.nch + W - 1) / W, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(scan, dim3(grid), dim3(W), 0, s, d_in, d_out, d_par, d_state_in, d_state_out, d_scratch, d_env, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.nblk > 0) {
        if ((e = grid_of(reinterpret_cast<const void *>(outs), bgroups, &grid)) != hipSuccess) return e;
        hipLaunchKernelGGL(outs, dim3(grid), dim3(W), 0, s, d_in, d_out, d_par, d_scratch, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_channel_agc(const KernelTables &t, const void *d_in, int in_s16, int nch, size_t nsamp, size_t in_stride,
                              unsigned block_pos, const float *d_par, const float *d_state_in, float *d_state_out,
                              float *d_scratch, void *d_out, int out_s16, size_t out_stride, float *d_env, int max_wgs,
                              int device, hipStream_t s)
{
    if (!d_in || !d_out || !d_par || !d_state_in || !d_state_out || nch < 1 || nsamp == 0 || nsamp > ((size_t)1 << 40) ||
        block_pos >= (unsigned)B)
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
    const float4 *par = reinterpret_cast<const float4 *>(d_par);   // hipMalloc'ed: 16-byte aligned
    if (in_s16)
        return out_s16 ? launch_run<true, true>(t, d_in, d_out, par, d_state_in, d_state_out, d_scratch, d_env, a, max_wgs, device, s)
                       : launch_run<true, false>(t, d_in, d_out, par, d_state_in, d_state_out, d_scratch, d_env, a, max_wgs, device, s);
    return out_s16 ? launch_run<false, true>(t, d_in, d_out, par, d_state_in, d_state_out, d_scratch, d_env, a, max_wgs, device, s)
                   : launch_run<false, false>(t, d_in, d_out, par, d_state_in, d_state_out, d_scratch, d_env, a, max_wgs, device, s);
}

}  // namespace sddc
