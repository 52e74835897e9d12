// ddc_channel_blank.hip — the channel noise blanker for gfx950 (sddc_ddc_channel_blank_device): a
// feed-forward impulse blanker per channel on IQ streams, CF32 or CS16 in and out, streaming (each
// channel's block powers, unfinished block, last g samples and last hit live in the handle), in the
// block form that blanker_math.h defines.
//
// A call covers the stream blocks (B = 256 samples, anchored to the stream position) that hold one of
// its samples; u is a sample's index counted from the start of the first of them, so the call's samples
// are hb <= u < end.  Two launches on the caller's stream, both reading the handle's state as it was
// before the call:
//   outputs  channel_blank_kernel: a wave owns a run of consecutive blocks of one channel.  Lane l holds
//            samples l, l + 64, l + 128, l + 192 of a block (512 contiguous bytes per load instruction in
//            CF32, every access aligned to a sample, whatever the base).  Per block: q per sample, the
//            block power as six xor-shuffle levels on the four values and two additions in the lane (the
//            definition's tree), the reference and the threshold from the last M powers, which stay in
//            registers, the hits as four 64-bit ballots = the block's 256-bit mask in sample order, and
//            from them the index of the last hit at or before each sample (a count of leading zeros; the
//            carry into a block is wave-uniform).  Output u is x[u - g], or zero if that last hit is at
//            u - 2 g or later; x[u - g] is a second, shifted read of lines the wave has just read, and
//            the next block's samples are loaded before the current block's arithmetic.
//            Organised by output index the guard needs no look-ahead.  A run that does not start the
//            call recomputes what it needs of the blocks before it: the powers of M + 1 blocks and the
//            hits of one, (M + 1) / run_blocks extra reads (no hits and M blocks if g == 0).
//   state    channel_blank_state_kernel: a wave per channel walks the last M + 2 blocks of the call the
//            same way without outputs and writes the other state buffer (the host swaps the two per
//            call, so no wave reads what another one writes).
// Samples before the call come from the state: q of the unfinished block, the last g stored samples,
// the last hit.  The optional count is an integer atomic per run.  Nothing outside the streams is read
// or written.
//
// Determinism: every value is blanker_math.h's fixed sequence of float operations; the grid, the run
// length, the stream and the other channels decide only which wave does it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ddc_kernels.h"

#pragma clang fp contract(off)
#include "blanker_math.h"

namespace sddc {
namespace {

using namespace blank;

constexpr int B = kBlankBlock;
constexpr int W = 64;   // threads per workgroup: one wave
constexpr int NR = kBlankMaxRef;
// a channel's state, in 32-bit words
constexpr int PW_OFF = 0;              // NR block powers, the newest one last
constexpr int Q_OFF = PW_OFF + NR;     // the unfinished block's q values
constexpr int H_OFF = Q_OFF + B;       // the last g stored samples, the oldest one first
constexpr int S_OFF = H_OFF + 2 * kBlankMaxGuard;   // 0: no hit in the last 2 g samples; else 2 g + 1 - (samples since it)
static_assert(S_OFF + 1 <= kBlankStateWords && H_OFF % 2 == 0 && kBlankStateWords % 2 == 0, "state layout");
constexpr int kNoHit = -(1 << 30);

struct Args {
    int hb, end;       // the call's samples are hb <= u < end
    int n0;            // min(the stream block of u = 0, M)
    int nblocks, nc;   // blocks that hold samples of the call; blocks complete at its end
    int g, M, mode;
    int skip;          // outputs of the call whose stream index is below g: not counted
    int nch, run, nruns;
    long long in_stride, out_stride;   // samples per channel
};

template <bool CS16> using Raw = std::conditional_t<CS16, uint32_t, uint2>;

template <bool CS16> __device__ __forceinline__ float raw_power(Raw<CS16> r)
{
    if constexpr (CS16) return blank_power((float)(short)(r & 0xffffu), (float)(short)(r >> 16));
    else return blank_power(__uint_as_float(r.x), __uint_as_float(r.y));
}

// P of the last n of pw (wave-uniform), n >= 1
__device__ __forceinline__ float reference(const float (&pw)[NR], int n, int mode, int lane)
{
    const int lo = NR - n;
    if (mode == kBlankMean) {
        float S = 0.f;
#pragma unroll
        for (int b = 0; b < NR; b++)
            if (b >= lo) S = b == lo ? pw[b] : S + pw[b];
        return S * blank_rn(n);
    }
    // MEDIAN: lane a < NR ranks pw[a] among the window (ties by index); the lane of rank r has the value
    const int a = lane & (NR - 1);
    float v = pw[0];
#pragma unroll
    for (int b = 1; b < NR; b++) v = a == b ? pw[b] : v;
    int rank = 0;
#pragma unroll
    for (int b = 0; b < NR; b++) rank += (b >= lo && (pw[b] < v || (pw[b] == v && b < a))) ? 1 : 0;
    const unsigned long long m = __ballot(lane < NR && a >= lo && rank == (n - 1) / 2);
    return __shfl(v, __ffsll((long long)m) - 1);
}

// Blocks kp .. kb - 1 of channel data in/out: powers from kp on, hits from kt on, outputs from ka on.
// STATE: the state after the call into st_out.
template <bool CS16, bool STATE>
__device__ __forceinline__ void walk(const Raw<CS16> *__restrict__ in, Raw<CS16> *__restrict__ out,
                                     const uint32_t *__restrict__ st_in, uint32_t *__restrict__ st_out, float thr, float qmin,
                                     uint32_t *__restrict__ count, const Args &a, int kt, int ka, int kb)
{
    using R = Raw<CS16>;
    const int lane = (int)threadIdx.x;
    const R *__restrict__ hist = reinterpret_cast<const R *>(st_in + H_OFF);
    float pw[NR];
#pragma unroll
    for (int b = 0; b < NR; b++) pw[b] = __uint_as_float(st_in[PW_OFF + b]);
    const int code = (int)st_in[S_OFF];
    int carry = code ? a.hb - (2 * a.g + 1 - code) : kNoHit;   // the last hit before the block at hand
    unsigned cnt = 0;
    const int kp = kt - a.M > 0 ? kt - a.M : 0;

    // a block's samples of this lane; outside the call: zero
    auto load_block = [&](int kk, R (&dst)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int u = kk * B + W * j + lane;
            dst[j] = R{};
            if (u >= a.hb && u < a.end) dst[j] = in[u - a.hb];
        }
    };
    R nxt[4];
    load_block(kp, nxt);
    for (int kk = kp; kk < kb; kk++) {
        const int base = kk * B;
        R raw[4], xs[4];
        float q[4], s[4];
        bool valid[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int u = base + W * j + lane;
            valid[j] = u >= a.hb && u < a.end;
            raw[j] = nxt[j];
            xs[j] = raw[j];
        }
        // issued before the arithmetic, in this order (loads return in order): the delayed samples of this
        // block's outputs, lines the wave read a block ago, then the next block's samples
        if (a.g > 0 && kk >= ka) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = base + W * j + lane;
                if (valid[j]) xs[j] = u - a.g >= a.hb ? in[u - a.g - a.hb] : hist[u - a.hb];   // u - hb < g
            }
        }
        if (kk + 1 < kb) load_block(kk + 1, nxt);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int u = base + W * j + lane;
            q[j] = raw_power<CS16>(raw[j]);
            s[j] = blank_finite(q[j]) ? q[j] : 0.f;
            if (!valid[j]) s[j] = u < a.hb ? __uint_as_float(st_in[Q_OFF + u]) : 0.f;   // u < hb: block 0, u < B
        }
        if constexpr (STATE) {
            if (kk == a.nc) {
#pragma unroll
                for (int j = 0; j < 4; j++) st_out[Q_OFF + W * j + lane] = __float_as_uint(s[j]);
            }
        }
#pragma unroll
        for (int m = 1; m < W; m <<= 1) {
#pragma unroll
            for (int j = 0; j < 4; j++) s[j] = s[j] + __shfl_xor(s[j], m);
        }
        const float p = (s[0] + s[1]) + (s[2] + s[3]);

        if (kk >= kt) {
            const int nn = a.n0 + kk < a.M ? a.n0 + kk : a.M;
            float t = 0.f;
            if (nn > 0) t = blank_threshold(thr, reference(pw, nn, a.mode, lane), qmin);
            unsigned long long bal[4];
#pragma unroll
            for (int j = 0; j < 4; j++) bal[j] = __ballot(valid[j] && thr > 0.f && blank_hit(q[j], t, nn));
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (kk >= ka) {
                    const int u = base + W * j + lane;
                    const unsigned long long m = bal[j] & (~0ull >> (63 - lane));
                    const int last = m ? base + W * j + 63 - __clzll((long long)m) : carry;
                    const bool blanked = last >= u - 2 * a.g;
                    if (valid[j]) out[u - a.hb] = blanked ? R{} : xs[j];
                    cnt += (unsigned)__popcll(__ballot(valid[j] && blanked && u - a.hb >= a.skip));
                }
                if (bal[j]) carry = base + W * j + 63 - __clzll((long long)bal[j]);
            }
        }
        if (kk < a.nc) {   // a complete block: its power joins the window
#pragma unroll
            for (int b = 0; b + 1 < NR; b++) pw[b] = pw[b + 1];
            pw[NR - 1] = p;
        }
    }
    if constexpr (STATE) {
#pragma unroll
        for (int b = 0; b < NR; b++)
            if (lane == b) st_out[PW_OFF + b] = __float_as_uint(pw[b]);
        if (lane < a.g) {   // the last g stored samples: u = end - g + lane
            const int u = a.end - a.g + lane;
            reinterpret_cast<R *>(st_out + H_OFF)[lane] = u >= a.hb ? in[u - a.hb] : hist[u - a.hb + a.g];
        }
        if (lane == 0) {
            const long long d = (long long)a.end - carry;
            st_out[S_OFF] = d <= 2 * a.g ? (uint32_t)(2 * a.g + 1 - d) : 0u;
        }
    } else {
        if (count && lane == 0 && cnt) atomicAdd(count, cnt);
    }
}

// par: [nch] (thr, qmin).  state: [nch][kBlankStateWords].  count: null, or [nch], zeroed before the call.
template <bool CS16>
__global__ __launch_bounds__(W) void channel_blank_kernel(const void *__restrict__ in_, void *__restrict__ out_,
                                                          const float2 *__restrict__ par,
                                                          const uint32_t *__restrict__ state_in,
                                                          uint32_t *__restrict__ count, const Args a)
{
    const long long nitems = (long long)a.nch * a.nruns;
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c = (int)(item / a.nruns), r = (int)(item - (long long)c * a.nruns);
        const int ka = r * a.run, kb = ka + a.run < a.nblocks ? ka + a.run : a.nblocks;
        const int kt = (a.g > 0 && ka > 0) ? ka - 1 : ka;
        const float2 p = par[c];
        walk<CS16, false>(static_cast<const Raw<CS16> *>(in_) + c * a.in_stride, static_cast<Raw<CS16> *>(out_) + c * a.out_stride,
                          state_in + (size_t)c * kBlankStateWords, nullptr, p.x, p.y, count ? count + c : nullptr, a, kt, ka, kb);
    }
}

template <bool CS16>
__global__ __launch_bounds__(W) void channel_blank_state_kernel(const void *__restrict__ in_, const float2 *__restrict__ par,
                                                                const uint32_t *__restrict__ state_in,
                                                                uint32_t *__restrict__ state_out, const Args a)
{
    for (int c = (int)blockIdx.x; c < a.nch; c += (int)gridDim.x) {
        const float2 p = par[c];
        const int kt = a.nc > 0 ? a.nc - 1 : 0;   // the last 2 g <= B / 2 samples lie in blocks nc - 1 and nc
        walk<CS16, true>(static_cast<const Raw<CS16> *>(in_) + c * a.in_stride, nullptr, state_in + (size_t)c * kBlankStateWords,
                         state_out + (size_t)c * kBlankStateWords, p.x, p.y, nullptr, a, kt, a.nblocks, a.nblocks);
    }
}

template <bool CS16>
hipError_t launch_both(const KernelTables &t, const void *d_in, void *d_out, const float2 *d_par, const uint32_t *d_state_in,
                       uint32_t *d_state_out, uint32_t *d_count, Args &a, int max_wgs, int run_blocks, int device,
                       hipStream_t s)
{
    const auto outs = channel_blank_kernel<CS16>;
    const auto state = channel_blank_state_kernel<CS16>;
    int occ = 0, cus = 0;
    hipError_t e = launch_geometry(t.lc, reinterpret_cast<const void *>(outs), W, device, &occ, &cus);
    if (e != hipSuccess) return e;
    const long long resident = (long long)cus * occ;
    if (run_blocks > 0) {
        a.run = run_blocks;
    } else {
        // long runs keep the recomputed share small, short ones even out the waves' ends: about four
        // rounds of resident waves, 32..128 blocks (measured: DESIGN.md §4.17)
        long long r = ((long long)a.nch * a.nblocks) / (4 * resident);
        a.run = (int)(r < 32 ? 32 : r > 128 ? 128 : r);
    }
    a.nruns = (a.nblocks + a.run - 1) / a.run;
    long long grid = (long long)a.nch * a.nruns;
    if (grid > resident) grid = resident;
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    hipLaunchKernelGGL(outs, dim3((unsigned)grid), dim3(W), 0, s, d_in, d_out, d_par, d_state_in, d_count, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = launch_geometry(t.lc, reinterpret_cast<const void *>(state), W, device, &occ, &cus);
    if (e != hipSuccess) return e;
    grid = a.nch;
    if (grid > (long long)cus * occ) grid = (long long)cus * occ;
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    hipLaunchKernelGGL(state, dim3((unsigned)grid), dim3(W), 0, s, d_in, d_par, d_state_in, d_state_out, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_channel_blank(const KernelTables &t, const void *d_iq, int cs16, int nch, size_t nsamp, size_t in_stride,
                                uint64_t pos, const float *d_par, int guard, int ref_blocks, int ref_mode,
                                const uint32_t *d_state_in, uint32_t *d_state_out, void *d_out, size_t out_stride,
                                uint32_t *d_count, int max_wgs, int run_blocks, int device, hipStream_t s)
{
    if (!d_iq || !d_out || !d_par || !d_state_in || !d_state_out || nch < 1 || nsamp == 0 || nsamp > kBlankMaxLaunch ||
        guard < 0 || guard > kBlankMaxGuard || ref_blocks < 1 || ref_blocks > NR || (ref_mode != kBlankMean && ref_mode != kBlankMedian))
        return hipErrorInvalidValue;
    Args a;
    const uint64_t kf = pos / (uint64_t)B;
    a.hb = (int)(pos % (uint64_t)B);
    a.end = a.hb + (int)nsamp;
    a.n0 = kf < (uint64_t)ref_blocks ? (int)kf : ref_blocks;
    a.nblocks = (a.end + B - 1) / B;
    a.nc = a.end / B;
    a.g = guard;
    a.M = ref_blocks;
    a.mode = ref_mode;
    a.skip = pos < (uint64_t)guard ? (int)((uint64_t)guard - pos) : 0;
    a.nch = nch;
    a.run = a.nruns = 0;
    a.in_stride = nch > 1 ? (long long)(in_stride / 2) : 0;
    a.out_stride = nch > 1 ? (long long)(out_stride / 2) : 0;
    const float2 *par = reinterpret_cast<const float2 *>(d_par);   // hipMalloc'ed: aligned
    return cs16 ? launch_both<true>(t, d_iq, d_out, par, d_state_in, d_state_out, d_count, a, max_wgs, run_blocks, device, s)
                : launch_both<false>(t, d_iq, d_out, par, d_state_in, d_state_out, d_count, a, max_wgs, run_blocks, device, s);
}

}  // namespace sddc
