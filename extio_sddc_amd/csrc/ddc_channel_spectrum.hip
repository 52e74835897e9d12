// ddc_channel_spectrum.hip — the averaged power spectrum of the DDC's IQ output for gfx950
// (sddc_ddc_channel_spectrum_device): the "zoom" panadapter of a tuned channel, computed on the
// decimated stream that process_device / process_channels_device wrote, CF32 or CS16.
//
//   X_f[k]       = sum_j w[j] x[start_f + j] e^{-2 pi i jk/n},   start_f = (r fpr + f) hop
//   psd[c][r][q] = scale * sum_{f < fpr} |X_f[(q + n/2) mod n]|^2,   n = 256 .. 4096
//
// Work item: one (channel, row).  The n / 16 threads that own it (fft_batch.hip's geometry: a
// 256-thread workgroup holds 4096 / n items in padded LDS) run the item's fpr frames in frame
// order.  Per frame:
//   pass 0 (radix 16, NS 1)   the thread's 16 samples lt + r n/16 come straight from global memory
//                             (8 bytes per lane CF32, 4 bytes CS16, consecutive lanes consecutive
//                             samples), converted and windowed in registers; the window's 16
//                             values per thread are loaded once per launch; the rectangular
//                             instance has no multiply
//   pass 1 (radix 16, NS 16)  n >= 512 only
//   last pass (radix n / 16 for n = 256, else n / 256)   its 16 outputs per thread are squared
//                             and added to 16 register sums instead of stored: the thread owns
//                             the same bins in every frame
// and after the item's last frame the sums are scaled and stored at (bin + n/2) mod n.  The next
// frame's 16 loads are issued before the current frame's first DFT.
//
// Every stored value is a fixed sequence of float operations on the samples of its row, given by
// the thread's place in its transform alone: the grid, the workgroup, the sub-group and the other
// items do not enter, and there are no atomics and no scratch memory.
//
// Barriers: the passes exchange through LDS with workgroup barriers, so every thread of a
// workgroup must reach each one the same number of times.  The loop runs rounds * fpr trips with
// rounds = ceil(items / (grid * items per workgroup)), the same for every workgroup and sub-group;
// a sub-group whose item index is past the end transforms zeros (or stale registers) and stores
// nothing.  No barrier sits under a condition that differs between threads.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ddc_kernels.h"
#include "fft_device.hpp"

namespace sddc {
namespace {

constexpr int NT = 256;
constexpr int kTw = 8192;   // tw[k] = e^{-2 pi i k / 8192} (KernelTables::post8192)

// one LDS read per instruction (ddc_frame_common.hpp XRD: the compiler's ds_read2 pairs cost 8
// LDS cycles against 2 for a ds_read_b64)
#define CSP_RD(dst, expr) do { dst = (expr); asm volatile("" ::: "memory"); } while (0)

template <int n>
struct Geo {
    static constexpr int TPT = n / 16;                       // threads per transform
    static constexpr int TPW = NT / TPT;                     // transforms per workgroup
    static constexpr int RL = n <= 256 ? n / 16 : n / 256;   // the last pass's radix
    static constexpr int NSL = n / RL;                       // its NS = its butterflies
    static constexpr int PERL = NSL / TPT;                   // butterflies per thread: PERL * RL = 16
    static_assert(PERL * RL == 16 && NT % TPT == 0, "channel spectrum geometry");
};

// W_m^e, m | 8192 (forward)
__device__ __forceinline__ float2 twd(const float2 *__restrict__ tw, int e, int m)
{
    return tw[(e * (kTw / m)) & (kTw - 1)];
}

// CF32: (I, Q) floats; CS16: (I, Q) int16 in one dword, I in the low half
template <bool CS16> using Raw = std::conditional_t<CS16, int, float2>;

template <bool CS16>
__device__ __forceinline__ float2 to_float(Raw<CS16> x)
{
    if constexpr (CS16) return make_float2((float)(int)(short)(x & 0xffff), (float)(x >> 16));
    else return x;
}

template <int n, bool CS16, bool WIN>
__global__ __launch_bounds__(NT) void channel_spectrum_kernel(const Raw<CS16> *__restrict__ iq,
                                                              float *__restrict__ psd,
                                                              const float *__restrict__ win,
                                                              const float2 *__restrict__ tw, long long nitems,
                                                              int nrows, size_t stride, size_t hop, int fpr,
                                                              float scale)
{
    using G = Geo<n>;
    constexpr int TPT = G::TPT, TPW = G::TPW, RL = G::RL, NSL = G::NSL, PERL = G::PERL;
    __shared__ float2 lds[TPW * lds_slots(n)];
    const int sub = (int)threadIdx.x / TPT, lt = (int)threadIdx.x % TPT;
    float2 *sl = lds + sub * lds_slots(n);

    float wn[WIN ? 16 : 1];
    if constexpr (WIN) {
#pragma unroll
        for (int r = 0; r < 16; r++) wn[r] = win[lt + r * TPT];
    }

    // the same trip count in every workgroup and sub-group
    const long long per_round = (long long)gridDim.x * TPW;
    const int rounds = (int)((nitems + per_round - 1) / per_round);

    // frame 0 of item it = c nrows + r: channel c's stream + r fpr hop samples (+ this thread's lt)
    auto frame0 = [&](long long it) {
        const unsigned c = (unsigned)it / (unsigned)nrows, r = (unsigned)it % (unsigned)nrows;
        return iq + (size_t)c * stride + (size_t)r * (size_t)fpr * hop + lt;
    };

    long long item = (long long)blockIdx.x * TPW + sub;
    bool ok = item < nitems;
    const Raw<CS16> *src = ok ? frame0(item) : iq;
    Raw<CS16> x[16];
#pragma unroll
    for (int r = 0; r < 16; r++) x[r] = Raw<CS16>();
    if (ok) {
#pragma unroll
        for (int r = 0; r < 16; r++) x[r] = src[r * TPT];
    }
    float acc[16];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;

    int round = 0, f = 0;
    for (;;) {
        // the frame after this one: the item's next, or frame 0 of the sub-group's next item
        const bool last = f + 1 == fpr;                   // workgroup-uniform
        const int fn = last ? 0 : f + 1, roundn = last ? round + 1 : round;
        const bool more = roundn < rounds;                // workgroup-uniform
        long long itemn = item;
        bool okn = ok;
        const Raw<CS16> *srcn = src + hop;
        if (last) {
            itemn = item + per_round;
            okn = more && itemn < nitems;
            srcn = okn ? frame0(itemn) : iq;
        }

        // An opaque per-iteration copy of lt (ddc_spectrum.hip): without it the compiler hoists the
        // frame-invariant twiddle loads out of the loop and holds 30 float2 in registers (200+
        // VGPRs, 2 workgroups per CU); with it they are re-read from L1 each frame.
        int z = 0;
        asm volatile("" : "+s"(z));
        const int tl = lt + z;
        float2 v[16];
        // ---- pass 0 (R16, NS 1): convert, window, prefetch, DFT16 ----
        {
            float2 a[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                a[r] = to_float<CS16>(x[r]);
                if constexpr (WIN) a[r] = make_float2(a[r].x * wn[r], a[r].y * wn[r]);
            }
            if (okn) {
#pragma unroll
                for (int r = 0; r < 16; r++) x[r] = srcn[r * TPT];
            }
            dft16<-1>(a, v);
        }
        __syncthreads();   // the previous frame's last-pass reads are done
#pragma unroll
        for (int r = 0; r < 16; r++) sl[lds_pad(16 * lt + r)] = v[r];
        __syncthreads();
        if constexpr (n > 256) {
            // ---- pass 1 (R16, NS 16): W_256^{(lt % 16) r} ----
            {
                float2 a[16];
#pragma unroll
                for (int r = 0; r < 16; r++) CSP_RD(a[r], sl[lds_pad(lt + r * TPT)]);
#pragma unroll
                for (int r = 1; r < 16; r++) a[r] = cmul(a[r], twd(tw, (tl % 16) * r, 256));
                dft16<-1>(a, v);
            }
            __syncthreads();
            {
                const int base = (lt / 16) * 256 + (lt % 16);
#pragma unroll
                for (int r = 0; r < 16; r++) sl[lds_pad(base + 16 * r)] = v[r];
            }
            __syncthreads();
        }
        // ---- last pass (radix RL, NS NSL): |X|^2 into the thread's 16 sums ----
#pragma unroll
        for (int i = 0; i < PERL; i++) {
            const int j = tl + i * TPT;   // j < NSL
            float2 a[RL], o[RL];
#pragma unroll
            for (int r = 0; r < RL; r++) CSP_RD(a[r], sl[lds_pad(j + r * NSL)]);
#pragma unroll
            for (int r = 1; r < RL; r++) a[r] = cmul(a[r], twd(tw, j * r, n));
            dft<RL, -1>(a, o);
#pragma unroll
            for (int r = 0; r < RL; r++) acc[i * RL + r] = fmaf(o[r].x, o[r].x, fmaf(o[r].y, o[r].y, acc[i * RL + r]));
        }
        if (last) {
            // bin j + r NSL goes to q = (bin + n/2) mod n: 4 bytes per lane, consecutive lanes
            // consecutive floats
            if (ok) {
                float *dst = psd + (size_t)item * n;
#pragma unroll
                for (int i = 0; i < PERL; i++)
#pragma unroll
                    for (int r = 0; r < RL; r++)
                        dst[(lt + i * TPT + r * NSL + n / 2) & (n - 1)] = acc[i * RL + r] * scale;
            }
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
        }
        if (!more) break;
        f = fn;
        round = roundn;
        item = itemn;
        ok = okn;
        src = srcn;
    }
}

template <int n, bool CS16, bool WIN>
hipError_t launch_n(const KernelTables &t, const void *d_iq, long long nitems, int nrows, size_t stride, size_t hop,
                    int fpr, float *d_psd, const float *d_win, float scale, int max_wgs, int device, hipStream_t s)
{
    auto kern = channel_spectrum_kernel<n, CS16, WIN>;
    int occ = 0, cus = 0;
    hipError_t e = launch_geometry(t.lc, reinterpret_cast<const void *>(kern), NT, device, &occ, &cus);
    if (e != hipSuccess) return e;
    // enough workgroups for all items, or full residency with a loop
    long long grid = (nitems + Geo<n>::TPW - 1) / Geo<n>::TPW;
    if (grid > (long long)cus * occ) grid = (long long)cus * occ;
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), 0, s, static_cast<const Raw<CS16> *>(d_iq), d_psd, d_win,
                       t.post8192, nitems, nrows, stride, hop, fpr, scale);
    return hipGetLastError();
}

template <int n>
hipError_t launch_fmt(const KernelTables &t, const void *d_iq, int cs16, long long nitems, int nrows, size_t stride,
                      size_t hop, int fpr, float *d_psd, const float *d_win, float scale, int max_wgs, int device,
                      hipStream_t s)
{
    if (cs16)
        return d_win ? launch_n<n, true, true>(t, d_iq, nitems, nrows, stride, hop, fpr, d_psd, d_win, scale, max_wgs, device, s)
                     : launch_n<n, true, false>(t, d_iq, nitems, nrows, stride, hop, fpr, d_psd, d_win, scale, max_wgs, device, s);
    return d_win ? launch_n<n, false, true>(t, d_iq, nitems, nrows, stride, hop, fpr, d_psd, d_win, scale, max_wgs, device, s)
                 : launch_n<n, false, false>(t, d_iq, nitems, nrows, stride, hop, fpr, d_psd, d_win, scale, max_wgs, device, s);
}

}  // namespace

hipError_t launch_channel_spectrum(const KernelTables &t, const void *d_iq, int cs16, int nch, int nrows,
                                   size_t stride_samples, int n, int hop, int fpr, float *d_psd,
                                   const float *d_window, float scale, int max_wgs, int device, hipStream_t s)
{
    if (!d_iq || !d_psd || nch < 1 || nrows < 1 || hop < 1 || fpr < 1) return hipErrorInvalidValue;
    const long long nitems = (long long)nch * nrows;
    if (nitems > 0x7fffffffLL) return hipErrorInvalidValue;
    switch (n) {
    case 256: return launch_fmt<256>(t, d_iq, cs16, nitems, nrows, stride_samples, (size_t)hop, fpr, d_psd, d_window, scale, max_wgs, device, s);
    case 512: return launch_fmt<512>(t, d_iq, cs16, nitems, nrows, stride_samples, (size_t)hop, fpr, d_psd, d_window, scale, max_wgs, device, s);
    case 1024: return launch_fmt<1024>(t, d_iq, cs16, nitems, nrows, stride_samples, (size_t)hop, fpr, d_psd, d_window, scale, max_wgs, device, s);
    case 2048: return launch_fmt<2048>(t, d_iq, cs16, nitems, nrows, stride_samples, (size_t)hop, fpr, d_psd, d_window, scale, max_wgs, device, s);
    case 4096: return launch_fmt<4096>(t, d_iq, cs16, nitems, nrows, stride_samples, (size_t)hop, fpr, d_psd, d_window, scale, max_wgs, device, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace sddc
