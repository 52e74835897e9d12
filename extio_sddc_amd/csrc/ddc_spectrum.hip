// ddc_spectrum.hip — the wideband averaged power spectrum of the ADC stream for gfx950
// (sddc_ddc_spectrum_device): the DDC's own frames as a Welch schedule, 8192-sample frames at
// hop 6144, 11 per input block.
//
// Per frame (the forward side of ddc_persistent.hip at d = 0, without rotation or pruning):
//   convert (+ rand) x window -> Z = FFT4096(x[2j] + i x[2j+1]) (3 radix-16 LDS passes)
//   -> the plain r2c split of the pair (k, 4096 - k):
//        A = Zk + conj Zc,  B = -i W^k (Zk - conj Zc)   (Zc = Z[4096 - k], W = e^{-2 pi i / 8192})
//        |X[k]|^2 = 1/4 |A + B|^2,   |X[4096 - k]|^2 = 1/4 |A - B|^2
//      (k = 0 gives bins 0 and 4096, the Nyquist bin, which is not output; bin 2048 is its own
//      mirror, X[2048] = conj Z[2048]), accumulated in registers.
// The (P, r) form of the DDC's split is not used: its r = cot(pi/4 - pi k / 8192) grows without
// bound towards bin 2048 and amplifies every error of its table by as much, so the DDC builds it
// from W in double (split_coeffs.h), not from the float post8192 table read here; the plain split
// below does not amplify that table's rounding, and there is no filter to fold into P here.
//
// Work item: one input block, its 11 frames summed in frame order by one workgroup.  Thread t owns
// the pairs k = t + 256 r (r < 8): 16 sums per thread, bins k and 4096 - k (thread 0 holds bin 2048
// in the place of bin 4096).  With one block per row the workgroup scales and stores the row;
// otherwise it stores the unscaled sums of its block to partial[block][4096] and
// spectrum_reduce_kernel adds each row's blocks in block order.  Every sum is a fixed sequence of
// float operations given by the frame's place in its block and the block's place in its row: the
// grid, the CU count and the workgroup that ran an item do not enter, and there are no atomics.
#include <hip/hip_runtime.h>

#include "ddc_frame_common.hpp"

namespace sddc {
namespace {

constexpr int PAIRS = 8;   // (k, 4096 - k) pairs per thread: k = t + 256 r, r < 8

// WIN: multiply by the window (the thread's 32 values, held in registers for the launch); the
// rectangular instance skips the multiply and keeps the int16 -> float conversion exact.
template <bool RAND, bool WIN>
__global__ __launch_bounds__(NT, 3) void spectrum_kernel(
    const int *__restrict__ in32, float *__restrict__ out, int nblk, const float2 *__restrict__ tw_p1,
    const float2 *__restrict__ tw4096, const float2 *__restrict__ post8192, const float2 *__restrict__ win,
    float scale)
{
    __shared__ __attribute__((aligned(16))) float2 lds[HALF];
    __shared__ __attribute__((aligned(16))) float2 twl[15 * 16];   // pass-1 twiddles W_256^{s r}
    const int tid = (int)threadIdx.x;
    const int G = (int)gridDim.x;

    // per-thread constants, live for the whole launch: forward pass 2's anchors W_4096^{t m}
    // (twiddle_anchor6), the split twiddles W_8192^{t + 256 r} and the window of the thread's
    // sample pairs t + 256 r
    const float2 fw1_ = tw4096[tid], fw2_ = tw4096[2 * tid], fw3_ = tw4096[3 * tid];
    const float2 fw4_ = tw4096[(4 * tid) & (HALF - 1)], fw8_ = tw4096[(8 * tid) & (HALF - 1)];
    const float2 fw12_ = tw4096[(12 * tid) & (HALF - 1)];
    float2 pw[PAIRS];
#pragma unroll
    for (int r = 0; r < PAIRS; r++) pw[r] = post8192[tid + NT * r];
    float2 wn[WIN ? 16 : 1];
    if constexpr (WIN) {
#pragma unroll
        for (int r = 0; r < 16; r++) wn[r] = win[tid + NT * r];
    }
    if (tid < 15 * 16) twl[tid] = tw_p1[tid];   // visible after the first frame's pass-0 barrier

    int blk = (int)blockIdx.x, k = 0;   // grid <= nblk: every workgroup has an item
    int x[16];
    load_frame(in32, blk, k, x);
    float accp[PAIRS], accm[PAIRS];   // bins t + 256 r and 4096 - (t + 256 r)
#pragma unroll
    for (int r = 0; r < PAIRS; r++) accp[r] = accm[r] = 0.f;

    for (;;) {
        // the frame after this one: the next of the block, or frame 0 of the workgroup's next item
        const int kn = k + 1 < FRAMES ? k + 1 : 0;
        const int bn = k + 1 < FRAMES ? blk : blk + G;
        // Opaque per-iteration copies (ddc_persistent.hip): without them the compiler hoists the
        // loop-invariant LDS addresses out of the frame loop and spills them.
        int z = 0;
        asm volatile("" : "+s"(z));
        const int t = tid + z;
        float2 fw1 = fw1_, fw2 = fw2_, fw3 = fw3_, fw4 = fw4_, fw8 = fw8_, fw12 = fw12_;
        asm volatile("" : "+v"(fw1), "+v"(fw2), "+v"(fw3), "+v"(fw4), "+v"(fw8), "+v"(fw12));
        const int sT = swz(t);   // swz(t + 256 r) = sT + 256 r
        const int x15 = t & 15;
        // ---- forward pass 0 (R16, NS1): convert, window, DFT16 from registers ----
        float2 v[16];
        {
            float2 a[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                int w = x[r];
                // convert_float<rand> on the int16 pair: an odd sample is XORed with 0xFFFE
                if constexpr (RAND) w ^= (int)(((unsigned)w & 0x10001u) * 0xFFFEu);
                a[r] = make_float2((float)(int)(short)(w & 0xffff), (float)(w >> 16));
                if constexpr (WIN) a[r] = make_float2(a[r].x * wn[r].x, a[r].y * wn[r].y);
            }
            if (bn < nblk) load_frame(in32, bn, kn, x);   // prefetch
            dft16<-1>(a, v);
        }
        __syncthreads();   // the previous frame's mirror reads are done
#pragma unroll
        for (int r = 0; r < 16; r++) lds[16 * t + (r ^ x15)] = v[r];   // swz(16 t + r)
        __syncthreads();
        // ---- forward pass 1 (R16, NS16): table twiddles W_256^{(t % 16) r} ----
        {
            float2 a[16];
#pragma unroll
            for (int r = 0; r < 16; r++) XRD(a[r], lds[sT + NT * r]);
            table_twiddle<-1, false>(a, twl, 16, x15);
            dft16<-1>(a, v);
        }
        __syncthreads();
        {
            const int b1 = (t >> 4) * 256;   // swz(b1 + x15 + 16 r)
#pragma unroll
            for (int r = 0; r < 16; r++) lds[b1 + 16 * r + (x15 ^ r)] = v[r];
        }
        __syncthreads();
        // ---- forward pass 2 (R16, NS256): anchor twiddles W_4096^{t r}; v[r] = Z[t + 256 r] ----
        {
            float2 a[16];
#pragma unroll
            for (int r = 0; r < 16; r++) XRD(a[r], lds[sT + NT * r]);
            twiddle_anchor6<-1>(a, fw1, fw2, fw3, fw4, fw8, fw12);
            dft16<-1>(a, v);
        }
        __syncthreads();
        // Z in natural order, bin j at j: the mirrors 4096 - k of k < 2048 are the bins of
        // registers 8..15, and bin 0 (the mirror of k = 0)
        lds[t] = v[0];
#pragma unroll
        for (int r = 8; r < 16; r++) lds[t + NT * r] = v[r];
        __syncthreads();
        // ---- split, |X|^2, accumulate ----
        {
            const float2 zn = lds[HALF / 2];   // bin 2048 (every lane reads it: a broadcast)
#pragma unroll
            for (int r = 0; r < PAIRS; r++) {
                const float2 zk = v[r];
                const float2 zc = lds[(HALF - t - NT * r) & (HALF - 1)];
                const float ax = zk.x + zc.x, ay = zk.y - zc.y;   // A = Zk + conj Zc
                const float dx = zk.x - zc.x, dy = zk.y + zc.y;   // D = Zk - conj Zc
                const float2 wd = cmul(make_float2(dx, dy), pw[r]);
                const float bx = wd.y, by = -wd.x;                // B = -i W^k D
                const float px = ax + bx, py = ay + by, mx = ax - bx, my = ay - by;
                accp[r] = fmaf(px, px, fmaf(py, py, accp[r]));
                float m2x = mx, m2y = my;
                if (r == 0 && t == 0) {   // bin 2048 in the place of bin 4096: 4 |Z[2048]|^2
                    m2x = 2.f * zn.x;
                    m2y = 2.f * zn.y;
                }
                accm[r] = fmaf(m2x, m2x, fmaf(m2y, m2y, accm[r]));
            }
        }
        if (kn == 0) {
            // the block's 11 frames are summed: bins t + 256 r ascending, 4096 - t - 256 r descending
            // (thread 0's r = 0: bin 2048); 4 bytes per lane, whole lines per wave
            const __amdgpu_buffer_rsrc_t ro = buf_rsrc(out + (size_t)blk * HALF);
            const unsigned up = 4u * (unsigned)t, dn = 4u * (unsigned)(HALF - t);
#pragma unroll
            for (int r = 0; r < PAIRS; r++) {
                buf_store4<0>(__float_as_uint(accp[r] * scale), ro, up, 4u * NT * r);
                const unsigned m = r == 0 && t == 0 ? 4u * (HALF / 2) : dn - 4u * NT * r;   // <= 4 * 4095
                buf_store4<0>(__float_as_uint(accm[r] * scale), ro, m, 0u);
                accp[r] = accm[r] = 0.f;
            }
        }
        if (bn >= nblk) break;
        blk = bn;
        k = kn;
    }
}

// psd[row][bin] = scale * (partial[row bpr][bin] + ... + partial[row bpr + bpr - 1][bin]), summed
// in block order within S = min(bpr, 16) runs of ceil(bpr / S) consecutive blocks, then the runs in
// order: a fixed sequence given by bpr alone.  One workgroup of S waves per (row, 256 bins): wave s
// sums run s, 4 bins per lane; wave 0 adds the runs and stores (4-byte stores: the caller's psd is
// only 4-byte aligned).
constexpr int kReduceRuns = 16;
__global__ __launch_bounds__(64 * kReduceRuns) void spectrum_reduce_kernel(const float4 *__restrict__ partial,
                                                                           float *__restrict__ psd, int bpr,
                                                                           float scale)
{
    __shared__ float4 sums[kReduceRuns][64];
    const int S = (int)blockDim.x >> 6, s = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const size_t row = blockIdx.x / (HALF / 256);
    const int q = (int)(blockIdx.x % (HALF / 256)) * 64 + lane;   // float4 index in the row
    const int per = (bpr + S - 1) / S;
    const int b0 = s * per, b1 = min(bpr, b0 + per);
    const float4 *p = partial + row * (size_t)bpr * (HALF / 4) + q;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 < b1) a = p[(size_t)b0 * (HALF / 4)];
    for (int b = b0 + 1; b < b1; b++) {
        const float4 u = p[(size_t)b * (HALF / 4)];
        a.x += u.x;
        a.y += u.y;
        a.z += u.z;
        a.w += u.w;
    }
    sums[s][lane] = a;
    __syncthreads();
    if (s != 0) return;
    for (int r = 1; r < S; r++) {
        if (r * per >= bpr) break;   // an empty run
        const float4 u = sums[r][lane];
        a.x += u.x;
        a.y += u.y;
        a.z += u.z;
        a.w += u.w;
    }
    float *o = psd + row * HALF + 4 * (size_t)q;
    o[0] = a.x * scale;
    o[1] = a.y * scale;
    o[2] = a.z * scale;
    o[3] = a.w * scale;
}

template <bool RAND, bool WIN>
hipError_t launch_s(const KernelTables &t, const int16_t *d_in, int nblk, float *d_out, const float2 *d_win,
                    float scale, int max_wgs, int device, hipStream_t s)
{
    auto kern = spectrum_kernel<RAND, WIN>;
    int occ = 0, cus = 0;
    hipError_t e = launch_geometry(t.lc, reinterpret_cast<const void *>(kern), NT, device, &occ, &cus);
    if (e != hipSuccess) return e;
    int grid = cus * occ;
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    if (grid > nblk) grid = nblk;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), 0, s, reinterpret_cast<const int *>(d_in), d_out, nblk,
                       t.tw_p1, t.tw4096, t.post8192, d_win, scale);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_spectrum(const KernelTables &t, const int16_t *d_in, int nblk, float *d_out, const float *d_window,
                           float scale, int rand, int max_wgs, int device, hipStream_t s)
{
    if (nblk <= 0 || !d_in || !d_out) return hipErrorInvalidValue;
    const float2 *w = reinterpret_cast<const float2 *>(d_window);
    if (w) return rand ? launch_s<true, true>(t, d_in, nblk, d_out, w, scale, max_wgs, device, s)
                       : launch_s<false, true>(t, d_in, nblk, d_out, w, scale, max_wgs, device, s);
    return rand ? launch_s<true, false>(t, d_in, nblk, d_out, w, scale, max_wgs, device, s)
                : launch_s<false, false>(t, d_in, nblk, d_out, w, scale, max_wgs, device, s);
}

hipError_t launch_spectrum_reduce(const float *d_partial, int rows, int blocks_per_row, float scale, float *d_psd,
                                  hipStream_t s)
{
    if (rows <= 0 || blocks_per_row <= 0 || !d_partial || !d_psd) return hipErrorInvalidValue;
    const int runs = blocks_per_row < kReduceRuns ? blocks_per_row : kReduceRuns;
    hipLaunchKernelGGL(spectrum_reduce_kernel, dim3((unsigned)rows * (HALF / 256)), dim3(64u * (unsigned)runs), 0, s,
                       reinterpret_cast<const float4 *>(d_partial), d_psd, blocks_per_row, scale);
    return hipGetLastError();
}

}  // namespace sddc
