// r2iq_cpu.cpp — the CPU r2iq backend (r2iq_cpu.h), AVX2 + FMA.
//
// Built with -ffp-contract=off: every fused multiply-add below is an explicit intrinsic, and
// the fine-tune NCO's scalar mix keeps pf_mixer's float operation order (fine_tune.h), so
// its output is bit-identical to the GPU output stage's.
#include "r2iq_cpu.h"

#include <immintrin.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

namespace sddc {
namespace cpu {
namespace {

constexpr int kHalf = 4096;     // halfFft           fft_mt_r2iq.h:18
constexpr int kBlock = 65536;   // transferSamples   config.h:80-81
constexpr int kHop = 6144;      // 3 halfFft / 2     impl.hpp:88
constexpr int kFrames = 11;     // fftPerBuf         fft_mt_r2iq.h:19

template <class T>
struct Aligned {
    T *p = nullptr;
    explicit Aligned(size_t n)
    {
        p = static_cast<T *>(std::aligned_alloc(64, ((n * sizeof(T) + 63) / 64) * 64));
        if (!p) throw std::bad_alloc();
        std::memset(p, 0, n * sizeof(T));
    }
    ~Aligned() { std::free(p); }
    Aligned(const Aligned &) = delete;
    Aligned &operator=(const Aligned &) = delete;
};

// 8 lanes reversed
inline __m256 reverse8(__m256 v) { return _mm256_permutevar8x32_ps(v, _mm256_setr_epi32(7, 6, 5, 4, 3, 2, 1, 0)); }

}  // namespace

bool supported()
{
    __builtin_cpu_init();
    return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
}

struct R2iq::Buf {
    Aligned<int16_t> hist{kHalf}, frame0{2 * kHalf};
    // Z = forward output (+ Z[4096] = Z[0], so the mirror index 4096 - j needs no wrap)
    Aligned<float> ar{kHalf + 8}, ai{kHalf + 8}, br{kHalf + 8}, bi{kHalf + 8};
    Aligned<float> pr{kHalf}, pi{kHalf}, qr{kHalf}, qi{kHalf};
    Aligned<float> stage{(size_t)2 * 8 * kHalf};   // one block of CF32 output (NCO / CS16 path)
};

R2iq::R2iq(const std::complex<double> *H) : b_(new Buf), fwd_(kHalf), H_(H, H + 7 * kHalf)
{
    for (int d = 0; d < 7; d++) inv_.emplace_back(new FftPlan(kHalf >> d));
}

R2iq::~R2iq() = default;

void R2iq::reset() { std::memset(b_->hist.p, 0, kHalf * sizeof(int16_t)); }

void R2iq::set_history(const int16_t *last) { std::memcpy(b_->hist.p, last, kHalf * sizeof(int16_t)); }

// (P, Q) of (d, tb): the split x filter coefficients of every inverse-input bin m, and the
// two valid m ranges of the reference's shift with zero fill (impl.hpp:76-96):
//   [0, count)            j = tb + m,          count = min(mfft/2, 4096 - tb)
//   [mfft/2 + start, mfft) j = tb - mfft + m,  start = max(0, mfft/2 - tb)
void R2iq::build_pq(int d, int tb)
{
    if (d == pq_d_ && tb == pq_tb_) return;
    const int mfft = kHalf >> d, half = mfft / 2;
    const int count = std::min(half, kHalf - tb), start = std::max(0, half - tb);
    lo_ = count;
    hi_ = half + start;
    const std::complex<double> *Hd = H_.data() + (size_t)d * kHalf;
    for (int m = 0; m < mfft; m++) {
        const bool ok = m < count || m >= half + start;
        std::complex<double> P = 0, Q = 0;
        if (ok) {
            const int j = m < half ? tb + m : tb - mfft + m;
            const std::complex<double> h = 0.5 * Hd[m < half ? m : kHalf - mfft + m];   // filter2, impl.hpp:7
            const double a = -2.0 * M_PI * j / (2.0 * kHalf);
            const std::complex<double> iw(-std::sin(a), std::cos(a));                  // i W_8192^j
            P = h * (1.0 - iw);
            Q = h * (1.0 + iw);
        }
        b_->pr.p[m] = (float)P.real();
        b_->pi.p[m] = (float)P.imag();
        b_->qr.p[m] = (float)Q.real();
        b_->qi.p[m] = (float)Q.imag();
    }
    pq_d_ = d;
    pq_tb_ = tb;
}

// One 8192-sample frame x -> y = IFFT_mfft(T) (mfft = 4096 >> d); *yr, *yi point at y
// (in the work buffers, valid until the next frame).
void R2iq::frame(const int16_t *x, int d, bool rand, const float **yr, const float **yi)
{
    Buf &B = *b_;
    // ---- Z = FFT4096 of x[2n] + i x[2n+1] (the r2c 8192 before its split, impl.hpp:88), the
    // int16 -> float conversion (+ rand, fft_mt_r2iq.h:36-51) done by the first pass ----
    float *zr = B.ar.p, *zi = B.ai.p;
    if (fwd_.forward_i16(x, rand, B.ar.p, B.ai.p, B.br.p, B.bi.p)) {
        zr = B.br.p;
        zi = B.bi.p;
    }
    zr[kHalf] = zr[0];
    zi[kHalf] = zi[0];
    // ---- T[m] = Z_j P[m] + conj(Z_-j) Q[m] on the two valid ranges, 0 elsewhere ----
    const int mfft = kHalf >> d;
    float *tr = zr == B.ar.p ? B.br.p : B.ar.p, *ti = zr == B.ar.p ? B.bi.p : B.ai.p;
    const int tb = pq_tb_;
    auto run = [&](int m0, int m1, int joff) {   // j = m + joff
        int m = m0;
        for (; m + 8 <= m1; m += 8) {
            const int j = m + joff;
            const __m256 ajr = _mm256_loadu_ps(zr + j), aji = _mm256_loadu_ps(zi + j);
            const __m256 bmr = reverse8(_mm256_loadu_ps(zr + kHalf - j - 7));
            const __m256 bmi = reverse8(_mm256_loadu_ps(zi + kHalf - j - 7));
            const __m256 Pr = _mm256_loadu_ps(B.pr.p + m), Pi = _mm256_loadu_ps(B.pi.p + m);
            const __m256 Qr = _mm256_loadu_ps(B.qr.p + m), Qi = _mm256_loadu_ps(B.qi.p + m);
            // Re = ajr Pr - aji Pi + bmr Qr + bmi Qi;  Im = ajr Pi + aji Pr + bmr Qi - bmi Qr
            __m256 re = _mm256_mul_ps(ajr, Pr);
            re = _mm256_fnmadd_ps(aji, Pi, re);
            re = _mm256_fmadd_ps(bmr, Qr, re);
            re = _mm256_fmadd_ps(bmi, Qi, re);
            __m256 im = _mm256_mul_ps(ajr, Pi);
            im = _mm256_fmadd_ps(aji, Pr, im);
            im = _mm256_fmadd_ps(bmr, Qi, im);
            im = _mm256_fnmadd_ps(bmi, Qr, im);
            _mm256_storeu_ps(tr + m, re);
            _mm256_storeu_ps(ti + m, im);
        }
        for (; m < m1; m++) {
            const int j = m + joff;
            const float a_r = zr[j], a_i = zi[j], b_r = zr[kHalf - j], b_i = zi[kHalf - j];
            const float *P_r = B.pr.p, *P_i = B.pi.p, *Q_r = B.qr.p, *Q_i = B.qi.p;
            tr[m] = a_r * P_r[m] - a_i * P_i[m] + b_r * Q_r[m] + b_i * Q_i[m];
            ti[m] = a_r * P_i[m] + a_i * P_r[m] + b_r * Q_i[m] - b_i * Q_r[m];
        }
    };
    run(0, lo_, tb);
    std::memset(tr + lo_, 0, (size_t)(hi_ - lo_) * sizeof(float));
    std::memset(ti + lo_, 0, (size_t)(hi_ - lo_) * sizeof(float));
    run(hi_, mfft, tb - mfft);
    // ---- y = IFFT_mfft(T) (impl.hpp:98) ----
    float *wr = tr == B.ar.p ? B.br.p : B.ar.p, *wi = tr == B.ar.p ? B.bi.p : B.ai.p;
    const bool w = inv_[d]->backward(tr, ti, wr, wi) != 0;
    *yr = w ? wr : tr;
    *yi = w ? wi : ti;
}

void R2iq::process(const int16_t *const *blocks, int nblk, void *out, const Params &p)
{
    Buf &B = *b_;
    const int d = p.d, mfft = kHalf >> d, half = mfft / 2, keep = 3 * mfft / 4;
    build_pq(d, p.tunebin);
    const bool post = p.cs16 || p.nco_trig;
    const size_t per_blk = (size_t)8 * mfft;   // complex outputs per block
    const __m256 sgn = _mm256_castsi256_ps(_mm256_set1_epi32(p.lsb ? (int)0x80000000 : 0));
    for (int b = 0; b < nblk; b++) {
        const int16_t *blk = blocks[b];
        float *o = post ? B.stage.p : static_cast<float *>(out) + 2 * per_blk * b;
        for (int k = 0; k < kFrames; k++) {
            const int16_t *x;
            if (k == 0) {   // [history | block[0, 4096)]
                std::memcpy(B.frame0.p, B.hist.p, kHalf * sizeof(int16_t));
                std::memcpy(B.frame0.p + kHalf, blk, kHalf * sizeof(int16_t));
                x = B.frame0.p;
            } else {
                x = blk + kHop * k - kHalf;
            }
            const float *yr, *yi;
            frame(x, d, p.rand, &yr, &yi);
            // ---- overlap-discard + sideband (impl.hpp:117-138, fft_mt_r2iq.h:63-81) ----
            const int i0 = k == 0 ? mfft / 4 : 0, n = k == 0 ? half : keep;
            float *dst = o + 2 * (k == 0 ? 0 : half + (size_t)keep * (k - 1));
            for (int i = 0; i < n; i += 8) {
                const __m256 re = _mm256_loadu_ps(yr + i0 + i);
                const __m256 im = _mm256_xor_ps(_mm256_loadu_ps(yi + i0 + i), sgn);
                const __m256 lo = _mm256_unpacklo_ps(re, im), hi = _mm256_unpackhi_ps(re, im);
                _mm256_storeu_ps(dst + 2 * i, _mm256_permute2f128_ps(lo, hi, 0x20));
                _mm256_storeu_ps(dst + 2 * i + 8, _mm256_permute2f128_ps(lo, hi, 0x31));
            }
        }
        std::memcpy(B.hist.p, blk + kBlock - kHalf, kHalf * sizeof(int16_t));
        if (!post) continue;
        // ---- fused fine-tune NCO (pf_mixer.cpp:808-833 order) and CS16 ----
        float *s = B.stage.p;
        if (p.nco_trig) {
            for (size_t i = 0; i < per_blk; i++) {
                const size_t ot = per_blk * b + i;   // sample index in this call's output
                const float *sb = p.nco_starts + 2 * ((ot >> 7) * 4 + (ot & 3));
                const int q = (int)((ot >> 2) & 31);
                float px = sb[0], py = sb[1];
                if (q) {
                    const float *tq = p.nco_trig + 2 * (q - 1);
                    px = tq[0] * sb[0] - tq[1] * sb[1];
                    py = tq[1] * sb[0] + tq[0] * sb[1];
                }
                const float vx = s[2 * i], vy = s[2 * i + 1];
                s[2 * i] = vx * px - vy * py;
                s[2 * i + 1] = vy * px + vx * py;
            }
        }
        if (p.cs16) {
            int16_t *c = static_cast<int16_t *>(out) + 2 * per_blk * b;
            for (size_t i = 0; i < 2 * per_blk; i++) {
                float v = std::nearbyint(s[i] * p.scale);   // round half even (default mode)
                v = std::min(std::max(v, -32768.f), 32767.f);
                c[i] = (int16_t)v;
            }
        } else {
            std::memcpy(static_cast<float *>(out) + 2 * per_blk * b, s, 2 * per_blk * sizeof(float));
        }
    }
}

// The averaged power spectrum (sddc_ddc_spectrum_host on a CPU handle): per frame the windowed
// samples as x[2j] + i x[2j+1] through the forward plan, the plain r2c split
//   A = Zk + conj Zc, B = -i W^k (Zk - conj Zc), |X[k]|^2 = |A + B|^2 / 4, |X[4096 - k]|^2 = |A - B|^2 / 4
// and a float sum per bin over the row's frames in frame order, scaled once at the end.
void R2iq::spectrum(const int16_t *in, int nblk, int bpr, const float *w, float scale, bool rand, float *psd)
{
    Buf &B = *b_;
    if (sw_.empty()) {
        sw_.resize(2 * (size_t)(kHalf / 2 + 1));
        for (int k = 0; k <= kHalf / 2; k++) {
            const double a = -2.0 * M_PI * k / (2.0 * kHalf);
            sw_[2 * (size_t)k] = (float)std::cos(a);
            sw_[2 * (size_t)k + 1] = (float)std::sin(a);
        }
    }
    std::vector<float> acc(kHalf);
    const float s4 = 0.25f * scale;
    for (int row = 0; row < nblk / bpr; row++) {
        std::fill(acc.begin(), acc.end(), 0.f);
        for (int f = 0; f < bpr * kFrames; f++) {
            const int16_t *x = in + (size_t)(row * bpr + f / kFrames) * kBlock + (size_t)(f % kFrames) * kHop;
            float *re = B.ar.p, *im = B.ai.p;
            for (int j = 0; j < kHalf; j++) {
                int a = x[2 * j], b = x[2 * j + 1];
                if (rand) {   // fft_mt_r2iq.h:36-51: an odd sample is XORed with 0xFFFE (its negation)
                    a = (a & 1) ? -a : a;
                    b = (b & 1) ? -b : b;
                }
                re[j] = w ? w[2 * j] * (float)a : (float)a;
                im[j] = w ? w[2 * j + 1] * (float)b : (float)b;
            }
            if (fwd_.forward(B.ar.p, B.ai.p, B.br.p, B.bi.p)) {
                re = B.br.p;
                im = B.bi.p;
            }
            // k = 0: X[0] = Re Z0 + Im Z0; k = 2048: X = conj Z[2048]
            acc[0] += 4.f * (re[0] + im[0]) * (re[0] + im[0]);
            acc[kHalf / 2] += 4.f * (re[kHalf / 2] * re[kHalf / 2] + im[kHalf / 2] * im[kHalf / 2]);
            for (int k = 1; k < kHalf / 2; k++) {
                const float zkx = re[k], zky = im[k], zcx = re[kHalf - k], zcy = im[kHalf - k];
                const float ax = zkx + zcx, ay = zky - zcy, dx = zkx - zcx, dy = zky + zcy;
                const float wx = sw_[2 * (size_t)k], wy = sw_[2 * (size_t)k + 1];
                const float bx = wx * dy + wy * dx, by = -(wx * dx - wy * dy);   // B = -i W D
                const float px = ax + bx, py = ay + by, mx = ax - bx, my = ay - by;
                acc[k] += px * px + py * py;
                acc[kHalf - k] += mx * mx + my * my;
            }
        }
        for (int k = 0; k < kHalf; k++) psd[(size_t)row * kHalf + k] = acc[k] * s4;
    }
}

// The channel spectrum (sddc_ddc_channel_spectrum_host on a CPU handle): per frame the windowed
// samples through the n-point forward plan, |X|^2 added per bin in frame order (plain float
// multiplies and adds: contraction is off), one scale and the n/2 rotation at the end.
void R2iq::channel_spectrum(const void *iq, bool cs16, int nch, size_t stride, int n, int hop, int fpr, int nrows,
                            const float *w, float scale, float *psd)
{
    Buf &B = *b_;   // n <= 4096: the frame buffers hold it
    const FftPlan *plan = nullptr;
    for (const auto &p : csp_)
        if (p->size() == n) plan = p.get();
    if (!plan) {
        csp_.emplace_back(new FftPlan(n));
        plan = csp_.back().get();
    }
    std::vector<float> acc((size_t)n);
    for (int c = 0; c < nch; c++) {
        for (int row = 0; row < nrows; row++) {
            std::fill(acc.begin(), acc.end(), 0.f);
            for (int f = 0; f < fpr; f++) {
                const size_t start = (size_t)c * stride + ((size_t)row * (size_t)fpr + (size_t)f) * (size_t)hop;
                float *re = B.ar.p, *im = B.ai.p;
                if (cs16) {
                    const int16_t *x = static_cast<const int16_t *>(iq) + 2 * start;
                    for (int j = 0; j < n; j++) {
                        re[j] = w ? w[j] * (float)x[2 * j] : (float)x[2 * j];
                        im[j] = w ? w[j] * (float)x[2 * j + 1] : (float)x[2 * j + 1];
                    }
                } else {
                    const float *x = static_cast<const float *>(iq) + 2 * start;
                    for (int j = 0; j < n; j++) {
                        re[j] = w ? w[j] * x[2 * j] : x[2 * j];
                        im[j] = w ? w[j] * x[2 * j + 1] : x[2 * j + 1];
                    }
                }
                if (plan->forward(B.ar.p, B.ai.p, B.br.p, B.bi.p)) {
                    re = B.br.p;
                    im = B.bi.p;
                }
                for (int k = 0; k < n; k++) acc[(size_t)k] += re[k] * re[k] + im[k] * im[k];
            }
            float *out = psd + ((size_t)c * (size_t)nrows + (size_t)row) * (size_t)n;
            for (int q = 0; q < n; q++) out[q] = acc[(size_t)((q + n / 2) & (n - 1))] * scale;
        }
    }
}

// The channel stream stages (sddc_ddc_channel_{decimate,resample}_host on a CPU handle) share three
// steps.  split_stream: per channel the stream [tail | the call's samples] is split into I and Q
// rows.  dot_iq (the resampler; the decimator's dot_iq_phases follows the device's order instead): an
// output is the dot product of n reversed taps with n consecutive values of the
// rows: eight lane sums of explicit FMAs over k = 8 i + lane, added in a fixed tree, then the last
// n mod 8 taps one by one.  keep_tail: the last H values of the rows are the next call's tail.
// The order depends on the tap index alone, so any cut of a stream into calls gives the same bits.
static inline float hsum8(__m256 v)
{
    const __m128 s4 = _mm_add_ps(_mm256_castps256_ps128(v), _mm256_extractf128_ps(v, 1));
    const __m128 s2 = _mm_add_ps(s4, _mm_movehl_ps(s4, s4));
    return _mm_cvtss_f32(_mm_add_ss(s2, _mm_shuffle_ps(s2, s2, 1)));
}

// x: the channel's first component of the call; tl: its H kept values; xr, xi: H + nsamp floats each
static void split_stream(const void *x, bool cs16, float inv_s, size_t nsamp, const float *tl, size_t H, float *xr,
                         float *xi)
{
    for (size_t k = 0; k < H; k++) {
        xr[k] = tl[2 * k];
        xi[k] = tl[2 * k + 1];
    }
    if (cs16) {
        const int16_t *v = static_cast<const int16_t *>(x);
        for (size_t i = 0; i < nsamp; i++) {
            xr[H + i] = (float)v[2 * i] * inv_s;
            xi[H + i] = (float)v[2 * i + 1] * inv_s;
        }
    } else {
        const float *v = static_cast<const float *>(x);
        for (size_t i = 0; i < nsamp; i++) {
            xr[H + i] = v[2 * i];
            xi[H + i] = v[2 * i + 1];
        }
    }
}

static inline void dot_iq(const float *g, const float *pr, const float *pi, int n, float *y)
{
    __m256 ar = _mm256_setzero_ps(), ai = _mm256_setzero_ps();
    int k = 0;
    for (; k + 8 <= n; k += 8) {
        const __m256 gv = _mm256_loadu_ps(g + k);
        ar = _mm256_fmadd_ps(gv, _mm256_loadu_ps(pr + k), ar);
        ai = _mm256_fmadd_ps(gv, _mm256_loadu_ps(pi + k), ai);
    }
    float sr = hsum8(ar), si = hsum8(ai);
    for (; k < n; k++) {
        sr = std::fmaf(g[k], pr[k], sr);
        si = std::fmaf(g[k], pi[k], si);
    }
    y[0] = sr;
    y[1] = si;
}

static void keep_tail(const float *xr, const float *xi, size_t nsamp, size_t H, float *tl)
{
    for (size_t k = 0; k < H; k++) {   // the last H values of [tail | samples]
        tl[2 * k] = xr[nsamp + k];
        tl[2 * k + 1] = xi[nsamp + k];
    }
}

// The channel decimator: output m is the dot product of the reversed taps g[k] = h[L - k] with the
// ntaps values w[k] from sample m R on, added in the device kernel's order (ddc_channel_decimate.hip):
// with k = q R + r, a[q mod 4] = fma(g[k], w[k], a[q mod 4]) for r = 0 .. R - 1, q = 0, 1, ..., and
// y = (a0 + a1) + (a2 + a3).  The same correctly rounded operations on the same floats: a CPU handle
// and a GPU handle produce the same bits.
static inline void dot_iq_phases(const float *g, const float *pr, const float *pi, int n, int R, float *y)
{
    float ar[4] = {0.f, 0.f, 0.f, 0.f}, ai[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < R && r < n; r++) {
        int q = 0;
        for (int k = r; k < n; k += R, q++) {
            ar[q & 3] = std::fmaf(g[k], pr[k], ar[q & 3]);
            ai[q & 3] = std::fmaf(g[k], pi[k], ai[q & 3]);
        }
    }
    y[0] = (ar[0] + ar[1]) + (ar[2] + ar[3]);
    y[1] = (ai[0] + ai[1]) + (ai[2] + ai[3]);
}

void R2iq::channel_decimate(const void *iq, bool cs16, float inv_s, int nch, size_t nsamp, size_t in_stride,
                            const float *taps, int ntaps, int R, float *tail, float *out, size_t out_stride)
{
    const size_t L = (size_t)ntaps - 1, nout = nsamp / (size_t)R;
    std::vector<float> g((size_t)ntaps), xr(L + nsamp), xi(L + nsamp);
    for (int k = 0; k < ntaps; k++) g[(size_t)k] = taps[L - (size_t)k];
    for (int c = 0; c < nch; c++) {
        float *tl = tail + (size_t)c * L * 2;
        split_stream(static_cast<const char *>(iq) + (size_t)c * in_stride * (cs16 ? 2 : 4), cs16, inv_s, nsamp, tl, L,
                     xr.data(), xi.data());
        float *y = out + (size_t)c * out_stride;
        for (size_t m = 0; m < nout; m++)
            dot_iq_phases(g.data(), xr.data() + m * (size_t)R, xi.data() + m * (size_t)R, ntaps, R, y + 2 * m);
        keep_tail(xr.data(), xi.data(), nsamp, L, tl);
    }
}

// The channel resampler: output k of the call has e + k M = s L + p and is the dot product of phase
// p's reversed taps r_p[i] = h[p + (K - 1 - i) L] with the K values from sample s - (K - 1) on.  The
// order depends on (p, i, K) alone, so the position does not change the bits either.
void R2iq::channel_resample(const void *iq, bool cs16, float inv_s, int nch, size_t nsamp, size_t in_stride,
                            const float *taps, int ntaps, int L, int M, int e, size_t nout, float *tail, float *out,
                            size_t out_stride)
{
    const int K = (ntaps + L - 1) / L;
    const size_t H = (size_t)K - 1;
    std::vector<float> g((size_t)L * (size_t)K), xr(H + nsamp), xi(H + nsamp);
    for (int p = 0; p < L; p++)
        for (int i = 0; i < K; i++) {
            const int k = p + (K - 1 - i) * L;
            g[(size_t)p * (size_t)K + (size_t)i] = k < ntaps ? taps[k] : 0.f;
        }
    for (int c = 0; c < nch; c++) {
        float *tl = tail + (size_t)c * H * 2;
        split_stream(static_cast<const char *>(iq) + (size_t)c * in_stride * (cs16 ? 2 : 4), cs16, inv_s, nsamp, tl, H,
                     xr.data(), xi.data());
        float *y = out + (size_t)c * out_stride;
        uint64_t s = (uint64_t)e / (uint64_t)L;   // output k's sample and phase, stepped by M / L
        int p = e % L;
        const uint64_t ds = (uint64_t)(M / L);
        const int dp = M % L;
        for (size_t m = 0; m < nout; m++) {
            // row index H + s - (K - 1) = s
            dot_iq(g.data() + (size_t)p * (size_t)K, xr.data() + s, xi.data() + s, K, y + 2 * m);
            s += ds;
            p += dp;
            if (p >= L) {
                p -= L;
                s++;
            }
        }
        keep_tail(xr.data(), xi.data(), nsamp, H, tl);
    }
}

// The channel audio resampler: per channel the stream [tail | the call's sample values] as floats, and
// per output audio_resample_math.h's ars_dot on its phase's taps g[p][.] and its newest sample: scalar
// fmaf in the definition's four-sum order, the device kernel's sequence on the same floats.
void R2iq::channel_audio_resample(const void *in, bool in16, int nch, size_t nsamp, size_t in_stride, const float *taps,
                                  int ntaps, int L, int M, int e, size_t nout, float *tail, void *out, bool out16,
                                  size_t out_stride)
{
    const int K = (ntaps + L - 1) / L;
    const size_t H = (size_t)K - 1;
    std::vector<float> g((size_t)L * (size_t)K), x(H + nsamp);
    ars::ars_order_taps(taps, ntaps, L, g.data());
    const uint64_t ds = (uint64_t)(M / L);
    const int dp = M % L;
    for (int c = 0; c < nch; c++) {
        float *tl = tail + (size_t)c * H;
        std::copy(tl, tl + H, x.begin());
        if (in16) {
            const int16_t *v = static_cast<const int16_t *>(in) + (size_t)c * in_stride;
            for (size_t i = 0; i < nsamp; i++) x[H + i] = ars::ars_value(v[i]);
        } else {
            const float *v = static_cast<const float *>(in) + (size_t)c * in_stride;
            std::copy(v, v + nsamp, x.begin() + (ptrdiff_t)H);
        }
        float *yf = static_cast<float *>(out) + (size_t)c * out_stride;
        int16_t *ys = static_cast<int16_t *>(out) + (size_t)c * out_stride;
        uint64_t s = (uint64_t)e / (uint64_t)L;   // output k's sample and phase, stepped by M / L
        int p = e % L;
        for (size_t m = 0; m < nout; m++) {
            const float y = ars::ars_dot(g.data() + (size_t)p * (size_t)K, x.data() + H + s, K);
            if (out16) ys[m] = demod::demod_s16(y);
            else yf[m] = y;
            s += ds;
            p += dp;
            if (p >= L) {
                p -= L;
                s++;
            }
        }
        std::copy(x.end() - (ptrdiff_t)H, x.end(), tl);
    }
}

// The channel demodulator: demod_math.h's formulas sample by sample; the previous sample of the
// call's first one is the kept value, and the call's last sample value is kept for the next call.
void R2iq::channel_demodulate(const void *iq, bool cs16, float inv_s, int nch, size_t nsamp, size_t in_stride,
                              const ChDemChannel *chan, uint32_t pos, float *last, void *out, bool s16,
                              size_t out_stride, float *power)
{
    for (int c = 0; c < nch; c++) {
        const char *x = static_cast<const char *>(iq) + (size_t)c * in_stride * (cs16 ? 2 : 4);
        const int16_t *xs = reinterpret_cast<const int16_t *>(x);
        const float *xf = reinterpret_cast<const float *>(x);
        float *yf = static_cast<float *>(out) + (size_t)c * out_stride;
        int16_t *ys = static_cast<int16_t *>(out) + (size_t)c * out_stride;
        const ChDemChannel ch = chan[c];
        float Ip = last[2 * c], Qp = last[2 * c + 1], acc = 0.f;
        for (size_t i = 0; i < nsamp; i++) {
            const float I = cs16 ? (float)xs[2 * i] * inv_s : xf[2 * i];
            const float Q = cs16 ? (float)xs[2 * i + 1] * inv_s : xf[2 * i + 1];
            float y;
            if (ch.mode == 0) y = demod::demod_am(I, Q, ch.gain);
            else if (ch.mode == 1) y = demod::demod_fm(I, Q, Ip, Qp, ch.gain);
            else y = demod::demod_bfo(I, Q, ch.word * (pos + (uint32_t)i), ch.gain);
            if (s16) ys[i] = demod::demod_s16(y);
            else yf[i] = y;
            if (power) acc += demod::demod_power(I, Q);
            Ip = I;
            Qp = Q;
        }
        last[2 * c] = Ip;
        last[2 * c + 1] = Qp;
        if (power) power[c] = acc * (float)(1.0 / (double)nsamp);
    }
}

void R2iq::demod_angle_n(const float *im, const float *re, size_t n, float *out)
{
    for (size_t i = 0; i < n; i++) out[i] = demod::demod_angle(im[i], re[i]);
}

void R2iq::demod_sincos_n(const uint32_t *words, size_t n, float *c, float *s)
{
    for (size_t i = 0; i < n; i++) demod::demod_sincos_word(words[i], c + i, s + i);
}

// The channel audio filter: audio_iir_math.h's stream, sample by sample.
template <int S>
static void channel_audio_filter_s(const void *in, bool in16, int nch, size_t nsamp, size_t in_stride, const float *coef,
                                   const float *mat, unsigned block_pos, float *state, void *out, bool out16,
                                   size_t out_stride)
{
    constexpr int N = 2 * S;
    for (int c = 0; c < nch; c++) {
        const float *xf = static_cast<const float *>(in) + (size_t)c * in_stride;
        const int16_t *xs = static_cast<const int16_t *>(in) + (size_t)c * in_stride;
        float *yf = static_cast<float *>(out) + (size_t)c * out_stride;
        int16_t *ys = static_cast<int16_t *>(out) + (size_t)c * out_stride;
        const float *cf = coef + (size_t)c * 5 * S, *M = mat + (size_t)c * N * N;
        float *E = state + (size_t)c * 3 * N, *R = E + N, *Zr = R + N;
        unsigned n = block_pos;
        for (size_t i = 0; i < nsamp; i++) {
            const float x = in16 ? (float)xs[i] : xf[i];
            const float y = audio::audio_step<S>(cf, R, x);
            (void)audio::audio_step<S>(cf, Zr, x);
            if (out16) ys[i] = demod::demod_s16(y);
            else yf[i] = y;
            if (++n == (unsigned)audio::kAudioBlock) {
                float nE[N];
                audio::audio_adv<S>(M, E, Zr, nE);
                for (int q = 0; q < N; q++) {
                    E[q] = R[q] = nE[q];
                    Zr[q] = 0.f;
                }
                n = 0;
            }
        }
    }
}

void R2iq::channel_audio_filter(const void *in, bool in16, int nch, int nsec, size_t nsamp, size_t in_stride,
                                const float *coef, const float *mat, unsigned block_pos, float *state, void *out,
                                bool out16, size_t out_stride)
{
    switch (nsec) {
    case 1: return channel_audio_filter_s<1>(in, in16, nch, nsamp, in_stride, coef, mat, block_pos, state, out, out16, out_stride);
    case 2: return channel_audio_filter_s<2>(in, in16, nch, nsamp, in_stride, coef, mat, block_pos, state, out, out16, out_stride);
    case 3: return channel_audio_filter_s<3>(in, in16, nch, nsamp, in_stride, coef, mat, block_pos, state, out, out16, out_stride);
    default: return channel_audio_filter_s<4>(in, in16, nch, nsamp, in_stride, coef, mat, block_pos, state, out, out16, out_stride);
    }
}

// The channel AGC: agc_math.h's stream, sample by sample.
void R2iq::channel_agc(const void *in, bool in16, int nch, size_t nsamp, size_t in_stride, const float *par,
                       unsigned block_pos, float *state, void *out, bool out16, size_t out_stride, float *env)
{
    for (int c = 0; c < nch; c++) {
        const float *xf = static_cast<const float *>(in) + (size_t)c * in_stride;
        const int16_t *xs = static_cast<const int16_t *>(in) + (size_t)c * in_stride;
        float *yf = static_cast<float *>(out) + (size_t)c * out_stride;
        int16_t *ys = static_cast<int16_t *>(out) + (size_t)c * out_stride;
        const float *p = par + (size_t)c * agc::kAgcParams;
        const float T = p[0], d = p[1], F = p[2], dB = p[3];
        float *st = state + (size_t)c * 3;
        float E = st[0], R = st[1], Zr = st[2];
        unsigned n = block_pos;
        for (size_t i = 0; i < nsamp; i++) {
            const float x = in16 ? (float)xs[i] : xf[i];
            const float a = agc::agc_abs(x);
            R = agc::agc_env(a, d, R);
            Zr = agc::agc_env(a, d, Zr);
            const float y = agc::agc_out(T, F, R, x);
            if (out16) ys[i] = demod::demod_s16(y);
            else yf[i] = y;
            if (++n == (unsigned)agc::kAgcBlock) {
                E = agc::agc_boundary(dB, E, Zr);
                R = E;
                Zr = 0.f;
                n = 0;
            }
        }
        st[0] = E;
        st[1] = R;
        st[2] = Zr;
        if (env) env[c] = R;
    }
}

// The channel noise blanker: blanker_math.h's stream, sample by sample.
void R2iq::channel_blank(const void *in, bool cs16, int nch, size_t nsamp, size_t in_stride, const float *par, int guard,
                         int ref_blocks, int ref_mode, uint64_t pos, BlankerChannel *state, void *out, size_t out_stride,
                         uint32_t *count)
{
    using namespace blank;
    const int B = kBlankBlock, g = guard, M = ref_blocks;
    const size_t words = cs16 ? 1 : 2;   // 32-bit words per stored sample
    for (int c = 0; c < nch; c++) {
        const uint32_t *x = static_cast<const uint32_t *>(in) + (size_t)c * in_stride / (cs16 ? 2 : 1);
        uint32_t *y = static_cast<uint32_t *>(out) + (size_t)c * out_stride / (cs16 ? 2 : 1);
        const float thr = par[2 * c], qmin = par[2 * c + 1];
        BlankerChannel &st = state[c];
        uint64_t k = pos / (uint64_t)B;
        int b = (int)(pos % (uint64_t)B);
        int n = k < (uint64_t)M ? (int)k : M;
        auto threshold = [&]() { return n > 0 ? blank_threshold(thr, blank_reference(st.pw + kBlankMaxRef - n, n, ref_mode), qmin) : 0.f; };
        float t = threshold();
        uint32_t cnt = 0;
        for (size_t i = 0; i < nsamp; i++) {
            uint32_t w[2] = {x[i * words], cs16 ? 0u : x[i * words + 1]};
            float fi, fq;
            if (cs16) {
                fi = (float)(int16_t)(w[0] & 0xffffu);
                fq = (float)(int16_t)(w[0] >> 16);
            } else {
                __builtin_memcpy(&fi, &w[0], 4);
                __builtin_memcpy(&fq, &w[1], 4);
            }
            const float q = blank_power(fi, fq);
            st.q[b] = blank_finite(q) ? q : 0.f;
            const bool hit = thr > 0.f && blank_hit(q, t, n);
            st.since = hit ? 0u : (st.since < kBlankNoHit ? st.since + 1 : kBlankNoHit);
            const bool blanked = st.since <= (uint32_t)(2 * g);
            uint32_t d[2] = {w[0], w[1]};
            if (g > 0) {   // the slot of x[i - g] is the one x[i] goes into
                uint32_t *slot = st.hist + (size_t)((pos + i) % (uint64_t)g) * words;
                for (size_t j = 0; j < words; j++) {
                    d[j] = slot[j];
                    slot[j] = w[j];
                }
            }
            for (size_t j = 0; j < words; j++) y[i * words + j] = blanked ? 0u : d[j];
            if (blanked && pos + i >= (uint64_t)g) cnt++;
            if (++b == B) {
                const float p = blank_tree(st.q);
                for (int j = 0; j + 1 < kBlankMaxRef; j++) st.pw[j] = st.pw[j + 1];
                st.pw[kBlankMaxRef - 1] = p;
                b = 0;
                k++;
                n = k < (uint64_t)M ? (int)k : M;
                t = threshold();
            }
        }
        if (count) count[c] = cnt;
    }
}

// The channel squelch: squelch_math.h's stream, sample by sample.
void R2iq::channel_squelch(const void *audio, bool in16, const void *sense, int kind, int nch, size_t nsamp, size_t in_stride,
                           size_t sense_stride, const int *modes, const float *thr, int attack, int hang, int fade,
                           uint64_t pos, SquelchChannel *state, void *out, bool out16, size_t out_stride, uint32_t *open,
                           uint32_t *count, float *level)
{
    using namespace squelch;
    const int B = kSquelchBlock;
    for (int c = 0; c < nch; c++) {
        const float *xf = static_cast<const float *>(audio) + (size_t)c * in_stride;
        const int16_t *xs = static_cast<const int16_t *>(audio) + (size_t)c * in_stride;
        const float *sf = static_cast<const float *>(sense) + (size_t)c * sense_stride;
        const int16_t *ss = static_cast<const int16_t *>(sense) + (size_t)c * sense_stride;
        float *yf = static_cast<float *>(out) + (size_t)c * out_stride;
        int16_t *ys = static_cast<int16_t *>(out) + (size_t)c * out_stride;
        const int mode = modes[c];
        const float To = thr[2 * c], Tc = thr[2 * c + 1];
        const bool gated = mode == kSquelchLevel || mode == kSquelchNoise;
        SquelchChannel &st = state[c];
        int b = (int)(pos % (uint64_t)B);
        uint32_t cnt = 0;
        for (size_t i = 0; i < nsamp; i++) {
            const float x = in16 ? (float)xs[i] : xf[i];
            float q;
            switch (kind) {
            case kSenseSelf: q = squelch_q_real(x); break;
            case kSenseF32: q = squelch_q_real(sf[i]); break;
            case kSenseS16: q = squelch_q_real((float)ss[i]); break;
            case kSenseCF32: q = blank::blank_power(sf[2 * i], sf[2 * i + 1]); break;
            default: q = blank::blank_power((float)ss[2 * i], (float)ss[2 * i + 1]); break;
            }
            const bool fin = blank::blank_finite(q);
            st.q[b] = fin ? q : 0.f;
            st.bad |= fin ? 0u : 1u;
            const uint32_t g = mode == kSquelchOff ? 1u : (gated ? st.open : 0u);
            const int k = squelch_kind(mode, g, st.gprev, fade);
            if (out16) {
                ys[i] = demod::demod_s16(squelch_apply(k, b, x));
            } else if (k == kPass && !in16) {
                __builtin_memcpy(&yf[i], &xf[i], 4);   // the stored word: a NaN keeps its payload
            } else {
                yf[i] = squelch_apply(k, b, x);
            }
            cnt += g;
            if (++b == B) {
                const float p = blank::blank_tree(st.q);
                if (gated) {
                    bool u, v;
                    squelch_flags(p, st.bad != 0, mode, To, Tc, &u, &v);
                    st.gprev = st.open;
                    squelch_step(u, v, (uint32_t)attack, (uint32_t)hang, &st.r, &st.n, &st.open);
                }
                st.level = p;
                st.bad = 0;
                b = 0;
            }
        }
        if (open) open[c] = mode == kSquelchOff ? 1u : (gated ? st.open : 0u);
        if (count) count[c] = cnt;
        if (level) level[c] = st.level;
    }
}

// The channel tone detector: tone_math.h's stream, sample by sample; a block's sums when it completes.
void R2iq::channel_tone(const void *sense, bool sense16, const void *audio, bool in16, int nch, size_t nsamp,
                        size_t sense_stride, size_t in_stride, const uint32_t *words, int ntones, const uint64_t *masks,
                        const float *thr, int window, int attack, int hang, uint64_t pos, ToneChannel *state, void *out,
                        bool out16, size_t out_stride, int32_t *tone_out, uint32_t *open, uint32_t *count, float *level,
                        float *powers)
{
    using namespace tone;
    const int B = kToneBlock;
    // (c_i, s_i) of every tone: they depend on the tone and on i alone
    std::vector<float> pc((size_t)ntones * B), ps((size_t)ntones * B);
    for (int t = 0; t < ntones; t++)
        for (int i = 0; i < B; i++) tone_phasor(words[t], (uint32_t)i, &pc[(size_t)t * B + i], &ps[(size_t)t * B + i]);
    for (int c = 0; c < nch; c++) {
        const float *sf = static_cast<const float *>(sense) + (size_t)c * sense_stride;
        const int16_t *ss = static_cast<const int16_t *>(sense) + (size_t)c * sense_stride;
        const float *xf = static_cast<const float *>(audio) + (size_t)c * in_stride;
        const int16_t *xs = static_cast<const int16_t *>(audio) + (size_t)c * in_stride;
        float *yf = static_cast<float *>(out) + (size_t)c * out_stride;
        int16_t *ys = static_cast<int16_t *>(out) + (size_t)c * out_stride;
        const uint64_t mask = masks[c];
        const float To = thr[3 * c], Tc = thr[3 * c + 1], Emin = thr[3 * c + 2];
        ToneChannel &st = state[c];
        int b = (int)(pos % (uint64_t)B);
        uint64_t k = pos / (uint64_t)B;   // the stream's block index
        uint32_t cnt = 0;
        for (size_t i = 0; i < nsamp; i++) {
            const float s = sense16 ? (float)ss[i] : sf[i];
            const bool fin = blank::blank_finite(s * s);
            st.x[b] = fin ? s : 0.f;
            st.bad |= fin ? 0u : 1u;
            const uint32_t g = mask == 0 ? 1u : st.open;
            if (audio) {
                if (out16) {
                    ys[i] = g ? demod::demod_s16(in16 ? (float)xs[i] : xf[i]) : (int16_t)0;
                } else if (!g) {
                    yf[i] = 0.f;
                } else if (in16) {
                    yf[i] = (float)xs[i];
                } else {
                    __builtin_memcpy(&yf[i], &xf[i], 4);   // the stored word: a NaN keeps its payload
                }
            }
            cnt += g;
            if (++b < B) continue;
            b = 0;
            float tmp[kToneBlock];
            for (int m = 0; m < B; m++) tmp[m] = st.x[m] * st.x[m];
            st.E = st.E + blank::blank_tree(tmp);
            const uint32_t pos256 = (uint32_t)(k * (uint64_t)B);
            for (uint64_t mm = mask; mm; mm &= mm - 1) {
                const int t = __builtin_ctzll(mm);
                const float *ct = &pc[(size_t)t * B], *sn = &ps[(size_t)t * B];
                for (int m = 0; m < B; m++) tmp[m] = st.x[m] * ct[m];
                const float Ck = blank::blank_tree(tmp);
                for (int m = 0; m < B; m++) tmp[m] = st.x[m] * sn[m];
                const float Sk = blank::blank_tree(tmp);
                float cr, sr, re, im;
                tone_phasor(words[t], pos256, &cr, &sr);
                tone_rotate(Ck, Sk, cr, sr, &re, &im);
                st.zr[t] = st.zr[t] + re;
                st.zi[t] = st.zi[t] + im;
            }
            k++;
            if (k % (uint64_t)window != 0) continue;
            // the window is complete
            int best = -1;
            float Pbest = 0.f;
            for (int t = 0; t < kToneMaxTones; t++) {
                const bool in = (mask >> t) & 1;
                st.pow[t] = in ? blank::blank_power(st.zr[t], st.zi[t]) : 0.f;
                if (in) tone_best(t, st.pow[t], &best, &Pbest);
                st.zr[t] = st.zi[t] = 0.f;
            }
            bool u, v;
            tone_flags(Pbest, st.E, st.bad != 0, To, Tc, Emin, &u, &v);
            squelch::squelch_step(u, v, (uint32_t)attack, (uint32_t)hang, &st.r, &st.n, &st.open);
            st.tone = v ? best : -1;
            st.pbest = Pbest;
            st.elast = st.E;
            st.E = 0.f;
            st.bad = 0;
        }
        if (tone_out) tone_out[c] = st.tone;
        if (open) open[c] = mask == 0 ? 1u : st.open;
        if (count) count[c] = cnt;
        if (level) level[2 * c] = st.pbest, level[2 * c + 1] = st.elast;
        if (powers)
            for (int t = 0; t < ntones; t++) powers[(size_t)c * ntones + t] = st.pow[t];
    }
}

// The channel DCS decoder: dcs_math.h's stream, sample by sample; a window's decode when it completes.
void R2iq::channel_dcs(const void *sense, bool sense16, const void *audio, bool in16, int nch, size_t nsamp,
                       size_t sense_stride, size_t in_stride, const uint32_t *cws, int ncodes, const int32_t *params,
                       uint32_t word, const uint32_t *counts, int window, int e_open, int e_close, int attack, int hang,
                       uint64_t pos, DcsChannel *state, void *out, bool out16, size_t out_stride, int32_t *code_out,
                       uint32_t *open, uint32_t *count, uint32_t *info)
{
    using namespace dcs;
    const uint32_t WB = (uint32_t)(kDcsBlock * window);
    for (int c = 0; c < nch; c++) {
        const float *sf = static_cast<const float *>(sense) + (size_t)c * sense_stride;
        const int16_t *ss = static_cast<const int16_t *>(sense) + (size_t)c * sense_stride;
        const float *xf = static_cast<const float *>(audio) + (size_t)c * in_stride;
        const int16_t *xs = static_cast<const int16_t *>(audio) + (size_t)c * in_stride;
        float *yf = static_cast<float *>(out) + (size_t)c * out_stride;
        int16_t *ys = static_cast<int16_t *>(out) + (size_t)c * out_stride;
        const int code = params[3 * c], invert = params[3 * c + 1];
        const uint32_t eye = (uint32_t)params[3 * c + 2];
        DcsChannel &st = state[c];
        uint32_t n = (uint32_t)(pos % (uint64_t)WB);   // the window-local index
        uint32_t cnt = 0;
        for (size_t i = 0; i < nsamp; i++) {
            const int s = sense16 ? dcs_sign_s16((int)ss[i]) : dcs_sign(sf[i]);
            const uint32_t m = dcs_subbin(word, n);
            if (m < (uint32_t)kDcsSubBins) st.S[m] += s;
            const uint32_t g = code == kDcsOff ? 1u : st.open;
            if (audio) {
                if (out16) {
                    ys[i] = g ? demod::demod_s16(in16 ? (float)xs[i] : xf[i]) : (int16_t)0;
                } else if (!g) {
                    yf[i] = 0.f;
                } else if (in16) {
                    yf[i] = (float)xs[i];
                } else {
                    __builtin_memcpy(&yf[i], &xf[i], 4);   // the stored word: a NaN keeps its payload
                }
            }
            cnt += g;
            if (++n < WB) continue;
            n = 0;
            // the window is complete
            uint32_t Q, d;
            int t, best;
            dcs_window(st.S, cws, ncodes, code, invert, &Q, &t, &best, &d);
            bool u, v;
            dcs_flags(Q, counts[t], d, eye, (uint32_t)e_open, (uint32_t)e_close, &u, &v);
            squelch::squelch_step(u, v, (uint32_t)attack, (uint32_t)hang, &st.r, &st.n, &st.open);
            st.code = v ? best : -1;
            st.q = Q;
            st.nt = counts[t];
            st.d = d;
            st.t = (uint32_t)t;
            for (int32_t &x : st.S) x = 0;
        }
        if (code_out) code_out[c] = st.code;
        if (open) open[c] = code == kDcsOff ? 1u : st.open;
        if (count) count[c] = cnt;
        if (info) info[4 * c] = st.q, info[4 * c + 1] = st.nt, info[4 * c + 2] = st.d, info[4 * c + 3] = st.t;
    }
}

// The channel stereo decoder: stereo_math.h's stream, sample by sample; a block's sums when it completes.
void R2iq::channel_stereo(const void *in, bool in16, int nch, size_t nsamp, size_t in_stride, uint32_t word,
                          const uint8_t *modes, const float *thr, int window, int attack, int hang, uint64_t pos,
                          StereoChannel *state, void *left, void *right, bool out16, size_t out_stride,
                          uint32_t *stereo_out, uint32_t *count, float *level, float *phase)
{
    using namespace stereo;
    const int B = kStereoBlock;
    const uint32_t w2 = word * 2u;
    // the pilot's and the carrier's phasors of a block's samples: they depend on i alone
    float pc[kStereoBlock], ps[kStereoBlock], tc[kStereoBlock], ts[kStereoBlock];
    for (int i = 0; i < B; i++) {
        tone::tone_phasor(word, (uint32_t)i, &pc[i], &ps[i]);
        tone::tone_phasor(w2, (uint32_t)i, &tc[i], &ts[i]);
    }
    for (int c = 0; c < nch; c++) {
        const float *xf = static_cast<const float *>(in) + (size_t)c * in_stride;
        const int16_t *xs = static_cast<const int16_t *>(in) + (size_t)c * in_stride;
        float *lf = static_cast<float *>(left) + (size_t)c * out_stride, *rf = static_cast<float *>(right) + (size_t)c * out_stride;
        int16_t *ls = static_cast<int16_t *>(left) + (size_t)c * out_stride, *rs = static_cast<int16_t *>(right) + (size_t)c * out_stride;
        const bool autom = modes[c] == kStereoAuto;
        const float To = thr[4 * c], Tc = thr[4 * c + 1], Emin = thr[4 * c + 2], g2 = thr[4 * c + 3];
        StereoChannel &st = state[c];
        int b = (int)(pos % (uint64_t)B);
        uint64_t k = pos / (uint64_t)B;   // the stream's block index
        uint32_t cnt = 0;
        bool have = false;                // rr, ri are block k's
        float rr = 0.f, ri = 0.f;
        for (size_t i = 0; i < nsamp; i++) {
            const float x = in16 ? (float)xs[i] : xf[i];
            const bool fin = blank::blank_finite(x * x);
            st.x[b] = fin ? x : 0.f;
            st.bad |= fin ? 0u : 1u;
            if (autom && st.open) {
                if (!have) stereo_block(st.qr, st.qi, w2, (uint32_t)(k * (uint64_t)B), &rr, &ri);
                have = true;
                float L, R;
                stereo_lr(x, g2, stereo_sub(tc[b], ts[b], rr, ri), &L, &R);
                if (out16) ls[i] = demod::demod_s16(L), rs[i] = demod::demod_s16(R);
                else lf[i] = L, rf[i] = R;
                cnt++;
            } else if (out16) {
                ls[i] = rs[i] = demod::demod_s16(x);
            } else if (in16) {
                lf[i] = rf[i] = x;
            } else {
                __builtin_memcpy(&lf[i], &xf[i], 4);   // the stored word: a NaN keeps its payload
                __builtin_memcpy(&rf[i], &xf[i], 4);
            }
            if (++b < B) continue;
            b = 0;
            have = false;
            float tmp[kStereoBlock];
            for (int m = 0; m < B; m++) tmp[m] = st.x[m] * st.x[m];
            st.E = st.E + blank::blank_tree(tmp);
            for (int m = 0; m < B; m++) tmp[m] = st.x[m] * pc[m];
            const float Ck = blank::blank_tree(tmp);
            for (int m = 0; m < B; m++) tmp[m] = st.x[m] * ps[m];
            const float Sk = blank::blank_tree(tmp);
            float cr, sr, re, im;
            tone::tone_phasor(word, (uint32_t)(k * (uint64_t)B), &cr, &sr);
            tone::tone_rotate(Ck, Sk, cr, sr, &re, &im);
            st.zr = st.zr + re;
            st.zi = st.zi + im;
            k++;
            if (k % (uint64_t)window != 0) continue;
            // the window is complete
            const float P = blank::blank_power(st.zr, st.zi);
            bool u, v;
            tone::tone_flags(P, st.E, st.bad != 0, To, Tc, Emin, &u, &v);
            if (v) stereo_phase(st.zr, st.zi, P, &st.qr, &st.qi);
            squelch::squelch_step(u, v, (uint32_t)attack, (uint32_t)hang, &st.r, &st.n, &st.open);
            st.plast = P;
            st.elast = st.E;
            st.zr = st.zi = st.E = 0.f;
            st.bad = 0;
        }
        if (stereo_out) stereo_out[c] = autom ? st.open : 0u;
        if (count) count[c] = cnt;
        if (level) level[2 * c] = st.plast, level[2 * c + 1] = st.elast;
        if (phase) phase[2 * c] = st.qr, phase[2 * c + 1] = st.qi;
    }
}

}  // namespace cpu
}  // namespace sddc
