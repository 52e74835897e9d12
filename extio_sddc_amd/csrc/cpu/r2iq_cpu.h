// r2iq_cpu.h — the CPU r2iq backend: the reference's overlap-save worker
// (Core/fft_mt_r2iq_impl.hpp:15-152, AVX2 variant Core/fft_mt_r2iq_avx2.cpp:11-328) restated
// for x86-64 AVX2 + FMA on this library's own FFTs (fft_avx2.hpp), without FFTW.
//
// It is the host half of the C ABI's CPU handles (sddc_ddc_create with device
// SDDC_DDC_DEVICE_CPU): an explicit backend choice, never a silent fallback of a GPU handle.
// No HIP header is included here, so the drop-in class, the C ABI front and this file can be
// built and run under ASan/UBSan/TSan in a container without a GPU.
//
// Per input block (65536 int16) and frame k = 0..10 (8192 samples at 6144 k of
// [history 4096 | block], impl.hpp:84-88):
//   convert (+ rand: v odd ? -v : v)       fft_mt_r2iq.h:36-51
//   Z = FFT4096(x[2n] + i x[2n+1])          r2c 8192 (impl.hpp:88) as a packed complex FFT
//   T[m] = Z_j P[m] + conj(Z_-j) Q[m]       split x shift x filter with zero fill
//          (j = tb + m, or tb - mfft + m for m >= mfft/2; P = H/2 (1 - i W^j), Q = H/2 (1 + i W^j))
//   y = IFFT_mfft(T)                         impl.hpp:98 (unnormalised, FFTW_BACKWARD)
//   keep y[mfft/4, 3mfft/4) (k = 0) or y[0, 3mfft/4) (k >= 1), conj if lsb   impl.hpp:117-138
#pragma once

#include <complex>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../agc_math.h"
#include "../audio_iir_math.h"
#include "../audio_resample_math.h"
#include "../blanker_math.h"
#include "../demod_math.h"
#include "../squelch_math.h"
#include "../tone_math.h"
#include "../stereo_math.h"
#include "../dcs_math.h"
#include "fft_avx2.hpp"

namespace sddc {
namespace cpu {

struct Params {
    int d = 0;              // decimation index 0..6, mfft = 4096 >> d
    int tunebin = 1024;     // multiple of 4 in [0, 4096)
    bool lsb = false;       // sideband flip (conj)
    bool rand = false;      // ADC de-randomiser
    bool cs16 = false;      // output int16 (I, Q) = saturate(rint(x * scale)) instead of float
    float scale = 1.f;
    // fused fine-tune NCO (fine_tune.h): T[32] and per-128-sample lane starts [blocks][4] of
    // this call's output, as (cos, sin) float pairs; null = off
    const float *nco_trig = nullptr;
    const float *nco_starts = nullptr;
};

bool supported();   // this CPU has AVX2 and FMA

class R2iq {
public:
    // H[d][4096]: the filter bank (filterbank.h filter_response), double precision
    explicit R2iq(const std::complex<double> *H);
    ~R2iq();
    R2iq(const R2iq &) = delete;
    R2iq &operator=(const R2iq &) = delete;

    void reset();                                   // zero history (TurnOn)
    void set_history(const int16_t *last4096);      // history = these 4096 samples
    // nblk blocks, block i at blocks[i]; writes nblk * (32768 >> d) complex samples to out
    // (CF32: float (I, Q); CS16: int16 (I, Q)) and keeps the last 4096 input samples
    void process(const int16_t *const *blocks, int nblk, void *out, const Params &p);
    // The averaged power spectrum of in = [history 4096 | nblk blocks] (sddc_ddc.h,
    // sddc_ddc_spectrum_host): psd[nblk / bpr][4096], row r = scale x the sum of |X_f[k]|^2 over the
    // 11 bpr frames of blocks r bpr .. r bpr + bpr - 1 in frame order; w = the 8192-point window
    // (null: rectangular).  Stateless: it neither reads nor changes the kept history.
    void spectrum(const int16_t *in, int nblk, int bpr, const float *w, float scale, bool rand, float *psd);
    // The channel spectrum (sddc_ddc.h, sddc_ddc_channel_spectrum_host): nch streams of complex
    // samples (cs16: int16 (I, Q), else float (I, Q)), channel c at c * stride samples; frame f of
    // row r = the n samples at (r fpr + f) hop, windowed by w[n] (null: rectangular);
    // psd[c][r][q] = scale x the sum over the row's frames, in frame order, of |X_f[(q + n/2) mod n]|^2.
    void channel_spectrum(const void *iq, bool cs16, int nch, size_t stride, int n, int hop, int fpr, int nrows,
                          const float *w, float scale, float *psd);
    // The channel decimator (sddc_ddc.h, sddc_ddc_channel_decimate_host): y_c[m] = sum_j taps[j]
    // x_c[m R - j] on nch streams (cs16: int16 (I, Q) read as v * inv_s, else float (I, Q)), channel c
    // at c * in_stride components, nsamp = a multiple of R samples each; channel c's nsamp / R
    // (I, Q) float outputs at out + c * out_stride floats.  tail: [nch][ntaps - 1][2] floats, each
    // channel's last sample values before the call, replaced by those after it.  Stateless otherwise.
    static void channel_decimate(const void *iq, bool cs16, float inv_s, int nch, size_t nsamp, size_t in_stride,
                                 const float *taps, int ntaps, int R, float *tail, float *out, size_t out_stride);
    // The channel resampler (sddc_ddc.h, sddc_ddc_channel_resample_host): output k of the call has
    // e + k M = s L + p and is sum_{j < K} taps[p + j L] x_c[s - j], K = ceil(ntaps / L), s counted from
    // the call's first sample; e (0 <= e < M) is the call's reduced stream position and nout its
    // outputs per channel (every s < nsamp).  Streams, formats, strides and tail ([nch][K - 1][2]
    // floats) as for channel_decimate.  Stateless otherwise.
    static void channel_resample(const void *iq, bool cs16, float inv_s, int nch, size_t nsamp, size_t in_stride,
                                 const float *taps, int ntaps, int L, int M, int e, size_t nout, float *tail, float *out,
                                 size_t out_stride);
    // The channel audio resampler (sddc_ddc.h, sddc_ddc_channel_audio_resample_host;
    // audio_resample_math.h): the resampler's outputs on nch REAL streams (float, or int16 read as
    // (float)v when in16, channel c at in + c * in_stride samples), each the definition's fixed
    // sequence of fmaf, the device kernel's.  tail: [nch][K - 1] floats, each channel's last sample
    // values before the call, replaced by those after it.  Outputs float, or int16 (demod_s16) when
    // out16, at out + c * out_stride samples.  Stateless otherwise.
    static void channel_audio_resample(const void *in, bool in16, int nch, size_t nsamp, size_t in_stride,
                                       const float *taps, int ntaps, int L, int M, int e, size_t nout, float *tail,
                                       void *out, bool out16, size_t out_stride);
    // The channel demodulator (sddc_ddc.h, sddc_ddc_channel_demodulate_host; demod_math.h): channel c's
    // nsamp samples demodulated by chan[c] (mode, gain, BFO word) at stream position pos, streams and
    // formats as for channel_decimate; channel c's outputs (float, or int16 when s16) at out + c *
    // out_stride samples.  last: [nch][2] floats, each channel's last sample value before the call,
    // replaced by the one after it.  power: null, or [nch] floats that receive the mean of
    // fmaf(I, I, Q Q) over the call, summed sample by sample.  Stateless otherwise.
    static void channel_demodulate(const void *iq, bool cs16, float inv_s, int nch, size_t nsamp, size_t in_stride,
                                   const ChDemChannel *chan, uint32_t pos, float *last, void *out, bool s16,
                                   size_t out_stride, float *power);
    // The channel audio filter (sddc_ddc.h, sddc_ddc_channel_audio_filter_host; audio_iir_math.h): channel
    // c's nsamp samples (float, or int16 when in16, at in + c * in_stride samples) through its nsec
    // sections coef [nch][nsec][5] with the block matrices mat [nch][2 nsec][2 nsec]; the call's first
    // sample is block_pos samples into a block.  state: [nch][3][2 nsec] floats (E, R, Zr) before the
    // call, replaced by the ones after it.  Outputs float, or int16 when out16, at out + c * out_stride.
    static void channel_audio_filter(const void *in, bool in16, int nch, int nsec, size_t nsamp, size_t in_stride,
                                     const float *coef, const float *mat, unsigned block_pos, float *state, void *out,
                                     bool out16, size_t out_stride);
    // The channel AGC (sddc_ddc.h, sddc_ddc_channel_agc_host; agc_math.h): channel c's nsamp samples,
    // laid out and formatted as for channel_audio_filter, through the peak AGC of par [nch][4] = (T, d,
    // F, dB); the call's first sample is block_pos samples into a block.  state: [nch][3] floats (E, R,
    // Zr) before the call, replaced by the ones after it.  env: null, or [nch] floats that receive R
    // after the call's last sample.
    static void channel_agc(const void *in, bool in16, int nch, size_t nsamp, size_t in_stride, const float *par,
                            unsigned block_pos, float *state, void *out, bool out16, size_t out_stride, float *env);
    // The channel noise blanker (sddc_ddc.h, sddc_ddc_channel_blank_host; blanker_math.h): the definition's
    // loop, sample by sample.  Channel c's nsamp IQ samples (float pairs, or int16 pairs when cs16) at in +
    // c * in_stride components, its outputs in the same format at out + c * out_stride components.  par:
    // [nch][2] = (thr, qmin); pos: the stream index of the call's first sample; state: [nch], before the
    // call and replaced by the one after it; count: null, or [nch] blanked outputs of this call.
    struct BlankerChannel {
        float pw[blank::kBlankMaxRef] = {};       // the last block powers, the newest one last
        float q[blank::kBlankBlock] = {};         // the unfinished block's q values, non-finite ones as 0
        uint32_t hist[2 * blank::kBlankMaxGuard] = {};   // ring of the last g stored samples (CS16: one word each)
        uint32_t since = kBlankNoHit;             // samples since the last hit, saturating
    };
    static constexpr uint32_t kBlankNoHit = 1u << 20;
    static void channel_blank(const void *in, bool cs16, int nch, size_t nsamp, size_t in_stride, const float *par,
                              int guard, int ref_blocks, int ref_mode, uint64_t pos, BlankerChannel *state, void *out,
                              size_t out_stride, uint32_t *count);
    // The channel squelch (sddc_ddc.h, sddc_ddc_channel_squelch_host; squelch_math.h): the definition's loop,
    // sample by sample.  Channel c's nsamp audio samples (float, or int16 when in16) at audio + c * in_stride,
    // its sense samples at sense + c * sense_stride components (kind: squelch::kSense*; kSenseSelf: the
    // audio), its outputs (float, or int16 when out16) at out + c * out_stride.  modes: [nch]; thr: [nch][2]
    // = (256 To, 256 Tc); pos: the stream index of the call's first sample; state: [nch], before the call and
    // replaced by the one after it; open, count, level: null, or [nch].
    struct SquelchChannel {
        uint32_t r = 0, n = 0, open = 0;   // the state machine after the last completed block
        uint32_t gprev = 0;                // the gate of the block before the unfinished one
        uint32_t bad = 0;                  // the unfinished block holds a non-finite q
        float level = 0.f;                 // p of the last completed block
        float q[squelch::kSquelchBlock] = {};   // the unfinished block's q values, non-finite ones as 0
    };
    static void channel_squelch(const void *audio, bool in16, const void *sense, int kind, int nch, size_t nsamp,
                                size_t in_stride, size_t sense_stride, const int *modes, const float *thr, int attack,
                                int hang, int fade, uint64_t pos, SquelchChannel *state, void *out, bool out16,
                                size_t out_stride, uint32_t *open, uint32_t *count, float *level);
    // The channel tone detector (sddc_ddc.h, sddc_ddc_channel_tone_host; tone_math.h): the definition's loop,
    // sample by sample.  Channel c's nsamp sense samples (float, or int16 when sense16) at sense + c *
    // sense_stride, its audio (null: detect only; float, or int16 when in16) at audio + c * in_stride, its
    // outputs (float, or int16 when out16) at out + c * out_stride.  words: [ntones]; masks: [nch]; thr:
    // [nch][3] = (To, Tc, Emin), scaled; window: W; pos: the stream index of the call's first sample; state:
    // [nch], before the call and replaced by the one after it; tone, open, count: null or [nch]; level: null
    // or [nch][2]; powers: null or [nch][ntones].
    struct ToneChannel {
        uint32_t r = 0, n = 0, open = 0;   // the gate after the last completed window
        int32_t tone = -1;                 // the last completed window's: the best tone where v held, P_best, E
        float pbest = 0.f, elast = 0.f;
        float E = 0.f;                     // the unfinished window's energy, and whether it holds a non-finite q
        uint32_t bad = 0;
        float zr[tone::kToneMaxTones] = {}, zi[tone::kToneMaxTones] = {};   // the unfinished window's sums
        float pow[tone::kToneMaxTones] = {};                                // every P_t of the last completed window
        float x[tone::kToneBlock] = {};    // the unfinished block's samples, non-finite ones as 0
    };
    static void channel_tone(const void *sense, bool sense16, const void *audio, bool in16, int nch, size_t nsamp,
                             size_t sense_stride, size_t in_stride, const uint32_t *words, int ntones, const uint64_t *masks,
                             const float *thr, int window, int attack, int hang, uint64_t pos, ToneChannel *state, void *out,
                             bool out16, size_t out_stride, int32_t *tone, uint32_t *open, uint32_t *count, float *level,
                             float *powers);
    // The channel DCS decoder (sddc_ddc.h, sddc_ddc_channel_dcs_host; dcs_math.h): the definition's loop, sample
    // by sample.  The streams as in channel_tone.  cws: [ncodes]; params: [nch][3] = (code, invert, eye); word:
    // the bit phase word; counts: [8] = N[t]; window: W; pos: the stream index of the call's first sample; state:
    // [nch], before the call and replaced by the one after it; code, open, count: null or [nch]; info: null or
    // [nch][4].
    struct DcsChannel {
        uint32_t r = 0, n = 0, open = 0;   // the gate after the last completed window
        int32_t code = -1;                 // the last completed window's: the best index where v held, Q, N, d, t
        uint32_t q = 0, nt = 0, d = 0, t = 0;
        int32_t S[dcs::kDcsSubBins] = {};  // the unfinished window's sub-bin sums
    };
    static void channel_dcs(const void *sense, bool sense16, const void *audio, bool in16, int nch, size_t nsamp,
                            size_t sense_stride, size_t in_stride, const uint32_t *cws, int ncodes, const int32_t *params,
                            uint32_t word, const uint32_t *counts, int window, int e_open, int e_close, int attack, int hang,
                            uint64_t pos, DcsChannel *state, void *out, bool out16, size_t out_stride, int32_t *code,
                            uint32_t *open, uint32_t *count, uint32_t *info);
    // The channel stereo decoder (sddc_ddc.h, sddc_ddc_channel_stereo_host; stereo_math.h): the definition's
    // loop, sample by sample.  Channel c's nsamp MPX samples (float, or int16 when in16) at in + c * in_stride,
    // its outputs (float, or int16 when out16) at left + c * out_stride and right + c * out_stride.  word: the
    // pilot's phase word; modes: [nch]; thr: [nch][4] = (To, Tc, Emin, g2), scaled; window: W; pos: the stream
    // index of the call's first sample; state: [nch], before the call and replaced by the one after it;
    // stereo, count: null or [nch]; level, phase: null or [nch][2].
    struct StereoChannel {
        uint32_t r = 0, n = 0, open = 0;   // the gate after the last completed window
        float qr = 1.f, qi = 0.f;          // the carrier's phase in force
        float plast = 0.f, elast = 0.f;    // P and E of the last completed window
        float zr = 0.f, zi = 0.f, E = 0.f; // the unfinished window's sums, and whether it holds a non-finite q
        uint32_t bad = 0, pad = 0;
        float x[stereo::kStereoBlock] = {};   // the unfinished block's samples, non-finite ones as 0
    };
    static void channel_stereo(const void *in, bool in16, int nch, size_t nsamp, size_t in_stride, uint32_t word,
                               const uint8_t *modes, const float *thr, int window, int attack, int hang, uint64_t pos,
                               StereoChannel *state, void *left, void *right, bool out16, size_t out_stride,
                               uint32_t *stereo_out, uint32_t *count, float *level, float *phase);
    // demod_math.h's routines on arrays (the accuracy sweeps of tests/test_channel_demod_cpu.py)
    static void demod_angle_n(const float *im, const float *re, size_t n, float *out);
    static void demod_sincos_n(const uint32_t *words, size_t n, float *c, float *s);

private:
    struct Buf;
    void build_pq(int d, int tb);
    void frame(const int16_t *x, int d, bool rand, const float **yr, const float **yi);

    std::unique_ptr<Buf> b_;
    FftPlan fwd_;
    std::vector<std::unique_ptr<FftPlan>> inv_;     // per d
    std::vector<std::complex<double>> H_;           // [7][4096]
    int pq_d_ = -1, pq_tb_ = -1;
    int lo_ = 0, hi_ = 0;                           // valid m ranges of the (P, Q) table
    std::vector<float> sw_;                         // spectrum(): W_8192^k, k <= 2048, as (cos, sin)
    std::vector<std::unique_ptr<FftPlan>> csp_;     // channel_spectrum(): the plans used so far
};

}  // namespace cpu
}  // namespace sddc
