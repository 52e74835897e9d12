/*
 * sddc_ddc.h — C ABI of the MI355X-native real-to-IQ down-converter.
 *
 * This is the thin C boundary UNDER the drop-in C++ class `fft_mt_r2iq`
 * (include/fft_mt_r2iq.h), which keeps the reference's r2iqControlClass
 * interface (Core/r2iq.h:16-48) so RadioHandler / libsddc / ExtIO / SoapySDDC
 * load it unchanged.  Plain pointers and sizes only; no C++ or torch types.
 * Every entry point names the reference interface it replaces (file:line,
 * relative to the ExtIO_sddc tree).
 *
 * Conventions (pinned to the reference):
 *   block      = 65536 int16 real ADC samples           (config.h:80-81 transferSamples)
 *   history    = the 4096 samples preceding a block      (fft_mt_r2iq_impl.hpp:32)
 *   d          = decimation index 0..6, mfft = 4096>>d   (r2iq.h:5,39; fft_mt_r2iq.cpp:44-48)
 *   output     = 8*mfft = 32768>>d complex float32 (I,Q interleaved) per input block
 *                (fft_mt_r2iq_impl.hpp:117-138); 2^d blocks fill one 32768-sample
 *                EXT_BLOCKLEN output block (config.h:62)
 *   tunebin    = forward-FFT bin moved to DC, multiple of 4 in [0,4096)
 *                (fft_mt_r2iq.cpp:101-109)
 *
 * Errors: every int-returning call returns SDDC_OK (0) or a negative SDDC_ERR_*;
 * sddc_ddc_last_error() gives a thread-local message.  Nothing throws across this
 * boundary (the reference's r2iq methods are void/bool/float).
 *
 * Backends.  A handle created on a device index >= 0 runs the gfx950 kernels; without a
 * usable gfx950 device sddc_ddc_create() fails with SDDC_ERR_NODEV, and a HIP error fails
 * the call — a GPU handle never falls back to the CPU.  A handle created on
 * SDDC_DDC_DEVICE_CPU runs the library's AVX2 r2iq (the reference's fft_mt_r2iq_avx2.cpp
 * worker, restated without FFTW) on the calling thread: the host path (process_host /
 * process_blocks) with the same controls, output formats, fine-tune NCO and history
 * semantics; its device-path calls return SDDC_ERR_STATE.  Choosing it is the caller's
 * explicit decision (the drop-in class: SDDC_DDC_BACKEND=cpu|auto).
 */
#ifndef SDDC_DDC_H
#define SDDC_DDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDDC_DDC_ABI_VERSION 3   /* 2: + set_fine_tune, set_output_format, process_blocks, register_host;
                                    3: + CPU handles (SDDC_DDC_DEVICE_CPU), backend, set_history;
                                       still 3: + set_channel_fine_tune, channel_tuning (new symbols
                                       only, no existing call changed);
                                       still 3: + spectrum_window, set_spectrum_window, spectrum_device,
                                       spectrum_host (new symbols only);
                                       still 3: + window, set_channel_spectrum_window,
                                       channel_spectrum_device, channel_spectrum_host (new symbols only);
                                       still 3: + set_channel_decimator, channel_decimator_reset,
                                       channel_decimate_samples, channel_decimate_device,
                                       channel_decimate_host (new symbols only);
                                       still 3: + set_channel_resampler, channel_resampler_reset,
                                       resample_count, channel_resample_samples,
                                       channel_resample_device, channel_resample_host (new symbols only);
                                       still 3: + bfo_word, set_channel_demodulator, channel_demodulator_reset,
                                       channel_demodulate_device, channel_demodulate_host (new symbols only);
                                       still 3: + biquad, set_channel_audio_filter, channel_audio_filter_reset,
                                       channel_audio_filter_device, channel_audio_filter_host (new symbols only);
                                       still 3: + agc_decay, set_channel_agc, channel_agc_reset,
                                       channel_agc_device, channel_agc_host (new symbols only);
                                       still 3: + set_channel_audio_resampler, channel_audio_resampler_formats, channel_audio_resampler_reset,
                                       channel_audio_resample_samples, channel_audio_resample_device,
                                       channel_audio_resample_host (new symbols only) */

#define SDDC_DDC_HALF_FFT   4096    /* halfFft               fft_mt_r2iq.h:18 */
#define SDDC_DDC_FFTN       8192    /* FFTN_R_ADC            config.h:49 */
#define SDDC_DDC_HOP        6144    /* 3*halfFft/2           fft_mt_r2iq_impl.hpp:88 */
#define SDDC_DDC_BLOCK      65536   /* transferSamples       config.h:80-81 */
#define SDDC_DDC_FRAMES     11      /* fftPerBuf             fft_mt_r2iq.h:19 */
#define SDDC_DDC_NDEC       7       /* NDECIDX               r2iq.h:5 */
#define SDDC_DDC_NTAPS      1025    /* halfFft/4+1 taps      fft_mt_r2iq.cpp:181 */
#define SDDC_DDC_OUT_BLOCK  32768   /* EXT_BLOCKLEN          config.h:62 */
#define SDDC_DDC_MAX_CHANNELS 1024  /* 1024 legal tune bins (tunebin = 4c) */
#define SDDC_DDC_MAX_BLOCKS 32768   /* blocks per process_* call (2^31 input samples, 4 GiB) */

enum {
    SDDC_OK = 0,
    SDDC_ERR_ARG = -1,     /* bad argument (range, null, alignment)           */
    SDDC_ERR_HIP = -2,     /* a HIP runtime call or kernel launch failed       */
    SDDC_ERR_NODEV = -3,   /* no usable gfx950 device                          */
    SDDC_ERR_STATE = -4,   /* call not valid in the handle's current state     */
    SDDC_ERR_NOMEM = -5    /* host or device allocation failed                 */
};

typedef struct sddc_ddc sddc_ddc_t;

#define SDDC_DDC_DEVICE_CPU   (-1)  /* sddc_ddc_create(): the host AVX2 backend */
#define SDDC_DDC_BACKEND_HIP  0
#define SDDC_DDC_BACKEND_CPU  1

/* ---- library ------------------------------------------------------------ */
int         sddc_ddc_abi_version(void);
const char *sddc_ddc_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unusable). */
int         sddc_ddc_device_count(void);

/* ---- filter design (host; Core/fir.cpp, fft_mt_r2iq.cpp:163-208) ---------- */
/* KaiserWindow(num_taps, Astop, normFpass, normFstop, Coef)   fir.cpp:48-105.
 * Bit-identical float arithmetic.  coef == NULL with ntaps <= 0 returns the
 * tap-count estimate, exactly like the reference. */
int sddc_ddc_kaiser(int ntaps, float astop, float fpass, float fstop, float *coef);
/* The 1025 taps for decimation index d (fft_mt_r2iq.cpp:189-191). */
int sddc_ddc_filter_taps(int d, float *taps /* [1025] */);
/* H_d = FFT4096(time-reversed gain*2048/8192*taps)  (fft_mt_r2iq.cpp:193-205),
 * evaluated in double and rounded once to float. */
int sddc_ddc_filter_response(float gain, int d, float *H /* [4096][2] */);

/* ---- lifecycle: fft_mt_r2iq::Init (fft_mt_r2iq.cpp:147-227), dtor (:71-98) - */
/* Builds the 7 filter banks for `gain` (hardware->getGain(), RadioHandler.cpp:142)
 * and uploads them with the FFT twiddle tables to `device`. */
int sddc_ddc_create(float gain, int device, sddc_ddc_t **out);
int sddc_ddc_destroy(sddc_ddc_t *h);
/* SDDC_DDC_BACKEND_HIP or SDDC_DDC_BACKEND_CPU (negative on a null handle). */
int sddc_ddc_backend(const sddc_ddc_t *h);

/* ---- control: r2iqControlClass (r2iq.h:23-31) and fft_mt_r2iq -------------- */
int   sddc_ddc_set_decimation(sddc_ddc_t *h, int d);        /* setDecimate   r2iq.h:31 */
int   sddc_ddc_set_sideband(sddc_ddc_t *h, int lsb);        /* setSideband   r2iq.h:28 */
int   sddc_ddc_set_rand(sddc_ddc_t *h, int rand);           /* updateRand    r2iq.h:25 */
int   sddc_ddc_set_tunebin(sddc_ddc_t *h, int tunebin);     /* mtunebin      fft_mt_r2iq.h:97 */
int   sddc_ddc_get_tunebin(const sddc_ddc_t *h);
/* setFreqOffset(offset)  fft_mt_r2iq.cpp:101-109: tunebin = int(offset*1024)*4,
 * returns the fine-tune residual (tunebin/4096 - offset) * 2^d.  Valid domain
 * 0 <= offset < 1 (fraction of Fs/2); outside it the tune bin is clamped into
 * [0, 4092] (the reference would read out of range, impl.hpp:76-79). */
float sddc_ddc_set_freq_offset(sddc_ddc_t *h, float offset);
/* TurnOn() stream reset (fft_mt_r2iq.cpp:111-129): zero history, seq = 0.  The
 * fine-tune NCO keeps its phase (the reference's mixer state lives in RadioHandler). */
int   sddc_ddc_reset(sddc_ddc_t *h);
/* Host path: the next process_host/process_blocks call starts from these 4096 samples as
 * its history instead of the kept one (the reference's peekReadPtr(-1) tail,
 * fft_mt_r2iq_impl.hpp:32) — e.g. to continue a stream on another handle. */
int   sddc_ddc_set_history(sddc_ddc_t *h, const int16_t *last4096);

/* Fused fine-tune NCO: mixes the output with the reference's
 * fine-tune mixer, pf_mixer's shift_limited_unroll_C_sse (Core/pffft/pf_mixer.cpp:
 * 750-856), as RadioHandlerClass::OnDataPacket does after the r2iq when fc != 0
 * (Core/RadioHandler.cpp:33-37).  relative_freq = fc, the residual returned by
 * sddc_ddc_set_freq_offset; a new fc restarts the phase at 0 like
 * shift_limited_unroll_C_sse_init(fc, 0) (RadioHandler.cpp:291-296), the same fc keeps
 * it; 0 turns the mixer off.  While on, process_device / process_host advance the
 * mixer phase by their output length (stream order).  This one fc belongs to the
 * single-channel path: while it is non-zero process_channels_device returns
 * SDDC_ERR_STATE; the many-channel path has an NCO per channel,
 * sddc_ddc_set_channel_fine_tune below.  Not for the drop-in class, whose caller
 * (RadioHandler) still mixes on the CPU. */
int   sddc_ddc_set_fine_tune(sddc_ddc_t *h, float relative_freq);

/* The same mixer per channel of the many-channel path: relative_freqs[c] is channel c's fc
 * (host array of nch floats, 0 <= nch <= SDDC_DDC_MAX_CHANNELS; the meaning of
 * sddc_ddc_set_fine_tune's relative_freq).  NULL or nch == 0 turns it off.  A channel whose fc
 * is 0 is not mixed: its output is the plain DDC bit for bit.  Re-init rule per channel index
 * (RadioHandler.cpp:291-296), in stream order: an fc equal to the one already set keeps that
 * channel's phase, a changed fc restarts that channel at phase 0, another nch restarts every
 * channel.  While on, every process_channels_device call advances each channel's phase by its
 * output length; the phases live on the device (the lane-start chain of fine_tune.h runs there),
 * so a call makes no host round trip.  sddc_ddc_reset keeps the phases.  A change of the array
 * waits for the handle's many-channel launches in flight.  process_channels_device with another
 * channel count than nch returns SDDC_ERR_STATE; process_device and the host calls ignore the
 * setting.  Errors: a non-finite fc or nch outside 0..1024 SDDC_ERR_ARG, a CPU handle
 * SDDC_ERR_STATE.
 * Memory: the lane starts of a call take nch * nblk * (8192 >> d) bytes of device memory, at
 * most 128 MiB per handle; a larger call runs as several launches over whole blocks, with
 * identical output. */
int   sddc_ddc_set_channel_fine_tune(sddc_ddc_t *h, const float *relative_freqs, int nch);
/* setFreqOffset's arithmetic (fft_mt_r2iq.cpp:101-109) without a handle, to fill the tune bin
 * and fc arrays of the many-channel calls: *tunebin = int(offset*1024)*4 clamped into [0, 4092],
 * *relative_freq = (tunebin/4096 - offset) * 2^d of the unclamped bin, the same float operations
 * as sddc_ddc_set_freq_offset.  SDDC_ERR_ARG for a non-finite offset, d outside 0..6 or NULL. */
int   sddc_ddc_channel_tuning(float offset, int d, int *tunebin, float *relative_freq);

/* Complex samples produced per nblk input blocks at decimation d: nblk*(32768>>d). */
size_t sddc_ddc_output_samples(int d, int nblk);

/* ---- output format ---------------------------------- */
/* CF32 (default): (I,Q) float pairs, the reference's output (RadioHandler / Soapy
 * CF32, SoapySDDC/Streaming.cpp:12-50).  CS16: (I,Q) int16 pairs written by the
 * kernels' output stage, value = saturate_int16(rint(x * cs16_scale)) with
 * round-half-even; 4 bytes per complex sample instead of 8.  Applies to every
 * process_* call (the NCO, if on, mixes first).  CS16 scale must be > 0. */
#define SDDC_DDC_FMT_CF32 0
#define SDDC_DDC_FMT_CS16 1
int sddc_ddc_set_output_format(sddc_ddc_t *h, int format, float cs16_scale);

/* ---- the hot loop (fft_mt_r2iq_impl.hpp:15-152) ---------------------------- */
/* Device-resident; stateless apart from the fine-tune NCO phase.  d_in: device
 * int16 [4096 + nblk*65536] = the 4096-sample history followed by nblk blocks
 * (4-byte aligned start required).  d_out: device buffer of nblk*(32768>>d)
 * complex samples in the output format (CF32: float (I,Q), 8-byte aligned;
 * CS16: int16 (I,Q), 4-byte aligned), in stream order.  Uses the handle's
 * d / sideband / rand / tunebin.  Enqueued on `hip_stream` (a hipStream_t;
 * NULL = default stream); returns after launch.  A stream given to a call must
 * stay valid until the handle is destroyed: a later call on another stream (a
 * new tune bin, say) or the destroy orders itself after the stream's last call. */
int sddc_ddc_process_device(sddc_ddc_t *h, const int16_t *d_in, int nblk,
                            void *d_out, void *hip_stream);

/* Many-channel DDC: one forward transform per
 * frame, shared by `nch` channels with their own tune bins (host array, each a
 * multiple of 4 in [0,4096)).  Channel c's stream starts `c*out_stride`
 * components (floats for CF32, int16 for CS16; 2 per complex sample) into
 * d_out.  All channels use the handle's d/sideband/rand/output format, and each its own
 * fine-tune NCO when sddc_ddc_set_channel_fine_tune is on (nch must match). */
int sddc_ddc_process_channels_device(sddc_ddc_t *h, const int16_t *d_in, int nblk,
                                     const int *tunebins, int nch,
                                     void *d_out, size_t out_stride,
                                     void *hip_stream);

/* Stateful, host buffers: the r2iq worker body.  Consumes nblk consecutive
 * blocks from `in` (host int16 [nblk*65536]), keeps the 4096-sample history
 * across calls (zero after create/reset), writes nblk*(32768>>d) complex
 * samples to `out` (host, in the output format).  Synchronous. */
int sddc_ddc_process_host(sddc_ddc_t *h, const int16_t *in, int nblk, void *out);

/* The same for blocks scattered in host memory (e.g. ring-buffer slots,
 * Core/dsp/ringbuffer.h): block i is blocks[i] (65536 int16). */
int sddc_ddc_process_blocks(sddc_ddc_t *h, const int16_t *const *blocks, int nblk,
                            void *out);

/* ---- wideband averaged power spectrum (panadapter / waterfall) ----------------
 * The Welch spectrum of the ADC stream on the DDC's own frame schedule.  The input is the
 * buffer process_device takes, [history 4096 | nblk blocks of 65536] int16; frame k of block b is
 * the 8192 samples at 65536 b + 6144 k, k = 0..10.  With the window w[0..8191] and x the sample
 * as float (de-randomised when the handle's rand is on):
 *   X_f[k]    = sum_j w[j] x_f[j] e^{-2 pi i jk/8192}            k = 0..4095 (bin 4096 is not output)
 *   psd[r][k] = 1/(11 bpr) sum_{frames f of row r} |X_f[k]|^2 / (sum_j w[j])^2
 * Row r covers blocks r bpr .. r bpr + bpr - 1 (bpr = blocks_per_row >= 1, a divisor of nblk);
 * the output is nblk/bpr rows of SDDC_DDC_SPECTRUM_BINS float32, contiguous.  A real tone of
 * amplitude A (int16 units) at a bin centre reads A^2/4, so dBFS = 10 log10(4 psd / 32768^2).
 * The scale 1/(11 bpr (sum w)^2) is formed in double and applied once, at the final store.  Every
 * sum is taken in a fixed order given by a frame's place in its row: the output is bit-identical
 * from run to run, on any stream and for any grid.  The spectrum ignores d, the tune bin, the
 * sideband, the output format and both NCOs; it uses the handle's rand. */
#define SDDC_DDC_SPECTRUM_BINS 4096
#define SDDC_DDC_WINDOW_RECT 0
#define SDDC_DDC_WINDOW_HANN 1
#define SDDC_DDC_WINDOW_BLACKMAN_HARRIS 2   /* 4-term, 0.35875/0.48829/0.14128/0.01168 */
/* periodic (DFT-even) windows over 8192 points, evaluated in double, rounded once */
int sddc_ddc_spectrum_window(int kind, float *w /* [8192] */);
/* host array of 8192 floats copied to the handle (and device); NULL = rectangular (default).
 * SDDC_ERR_ARG: a non-finite value or sum <= 0.  A change waits for the handle's spectrum
 * launches in flight (the rule of set_channel_fine_tune). */
int sddc_ddc_set_spectrum_window(sddc_ddc_t *h, const float *w);
/* GPU handles; stateless; enqueued on hip_stream, returns after launch. d_psd 4-byte aligned.
 * With blocks_per_row > 1 the call keeps nblk partial rows (16 KB each) in device memory of the
 * handle, grown on demand; calls that share them are ordered one after the other, whatever
 * their streams.  A CPU handle returns SDDC_ERR_STATE. */
int sddc_ddc_spectrum_device(sddc_ddc_t *h, const int16_t *d_in, int nblk, int blocks_per_row,
                             float *d_psd, void *hip_stream);
/* Host buffers, the same [4096 + nblk*65536] layout (stateless: it neither reads nor changes the
 * history kept by process_host).  GPU handle: copy, kernel, copy back, synchronous.  CPU handle:
 * the AVX2 backend. */
int sddc_ddc_spectrum_host(sddc_ddc_t *h, const int16_t *in, int nblk, int blocks_per_row, float *psd);

/* ---- channel spectrum: the averaged power spectrum of the DDC's IQ output -----------------
 * The "zoom" panadapter / waterfall of a tuned channel, on the decimated stream, so its resolution
 * scales with the decimation (n = 4096 at d = 6 resolves fs / 2^19 per bin).  The input is what
 * process_device or process_channels_device wrote: nch channel streams, channel c starting
 * c*in_stride components into the buffer (a component is a float for CF32 and an int16 for CS16,
 * two per complex sample), nsamp complex samples each.  The call reads the buffer in the handle's
 * CURRENT output format (sddc_ddc_set_output_format); under CS16 the sample value is
 * v / cs16_scale.  With the window w[0..n-1] and fpr = frames_per_row, frame f of row r starts at
 * sample (r*fpr + f)*hop:
 *   X_f[k]       = sum_j w[j] x[start_f + j] e^{-2 pi i jk/n}                              k = 0..n-1
 *   psd[c][r][q] = 1/fpr sum_{f < fpr} |X_f[(q + n/2) mod n]|^2 / (sum_j w[j])^2          q = 0..n-1
 * Output index q ascends in frequency: q = n/2 is the channel's centre (DC), q = 0 is -fs_out/2.
 * The output is [nch][nrows][n] float32, contiguous.  A complex tone of amplitude A at a bin centre
 * reads A^2.  n is 256, 512, 1024, 2048 or 4096; hop >= 1 is any integer and may exceed n;
 * fpr >= 1, nrows >= 1, 1 <= nch <= SDDC_DDC_MAX_CHANNELS.  The call needs
 * (nrows*fpr - 1)*hop + n <= nsamp and, when nch > 1, an even in_stride >= 2*nsamp (every channel
 * starts on a complex sample), and nch*nrows < 2^31; a violation returns SDDC_ERR_ARG.
 * The scale 1/(fpr (sum w)^2 s^2), s = cs16_scale under CS16 and 1 under CF32, is formed in double
 * and applied once, at the final store, so CS16 samples enter the transform as exact integers.
 * A stored value depends only on the samples of its row and the call's parameters, through a fixed
 * sequence of float operations (no atomics): it is bit-identical from run to run, on any stream,
 * for any grid, for a channel computed alone or among others, and for row r of a call against
 * row 0 of a call whose buffer starts at sample r*fpr*hop.
 * The spectrum ignores d, the tune bin, the sideband, rand and the NCOs: it is the spectrum of the
 * samples it is given.  With the sideband set to lsb the DDC has already conjugated them, so the
 * display is mirrored, as the listener expects. */
/* The three SDDC_DDC_WINDOW_* kinds over n points (n = 2^k, 32..8192): periodic, evaluated in
 * double, rounded once.  sddc_ddc_window(kind, 8192, w) equals sddc_ddc_spectrum_window(kind, w)
 * bit for bit. */
int sddc_ddc_window(int kind, int n, float *w /* [n] */);
/* host array of n floats copied to the handle (and device); the handle keeps this one window with
 * its length.  NULL = rectangular (default; n is then ignored and calls of any n are valid).
 * SDDC_ERR_ARG: a non-finite value, a sum <= 0, an n outside the five sizes.  A change waits for
 * the handle's channel-spectrum launches in flight (the rule of set_spectrum_window). */
int sddc_ddc_set_channel_spectrum_window(sddc_ddc_t *h, const float *w, int n);
/* GPU handles; stateless; enqueued on hip_stream, returns after launch.  d_iq aligned to one
 * complex sample of the format (8 bytes CF32, 4 bytes CS16), d_psd 4-byte aligned.  Another n
 * than the stored window's returns SDDC_ERR_STATE, as does a CPU handle.  One work item per
 * (channel, row) runs on n/16 threads, so a call with a single row of a single channel uses one
 * sub-group of one workgroup: give it rows or channels to fill the device. */
int sddc_ddc_channel_spectrum_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride,
                                     int n, int hop, int frames_per_row, int nrows, float *d_psd, void *hip_stream);
/* Host buffers, the same layout.  GPU handle: copy in, kernel, copy back, synchronous, in device
 * buffers of its own (it never touches the host path's slots or history).  CPU handle: the AVX2
 * backend's FFT of n points, the same definition with the same single final scale. */
int sddc_ddc_channel_spectrum_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride,
                                   int n, int hop, int frames_per_row, int nrows, float *psd);

/* ---- channel decimator: a streaming second-stage FIR for narrowband channels --------------
 * An integer-factor decimating FIR with real taps, applied independently to every channel stream
 * of the DDC's output: the step between process_channels_device (1 MS/s per channel at d = 6 of a
 * 128 MS/s ADC) and a narrowband demodulator (a few tens of kS/s).  For channel c, the taps
 * h[0..ntaps-1] and the factor R:
 *   v_c[i] = sum_{j < ntaps} h[j] x_c[i - j]       i = stream index since the last set or reset
 *   y_c[m] = v_c[m*R]                               m = 0, 1, 2, ...
 * with x_c[i] = 0 for i < 0.  A call consumes nsamp samples per channel and produces nsamp / R
 * outputs; the handle keeps the last ntaps-1 sample values of each channel as float32 (on the
 * device for a GPU handle, on the host for a CPU handle) and the next call continues the stream.
 * nsamp is a positive multiple of R, so the decimation phase never moves (the DDC's output
 * lengths nblk*(32768>>d) make every power of two trivial).  The group delay is (ntaps-1)/2 input
 * samples, (ntaps-1)/(2R) output samples, for symmetric taps; y_c[0] is the response to x_c[0]
 * alone through h[0].
 * Input: as for the channel spectrum, channel c starts c*in_stride components into the buffer
 * (for nch > 1 in_stride is even and >= 2*nsamp), the base pointer is aligned to one complex
 * sample, and the buffer is read in the handle's CURRENT output format: CF32 the float pair as
 * stored, CS16 x = (float)v * inv_s with inv_s = (float)(1.0 / (double)cs16_scale).  The kept
 * values are sample values, not codes, so the format may change between calls.
 * Output: CF32; channel c's nsamp/R complex samples start c*out_stride floats into the output
 * (for nch > 1 out_stride is even and >= 2*nsamp/R), which is 8-byte aligned.  Nothing is written
 * between the streams or outside them.
 * A stored output depends only on its ntaps sample values and the taps, through a sequence of
 * float operations fixed by the tap index (no atomics): it is bit-identical from run to run, on any
 * stream, for any grid, for a channel alone or among others, and for one call of N samples
 * against any cut of the same samples into several calls.  Each component is within
 * gamma * sum_j |h[j]| |x[mR - j]|, gamma = n u / (1 - n u), n = ntaps + 1, u = 2^-24, of the exact sum. */
#define SDDC_DDC_DECIM_MAX_TAPS   1024
#define SDDC_DDC_DECIM_MAX_FACTOR 64
/* taps: host array of ntaps floats (1..1024, all finite), 2 <= factor <= 64, 1 <= nch <=
 * SDDC_DDC_MAX_CHANNELS; a violation returns SDDC_ERR_ARG.  NULL or ntaps == 0 turns the decimator
 * off and frees its state.  Every set call copies the taps, sizes the tails and zeroes them, even
 * with unchanged parameters.  A change waits for the handle's decimator launches in flight (the
 * rule of set_channel_fine_tune). */
int sddc_ddc_set_channel_decimator(sddc_ddc_t *h, const float *taps, int ntaps, int factor, int nch);
/* zero every channel's tail: the next call starts a new stream (SDDC_ERR_STATE: no decimator set) */
int sddc_ddc_channel_decimator_reset(sddc_ddc_t *h);
/* nsamp / factor; 0 if the factor is outside 2..64 or does not divide nsamp */
size_t sddc_ddc_channel_decimate_samples(int factor, size_t nsamp);
/* GPU handles; enqueued on hip_stream, returns after launch.  SDDC_ERR_STATE: no decimator set,
 * another nch than the set one, a CPU handle.  SDDC_ERR_ARG: nsamp == 0 or no multiple of the
 * factor, a bad stride or alignment, a null buffer.  A failed call changes no state.  The calls of
 * one handle share the tails: they run one after the other in call order, whatever their streams
 * (a call waits for the earlier calls' launches, as the spectrum calls do for their shared rows). */
int sddc_ddc_channel_decimate_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride,
                                     float *d_out, size_t out_stride, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernel, copy back, synchronous, in device
 * buffers of its own; it advances the same device tails as the device call.  CPU handle: the same
 * definition, bound and order of the sum as the device: bit-identical to a GPU handle. */
int sddc_ddc_channel_decimate_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride,
                                   float *out, size_t out_stride);

/* ---- channel resampler: a streaming rational L/M polyphase FIR per channel ------------------
 * The DDC and the channel decimator produce fs_adc / 2^(d+1) / R; the rates demodulators want (48 k
 * audio, 192 k or 250 k WFM, 2.048 M or 2.4 M, symbol-rate multiples) are rational multiples of
 * those.  For channel c, the real prototype taps h[0..ntaps-1], the interpolation factor L (up) and
 * the decimation factor M (down):
 *   u_c[i*L] = x_c[i], u_c = 0 elsewhere;   v_c[n] = sum_k h[k] u_c[n - k];   y_c[m] = v_c[m*M]
 * which, with m*M = s*L + p (0 <= p < L), K = ceil(ntaps / L) and h[k] = 0 for k >= ntaps, is
 *   y_c[m] = sum_{j < K} h[p + j*L] * x_c[s - j],      x_c[i] = 0 for i < 0.
 * There is NO implied gain: zero-stuffing divides the passband gain by L, so a caller who wants
 * unity gain designs h with DC gain L.  Example, 1 MS/s -> 48 kS/s (6/125): the prototype runs at
 * 6 MS/s; a pass band to 15 kHz = 0.0025 of that rate and a stop band from 48 - 15 = 33 kHz = 0.0055
 * keep every alias out of the pass band (70 dB with 1536 taps):
 *   sddc_ddc_kaiser(1536, 70.0f, 0.0025f, 0.0055f, taps);   for (i = 0; i < 1536; i++) taps[i] *= 6;
 *   sddc_ddc_set_channel_resampler(h, taps, 1536, 6, 125, nch);
 * Output m exists once sample s = floor(m*M/L) has been consumed: after N samples in total the
 * stream has produced ceil(N*L/M) outputs, so a call of nsamp samples at position N0 produces
 * ceil((N0+nsamp)*L/M) - ceil(N0*L/M) outputs per channel (sddc_ddc_resample_count).  That count
 * may be 0 (M > L and a short call): such a call is legal, writes nothing and still advances the
 * tails and the position.  nsamp is any value >= 1 (at most 2^40).
 * State per handle: each channel's last K-1 sample values as float32 (on the device for a GPU
 * handle, on the host for a CPU handle), and one stream position shared by all channels, kept on
 * the host in reduced form (the phase depends on it modulo M only), so a stream of any length
 * overflows nothing.
 * Input and output: exactly as for the channel decimator (in_stride / out_stride in components /
 * floats, even, >= 2*nsamp / 2*nout when nch > 1; the input is read in the handle's CURRENT output
 * format, CS16 as (float)v * (float)(1.0 / (double)cs16_scale); the output is CF32, 8-byte
 * aligned).  Nothing is written between the streams or outside them.
 * A stored output depends only on its K sample values and its phase's taps, through the sequence
 * a[j mod 4] = fma(h[p + j*L], x[s - j], a[j mod 4]), j = 0 .. K-1, y = (a0 + a1) + (a2 + a3) on the
 * device (another fixed order on a CPU handle): it is bit-identical from run to run, on any
 * stream, for any grid, for a channel alone or among others, for any cut of the same samples
 * into calls and at any stream position.  Each component is within
 * gamma * sum_j |h[p + j*L]| |x[s - j]|, gamma = n u / (1 - n u), n = K + 1, u = 2^-24, of the exact sum.
 * The decimator and the resampler may both be set on one handle; their states are independent. */
#define SDDC_DDC_RESAMPLE_MAX_UP         32
#define SDDC_DDC_RESAMPLE_MAX_DOWN       256
#define SDDC_DDC_RESAMPLE_MAX_TAPS       4096
#define SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS 1024   /* K = ceil(ntaps / up) */
/* taps: host array of ntaps floats (1..4096, all finite), 1 <= up <= 32, 1 <= down <= 256,
 * gcd(up, down) = 1 and not up = down = 1, ceil(ntaps / up) <= 1024, 1 <= nch <=
 * SDDC_DDC_MAX_CHANNELS; a violation returns SDDC_ERR_ARG.  NULL or ntaps == 0 turns the resampler
 * off and frees its state.  Every set call copies the taps, sizes the tails, zeroes them and sets
 * the position to 0.  A change waits for the handle's resampler launches in flight. */
int sddc_ddc_set_channel_resampler(sddc_ddc_t *h, const float *taps, int ntaps, int up, int down, int nch);
/* zero every channel's tail and the position: the next call starts a new stream (SDDC_ERR_STATE:
 * no resampler set) */
int sddc_ddc_channel_resampler_reset(sddc_ddc_t *h);
/* ceil((pos+nsamp)*up/down) - ceil(pos*up/down) for any pos; 0 on factors outside the ranges above
 * or nsamp > 2^40 */
size_t sddc_ddc_resample_count(int up, int down, uint64_t pos, size_t nsamp);
/* what the handle's NEXT call of nsamp samples would produce per channel (0 also: no resampler set) */
size_t sddc_ddc_channel_resample_samples(sddc_ddc_t *h, size_t nsamp);
/* GPU handles; enqueued on hip_stream, returns after launch.  *nout (may be NULL) receives the
 * call's outputs per channel; d_out needs room for them (channel_resample_samples beforehand).
 * SDDC_ERR_STATE: no resampler set, another nch than the set one, a CPU handle.  SDDC_ERR_ARG:
 * nsamp == 0, a bad stride or alignment, a null buffer.  A failed call changes no state.  The calls
 * of one handle share the tails and the position: they run one after the other in call order,
 * whatever their streams. */
int sddc_ddc_channel_resample_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride,
                                     float *d_out, size_t out_stride, size_t *nout, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernel, copy back, synchronous; it advances
 * the same device tails and position as the device call.  CPU handle: the AVX2 backend, the same
 * definition and bound (another fixed order of the sum, also independent of the cut). */
int sddc_ddc_channel_resample_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride,
                                   float *out, size_t out_stride, size_t *nout);

/* ---- channel demodulator: streaming AM / FM / BFO audio from the channel streams -----------
 * The last link of the chain DDC -> decimator -> resampler: real audio (or a discriminator / product
 * detector output) from every channel stream, on the device, continuous across calls.  For channel c
 * with mode m_c, gain g_c (a finite float), 32-bit phase increment w_c, stream index i = 0, 1, ..
 * since the last set or reset, sample values x_c[i] = (I, Q) read exactly as the decimator reads them
 * (the handle's CURRENT output format, CS16 as (float)v * (float)(1.0 / (double)cs16_scale)) and
 * x_c[-1] = 0:
 *   SDDC_DDC_DEMOD_AM   y = g * sqrtf(fmaf(I, I, Q*Q))
 *   SDDC_DDC_DEMOD_FM   the quadrature discriminator: with (I', Q') = x_c[i-1],
 *                       re = fmaf(I, I', Q*Q'),  im = fmaf(Q, I', -(I*Q')),  y = g * angle(im, re);
 *                       angle(0, 0) = +0.0f, so y_c[0] of a new stream is zero.  A tone e^{j 2 pi f i}
 *                       reads g * 2 pi f; for NBFM g = fs / (2 pi deviation) gives +-1 at full deviation.
 *   SDDC_DDC_DEMOD_BFO  the product detector (real part after a rotation):
 *                       phi_i = 2 pi ((w_c * (p + i)) mod 2^32) / 2^32, p the stream position, in
 *                       exact 32-bit modular arithmetic;  y = g * fmaf(I, cos phi_i, -(Q * sin phi_i)).
 *                       w = 0 gives y = g*I exactly, w = 2^30 the sequence g*I, -g*Q, -g*I, g*Q
 *                       exactly (the sine and cosine are exact at quarter cycles).  With the
 *                       per-channel fine-tune NCO and the decimator's real low-pass this is the third
 *                       step of a Weaver SSB / CW demodulator.
 * angle and the sine / cosine of a phase word are this library's own routines (csrc/demod_math.h):
 * fixed sequences of correctly rounded float operations (fmaf, +, *, /, sqrtf; no libm), the same
 * text on the device and in the CPU backend.  angle is within 4 ulp of the true angle (<= 8 u |theta|,
 * u = 2^-24), the sine and cosine within 4 u absolute, the rounding of the phase included.  So a GPU
 * handle and a CPU handle produce BIT-IDENTICAL demodulated samples in all three modes and both
 * output formats, for inputs whose components are 0 or of magnitude in [2^-40, 2^40] (no subnormal
 * intermediate).  Against the float64 value y64 of the same float32 sample values:
 *   AM   |y - y64| <= 4 u |y64|
 *   FM   |y - g theta64| <= |g| (4 u + 8 u |theta64|)      where |x[i]| |x[i-1]| > 0
 *   BFO  |y - y64| <= |g| (|I| + |Q|) 6 u
 * Output: SDDC_DDC_AUDIO_F32 writes y; SDDC_DDC_AUDIO_S16 writes y rounded to nearest even and
 * clamped to [-32768, 32767], NaN as 0.  Channel c's nsamp outputs start c*out_stride output samples
 * into the output (for nch > 1 out_stride >= nsamp, any parity), which is aligned to one output sample
 * (4 or 2 bytes).  Nothing is written between the streams or outside them; an S16 stream with an odd
 * start or length is finished with 2-byte stores.  Input: layout, strides and alignment exactly as
 * for the channel decimator; nsamp is any value >= 1 (at most 2^40).
 * Channel power (squelch, scanner): power may be NULL, else nch floats that receive
 *   P_c = (sum_i fmaf(I, I, Q*Q)) * (float)(1.0 / (double)nsamp)
 * over THIS call's samples, summed in an order that depends on nsamp only (fixed tile sums added in
 * a fixed order, no float atomics): bit-identical from run to run, for any grid and for a channel
 * alone or among others; a per-call figure, so not cut-invariant.  |P - P64| <= gamma_n P64 with
 * n = nsamp + 3, gamma_n = n u / (1 - n u); a GPU and a CPU handle agree within twice that.
 * State per handle, independent of the decimator's and the resampler's: each channel's last sample
 * value as float32 (I, Q) (on the device for a GPU handle), and one stream position shared by all
 * channels, kept on the host modulo 2^32, so a stream of any length overflows nothing.  A demodulated
 * sample depends only on its own sample value, the one before it and its stream index: it is
 * bit-identical from run to run, on any stream, for any grid, for a channel alone or among others, and
 * for any cut of the same samples into calls. */
#define SDDC_DDC_DEMOD_AM  0
#define SDDC_DDC_DEMOD_FM  1
#define SDDC_DDC_DEMOD_BFO 2
#define SDDC_DDC_AUDIO_F32 0
#define SDDC_DDC_AUDIO_S16 1
/* round(relative_freq * 2^32) mod 2^32: the BFO word of a frequency in cycles per sample,
 * relative_freq in [-0.5, 0.5) (other values are taken modulo 1; not finite: 0).  Stateless. */
uint32_t sddc_ddc_bfo_word(double relative_freq);
/* modes: host array of nch values SDDC_DDC_DEMOD_*; gains: nch finite floats (NULL: all 1);
 * bfo_words: nch phase increments (NULL: all 0; read in BFO mode only); 1 <= nch <=
 * SDDC_DDC_MAX_CHANNELS; out_format SDDC_DDC_AUDIO_*; a violation returns SDDC_ERR_ARG.  modes NULL
 * or nch == 0 turns the demodulator off and frees its state.  Every set call zeroes the last samples
 * and the position.  A change waits for the handle's demodulator launches in flight. */
int sddc_ddc_set_channel_demodulator(sddc_ddc_t *h, const int *modes, const float *gains, const uint32_t *bfo_words,
                                     int nch, int out_format);
/* zero every channel's last sample and the position: the next call starts a new stream
 * (SDDC_ERR_STATE: no demodulator set) */
int sddc_ddc_channel_demodulator_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  d_power: NULL or nch device floats.
 * SDDC_ERR_STATE: no demodulator set, another nch than the set one, a CPU handle.  SDDC_ERR_ARG:
 * nsamp == 0 or above 2^40, a bad stride or alignment, a null buffer.  A failed call changes no state.
 * The calls of one handle share the last samples and the position: they run one after the other in
 * call order, whatever their streams. */
int sddc_ddc_channel_demodulate_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride,
                                       void *d_out, size_t out_stride, float *d_power, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernel, copy back, synchronous; it advances
 * the same device state as the device call.  CPU handle: the same definition through the same
 * arithmetic header, sample by sample; its power is summed in sample order. */
int sddc_ddc_channel_demodulate_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride,
                                     void *out, size_t out_stride, float *power);

/* ---- channel audio resampler: a streaming rational L/M polyphase FIR on real audio ----------
 * The decimator and the resampler above change the rate of IQ; every stage from the demodulator on
 * works on real audio and none of them could change its rate.  This one does: the 48 kS/s
 * discriminator output of an NBFM channel to the 8 or 12 kS/s sense stream of the tone detector and
 * the DCS decoder (1/6, 1/4), the 250 kS/s output of a WFM discriminator to 48 kS/s audio (24/125),
 * 48 k to 8 k / 16 k S16 for a voice codec.  It is the channel resampler's sum on nch REAL streams:
 * real prototype taps h[0..ntaps-1], L = up, M = down, the resampler's limits (1 <= L <= 32, 1 <= M
 * <= 256, gcd = 1, not L = M = 1, ntaps <= 4096, K = ceil(ntaps / L) <= 1024), integer decimation is
 * L = 1, and there is NO implied gain (a caller who wants unity gain designs h with DC gain L).
 * Sample values: SDDC_DDC_AUDIO_F32 is read as stored, SDDC_DDC_AUDIO_S16 as (float)v, as the audio
 * filter reads it; there is no cs16_scale.  Output m has m*M = s*L + p (0 <= p < L), x[i] = 0 for
 * i < 0, and is the sequence
 *     a[j mod 4] = fmaf(h[p + j*L], x[s - j], a[j mod 4])   for j = 0 .. K-1;   y = (a0 + a1) + (a2 + a3)
 * (h[k] = 0 for k >= ntaps; csrc/audio_resample_math.h) on BOTH backends: unlike the IQ resampler, a
 * CPU handle runs the device's order.  S16 output is rounded as the demodulator rounds it: nearest
 * even, clamped to [-32768, 32767], NaN as 0.
 * Outputs per call: the resampler's count, ceil((N0+nsamp)*L/M) - ceil(N0*L/M)
 * (sddc_ddc_resample_count); 0 is legal, writes nothing and still advances the state; 1 <= nsamp <=
 * 2^40.  State per handle, independent of the IQ resampler's (both may be set): each channel's last
 * K-1 sample VALUES as float32 (on the device for a GPU handle, on the host for a CPU handle), and one
 * stream position on the host, reduced modulo M.  Values are kept, not codes, so the input format may
 * change between two calls of one stream (sddc_ddc_channel_audio_resampler_formats); a set call
 * starts a new stream.
 * Layout: the audio stages'.  Channel c starts c*in_stride input samples into the input and
 * c*out_stride output samples into the output; for nch > 1 in_stride >= nsamp and out_stride >= nout,
 * any parity.  The buffers are aligned to one sample of their format only (4 or 2 bytes).  Nothing is
 * written between the streams or outside them.
 * An output is BIT-IDENTICAL for any cut of the same samples into calls, at any position, for any
 * grid, on any stream, for a channel alone or among others, and between a GPU handle and a CPU handle.
 * Each F32 output is within gamma * sum_j |h[p + j*L]| |x[s - j]|, gamma = n u / (1 - n u), n = K + 1,
 * u = 2^-24, of the exact sum; S16 output adds 1/2 and the clamp. */
/* taps, ntaps, up, down, nch: as for sddc_ddc_set_channel_resampler; in_format, out_format:
 * SDDC_DDC_AUDIO_*; a violation (also a tap that is not finite) returns SDDC_ERR_ARG.  NULL or ntaps
 * == 0 turns the stage off and frees its state.  Every set call copies the taps, zeroes the tails and
 * the position, and waits for this stage's launches in flight. */
int sddc_ddc_set_channel_audio_resampler(sddc_ddc_t *h, const float *taps, int ntaps, int up, int down, int nch,
                                         int in_format, int out_format);
/* The formats of the NEXT calls, the stream left as it is: the tails hold sample values, not codes, so
 * the input (and the output) format may change between two calls of one stream.  SDDC_ERR_ARG: an
 * unknown format; SDDC_ERR_STATE: not set. */
int sddc_ddc_channel_audio_resampler_formats(sddc_ddc_t *h, int in_format, int out_format);
/* zero every channel's tail and the position: the next call starts a new stream (SDDC_ERR_STATE:
 * not set) */
int sddc_ddc_channel_audio_resampler_reset(sddc_ddc_t *h);
/* what the handle's NEXT call of nsamp samples would produce per channel (0 also: not set) */
size_t sddc_ddc_channel_audio_resample_samples(sddc_ddc_t *h, size_t nsamp);
/* GPU handles; enqueued on hip_stream, returns after launch.  *nout (may be NULL) receives the
 * call's outputs per channel; d_out needs room for them.  SDDC_ERR_STATE: not set, another nch than
 * the set one, a CPU handle.  SDDC_ERR_ARG: nsamp == 0 or above 2^40, a bad stride or alignment, a null
 * buffer.  A failed call changes no state.  The calls of one handle share the tails and the position:
 * they run one after the other in call order, whatever their streams. */
int sddc_ddc_channel_audio_resample_device(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride,
                                           void *d_out, size_t out_stride, size_t *nout, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernel, copy back, synchronous; it advances
 * the same device tails and position as the device call.  CPU handle: the same sequence, the same bits. */
int sddc_ddc_channel_audio_resample_host(sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride,
                                         void *out, size_t out_stride, size_t *nout);

/* ---- channel audio filter: a streaming biquad cascade per channel on the device -----------
 * What stands between the demodulator and playable audio: DC blocking, de-emphasis, the 300 Hz
 * high-pass of a voice channel, a notch.  Each of nch real audio streams runs through its own cascade
 * of S = nsec (1..4, the same count for every channel) biquad sections; a section is five floats
 * (b0, b1, b2, a1, a2) with a0 = 1, in transposed direct form II; a channel that wants fewer sections
 * pads with (1, 0, 0, 0, 0), which passes finite values through exactly.  AGC is the next stage
 * (sddc_ddc_channel_agc_* below): its recurrence is max-plus, not linear, and has a block form of its own.
 * Input: SDDC_DDC_AUDIO_F32, or SDDC_DDC_AUDIO_S16 read as (float)v; output F32, or S16 rounded as
 * the demodulator rounds it.  The demodulator's output feeds this stage directly: the same buffer,
 * stride and format.
 * The definition, which both backends compute bit for bit (csrc/audio_iir_math.h; fmaf and * are the
 * correctly rounded float operations, nothing is contracted).  One step of the cascade on a state
 * s[2S] with input x, for k = 0 .. S-1:
 *     y = fmaf(b0, x, s1);  s1 = fmaf(-a1, y, fmaf(b1, x, s2));  s2 = fmaf(-a2, y, b2 * x);  x = y
 * and the last y is the output.  With B = SDDC_DDC_AUDIO_BLOCK, A_c the 2S x 2S matrix of one
 * zero-input step of channel c in exact arithmetic on the float coefficients and M_c = float(A_c^B)
 * (computed at set time: B zero-input steps in double on each unit vector, every fmaf(a, b, c) as
 * a * b + c with plain, uncontracted * and +), adv(E, Z)_i is acc = Z_i; for j = 0 .. 2S-1:
 * acc = fmaf(M_ij, E_j, acc).  Each channel has three state vectors E (the entry state of the
 * current block), R (the running state) and Zr (the running zero-state state) and one position n, the
 * samples since the last set or reset, all zero then.  Per sample:
 *     y[n] = step(x, R);  step(x, Zr) with its output dropped;  n++;
 *     if n is a multiple of B:  E = adv(E, Zr),  R = E,  Zr = 0.
 * In exact arithmetic this is the plain recurrence.  In float it differs from it by roundings only,
 * and a block's outputs depend on the earlier stream through E alone, so the device runs the blocks
 * of a call in parallel.  The definition never mentions calls, grids or streams: an output sample is
 * BIT-IDENTICAL for any cut of the same samples into calls, for any grid and run length, on any
 * stream, for a channel alone or among others, and between a GPU handle and a CPU handle (the CPU
 * backend sets no FTZ / DAZ and gfx950 code keeps float subnormals, so this includes a decaying
 * filter's subnormal states).
 * Accuracy against the float64 plain recurrence y64 on the same float32 coefficients (u = 2^-24), to
 * first order in u.  A rounding of magnitude at most u |v| is made at each of these values v of a
 * step of section k: y_k (it enters section k's states through -a1, -a2 and the next sections as
 * their input), the new s1_k and the inner fmaf(b1, x, s2) (both enter s1_k), the new s2_k and b2 x
 * (both enter s2_k): 5 roundings per section and sample.  Each adv rounds 2S times per row and uses
 * M's rounded entries: at most (2S + 1) u (|Z_i| + sum_j |M_ij| |E_j|) enters E_i.  With g_q[m] the
 * response of the last section's output, m samples later, to a unit error at source q (g = c A^m v_q:
 * the ABSOLUTE VALUE OF THE POWERS' response, not powers of |A|),
 *     |y[n] - y64[n]| <= bound[n] = 1.01 * ( sum over sources q and samples t <= n of
 *                                             u |v_q[t]| |g_q[n - t]|
 *                                    + sum over boundaries b B <= n and rows i of
 *                                             (2S + 1) u (|Z_i| + sum_j |M_ij| |E_j|) |g_i[n - b B]| )
 * where v_q[t] is the running recurrence's value for t in n's own block and the zero-state
 * recurrence's for t in an earlier block (R restarts from E at every boundary, so only Zr's roundings
 * of earlier blocks survive).  tools/channel_audio_model.py evaluates it; the 1.01 covers the second
 * order.  It assumes no subnormal intermediate.  S16 output adds 1/2 and the clamp.
 * Validity, checked at set time: every coefficient finite, every section strictly inside the
 * stability triangle |a2| < 1 and |a1| < 1 + a2; anything else returns SDDC_ERR_ARG. */
#define SDDC_DDC_AUDIO_BLOCK 256
#define SDDC_DDC_AUDIO_MAX_SECTIONS 4
#define SDDC_DDC_BIQUAD_IDENTITY    0
#define SDDC_DDC_BIQUAD_DC_BLOCK    1
#define SDDC_DDC_BIQUAD_ONE_POLE_LP 2
#define SDDC_DDC_BIQUAD_LOWPASS     3
#define SDDC_DDC_BIQUAD_HIGHPASS    4
#define SDDC_DDC_BIQUAD_NOTCH       5
/* Stateless section designers, computed in double and rounded to float; f in cycles per sample,
 * 0 < f < 0.5; q > 0 is read by LOWPASS, HIGHPASS and NOTCH only.  coeffs receives (b0, b1, b2, a1, a2).
 *   IDENTITY     (1, 0, 0, 0, 0); f and q are not read
 *   DC_BLOCK     r = exp(-2 pi f): b = ((1+r)/2, -(1+r)/2, 0), a = (-r, 0); b1 = -b0 exactly
 *   ONE_POLE_LP  alpha = exp(-2 pi f): b0 = 1 - alpha, a1 = -alpha; a de-emphasis of time constant
 *                tau at sample rate fs is f = 1 / (2 pi tau fs)
 *   LOWPASS, HIGHPASS, NOTCH  the RBJ cookbook forms with Q = q: w = 2 pi f, alpha = sin w / (2 q),
 *                a0 = 1 + alpha, a1 = -2 cos w / a0, a2 = (1 - alpha) / a0; LOWPASS b0 = b2 =
 *                (1 - cos w) / (2 a0), b1 = 2 b0; HIGHPASS b0 = b2 = (1 + cos w) / (2 a0), b1 = -2 b0
 *                exactly; NOTCH b0 = b2 = 1 / a0, b1 = a1.  |H| = q at f for LOWPASS and HIGHPASS.
 * DC_BLOCK and HIGHPASS thus reject DC exactly in exact arithmetic.  A bad kind, f or q (NOT finite
 * included) or a null coeffs returns SDDC_ERR_ARG. */
int sddc_ddc_biquad(int kind, double f, double q, float coeffs[5]);
/* coeffs: host array [nch][nsec][5]; 1 <= nsec <= 4; 1 <= nch <= SDDC_DDC_MAX_CHANNELS; in_format and
 * out_format SDDC_DDC_AUDIO_*; a violation, a coefficient that is not finite or an unstable section
 * returns SDDC_ERR_ARG and sets nothing.  coeffs NULL or nch == 0 turns the stage off and frees its
 * state.  Every set call zeroes the state and the position, and waits for the stage's launches in
 * flight. */
int sddc_ddc_set_channel_audio_filter(sddc_ddc_t *h, const float *coeffs, int nsec, int nch, int in_format,
                                      int out_format);
/* zero every channel's state and the position: the next call starts a new stream (SDDC_ERR_STATE: no
 * filter set) */
int sddc_ddc_channel_audio_filter_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  Channel c's nsamp samples start
 * c*in_stride input samples into d_in and its outputs c*out_stride output samples into d_out (for
 * nch > 1 both strides >= nsamp); the buffers are aligned to one sample of their format and must not
 * overlap; 1 <= nsamp <= 2^40.  Nothing is written between the streams or outside them.
 * SDDC_ERR_STATE: no filter set, another nch than the set one, a CPU handle.  SDDC_ERR_ARG: nsamp == 0
 * or above 2^40, a bad stride or alignment, a null buffer.  A failed call changes no state.  The calls
 * of one handle share the state and the position: they run one after the other in call order, whatever
 * their streams.  A long call is processed in runs of a bounded number of blocks (the scratch of a run
 * is 2 nsec floats per channel and block), which changes no output bit. */
int sddc_ddc_channel_audio_filter_device(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride,
                                         void *d_out, size_t out_stride, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernels, copy back, synchronous; it advances
 * the same device state as the device call.  CPU handle: the definition's loop through the same
 * arithmetic header. */
int sddc_ddc_channel_audio_filter_host(sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride,
                                       void *out, size_t out_stride);

/* ---- channel AGC: a streaming per-channel peak AGC on the device ---------------------------
 * Level control between the demodulator (or the audio filter) and audio that can be played or fed to
 * a codec: an AM or SSB channel at S9+40 and one at S3 leave the device at the same peak level.  A
 * fast-attack, exponential-release peak AGC: the envelope e[n] = max(|x[n]|, d e[n-1]) and the output
 * y[n] = T x[n] / max(e[n], F).  Channel c has three floats: T, the target peak level (T == 0: the
 * channel is bypassed, y = x as it is), d, the release factor per sample (sddc_ddc_agc_decay), and F,
 * the envelope floor: the largest gain is T / F.  What this AGC is NOT: there is no hang timer, no
 * look-ahead and no attack smoothing (a new peak takes the gain down within its own sample); a hang
 * needs a sliding-window maximum and is a later step.
 * Input: SDDC_DDC_AUDIO_F32, or SDDC_DDC_AUDIO_S16 read as (float)v; output F32, or S16 rounded as the
 * demodulator rounds it.  The demodulator's or the audio filter's buffer feeds this stage as it lies:
 * the same buffer, stride and format.
 * The definition, which both backends compute bit for bit (csrc/agc_math.h: *, / and comparisons are
 * the correctly rounded float operations, nothing is contracted, no libm).  The recurrence above is a
 * max-plus recurrence: the maps e -> max(m, k e) compose associatively, as affine maps do, so a block
 * of B = SDDC_DDC_AGC_BLOCK samples collapses to a pair (m, k = d^B).  With dB = float(d^B), computed
 * at set time (eight squarings of (double)d with plain, uncontracted *, then one rounding to float;
 * it may underflow to 0), the magnitude a = |x| except that a NaN gives a = 0 and an infinity
 * a = FLT_MAX, and step(a, e): t = d * e; e = (a > t) ? a : t, each channel has the entry envelope E
 * of the current block, the running envelope R, the running envelope from a zero start Zr and one
 * position n, the samples since the last set or reset, all zero then.  Per sample:
 *     R = step(a, R);  Zr = step(a, Zr);  den = (R > F) ? R : F;  g = T / den;  y[n] = g * x
 *     (a bypassed channel: y[n] = x);  n++;
 *     if n is a multiple of B:  t = dB * E;  E = (Zr > t) ? Zr : t;  R = E;  Zr = 0.
 * In exact arithmetic this is the plain recurrence.  In float it differs from it by roundings only,
 * and a block's outputs depend on the earlier stream through E alone, so the device runs the blocks
 * of a call in parallel.  The envelope runs for bypassed channels too: it is their signal meter.  The
 * definition never mentions calls, grids or streams: an output sample and the envelope are
 * BIT-IDENTICAL for any cut of the same samples into calls, for any grid and run length, on any
 * stream, for a channel alone or among others, and between a GPU handle and a CPU handle (subnormal
 * envelopes of a decay included: no FTZ / DAZ on either side).  A NaN sample leaves the envelope as it
 * is and gives a NaN (S16: 0) at that sample only; an infinite sample sets the envelope to FLT_MAX.
 * den >= |x|, so |y| <= T (1 + 2 u), u = 2^-24: with T <= 32767 / (1 + 2 u) (32767 is not, 32766 is)
 * the stage cannot clip an S16 output.
 * Accuracy against the float64 plain recurrence y64 on the same float32 parameters and samples:
 * every candidate |x[t]| d^(n-t) of the maximum reaches R through at most B - 1 rounded multiplies in
 * the zero-start pass of its own block, one multiply by dB per later boundary (one rounding, plus
 * dB's own rounding) and at most B multiplies in n's block; max is monotone, so with
 * K(n) = ceil((n + 1) / B)
 *     |y[n] - y64[n]| <= 1.01 (2 B + 2 K(n) + 2) u |y64[n]|      (F32 out; S16 adds 1/2 and the clamp)
 * while no envelope on the deciding path is subnormal, which F >= 2^-60 ensures for den.
 * tools/channel_agc_model.py evaluates it.
 * Validity, checked at set time: everything finite; T == 0 or 2^-60 <= T <= 2^60; 2^-60 <= F <= 2^60;
 * 0 <= d < 1; anything else returns SDDC_ERR_ARG and sets nothing. */
#define SDDC_DDC_AGC_BLOCK 256
/* The release factor of a time constant of tau_samples samples: float(exp(-1 / tau_samples)), and
 * 1 - 2^-24 if that rounds to 1.0f.  tau_samples <= 0, a value that is not finite or a null pointer
 * returns SDDC_ERR_ARG.  Stateless. */
int sddc_ddc_agc_decay(double tau_samples, float *decay);
/* params: host array [nch][3] = (T, d, F); 1 <= nch <= SDDC_DDC_MAX_CHANNELS; in_format and out_format
 * SDDC_DDC_AUDIO_*; a violation returns SDDC_ERR_ARG and sets nothing.  params NULL or nch == 0 turns
 * the stage off and frees its state.  Every set call zeroes the envelopes and the position, and waits
 * for the stage's launches in flight.  The state is independent of every other stage's. */
int sddc_ddc_set_channel_agc(sddc_ddc_t *h, const float *params, int nch, int in_format, int out_format);
/* zero every channel's envelopes and the position: the next call starts a new stream (SDDC_ERR_STATE:
 * no AGC set) */
int sddc_ddc_channel_agc_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  Buffers, strides, alignment and
 * 1 <= nsamp <= 2^40 as for sddc_ddc_channel_audio_filter_device; the input and the output must not
 * overlap; nothing is written between the streams or outside them.  d_env: NULL, or nch device floats
 * that receive R_c after the call's last sample: the unfloored envelope, an S-meter per channel, part
 * of the bit-exact guarantee.  SDDC_ERR_STATE: no AGC set, another nch than the set one, a CPU handle.
 * SDDC_ERR_ARG: nsamp == 0 or above 2^40, a bad stride or alignment, a null buffer.  A failed call
 * changes no state.  The calls of one handle share the state and the position: they run one after the
 * other in call order, whatever their streams.  A long call is processed in runs of a bounded number
 * of blocks (the scratch of a run is one float per channel and block), which changes no output bit. */
int sddc_ddc_channel_agc_device(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride, void *d_out,
                                size_t out_stride, float *d_env, void *hip_stream);
/* Host buffers, the same layouts; env NULL or nch floats.  GPU handle: copy in, kernels, copy back,
 * synchronous; it advances the same device state as the device call.  CPU handle: the definition's
 * loop through the same arithmetic header. */
int sddc_ddc_channel_agc_host(sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, void *out,
                              size_t out_stride, float *env);

/* ---- channel noise blanker: a streaming per-channel impulse blanker on IQ -------------------
 * Every stage after the DDC is linear or memoryless on the IQ, so an impulse (ignition, power-line
 * arcs, switching supplies) that is a few samples long where the channel is still wide becomes a
 * filter-long ringing burst after the channel decimator.  The blanker therefore sits between the DDC's
 * channel output (sddc_ddc_process_channels_device, or a single d = 0..6 stream) and the decimator: it
 * zeroes the samples whose power exceeds a multiple of the recent mean block power, with a guard of g
 * samples on each side, and delays every channel by g samples.  It is feed-forward.  What this blanker
 * is NOT: it zeroes, it does not interpolate or hold.  The reference contains the impulses themselves:
 * MEAN is raised by them and reacts to a level jump within one block; MEDIAN ignores a minority of
 * contaminated blocks but takes M / 2 blocks to follow a jump, so a keyed strong carrier is chewed at
 * each attack.  After blocks of exact zeros the reference is 0, and only qmin keeps the next samples
 * from being blanked.
 *
 * The definition (normative; csrc/blanker_math.h holds the operations, shared by both backends, float,
 * contraction off, only *, +, comparisons and selects).  B = SDDC_DDC_BLANKER_BLOCK = 256.  Per handle:
 * the guard g (0..SDDC_DDC_BLANKER_MAX_GUARD), the reference length M (1..
 * SDDC_DDC_BLANKER_MAX_REF_BLOCKS blocks), the reference mode and the stream format (SDDC_DDC_FMT_CF32 or
 * _CS16: the format of the buffers given to this stage, not the handle's current output format).  Per
 * channel c two floats: k2_c, the threshold as a power ratio (0: the channel is bypassed, a pure delay),
 * and qmin_c, an absolute floor on |x|^2 below which nothing is ever a hit.  i >= 0 is the stream index
 * since the last set or reset, k = i div B its block, x[i] = (I, Q) as float: CF32 as stored, CS16
 * (float)v with no scale (qmin is in codes squared).
 *   Power.      q[i] = (I * I) + (Q * Q), three roundings; q is non-finite if !(q <= FLT_MAX).
 *   Block power. p_k: the balanced pairwise tree over the 256 values of block k in sample order (level 0
 *               adds (q[0] + q[1]), (q[2] + q[3]), ...; eight levels); a non-finite q enters as 0.
 *   Reference.  n = min(k, M); the values p_{k-n} .. p_{k-1} (full blocks only).  MEAN: S = (..((p_{k-n}
 *               + p_{k-n+1}) + p_{k-n+2}) ..) + p_{k-1}, P_k = S * rn[n], rn[n] = (float)(1.0 / n).
 *               MEDIAN: P_k is the value of rank (n - 1) div 2 (0-based, ascending) of the n values.
 *               n = 0 (block 0 of a stream): no finite sample of it is a hit.
 *   Threshold.  thr_c = (float)((double)k2_c / 256.0) at set time; t = thr_c * P_k; t_k = (t > qmin_c) ?
 *               t : qmin_c.
 *   Hit.        k2_c > 0: hit[i] = (q[i] > t_k) or q[i] non-finite.  A bypassed channel has no hits.
 *   Mask.       blank[i] if any hit[j] with |j - i| <= g, j >= 0.
 *   Output.     A call of nsamp samples writes nsamp samples per channel; y[n] = 0 for n < g, otherwise
 *               y[n] = blank[n - g] ? (+0, +0) : x[n - g], a kept sample bit for bit (float payloads,
 *               int16 codes).
 *   Count.      Optional: per channel the outputs n >= g of this call with blank[n - g].  The counts of
 *               the calls of a cut add up to the count of the uncut call.
 * A written sample depends only on the samples of its own block, the M blocks before it and g samples
 * after it, so outputs and counts are bit-identical from run to run, for any grid, run length and cut
 * of a stream into calls, for a channel alone or among others, and between a GPU handle and a CPU
 * handle.  Range of that guarantee: components that are 0 or of magnitude in [2^-40, 2^40] (then q and
 * the block powers are 0 or in [2^-80, 2^89], S < 2^93, thr in [2^-8, 2^32], t < 2^125 and, where
 * P > 0, t >= 2^-88: no overflow, nothing subnormal on the deciding path; blanker_math.h has the
 * derivation).  Validity, checked at set time: everything finite; k2 == 0 or 1 <= k2 <= 2^40;
 * 0 <= qmin <= 2^80; the ranges above; anything else returns SDDC_ERR_ARG and sets nothing.
 * State per handle, on the device for a GPU handle, independent of every other stage's: the position,
 * the last M block powers, the unfinished block's q values, the last g stored samples and the position
 * of the last hit among the last 2 g samples (all the mask needs of their hit flags). */
#define SDDC_DDC_BLANKER_BLOCK 256
#define SDDC_DDC_BLANKER_MAX_GUARD 64
#define SDDC_DDC_BLANKER_MAX_REF_BLOCKS 16
#define SDDC_DDC_BLANKER_MEAN 0
#define SDDC_DDC_BLANKER_MEDIAN 1
/* k2 = 10^(db / 10) rounded to float.  SDDC_ERR_ARG outside 0..120 dB, not finite, or k2 NULL.  Stateless. */
int sddc_ddc_blanker_threshold(double db, float *k2);
/* params: host array [nch][2] = (k2, qmin); 1 <= nch <= SDDC_DDC_MAX_CHANNELS; a violation returns
 * SDDC_ERR_ARG and sets nothing.  params NULL or nch == 0 turns the stage off and frees its state.  Every
 * set call zeroes the state and the position, and waits for the stage's launches in flight. */
int sddc_ddc_set_channel_blanker(sddc_ddc_t *h, const float *params, int nch, int guard, int ref_blocks, int ref_mode,
                                 int format);
/* zero the state and the position: the next call starts a new stream (SDDC_ERR_STATE: no blanker set) */
int sddc_ddc_channel_blanker_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  Layouts as for sddc_ddc_channel_decimate_
 * device, on both sides and in the set format: channel c's nsamp samples at c * stride components,
 * strides even and >= 2 nsamp for nch > 1, bases aligned to one complex sample; any 1 <= nsamp <= 2^40;
 * the input and the output must not overlap; nothing is written between the streams or outside them.
 * d_count: NULL, or nch device uint32_t.  SDDC_ERR_STATE: no blanker set, another nch than the set one,
 * a CPU handle.  SDDC_ERR_ARG: the rest.  A failed call changes no state.  The calls of one handle share
 * the state and the position: they run one after the other in call order, whatever their streams. */
int sddc_ddc_channel_blank_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride, void *d_out,
                                  size_t out_stride, uint32_t *d_count, void *hip_stream);
/* Host buffers, the same layouts; count NULL or nch uint32_t.  GPU handle: copy in, kernels, copy back,
 * synchronous; it advances the same device state as the device call.  CPU handle: the definition's
 * loop through the same arithmetic header. */
int sddc_ddc_channel_blank_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, void *out,
                                size_t out_stride, uint32_t *count);

/* ---- channel squelch: a streaming per-channel gate on the audio --------------------------------
 * An empty NBFM channel leaves the discriminator as full-scale hiss, and the AGC turns an empty AM or SSB
 * channel up to its target: the chain yields playable audio only for occupied channels.  The squelch is
 * the last stage: it gates each channel's audio (the demodulator's, the audio filter's or the AGC's
 * buffer as it lies) by the level of a sense stream, with an attack, a hang and an optional fade, and it
 * tells the host which channels are open without moving any audio.  Three uses: a carrier squelch (sense
 * = the demodulator's IQ input, LEVEL), an FM noise squelch (sense = the discriminator audio through a
 * high-pass of the audio filter into a second buffer, NOISE) and a plain audio-level gate (SELF).  What
 * this squelch is NOT: it has no look-ahead (up to A + 1 blocks of a transmission's start are lost), no
 * tone (CTCSS) decode (that is the channel tone detector below), and its thresholds do not adapt to the noise floor.
 *
 * The definition (normative; csrc/squelch_math.h holds the operations, shared by both backends, float,
 * contraction off, only *, +, comparisons, selects and integers).  B = SDDC_DDC_SQUELCH_BLOCK = 256; i >= 0
 * is the stream index since the last set or reset, k = i div B its block.
 *   Inputs.     The audio: nch x nsamp samples, SDDC_DDC_AUDIO_F32 or _S16 (read as (float)v).  The sense
 *               stream: nsamp samples per channel at the same rate, of the kind the set call fixes:
 *               SDDC_DDC_SQUELCH_SENSE_SELF   the audio itself (d_sense ignored)           q = x * x
 *               .._SENSE_F32 / .._SENSE_S16   a separate real buffer (S16 as (float)v)     q = x * x
 *               .._SENSE_CF32 / .._SENSE_CS16 the complex buffer the demodulator read      q = (I * I) + (Q * Q)
 *               (strides in components, even for the complex kinds, as the channel decimator's).
 *   Block level. p_k: the balanced pairwise tree over the 256 q values of block k in sample order (level 0
 *               adds (q[0] + q[1]), (q[2] + q[3]), ...; eight levels: the blanker's block power).  A q that
 *               is not finite (!(q <= FLT_MAX)) enters as 0 and marks the block bad.
 *   Per channel. A mode: SDDC_DDC_SQUELCH_OFF (always open, y = x from sample 0), _LEVEL (opens on a high
 *               level), _NOISE (opens on a low level), _MUTE (always closed); and two thresholds as
 *               mean-square per sample, T_open and T_close; the set call stores To = 256 T_open, Tc = 256
 *               T_close (exact).  LEVEL: u_k = p_k > To, v_k = p_k > Tc, and T_close <= T_open.  NOISE:
 *               u_k = p_k < To, v_k = p_k < Tc, and T_close >= T_open.  A bad block has u = v = false.
 *   Per handle. The attack A (1..255 blocks), the hang H (0..65535 blocks), fade (0 / 1), the sense kind,
 *               the audio formats in and out.
 *   State.      Per channel, integers, all zero on a new stream; after block k:
 *                   r = u_k ? min(r + 1, A) : 0
 *                   n = v_k ? 0 : min(n + 1, H + 1)
 *                   open = open ? (n <= H) : (r >= A)
 *               (open after k iff the last block ending a run of >= A u-blocks is later than the last block
 *               ending a run of >= H + 1 non-v blocks.)
 *   Gate.       G_k = open after block k - 1; G_0 = G_{-1} = 0.  OFF: G = 1 everywhere; MUTE: G = 0.  Block
 *               k's samples never need block k's level: the stage is causal and has no delay.
 *   Weight.     Of sample i of block k.  Fade off: w = G_k.  Fade on: w = G_k where G_k = G_{k-1}; on an
 *               opening block w = (i + 1) / 256, on a closing block w = (255 - i) / 256 (exact floats).
 *   Output.     w = 1: x unchanged (F32 words and S16 codes bit for bit; S16 to F32 is (float)v, F32 to S16
 *               the demodulator's conversion).  w = 0: +0.  Otherwise x * w, one rounding, then the
 *               demodulator's output conversion (round to nearest even, clamp, NaN -> 0).
 *   Side outputs, each NULL or nch entries: open (uint32): `open` after the last completed block of the
 *               stream so far (OFF: 1, MUTE: 0); count (uint32, modulo 2^32): the call's output samples
 *               whose block has G_k = 1, the counts of consecutive calls add up to the count of one call
 *               over the same samples; level (float): p of the last completed block, 0 before any, also in
 *               OFF and MUTE: the figure to calibrate thresholds from (divide by 256 for a mean square).
 * Outputs and side outputs are bit-identical from run to run, for any grid, run length and cut of a
 * stream into calls, for a channel alone or among others, and between a GPU handle and a CPU handle.
 * Range of that guarantee: the blanker's: components that are 0 or of magnitude in [2^-40, 2^40],
 * thresholds finite, >= 0 and <= 2^80.  Outside it both sides perform the same operations, and no value
 * is a reason for a memory fault.  Against a float64 evaluation of the same definition, u or v of a
 * block can differ only where |p - T| <= 1.01 * 11 * 2^-24 * T (3 roundings in q, 8 tree levels).
 * State per handle, on the device for a GPU handle, independent of every other stage's: the position;
 * per channel r, n, open, G of the block before the unfinished one, the last level and the unfinished
 * block's q values. */
#define SDDC_DDC_SQUELCH_BLOCK 256
#define SDDC_DDC_SQUELCH_OFF 0
#define SDDC_DDC_SQUELCH_LEVEL 1
#define SDDC_DDC_SQUELCH_NOISE 2
#define SDDC_DDC_SQUELCH_MUTE 3
#define SDDC_DDC_SQUELCH_SENSE_SELF 0
#define SDDC_DDC_SQUELCH_SENSE_F32 1
#define SDDC_DDC_SQUELCH_SENSE_S16 2
#define SDDC_DDC_SQUELCH_SENSE_CF32 3
#define SDDC_DDC_SQUELCH_SENSE_CS16 4
#define SDDC_DDC_SQUELCH_MAX_ATTACK 255
#define SDDC_DDC_SQUELCH_MAX_HANG 65535
/* blocks = round(seconds * fs / 256): an attack or a hang in blocks.  SDDC_ERR_ARG if the result is outside
 * 0..65535, an argument is not finite, fs <= 0 or blocks is NULL.  Stateless. */
int sddc_ddc_squelch_blocks(double seconds, double fs, int *blocks);
/* modes: host array [nch]; thresholds: host array [nch][2] = (T_open, T_close), finite, >= 0, <= 2^80, in
 * the order the channel's mode asks for (OFF and MUTE: any order); 1 <= nch <= SDDC_DDC_MAX_CHANNELS; a
 * violation returns SDDC_ERR_ARG and sets nothing.  modes or thresholds NULL or nch == 0 turns the stage off
 * and frees its state.  Every set call zeroes the state and the position, and waits for the stage's
 * launches in flight. */
int sddc_ddc_set_channel_squelch(sddc_ddc_t *h, const int *modes, const float *thresholds, int nch, int attack, int hang,
                                 int fade, int sense, int in_format, int out_format);
/* zero the state and the position: the next call starts a closed stream (SDDC_ERR_STATE: no squelch set) */
int sddc_ddc_channel_squelch_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  Channel c's nsamp audio samples at d_audio +
 * c * in_stride samples, its sense samples at d_sense + c * sense_stride components (complex kinds: even,
 * >= 2 nsamp), its outputs at d_out + c * out_stride samples; strides >= nsamp for nch > 1; bases aligned
 * to a sample (a complex sample for the complex kinds); any 1 <= nsamp <= 2^40.  The output must overlap
 * neither the audio nor the sense stream; nothing is written between the streams or outside them.
 * d_open, d_count, d_level: NULL or nch device entries.  SDDC_ERR_STATE: no squelch set, another nch than
 * the set one, a CPU handle.  SDDC_ERR_ARG: the rest (d_sense NULL with a sense kind other than SELF among
 * them).  A failed call changes no state.  The calls of one handle share the state and the position: they
 * run one after the other in call order, whatever their streams. */
int sddc_ddc_channel_squelch_device(sddc_ddc_t *h, const void *d_audio, const void *d_sense, int nch, size_t nsamp,
                                    size_t in_stride, size_t sense_stride, void *d_out, size_t out_stride, uint32_t *d_open,
                                    uint32_t *d_count, float *d_level, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernels, copy back, synchronous; it advances the
 * same device state as the device call.  CPU handle: the definition's loop through the same arithmetic
 * header. */
int sddc_ddc_channel_squelch_host(sddc_ddc_t *h, const void *audio, const void *sense, int nch, size_t nsamp,
                                  size_t in_stride, size_t sense_stride, void *out, size_t out_stride, uint32_t *open,
                                  uint32_t *count, float *level);

/* ---- channel tone detector: streaming per-channel CTCSS / tone squelch ---------------------------
 * The squelch opens on level alone.  Where a frequency is shared, a transmission is told from the others
 * by its sub-audible tone (CTCSS); a scanner wants to know which tone a transmission carries; a 1750 Hz
 * burst, a paging tone or a DTMF pair are the same question.  This stage is a bank of single-bin DFTs
 * (Goertzel filters) per channel over a real sense stream, a gate on the channel's audio that opens when
 * the strongest tone of the channel's mask holds enough of the window's energy, and side outputs that name
 * the tone and give every tone's power.  What it is NOT: no DCS (a digital code: that is the channel DCS
 * decoder below), no look-ahead (the gate of
 * a window comes from the windows before it), and the window length bounds the decode time.
 *
 * The definition (normative; csrc/tone_math.h holds the operations, shared by both backends, float,
 * contraction off, only *, +, explicit fmaf, comparisons, selects and integers).  B = SDDC_DDC_TONE_BLOCK =
 * 256; p >= 0 is the stream index since the last set or reset, k = p div B its block, j = k div W its window.
 *   Per handle.  A tone table of ntones (1..64) phase words w_t in 2^-32 cycles per sample (sddc_ddc_bfo_word
 *                makes them); a window of W blocks (1..256); an attack of A windows (1..255); a hang of H
 *                windows (0..65535); the formats of the sense stream, the audio and the output.
 *   Per channel. A 64-bit tone mask (a bit at or above ntones is an argument error; 0 is bypass: always
 *                open, the audio passes, the tone is -1) and three thresholds: rho_open >= rho_close, both in
 *                (0, 1], the share of the window's energy in the best tone, and e_min >= 0, a mean square per
 *                sample below which a window counts as silence.  Scaled once at set time: To = (float)((double)
 *                rho_open * 256 W), Tc likewise, Emin = (float)((double)e_min * 256 W).
 *   Sense.       Real, SDDC_DDC_AUDIO_F32 or _S16 (read as (float)v).  q = x * x; a sample with !(q <= FLT_MAX)
 *                enters every sum as x = 0, q = 0 and marks its window bad.
 *   Block k.     For each tone t of the mask: (c_i, s_i) = sincos_word(w_t * i) (the demodulator's
 *                demod_sincos_word; the product as a uint32; i = 0..255); a_i = x_i * c_i, b_i = x_i * s_i; Ck,
 *                Sk = the balanced pairwise tree (the blanker's) over a and over b; (cr, sr) = sincos_word(w_t *
 *                (uint32)(256 k)); Re_k = fmaf(Ck, cr, -(Sk * sr)), Im_k = fmaf(Ck, sr, Sk * cr).  p_k = the
 *                tree over q.
 *   Window j.    Zr, Zi, E = the left folds from +0, in block order, of Re_k, Im_k, p_k.  P_t = (Zr * Zr) + (Zi
 *                * Zi).  The best tone: the ascending scan of the mask, replaced only on a strict >.  u = !bad &&
 *                E > Emin && P_best > To * E; v the same with Tc.
 *   Gate.        The squelch's state machine, once per completed window: r = u ? min(r + 1, A) : 0; n = v ? 0 :
 *                min(n + 1, H + 1); open = open ? (n <= H) : (r >= A); all zero on a new stream.  The gate
 *                after window j applies to window j + 1.
 *   Audio.       Optional (d_audio NULL: detect only), F32 or S16 in and out.  A sample of an open window
 *                passes bit for bit (a NaN payload survives F32 to F32; S16 to F32 is (float)v, F32 to S16 the
 *                demodulator's conversion); a closed one is +0.
 *   Side outputs, each NULL or nch entries: tone (int32): the best tone of the last completed window if v
 *                held there, else -1; open (uint32): the gate after the last completed window (bypass: 1);
 *                count (uint32, modulo 2^32): the call's samples in open windows, consecutive calls add up;
 *                level ([nch][2] float): P_best and E of the last completed window, the figures to calibrate
 *                rho (P_best / (256 W E)) and e_min (E / (256 W)) from; powers ([nch][ntones] float): every
 *                P_t of the last completed window, 0 for tones outside the mask (a scanner's or a DTMF
 *                decoder's input).  Before any window completes: -1, 0 (bypass: 1), zeros.
 * Outputs and side outputs are bit-identical from run to run, for any grid, run length and cut of a
 * stream into calls, for a channel alone or among others, and between a GPU handle and a CPU handle, for
 * samples that are 0 or of magnitude in [2^-40, 2^40] (tone_math.h shows why nothing that decides
 * overflows or is subnormal there).  Against a float64 evaluation of the same definition, with X the sum
 * of |x| over the window, eps = (38 + W) 2^-24 and u = 2^-24: |P_t - P_t64| <= 1.01 (2 sqrt(2) eps X sqrt(P64) +
 * 2 eps^2 X^2 + 3 u P64) and |To E - (To E)64| <= 1.01 (W + 9) u To E64 (derived in tone_math.h).
 * State per handle, on the device for a GPU handle, independent of every other stage's: the position; per
 * channel the gate, the last completed window's results, the unfinished window's sums and bad flag, and
 * the unfinished block's samples. */
#define SDDC_DDC_TONE_BLOCK 256
#define SDDC_DDC_TONE_MAX_TONES 64
#define SDDC_DDC_TONE_MAX_WINDOW 256
#define SDDC_DDC_TONE_MAX_ATTACK 255
#define SDDC_DDC_TONE_MAX_HANG 65535
/* blocks = round(seconds * fs / 256), at least 1: a window in blocks.  SDDC_ERR_ARG if the result is above
 * 256, an argument is not finite, seconds < 0, fs <= 0 or blocks is NULL.  Stateless. */
int sddc_ddc_tone_window(double seconds, double fs, int *blocks);
/* words: host array [ntones]; masks: host array [nch]; thresholds: host array [nch][3] = (rho_open,
 * rho_close, e_min); 1 <= nch <= SDDC_DDC_MAX_CHANNELS; window, attack, hang in blocks / windows as above;
 * the formats SDDC_DDC_AUDIO_F32 or _S16.  A violation returns SDDC_ERR_ARG and sets nothing.  words, masks
 * or thresholds NULL or nch == 0 turns the stage off and frees its state.  Every set call zeroes the state
 * and the position, and waits for the stage's launches in flight. */
int sddc_ddc_set_channel_tone_detector(sddc_ddc_t *h, const uint32_t *words, int ntones, const uint64_t *masks,
                                       const float *thresholds, int nch, int window, int attack, int hang, int sense_format,
                                       int in_format, int out_format);
/* zero the state and the position: the next call starts a closed stream (SDDC_ERR_STATE: no detector set) */
int sddc_ddc_channel_tone_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  Channel c's nsamp sense samples at d_sense +
 * c * sense_stride samples; with d_audio not NULL its audio at d_audio + c * in_stride and its outputs at
 * d_out + c * out_stride; strides >= nsamp for nch > 1; bases aligned to a sample; any 1 <= nsamp <= 2^40.
 * The output must overlap neither input; nothing is written between the streams or outside them.  d_tone,
 * d_open, d_count: NULL or nch device entries; d_level: NULL or [nch][2]; d_powers: NULL or [nch][ntones].
 * SDDC_ERR_STATE: no detector set, another nch than the set one, a CPU handle.  SDDC_ERR_ARG: the rest
 * (d_out without d_audio and d_audio without d_out among them).  A failed call changes no state.  The calls
 * of one handle share the state and the position: they run one after the other in call order, whatever
 * their streams. */
int sddc_ddc_channel_tone_device(sddc_ddc_t *h, const void *d_sense, size_t sense_stride, const void *d_audio, int nch,
                                 size_t nsamp, size_t in_stride, void *d_out, size_t out_stride, int32_t *d_tone,
                                 uint32_t *d_open, uint32_t *d_count, float *d_level, float *d_powers, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernels, copy back, synchronous; it advances the
 * same device state as the device call.  CPU handle: the definition's loop through the same arithmetic
 * header. */
int sddc_ddc_channel_tone_host(sddc_ddc_t *h, const void *sense, size_t sense_stride, const void *audio, int nch, size_t nsamp,
                               size_t in_stride, void *out, size_t out_stride, int32_t *tone, uint32_t *open, uint32_t *count,
                               float *level, float *powers);

/* ---- channel DCS decoder: streaming per-channel digital code squelch -----------------------------
 * The tone detector tells CTCSS users apart.  The other half of selective calling on shared FM channels is
 * DCS: a 23-bit Golay (23, 12) codeword sent over and over as NRZ at 134.4 bit/s below the audio.  This stage
 * takes the sign of a real sense stream (the discriminator audio, low-passed and free of DC), sorts the signs
 * of a window into eighths of a bit, forms the 23 bit sums at each of the 8 timing phases, keeps the phase
 * with the widest eye, matches its word against a table of codewords over all 23 rotations, and gates the
 * channel's audio on the match.  What it is NOT: it does not detect the 134.4 Hz turn-off code (the eye
 * collapses and the hang decides); it has no DC removal (the caller high-passes or DC-blocks and low-passes
 * the discriminator audio, as for CTCSS); it does not track the bit clock across windows; the window bounds
 * the decode time.
 *
 * The definition (normative; csrc/dcs_math.h holds the operations, shared by both backends, integer-only
 * apart from the sign test).  B = SDDC_DDC_DCS_BLOCK = 256; p >= 0 is the stream index since the last set or
 * reset, k = p div B its block, j = k div W its window, n = p - 256 W j the window-local index.
 *   Per handle.  A bit phase word w in 2^-32 cycles per sample, 1 <= w <= 2^29 (a bit is at least 8 samples,
 *                an eighth of it at least one); a window of W blocks (1..256) with 256 W w >= 24 * 2^32 (23
 *                bits and a bit of timing slack); a table of ncodes (1..128) 23-bit codewords, bit 0 the first
 *                on the air; error limits 0 <= e_open <= e_close <= 3; an attack of A windows (1..255); a hang of
 *                H windows (0..65535); the formats of the sense stream, the audio and the output.
 *   Per channel. Three int32: code, an index into the table, or SDDC_DDC_DCS_ANY = -1 (match the whole table:
 *                scan), or SDDC_DDC_DCS_OFF = -2 (bypass: always open, the audio passes, the reported code is
 *                -1); invert, 0 or 1 (1: the received word is complemented before matching); eye, 0..256.
 *   Sense.       Real, SDDC_DDC_AUDIO_F32 or _S16.  s = +1 if x > 0, -1 if x < 0, else 0 (a NaN is 0).
 *   Sub-bins.    m(n) = (w n) >> 29, the product in 64 bits.  S[m] = the sum of s over the window's samples
 *                with that m, m = 0..191 (samples with m >= 192 do not count).
 *   Phases.      t = 0..7: c[t][b] = S[8 b + t] + .. + S[8 b + t + 7], b = 0..22, which is the sum of s over
 *                floor((w n - t 2^29) / 2^32) = b.  Q[t] = the sum over b of |c[t][b]|.  N[t] = the number of n <
 *                256 W with t <= m(n) < t + 184, a set-time constant.  The best phase: the largest Q, the
 *                lowest t on a tie.  The word: bit b = (c[t][b] > 0), complemented in 23 bits if invert.
 *   Match.       d(i) = the minimum over r = 0..22 of popcount(word xor rot_r(cw_i)), rotating in 23 bits.
 *                Over the channel's candidates (the one code, or the whole table) the best is the lowest d,
 *                then the lowest i; a channel without candidates (OFF) has d = 24.  good = 256 Q[t] >= eye N[t];
 *                u = good && d <= e_open; v = good && d <= e_close.
 *   Gate.        The squelch's state machine, once per completed window, exactly as in the tone detector: r = u
 *                ? min(r + 1, A) : 0; n = v ? 0 : min(n + 1, H + 1); open = open ? (n <= H) : (r >= A); all zero
 *                on a new stream.  The gate after window j applies to window j + 1.
 *   Audio.       Optional (d_audio NULL: detect only), F32 or S16 in and out.  A sample of an open window
 *                passes bit for bit, a closed one is +0; the conversions are the tone detector's.
 *   Side outputs, each NULL or per channel: code (int32): the best index of the last completed window if v
 *                held there, else -1; open (uint32) and count (uint32): as in the tone detector; info ([nch][4]
 *                uint32): Q, N, d and t of the last completed window, the figures to calibrate eye from (256 Q
 *                / N is the eye in the unit of `eye`).  Before any window completes: -1, 0 (bypass: 1), zeros.
 * Everything is bit-identical from run to run, for any cut of a stream into calls, stream, grid and run
 * length, for a channel alone or among others, and between a GPU handle and a CPU handle, with no condition
 * on the sample magnitudes: after the sign test every value is an integer and every sum is order-free.
 * State per handle, on the device for a GPU handle, independent of every other stage's: the position; per
 * channel the gate, the last completed window's results and the unfinished window's 192 sub-bin sums. */
#define SDDC_DDC_DCS_BLOCK 256
#define SDDC_DDC_DCS_MAX_CODES 128
#define SDDC_DDC_DCS_MAX_WINDOW 256
#define SDDC_DDC_DCS_MAX_WORD (1u << 29)
#define SDDC_DDC_DCS_MAX_ERRORS 3
#define SDDC_DDC_DCS_MAX_EYE 256
#define SDDC_DDC_DCS_MAX_ATTACK 255
#define SDDC_DDC_DCS_MAX_HANG 65535
#define SDDC_DDC_DCS_ANY (-1)
#define SDDC_DDC_DCS_OFF (-2)
/* The 23-bit codeword of the DCS code `code` = 0..511 (its three octal digits): d = 0x800 | code, parity = (d
 * x^11) mod g over GF(2) with g = 0xC75 (x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1), cw = parity << 12 | d; 023
 * (octal) gives 0x763813.  SDDC_ERR_ARG: code outside 0..511 or cw NULL.  Stateless. */
int sddc_ddc_dcs_codeword(int code, uint32_t *cw);
/* word = round(bitrate / fs * 2^32), blocks = ceil(24 * 2^32 / (256 word)): the phase word and the shortest
 * window for it (134.4 bit/s: 6 blocks at 8 kS/s, 34 at 48 kS/s).  SDDC_ERR_ARG if word is 0 or above 2^29,
 * blocks is above 256, an argument is not finite or not positive, or a pointer is NULL.  Stateless. */
int sddc_ddc_dcs_window(double fs, double bitrate, uint32_t *word, int *blocks);
/* codewords: host array [ncodes], each below 2^23; params: host array [nch][3] = (code, invert, eye); 1 <= nch
 * <= SDDC_DDC_MAX_CHANNELS; word, window, e_open, e_close, attack, hang as above; the formats
 * SDDC_DDC_AUDIO_F32 or _S16.  A violation returns SDDC_ERR_ARG and sets nothing.  codewords or params NULL
 * or nch == 0 turns the stage off and frees its state.  Every set call zeroes the state and the position,
 * and waits for the stage's launches in flight. */
int sddc_ddc_set_channel_dcs_decoder(sddc_ddc_t *h, const uint32_t *codewords, int ncodes, const int32_t *params, int nch,
                                     uint32_t word, int window, int e_open, int e_close, int attack, int hang, int sense_format,
                                     int in_format, int out_format);
/* zero the state and the position: the next call starts a closed stream (SDDC_ERR_STATE: no decoder set) */
int sddc_ddc_channel_dcs_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  The buffers, strides, alignment, overlap rules
 * and errors of sddc_ddc_channel_tone_device.  d_code, d_open, d_count: NULL or nch device entries; d_info:
 * NULL or [nch][4].  A failed call changes no state.  The calls of one handle share the state and the
 * position: they run one after the other in call order, whatever their streams. */
int sddc_ddc_channel_dcs_device(sddc_ddc_t *h, const void *d_sense, size_t sense_stride, const void *d_audio, int nch,
                                size_t nsamp, size_t in_stride, void *d_out, size_t out_stride, int32_t *d_code, uint32_t *d_open,
                                uint32_t *d_count, uint32_t *d_info, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernels, copy back, synchronous; it advances the
 * same device state as the device call.  CPU handle: the definition's loop through the same arithmetic
 * header. */
int sddc_ddc_channel_dcs_host(sddc_ddc_t *h, const void *sense, size_t sense_stride, const void *audio, int nch, size_t nsamp,
                              size_t in_stride, void *out, size_t out_stride, int32_t *code, uint32_t *open, uint32_t *count,
                              uint32_t *info);

/* ---- channel stereo decoder: streaming WFM stereo from the MPX -----------------------------------
 * The FM discriminator output of a broadcast station (192 or 250 kS/s) is the stereo multiplex (MPX): L + R up
 * to 15 kHz, a pilot at 19 kHz, and L - R double-sideband around a suppressed carrier at 38 kHz whose phase is
 * twice the pilot's.  This stage measures the pilot per channel (the tone detector's single-bin DFT over
 * windows of 256-sample blocks), decides stereo or mono with the squelch's gate, rebuilds the carrier from the
 * exact 32-bit phase word and the measured pilot phase, and writes L = x + d and R = x - d, d = 2 g x sin(2 psi),
 * at the MPX rate.  Matrixing commutes with the low-pass, so the existing stages finish the job unchanged: the
 * audio resampler (15 kHz low-pass, 24/125 from 250 kS/s) on the 2 nch output streams, then the audio filter
 * (de-emphasis, a 19 kHz notch where the resampler's stop band is not enough).  d_left and d_right are
 * separate pointers; a caller who passes d_right = d_left + nch * out_stride gets 2 nch streams of the stride
 * out_stride that one audio resampler call of a second handle takes.
 * What it is NOT: it does not track a pilot frequency offset (the carrier runs at exactly twice the set
 * word, the measured phase is constant over a window and applied to the next one, so an offset of df turns
 * the carrier by 2 pi df 256 W / fs per window: W is the trade between the noise on the phase and this
 * error); no de-emphasis, no 15 kHz low-pass and no pilot notch (the audio resampler and the audio filter);
 * no RDS; no blend by signal quality: a window is stereo or it is mono.
 *
 * The definition (normative; csrc/stereo_math.h holds the operations, shared by both backends, float,
 * contraction off, only *, +, -, explicit fmaf, one sqrt, correctly rounded /, comparisons, selects and
 * integers; the tone detector's, the blanker's, the demodulator's and the squelch's functions are used, not
 * restated).  B = SDDC_DDC_STEREO_BLOCK = 256; p >= 0 is the stream index since the last set or reset, k = p
 * div B its block, j = k div W its window.
 *   Per handle.  The pilot's phase word w in 2^-32 cycles per sample, sddc_ddc_bfo_word(19000 / fs), not 0; w2
 *                = 2 w mod 2^32; a window of W blocks (1..256); an attack of A windows (1..255); a hang of H
 *                windows (0..65535); the formats of the input and of the two outputs.
 *   Per channel. A mode: SDDC_DDC_STEREO_MONO (bypass: both outputs are the input; the pilot is still
 *                measured) or SDDC_DDC_STEREO_AUTO; rho_open >= rho_close, both in (0, 1], the share of the
 *                window's energy in the pilot that opens and that keeps open; e_min >= 0, a mean square per
 *                sample below which a window counts as silence; the separation gain g >= 0 (1 for a
 *                discriminator of flat response; above 1 makes up for the roll-off at 38 kHz).  Scaled once at
 *                set time: To = (float)((double)rho_open * 256 W), Tc and Emin likewise, g2 = 2 g.
 *   Sample.      x, SDDC_DDC_AUDIO_F32 or _S16 (read as (float)v).  q = x * x; a sample with !(q <= FLT_MAX)
 *                enters the sums as x = 0, q = 0 and marks its window bad (the tone detector's rule).
 *   Block, window.  Re_k, Im_k, p_k and the folds Zr, Zi, E: the tone detector's, for the single tone w.  P =
 *                (Zr * Zr) + (Zi * Zi); u = !bad && E > Emin && P > To * E; v the same with Tc.  (P, E) are the
 *                tone detector's d_level for the table {w} and the same W on the same stream, bit for bit.
 *   Pilot phase. For x_i = sin(phi_i + alpha) the sum Z = sum x_i e^{j phi_i} is (N / 2) (sin alpha + j cos
 *                alpha).  Where v_j holds: n = sqrtf(P), vr = Zi / n, vi = Zr / n, qr = fmaf(vr, vr, -(vi * vi)),
 *                qi = (2 * vr) * vi; otherwise q_j = q_{j-1}.  A new stream has q = (1, 0).
 *   Gate.        The squelch's state machine, once per completed window, as in the tone detector.  The gate and
 *                the q after window j apply to window j + 1: no look-ahead and no delay.
 *   Carrier.     Block k of an open window, sample i of the block: (tc_i, ts_i) = sincos_word(w2 * i); (rc, rs)
 *                = sincos_word(w2 * (uint32)(256 k)); rr = fmaf(qr, rc, -(qi * rs)), ri = fmaf(qr, rs, qi * rc);
 *                sub_i = fmaf(tc_i, ri, ts_i * rr): sin(2 psi) for a pilot sin(psi), the BS.450 relation.
 *   Outputs.     Open window of an AUTO channel: d = (g2 * x) * sub, L = x + d, R = x - d; S16 outputs by the
 *                demodulator's conversion.  Closed window or MONO channel: L = R = the input sample as it is
 *                (the tone detector's pass rule: a NaN payload survives F32 to F32, S16 to F32 is (float)v).
 *   Side outputs, each NULL or per channel: stereo (uint32): the gate for the next window (MONO: 0); count
 *                (uint32, modulo 2^32): the samples this call wrote in stereo; level ([nch][2] float): P and E
 *                of the last completed window, the figures to calibrate rho (P / (256 W E)) and e_min (E /
 *                (256 W)) from; phase ([nch][2] float): (qr, qi) in force.  Before any window completes: 0, 0,
 *                zeros, (1, 0).
 * Outputs and side outputs are bit-identical from run to run, for any grid, run length and cut of a stream
 * into calls, for a channel alone or among others, and between a GPU handle and a CPU handle, for samples
 * that are 0 or of magnitude in [2^-40, 2^40] and g 0 or in [2^-40, 2^40] (stereo_math.h shows why nothing that
 * decides depends on a subnormal or an overflow: P > Tc * E > 0 excludes P = 0, n is in (2^-50, 2^60), |vr|,
 * |vi| <= 1 + 3.02 u).  Against a float64 evaluation of the same definition (derived in stereo_math.h; u =
 * 2^-24, X the sum of |x| over the window, r = sqrt(2) (38 + W) u X / sqrt(P64), dv = r / (1 - r / 2) + 3.02 u):
 * |qr - qr64|, |qi - qi64| <= dv (2 + dv) + 2.02 u, and given the same float32 q: |L - L64|, |R - R64| <= 1.01 u
 * (|x| + 22 |g2 x|).  The decisions differ only inside the tone detector's bounds.
 * State per handle, on the device for a GPU handle, independent of every other stage's: the position; per
 * channel the gate, q, the last completed window's P and E, the unfinished window's sums and bad flag, and
 * the unfinished block's samples. */
#define SDDC_DDC_STEREO_BLOCK 256
#define SDDC_DDC_STEREO_MAX_WINDOW 256
#define SDDC_DDC_STEREO_MONO 0
#define SDDC_DDC_STEREO_AUTO 1
/* modes: host array [nch]; params: host array [nch][4] = (rho_open, rho_close, e_min, g); 1 <= nch <=
 * SDDC_DDC_MAX_CHANNELS; window, attack, hang with the tone detector's limits; the formats
 * SDDC_DDC_AUDIO_F32 or _S16.  A violation returns SDDC_ERR_ARG and sets nothing.  modes or params NULL or nch
 * == 0 turns the stage off and frees its state.  Every set call starts a new stream (state and position), and
 * waits for the stage's launches in flight. */
int sddc_ddc_set_channel_stereo_decoder(sddc_ddc_t *h, uint32_t pilot_word, const uint8_t *modes, const float *params, int nch,
                                        int window, int attack, int hang, int in_format, int out_format);
/* a new stream: state and position (SDDC_ERR_STATE: no decoder set) */
int sddc_ddc_channel_stereo_reset(sddc_ddc_t *h);
/* GPU handles; enqueued on hip_stream, returns after launch.  Channel c's nsamp MPX samples at d_mpx + c *
 * in_stride samples, its outputs at d_left + c * out_stride and d_right + c * out_stride; strides >= nsamp for
 * nch > 1; bases aligned to a sample; any 1 <= nsamp <= 2^40.  The outputs overlap neither the input nor each
 * other; nothing is written between the streams or outside them.  d_stereo, d_count: NULL or nch device
 * entries; d_level, d_phase: NULL or [nch][2].  SDDC_ERR_STATE: no decoder set, another nch than the set one, a
 * CPU handle.  SDDC_ERR_ARG: the rest.  A failed call changes no state.  The calls of one handle share the
 * state and the position: they run one after the other in call order, whatever their streams. */
int sddc_ddc_channel_stereo_device(sddc_ddc_t *h, const void *d_mpx, int nch, size_t nsamp, size_t in_stride, void *d_left,
                                   void *d_right, size_t out_stride, uint32_t *d_stereo, uint32_t *d_count, float *d_level,
                                   float *d_phase, void *hip_stream);
/* Host buffers, the same layouts.  GPU handle: copy in, kernels, copy back, synchronous; it advances the
 * same device state as the device call.  CPU handle: the definition's loop through the same arithmetic
 * header. */
int sddc_ddc_channel_stereo_host(sddc_ddc_t *h, const void *mpx, int nch, size_t nsamp, size_t in_stride, void *left, void *right,
                                 size_t out_stride, uint32_t *stereo, uint32_t *count, float *level, float *phase);

/* ---- ingest ---------------------------------------
 * Pin a caller-owned host region (hipHostRegister) so the host path DMAs blocks
 * from it and output into it directly instead of staging through the library's
 * pinned buffers.  Regions must not overlap; unregister before freeing them.
 * The host path runs chunks of 32 blocks through a two-slot pipeline (H2D,
 * kernel and D2H on separate streams), whichever memory is used. */
int sddc_ddc_register_host(sddc_ddc_t *h, void *ptr, size_t bytes);
int sddc_ddc_unregister_host(sddc_ddc_t *h, void *ptr);

#ifdef __cplusplus
}
#endif

#endif /* SDDC_DDC_H */
