// ddc_kernels.h — internal (C++) interface between the runtime and the HIP kernels of the
// product library.  (The measured-slower A/B kernels of rounds 1-5 are in git history; DESIGN.md
// §8 keeps their numbers.)
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stddef.h>
#include <stdint.h>

#include "fs_shares.h"

namespace sddc {

// Launch geometry, per handle: the device's CU count and, per kernel (function pointer), the
// resident workgroups per CU, queried on first use and kept in the handle (all launches run
// under the handle's lock), so no launch path writes namespace-scope state.
struct LaunchCache {
    static constexpr int kSlots = 256;
    int cus = 0;
    int n = 0;
    const void *fn[kSlots] = {};
    int occ[kSlots] = {};
};

// occ = resident workgroups per CU of kernel fn (`threads` per workgroup, static LDS), cus = the
// device's CUs; cached in *lc when lc is non-null.
inline hipError_t launch_geometry(LaunchCache *lc, const void *fn, int threads, int device, int *occ, int *cus)
{
    if (lc) {
        for (int i = 0; i < lc->n; i++)
            if (lc->fn[i] == fn) {
                *occ = lc->occ[i];
                *cus = lc->cus;
                return hipSuccess;
            }
    }
    int nb = 0, c = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, 0);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    *occ = nb > 0 ? nb : 1;
    *cus = c;
    if (lc && lc->n < LaunchCache::kSlots) {
        lc->cus = c;
        lc->fn[lc->n] = fn;
        lc->occ[lc->n] = *occ;
        lc->n++;
    }
    return hipSuccess;
}

// Device-resident constant tables, built once per handle (the reference's
// fft_mt_r2iq::Init builds filterHw and the FFTW plans, fft_mt_r2iq.cpp:147-227).
// All twiddles are evaluated in double on the host and rounded once to float.
struct KernelTables {
    const float2 *tw4096 = nullptr;    // e^{-2 pi i k/4096}, k < 4096 (v1 FFT twiddles)
    const float2 *post8192 = nullptr;  // e^{-2 pi i k/8192}, k < 8192 (r2c split twiddles)
    const float2 *hsel[7] = {};        // per d: mfft filter taps in inverse-input order, x 1/2
    // persistent kernel (v2) twiddle sets
    const float2 *tw_p1 = nullptr;     // [15][16]: W_256^{s r}     forward pass 1 (NS = 16)
    const float2 *tw_q1[7] = {};       // [15][S]:  W_{16S}^{s r}   inverse pass 1, S = NS of that pass
    const float2 *rec_f = nullptr;     // [2][256]: W_4096^{j}, W_4096^{4j}  forward pass 2 recurrence
    const float2 *rec_i[7] = {};       // [2][256]: W_N^{j}, W_N^{4j}        inverse pass 2 (N >= 512)
    LaunchCache *lc = nullptr;         // the handle's launch geometry (written under the handle's lock)
};

// v2 (default): persistent workgroups, input prefetch, swizzled LDS.  pq: the split x filter
// coefficients of (d, tunebin) built by launch_build_split_filter: N = HALF >> d float2 P, then N
// float r (12 N bytes of the HALF float4 allocation).
// nco_starts/nco_trig: fused fine-tune NCO tables (fine_tune.h), or nullptr for none.
// cs16: write saturate(rint(x * cs16_scale)) int16 (I, Q) pairs instead of complex float.
hipError_t launch_frames_persistent(const KernelTables &t, int d, const int16_t *d_in, int nblk,
                                    void *d_out, const float4 *pq, int tunebin, int lsb, int rand,
                                    int cs16, float cs16_scale, const float2 *nco_starts,
                                    const float2 *nco_trig, int slot_weights, int device, hipStream_t s);
// slot_weights: split the frames over the workgroups by their CU slot's measured speed
// (kSlotWeights[d]: slot 0 in the low byte; ddc_queue.hpp slot_split), 0: equal contiguous
// ranges.  The frames per slot of a balanced (queue-fed) run gave the weights: d = 1 29 / 25 /
// 19 / 15, d = 4 27 / 24 / 20 / 16, tuned at d >= 3 to 29 / 25 / 20 / 15 (+3-6 %,
// profiles/r04/ab/slot_weights_d3_6.txt; the four slots then end within 1 us of each other,
// stamps_p_d4_final_by_slot.txt) and at d <= 2 to 31 / 26 / 18 / 13 (d = 1 +4 %, d = 2 +2 %,
// slot_weights_tuning_d1_6.txt).
constexpr unsigned slot_weights4(unsigned a, unsigned b, unsigned c, unsigned e) { return a | (b << 8) | (c << 16) | (e << 24); }
constexpr unsigned kSlotWeights[7] = {slot_weights4(31, 26, 18, 13), slot_weights4(31, 26, 18, 13), slot_weights4(31, 26, 18, 13),
                                      slot_weights4(29, 25, 20, 15), slot_weights4(29, 25, 20, 15),
                                      slot_weights4(29, 25, 20, 15), slot_weights4(29, 25, 20, 15)};
constexpr int kSlotWeighting = 1;
hipError_t launch_build_split_filter(const KernelTables &t, int d, int tunebin, float4 *pq, hipStream_t s);

// d = 0 fused-split kernel (ddc_fs.hip, FS): used when fs_path(d, tunebin) (d = 0, tunebin a
// multiple of 4: every tune bin setFreqOffset produces, fft_mt_r2iq.cpp:104).  Its per-tunebin
// tables: pqf (4096 float4, the split x filter by bin in lane order) and fsl (3 x 256 float2, the
// output modulation's lane factors), built by launch_build_fs_tables.
bool fs_path(int d, int tunebin);
hipError_t launch_build_fs_tables(const KernelTables &t, int tunebin, float4 *pqf, float2 *fsl, hipStream_t s);
// wq: a zeroed slot of kFsQueueWords unsigned words (the dynamic frame queue); the launch leaves it
// zeroed again.  Launches that may run at the same time need different slots.
// static_pct: the share (percent) of each workgroup's frames taken statically before it draws
// from the queue (ddc_queue.hpp FrameSchedule); kFsStaticPct by default.
constexpr int kFsQueueLineWords = 16 * 9;                  // the dynamic queue's counters
constexpr int kFsStealMax = 2048;                         // steal slots (2 words): workgroups per launch
constexpr int kFsQueueWords = kFsQueueLineWords + 2 * kFsStealMax;
constexpr int kFsStaticPct = 100;   // (85 / 95 / 100 %: 0.240 / 0.238 / 0.235 ms, profiles/r04/ab/fs_static_share_d0.txt)
constexpr unsigned kFsSlotWeights = slot_weights4(31, 26, 18, 13);   // (between the boxes' optima, fs_slot_weights_d0.txt)
// The FS kernel's frame schedule (ddc_queue.hpp): sched 0 the slot-weighted static split alone
// (default; every output configuration), 2 work stealing, 1 the static prefix of static_pct
// percent + the dynamic queue (1 and 2: the plain configuration only, A/B and tests).  fpw > 0: a
// non-persistent grid of fpw frames per workgroup (A/B).  minrem: a thief steals only from ranges
// with at least minrem unclaimed frames (0: none, the static split inside the stealing kernel).
struct FsSched {
    int sched = 0;
    int static_pct = kFsStaticPct;
    int fpw = 0;
    int minrem = 1;
    int pub = 0;   // frames at the end of each range open to thieves (0: all but the first two)
    int zr = 1;    // skip the tune bin's whole zero rows of the inverse input (0: never; A/B)
    unsigned slotw = 0u;   // the static split's slot weights (slot_weights4 packing); 0: kFsSlotWeights
    // The adaptive split's hook (fs_split_controller.hpp; ddc_runtime.cpp fs_adapt_prepare), or
    // null: called for a launch of the static schedule at full residency (G = 4 x CUs <=
    // kFsShareMaxG workgroups, ns frames) with the built-in weights.  *tab: the launch's share table
    // (fs_shares.h), null for the built-in split; *tlog: G x 4 words of host-mapped memory where
    // each workgroup writes {start, end, tag, start ^ end ^ tag} as it exits (the constant-rate
    // 100 MHz counter's low words), or null.  false: the launch runs as without the hook.
    bool (*adapt)(void *ctx, int G, int ns, const FsShares **tab, unsigned **tlog, unsigned *tag) = nullptr;
    void *adapt_ctx = nullptr;
};
hipError_t launch_frames_fs(const KernelTables &t, const int16_t *d_in, int nblk, void *d_out, const float4 *pqf,
                            const float2 *fsl, int tunebin, int lsb, int rand, int cs16, float cs16_scale,
                            const float2 *nco_starts, const float2 *nco_trig, unsigned *wq, const FsSched &fs,
                            int device, hipStream_t s);

// Per-channel fine-tune NCO of the many-channel kernels (sddc_ddc_set_channel_fine_tune): device
// tables of one run of a call.  Channel c mixes its output sample o of the run (o = 128 b + 4 q + l)
// with T_c[q - 1] * S_c,b[l] (fine_tune.h), unless fc[c] == 0: that channel's output is the plain DDC.
struct ChNco {
    const float2 *starts = nullptr;   // [nch][nb][4] lane starts, written by launch_channel_nco_chain
    const float2 *trig = nullptr;     // [nch][32] T of each channel's fc (host, FineTune::init)
    const float *fc = nullptr;        // [nch]
    int nb = 0;                       // 128-sample blocks per channel in the run
};
// The lane-start chain S_{b+1} = normalise(T[31] S_b) of every channel (FineTune::starts, bit for
// bit), one thread per (channel, lane): reads state [nch][4], writes starts [nch][nb][4] and the
// advanced state back, so the phase lives on the device.
hipError_t launch_channel_nco_chain(float2 *d_state, const float2 *d_trig, float2 *d_starts, int nch, int nb,
                                    hipStream_t s);

// many-channel v2 (d = 4..6): persistent, forward once per (frame, 128-channel chunk)
// stride: scalar components (float or int16) per channel row; cs16 as above.  d_windows:
// per-128-channel-chunk forward-bin windows from channel_windows (device copy), or nullptr.
// d_scratch: scratch_rows x 4096 float2, one row per workgroup, where a frame's split spectrum
// is kept for its later chunks (used when the grid fits; nullptr = recompute per chunk).
// nco: the per-channel NCO tables of this launch (the NCO instances of the kernel), or nullptr.
hipError_t launch_channels_v2(const KernelTables &t, int d, const int16_t *d_in, int nblk, const int *d_tunebins,
                              int nch, void *d_out, size_t stride, int lsb, int rand, int cs16, float cs16_scale,
                              const int2 *d_windows, float2 *d_scratch, int scratch_rows, int device,
                              hipStream_t s, const ChNco *nco = nullptr);
// many-channel, d = 0..3: persistent, forward + split once per frame, 2^d channels' inverses
// in flight.  d_scratch (scratch_rows x 4096 float2, >= CUs x 4 rows) holds each workgroup's
// split spectrum in L2 instead of LDS; nullptr keeps it in LDS.
hipError_t launch_channels_p(const KernelTables &t, int d, const int16_t *d_in, int nblk, const int *d_tunebins,
                             int nch, void *d_out, size_t stride, int lsb, int rand, int cs16, float cs16_scale,
                             float2 *d_scratch, int scratch_rows, int device, hipStream_t s,
                             const ChNco *nco = nullptr);
// host: the compact windows of every chunk; false if a chunk's window does not fit
bool channel_windows(int d, const int *tunebins, int nch, int2 *windows);

// Wideband averaged power spectrum (ddc_spectrum.hip, sddc_ddc_spectrum_device): persistent
// workgroups, one input block (11 frames of the DDC's schedule) per work item.  d_out receives
// scale x the sum of 4 |X_f[k]|^2 over each block's frames, nblk rows of 4096 floats (4-byte
// aligned): the finished rows when a row is one block, else the partial rows (scale = 1) that
// launch_spectrum_reduce adds per row, in block order, and scales.  d_window: 8192 floats, or
// nullptr for the rectangular window (no multiply).  max_wgs > 0 caps the grid (tests).
hipError_t launch_spectrum(const KernelTables &t, const int16_t *d_in, int nblk, float *d_out, const float *d_window,
                           float scale, int rand, int max_wgs, int device, hipStream_t s);
// d_partial: rows x blocks_per_row x 4096 floats, 16-byte aligned; d_psd: rows x 4096, 4-byte aligned
hipError_t launch_spectrum_reduce(const float *d_partial, int rows, int blocks_per_row, float scale, float *d_psd,
                                  hipStream_t s);

// Channel spectrum (ddc_channel_spectrum.hip, sddc_ddc_channel_spectrum_device): the averaged
// power spectrum of nch IQ streams in the DDC's output format (cs16: int16 (I, Q) pairs, else
// float pairs), channel c at d_iq + c * stride_samples complex samples.  One work item per
// (channel, row): its fpr frames of n samples (n = 256..4096, frame f of row r at sample
// (r fpr + f) hop) are transformed and |X|^2 summed in frame order by the n / 16 threads that own
// it; d_psd[c][r][q] = scale x the sum at bin (q + n/2) mod n, 4-byte aligned.  d_window: n
// floats, or nullptr for the rectangular window (no multiply).  max_wgs > 0 caps the grid (tests).
// The caller has checked that every frame lies inside its stream.
hipError_t launch_channel_spectrum(const KernelTables &t, const void *d_iq, int cs16, int nch, int nrows,
                                   size_t stride_samples, int n, int hop, int fpr, float *d_psd,
                                   const float *d_window, float scale, int max_wgs, int device, hipStream_t s);

// Channel decimator (ddc_channel_decimate.hip, sddc_ddc_channel_decimate_device): y_c[m] =
// sum_j h[j] x_c[m R - j] on nch streams in the DDC's output format (cs16: int16 (I, Q) pairs read
// as v * (float)(1 / cs16_scale), else float pairs), channel c at d_iq + c * in_stride components,
// nsamp = a multiple of R samples each; channel c's nsamp / R float2 outputs at d_out + c *
// out_stride floats (8-byte aligned).  d_taps: the ntaps taps in the kernel's order
// (channel_decimate_order_taps: by phase of the polyphase rows).  d_tail_in: [nch][ntaps - 1] float2,
// each channel's last sample values before this call; d_tail_out: the same after it (another
// buffer; both may be null when ntaps == 1).  One work item per (channel, tile of at most
// kChDecTile outputs); max_wgs > 0 caps the grid (tests).  The caller has checked the strides.
constexpr int kChDecTile = 512;        // outputs per tile (two per thread), when the LDS holds them
constexpr int kChDecLds = 4864;        // float2 slots of LDS per tile (+ 256 of slack: 40 KiB, 4 workgroups per CU)
constexpr int kChDecPitchPad = 15;     // the pitch search's range above the rows needed
constexpr int kChDecMaxTaps = 1024;    // SDDC_DDC_DECIM_MAX_TAPS
constexpr int kChDecMaxFactor = 64;    // SDDC_DDC_DECIM_MAX_FACTOR
static_assert(kChDecLds / kChDecMaxFactor - kChDecPitchPad - (kChDecMaxTaps - 2 + kChDecMaxFactor) / kChDecMaxFactor >= 1,
              "a tile of both maxima holds an output");
// The tile of (R, ntaps): its outputs (kChDecTile, or what the LDS holds beside the halo's rows), the
// polyphase rows' pitch and the modelled extra LDS cycles of the stage's four stores per wave.
struct ChDecLayout {
    int tile = 0, pitch = 0, store_conflicts = 0;
};
ChDecLayout channel_decimate_layout(int R, int ntaps, int cs16);
void channel_decimate_order_taps(const float *h, int ntaps, int R, float *g /* [ntaps] */);
hipError_t launch_channel_decimate(const KernelTables &t, const void *d_iq, int cs16, float cs16_scale, int nch,
                                   size_t nsamp, size_t in_stride, const float *d_taps, int ntaps, int R,
                                   const float2 *d_tail_in, float2 *d_tail_out, float *d_out, size_t out_stride,
                                   int max_wgs, int device, hipStream_t s);

// Channel resampler (ddc_channel_resample.hip, sddc_ddc_channel_resample_device): the rational L / M
// polyphase FIR y_c[m] = sum_{j < K} h[p + jL] x_c[s - j], m M = s L + p, K = ceil(ntaps / L), on nch
// streams laid out as for the decimator; any nsamp >= 1.  e = the call's position (0 <= e < M: the
// first output's m M minus the first sample's i L), nout = the call's outputs per channel
// (= ceil((nsamp L - e) / M), checked), written as float2 at d_out + c * out_stride floats.
// d_taps: [L][K] floats in the kernel's order (channel_resample_order_taps: g[p][j] = h[p + jL],
// zero-padded).  d_tail_in / d_tail_out: [nch][K - 1] float2 as for the decimator (both may be null
// when K == 1).  One work item per (channel, tile of ta values of a = ta L outputs); a call without
// an output still moves the tails.  max_wgs > 0 caps the grid (tests).  The caller has checked the
// strides.
constexpr int kChResLds = 8128;        // float2 slots of LDS per tile (+ 64 of slack: 64 KiB, 2 workgroups per CU)
constexpr int kChResMaxA = 512;        // values of a per tile at most (16 half-wave units per phase)
constexpr int kChResPitchPad = 15;     // the pitch search's range above the columns needed
constexpr int kChResMaxTaps = 4096;    // SDDC_DDC_RESAMPLE_MAX_TAPS
constexpr int kChResMaxUp = 32;        // SDDC_DDC_RESAMPLE_MAX_UP
constexpr int kChResMaxDown = 256;     // SDDC_DDC_RESAMPLE_MAX_DOWN
constexpr int kChResMaxK = 1024;       // SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS
static_assert(kChResLds / kChResMaxDown - ((kChResMaxK - 2 + kChResMaxDown) / kChResMaxDown + 1) - 1 >= 1,
              "a tile of both maxima holds an output");
// The tile of (L, M, ntaps, format): K, the values of a per tile (ta L outputs), the polyphase rows'
// pitch and the modelled extra LDS cycles of the stage's stores per wave.
struct ChResLayout {
    int K = 0, ta = 0, pitch = 0, store_conflicts = 0;
};
ChResLayout channel_resample_layout(int L, int M, int ntaps, int cs16);
void channel_resample_order_taps(const float *h, int ntaps, int L, float *g /* [L][ceil(ntaps / L)] */);
hipError_t launch_channel_resample(const KernelTables &t, const void *d_iq, int cs16, float cs16_scale, int nch,
                                   size_t nsamp, size_t in_stride, const float *d_taps, int ntaps, int L, int M,
                                   int e, size_t nout, const float2 *d_tail_in, float2 *d_tail_out, float *d_out,
                                   size_t out_stride, int max_wgs, int device, hipStream_t s);

// Channel audio resampler (ddc_channel_audio_resample.hip, sddc_ddc_channel_audio_resample_device): the
// resampler's sum (audio_resample_math.h: the same fixed order on both backends) on nch REAL streams,
// float (in_s16 = 0) or int16 read as (float)v, channel c at c * in_stride samples, aligned to one sample,
// any nsamp >= 1; outputs float or int16 (demod_s16) at c * out_stride samples.  e, nout, d_taps as for the
// resampler.  d_tail_in / d_tail_out: [nch][K - 1] floats (two buffers; both may be null when K == 1).
// One work item per (channel, tile of ta values of a); a call without an output still moves the tails.
// An LDS slot is one float, so a tile holds twice the resampler's samples; a short tile (small M) takes
// the kernel instance with the small LDS, which doubles the workgroups per CU.  max_wgs > 0 caps the
// grid (tests).  The caller has checked the strides and the alignment of the bases to a sample.
constexpr int kChArsLds = 16256;       // float slots of LDS per tile (+ 128 of slack: 64 KiB, 2 workgroups per CU)
constexpr int kChArsLdsSmall = 8064;   // the small instance's (+ 128 of slack: 32 KiB, 5 workgroups per CU)
constexpr int kChArsMaxA = 1024;       // values of a per tile at most (16 wave units per phase)
constexpr int kChArsSmallMinA = 512;   // the small instance is taken when its tile holds this many a
constexpr int kChArsPitchPad = 31;     // the pitch search's range above the columns needed
static_assert((kChArsLds + 128) * 4 == 65536 && (kChArsLdsSmall + 128) * 4 == 32768, "LDS bytes per workgroup");
static_assert(kChArsLds / kChResMaxDown - ((kChResMaxK - 2 + kChResMaxDown) / kChResMaxDown + 1) - 1 >= 1,
              "a tile of both maxima holds an output");
static_assert(kChArsLds + kChResMaxDown < 65536, "a tile's positions divide by M through a 16-bit magic");
// The tile of (L, M, ntaps, input format): K, the values of a per tile, the LDS slots of the instance
// taken (kChArsLds or kChArsLdsSmall), the polyphase rows' pitch in float slots and the modelled extra
// LDS cycles of the stage's stores per wave (channel_audio_resample_pitch).
struct ChArsLayout {
    int K = 0, ta = 0, lds = 0, pitch = 0, store_conflicts = 0;
};
ChArsLayout channel_audio_resample_layout(int L, int M, int ntaps, int in_s16);
// The pitch in [need, max_pitch] of a transposition by `mod` into 4-byte slots whose stores cost the
// fewest extra LDS cycles, the smallest of equals: lane l of a 32-lane half holds samples V l + e (V = 4
// floats or 8 int16 of a 16-byte load) and stores e with one ds_write_b32, banked on the slot mod 32; the
// instruction's own 4 cycles hide a 2-way conflict in both halves (tools/channel_audio_resample_banks.py).
// A model at offset 0: the kernel's vectors start pg - al positions into the tile, which shifts the rows.
int channel_audio_resample_pitch(int mod, int need, int max_pitch, int V, int *store_conflicts);
hipError_t launch_channel_audio_resample(const KernelTables &t, const void *d_in, int in_s16, int nch, size_t nsamp,
                                         size_t in_stride, const float *d_taps, int ntaps, int L, int M, int e,
                                         size_t nout, const float *d_tail_in, float *d_tail_out, void *d_out,
                                         int out_s16, size_t out_stride, int max_wgs, int device, hipStream_t s);

// Channel demodulator (ddc_channel_demod.hip, sddc_ddc_channel_demodulate_device): AM / FM / BFO audio
// (demod_math.h) from nch streams laid out as for the decimator, any nsamp >= 1.  d_chan: [nch] mode,
// gain and BFO word; pos: the stream position of the call's first sample mod 2^32.  d_last_in /
// d_last_out: [nch] float2, each channel's last sample value before / after this call (two buffers).
// d_out: float (s16 = 0) or int16 (s16 = 1) samples, channel c at c * out_stride samples, aligned to
// one sample.  d_power: [nch] floats or nullptr; with it d_partial holds nch * channel_demod_tiles(nsamp)
// floats, the tile sums that a second launch adds per channel in a fixed order.  One work item per
// (channel, tile of kChDemTile samples); max_wgs > 0 caps the grid (tests).  The caller has checked
// the strides.
struct ChDemChannel;                   // demod_math.h: a channel's mode, gain and BFO word
constexpr int kChDemTile = 2048;       // samples per tile: 4 (CF32) or 2 (CS16) 16-byte loads per thread
inline size_t channel_demod_tiles(size_t nsamp) { return (nsamp + kChDemTile - 1) / kChDemTile; }
hipError_t launch_channel_demod(const KernelTables &t, const void *d_iq, int cs16, float cs16_scale, int nch,
                                size_t nsamp, size_t in_stride, const ChDemChannel *d_chan, uint32_t pos,
                                const float2 *d_last_in, float2 *d_last_out, void *d_out, int s16, size_t out_stride,
                                float *d_power, float *d_partial, int max_wgs, int device, hipStream_t s);

// Channel audio filter (ddc_channel_audio.hip, sddc_ddc_channel_audio_filter_device): one run of the
// block-form biquad cascade (audio_iir_math.h) over nch real streams of nsamp >= 1 samples, float
// (in_s16 = 0) or int16 read as (float)v, channel c at c * in_stride samples, aligned to one sample;
// outputs float or int16 (demod_s16) at c * out_stride samples.  block_pos: the stream position of
// the run's first sample mod kAudioBlock.  d_coef: [nch][nsec][5]; d_mat: [nch][2 nsec][2 nsec];
// d_state_in / d_state_out: [nch][3][2 nsec] floats (E, R, Zr) before / after the run (two buffers);
// d_scratch: 2 nsec floats per (channel, full block of the run), may be null when the run holds no
// full block (channel_audio_blocks).  Three launches on s; max_wgs > 0 caps their grids (tests).  The
// caller has checked the strides.
inline size_t channel_audio_blocks(unsigned block_pos, size_t nsamp)
{
    const size_t to_edge = (256u - block_pos) % 256u;
    return nsamp > to_edge ? (nsamp - to_edge) / 256u : 0;
}
hipError_t launch_channel_audio(const KernelTables &t, const void *d_in, int in_s16, int nch, int nsec, size_t nsamp,
                                size_t in_stride, unsigned block_pos, const float *d_coef, const float *d_mat,
                                const float *d_state_in, float *d_state_out, float *d_scratch, void *d_out, int out_s16,
                                size_t out_stride, int max_wgs, int device, hipStream_t s);

// Channel AGC (ddc_channel_agc.hip, sddc_ddc_channel_agc_device): one run of the max-plus block-form
// peak AGC (agc_math.h) over nch real streams, laid out and formatted as for the audio filter.
// block_pos: the stream position of the run's first sample mod kAgcBlock.  d_par: [nch][4] floats
// (T, d, F, dB), 16-byte aligned; d_state_in / d_state_out: [nch][3] floats (E, R, Zr) before / after
// the run (two buffers); d_scratch: one float per (channel, full block of the run), may be null when
// the run holds no full block (channel_audio_blocks counts them: the block lengths are equal); d_env:
// null, or [nch] floats that receive R after the run's last sample.  Three launches on s; max_wgs > 0
// caps their grids (tests).  The caller has checked the strides.
hipError_t launch_channel_agc(const KernelTables &t, const void *d_in, int in_s16, int nch, size_t nsamp, size_t in_stride,
                              unsigned block_pos, const float *d_par, const float *d_state_in, float *d_state_out,
                              float *d_scratch, void *d_out, int out_s16, size_t out_stride, float *d_env, int max_wgs,
                              int device, hipStream_t s);

// Channel noise blanker (ddc_channel_blank.hip, sddc_ddc_channel_blank_device): one call of the block-form
// impulse blanker (blanker_math.h) over nch IQ streams laid out as for the channel decimator (strides in
// components), CF32 or CS16 in and out.  pos: the stream index of the call's first sample; nsamp at most
// kBlankMaxLaunch (the runtime cuts longer calls).  d_par: [nch][2] floats (thr, qmin); d_state_in /
// d_state_out: [nch][kBlankStateWords] words before / after the call (two buffers); d_count: null, or
// [nch] counters that the caller has zeroed, to which the call adds its blanked outputs.  Two launches on
// s; max_wgs > 0 caps their grids and run_blocks > 0 sets the blocks per wave (tests; 0: chosen from the
// size).  The caller has checked the strides.
constexpr int kBlankStateWords = 404;
constexpr size_t kBlankMaxLaunch = (size_t)1 << 28;
hipError_t launch_channel_blank(const KernelTables &t, const void *d_iq, int cs16, int nch, size_t nsamp, size_t in_stride,
                                uint64_t pos, const float *d_par, int guard, int ref_blocks, int ref_mode,
                                const uint32_t *d_state_in, uint32_t *d_state_out, void *d_out, size_t out_stride,
                                uint32_t *d_count, int max_wgs, int run_blocks, int device, hipStream_t s);

// Channel squelch (ddc_channel_squelch.hip, sddc_ddc_channel_squelch_device): one launch set of the block-form
// gate (squelch_math.h) over nch real audio streams (F32 or S16 in and out, strides in samples) and their
// sense streams (sense_kind: squelch::kSense*; strides in components, even for the complex kinds; kSenseSelf:
// the audio, d_sense unused).  pos: the stream index of the first sample; nsamp at most kSquelchMaxLaunch.
// d_modes: [nch] ints; d_thr: [nch][2] floats (256 To, 256 Tc); d_state_in / d_state_out: [nch][
// kSquelchStateWords] words before / after (two buffers); d_words: [nch][blocks that hold a sample] words of
// scratch; d_open, d_count, d_level: null or [nch]; accumulate: d_count holds earlier launches of the same
// call and is added to.  Three launches on s; max_wgs > 0 caps their grids (tests).  The caller has checked
// the strides and the alignment of the bases to a sample.
constexpr int kSquelchStateWords = 264;
constexpr size_t kSquelchMaxLaunch = (size_t)1 << 28;
hipError_t launch_channel_squelch(const KernelTables &t, const void *d_audio, int in_s16, const void *d_sense, int sense_kind,
                                  int nch, size_t nsamp, size_t in_stride, size_t sense_stride, uint64_t pos,
                                  const int *d_modes, const float *d_thr, int attack, int hang, int fade,
                                  const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_words, void *d_out,
                                  int out_s16, size_t out_stride, uint32_t *d_open, uint32_t *d_count, float *d_level,
                                  int accumulate, int max_wgs, int device, hipStream_t s);

// Channel tone detector (ddc_channel_tone.hip, sddc_ddc_channel_tone_device): one launch set of the
// Goertzel bank and its gate (tone_math.h) over nch real sense streams (F32 or S16) and, where d_audio is not
// null, their audio streams (F32 or S16 in and out); strides in samples.  pos: the stream index of the first
// sample; nsamp at most kToneMaxLaunch.  d_tones: [ntones] phase words; d_masks: [nch], max_mask_tones: the most tones any of them has (it picks the windows kernel's shape, no
// bit depends on it); d_thr: [nch][3]
// floats (To, Tc, Emin); d_state_in / d_state_out: [nch][kToneStateWords] words before / after (two
// buffers); d_scratch: [nch][windows that hold a sample][4] words; d_tone, d_open, d_count: null or [nch];
// d_level: null or [nch][2]; d_powers: null or [nch][ntones]; accumulate: d_count holds earlier launches of
// the same call and is added to.  Two or three launches on s; max_wgs > 0 caps their grids (tests).  The
// caller has checked the strides and the alignment of the bases to a sample.
constexpr int kToneStateWords = 456;
constexpr size_t kToneMaxLaunch = (size_t)1 << 28;
hipError_t launch_channel_tone(const KernelTables &t, const void *d_sense, int sense_s16, size_t sense_stride, const void *d_audio,
                               int in_s16, int nch, size_t nsamp, size_t in_stride, uint64_t pos, const uint32_t *d_tones,
                               int ntones, const uint64_t *d_masks, int max_mask_tones, const float *d_thr, int window, int attack,
                               int hang, const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_scratch, void *d_out, int out_s16,
                               size_t out_stride, int *d_tone, uint32_t *d_open, uint32_t *d_count, float *d_level,
                               float *d_powers, int accumulate, int max_wgs, int device, hipStream_t s);

// Channel stereo decoder (ddc_channel_stereo.hip, sddc_ddc_channel_stereo_device): one launch set of the
// pilot measurement, its gate and the matrix (stereo_math.h) over nch real MPX streams (F32 or S16) into
// d_left and d_right (F32 or S16); strides in samples.  pos: the stream index of the first sample; nsamp at
// most kStereoMaxLaunch.  word: the pilot's phase word; d_modes: [nch] words (kStereoMono / kStereoAuto);
// d_thr: [nch][4] floats (To, Tc, Emin, g2); d_state_in / d_state_out: [nch][kStereoStateWords] words before
// / after (two buffers); d_scratch: kStereoScratchWords(nch, blocks that hold a sample) words; d_stereo,
// d_count: null or [nch]; d_level, d_phase: null or [nch][2]; accumulate: d_count holds earlier launches of
// the same call and is added to.  Three launches on s; max_wgs > 0 caps their grids (tests).  The caller has
// checked the strides and the alignment of the bases to a sample.
constexpr int kStereoStateWords = 268;
constexpr size_t kStereoMaxLaunch = (size_t)1 << 28;
constexpr size_t kStereoScratchWords(size_t nch, size_t blocks) { return nch * (2 * blocks + 1) * 4; }
hipError_t launch_channel_stereo(const KernelTables &t, const void *d_in, int in_s16, int nch, size_t nsamp, size_t in_stride,
                                 uint64_t pos, uint32_t word, const uint32_t *d_modes, const float *d_thr, int window, int attack,
                                 int hang, const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_scratch, void *d_left,
                                 void *d_right, int out_s16, size_t out_stride, uint32_t *d_stereo, uint32_t *d_count,
                                 float *d_level, float *d_phase, int accumulate, int max_wgs, int device, hipStream_t s);

// Channel DCS decoder (ddc_channel_dcs.hip, sddc_ddc_channel_dcs_device): one launch set of the sign
// sub-bins, the bit sums, the match and the gate (dcs_math.h) over nch real sense streams (F32 or S16) and,
// where d_audio is not null, their audio streams (F32 or S16 in and out); strides in samples.  pos: the
// stream index of the first sample; nsamp at most kDcsMaxLaunch.  d_cws: [ncodes] codewords; d_params:
// [nch][3] ints (code, invert, eye); word: the bit phase word; counts: the host's [8] N[t]; d_state_in /
// d_state_out: [nch][kDcsStateWords] words before / after (two buffers); d_scratch: [nch][windows that hold
// a sample][4] words; d_code, d_open, d_count: null or [nch]; d_info: null or [nch][4]; accumulate: d_count
// holds earlier launches of the same call and is added to; ballot: the windows kernel forms the sub-bin sums by
// ballots and popcounts instead of LDS atomics (the same integers).  Two or three launches on s; max_wgs > 0
// caps their grids (tests).  The caller has checked the strides and the alignment of the bases to a sample.
constexpr int kDcsStateWords = 200;
constexpr size_t kDcsMaxLaunch = (size_t)1 << 28;
hipError_t launch_channel_dcs(const KernelTables &t, const void *d_sense, int sense_s16, size_t sense_stride, const void *d_audio,
                              int in_s16, int nch, size_t nsamp, size_t in_stride, uint64_t pos, const uint32_t *d_cws, int ncodes,
                              const int *d_params, uint32_t word, const uint32_t *counts, int window, int e_open, int e_close,
                              int attack, int hang, const uint32_t *d_state_in, uint32_t *d_state_out, uint32_t *d_scratch,
                              void *d_out, int out_s16, size_t out_stride, int *d_code, uint32_t *d_open, uint32_t *d_count,
                              uint32_t *d_info, int accumulate, int ballot, int max_wgs, int device, hipStream_t s);

// batched FFTs (fft_batch.hip, include/sddc_fft.h); fft_prepare fills the device's twiddle
// table once (synchronises s the first time)
hipError_t fft_prepare(hipStream_t s);
hipError_t fft_c2c(const void *in, void *out, int n, int batch, int dir, hipStream_t s);
hipError_t fft_r2c(const float *in, void *out, int n, int batch, hipStream_t s);

}  // namespace sddc
