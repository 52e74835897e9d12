// ddc_runtime.cpp — implementation of the C ABI in include/sddc_ddc.h.
//
// Owns the per-handle device state that the reference keeps in fft_mt_r2iq
// (Core/fft_mt_r2iq.h:86-117): the filter bank (filterHw), the FFT "plans"
// (here: twiddle tables), the tune bin and the stream history.  A GPU handle's compute
// calls go to the gfx950 kernels only (no fallback); a handle created on
// SDDC_DDC_DEVICE_CPU holds the AVX2 backend (cpu/r2iq_cpu.h) instead and never calls HIP.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "cpu/r2iq_cpu.h"
#include "ddc_kernels.h"
#include "filterbank.h"
#include "fine_tune.h"
#include "fs_split_controller.hpp"
#include "sddc_fft.h"
#include "sddc_ddc.h"
#include "sddc_ddc_internal.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(SDDC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                                  \
    } while (0)

// Restores the caller's current device on scope exit (torch and other users of
// the same process keep their own current device).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

constexpr int kHistory = SDDC_DDC_HALF_FFT;
constexpr int kBlock = SDDC_DDC_BLOCK;
constexpr int kHostChunk = 32;   // blocks per pipeline chunk on the host path
constexpr size_t kOutBlockMax = (size_t)SDDC_DDC_OUT_BLOCK * 2 * sizeof(float);   // bytes, CF32 d = 0
// Per-channel NCO: the lane-start table holds 4 float2 per 128 output samples, i.e. 8192 >> d bytes
// per channel and input block.  Its size is capped: a call whose table would be larger runs as
// several runs of whole blocks.  128 MiB holds the bench's C5 step (1024 channels x 256 blocks at
// d = 4) in one run; one block of 1024 channels at d = 0 needs 8 MiB, so a run is never empty.
constexpr size_t kChNcoBlockBytes = (size_t)SDDC_DDC_OUT_BLOCK / sddc::FineTune::kBlock * sddc::FineTune::kLanes * sizeof(float2);
constexpr size_t kChNcoTableCap = (size_t)128 << 20;
static_assert(kChNcoBlockBytes == 8192, "4 lane starts per 128 output samples");
static_assert(SDDC_DDC_MAX_CHANNELS * kChNcoBlockBytes <= kChNcoTableCap, "one block of every channel fits the cap");

// The streams whose launches read a per-handle device table (the (P, Q) coefficients, the NCO
// staging buffer, the channel tune bins, the channel scratch rows).  The C ABI accepts any
// stream per call, so before a table is rewritten the writing stream waits for the last launch
// of EVERY stream that may still read it, not only the most recent one.
//
// lazy (the single-channel launches' set, sddc_ddc::readers, only): a launch only notes that its
// stream has work the event does not cover yet (pending), and the event is recorded on that stream
// when somebody is about to wait for it.  An event recorded later covers a superset of the
// launches, so every wait orders at least what it did, and a stream that is the handle's only one
// never gets an event marker between its kernels: a steady-state call enqueues its kernel and
// nothing else.  The record happens whether or not the stream's work has completed, at the latest
// in the handle's destroy, so a stream given to sddc_ddc_process_device must stay valid until the
// handle is destroyed (include/sddc_ddc.h).  Every other set records at each launch.
struct Readers {
    struct Entry {
        hipStream_t first;
        hipEvent_t second;
        bool pending;   // launches on `first` since `second` was recorded
    };
    std::vector<Entry> v;
    bool lazy = false;   // true: sddc_ddc::readers (SDDC_DDC_PARAM_LAZY_RECORD = 0 turns it off, A/B)

    // after a launch on s that reads the tables
    hipError_t record(hipStream_t s)
    {
        for (auto &p : v)
            if (p.first == s) {
                p.pending = true;
                return lazy ? hipSuccess : flush(p);
            }
        if (v.size() >= 16) {   // bound the set: wait for all, forget them
            hipError_t e = sync();
            if (e != hipSuccess) return e;
            clear();
        }
        hipEvent_t ev = nullptr;
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        v.push_back(Entry{s, ev, true});
        return lazy ? hipSuccess : flush(v.back());
    }
    // the entry's event covers every launch noted so far
    static hipError_t flush(Entry &p)
    {
        if (!p.pending) return hipSuccess;
        hipError_t e = hipEventRecord(p.second, p.first);
        if (e == hipSuccess) p.pending = false;
        return e;
    }
    // stream s (about to rewrite a table) waits for every other reader's last launch
    hipError_t order_before(hipStream_t s)
    {
        for (auto &p : v)
            if (p.first != s) {
                hipError_t e = flush(p);
                if (e == hipSuccess) e = hipStreamWaitEvent(s, p.second, 0);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    }
    // stream s waits for the last launch on stream `other` (nothing to do when other is s, or
    // when `other` has no entry: entries are dropped only after a host sync of all of them)
    hipError_t order_after(hipStream_t other, hipStream_t s)
    {
        if (other == s) return hipSuccess;
        for (auto &p : v)
            if (p.first == other) {
                hipError_t e = flush(p);
                return e == hipSuccess ? hipStreamWaitEvent(s, p.second, 0) : e;
            }
        return hipSuccess;
    }
    // the host waits for every reader (before a synchronous copy or a free).  An entry that fails
    // (a stream that is no longer valid cannot take its pending record) does not end the wait:
    // its event is waited for as last recorded, the remaining entries follow, and the first error
    // is returned.
    hipError_t sync()
    {
        hipError_t first = hipSuccess;
        for (auto &p : v) {
            hipError_t e = flush(p);
            const hipError_t es = hipEventSynchronize(p.second);
            if (e == hipSuccess) e = es;
            if (e != hipSuccess && first == hipSuccess) first = e;
        }
        return first;
    }
    void clear()
    {
        for (auto &p : v) (void)hipEventDestroy(p.second);
        v.clear();
    }
};

// The state of a streaming channel stage (the channel decimator, the channel resampler): the taps
// (empty = off) with the channel count, their device copy in the kernel's order, and each
// channel's last H sample values as float2 in two device buffers: a launch reads d_tail[cur] and
// writes the other one, and the host swaps them after it.  The tails are per handle, so every
// launch first waits for the other streams' last launches (readers).  A CPU handle keeps the
// tails in tail_h.  d_in / d_out are the host call's device buffers, grown on demand.
// Every member function runs under the handle's mu.
struct ChannelStream {
    std::vector<float> taps;
    int nch = 0, H = 0;
    float *d_taps = nullptr;
    size_t taps_cap = 0;                   // floats
    float2 *d_tail[2] = {};                // [nch][H] each
    int cur = 0;
    std::vector<float> tail_h;             // CPU handle: [nch][H][2]
    Readers readers;
    int max_wgs = 0;
    void *d_in = nullptr;
    float *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;        // bytes, floats

    // off: no taps, no tails (the caller has waited for the launches in flight)
    void clear()
    {
        taps.clear();
        nch = H = 0;
        tail_h.clear();
        for (float2 *&p : d_tail) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_taps) (void)hipFree(d_taps);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        d_taps = nullptr;
        d_in = nullptr;
        d_out = nullptr;
        taps_cap = in_cap = out_cap = 0;
        readers.clear();
    }
    // Validated taps (null or ntaps == 0: off) with their `nordered` floats in the kernel's order
    // and H_ kept values for each of nch_ channels; the tails start as zeros.
    int configure(sddc_ddc *h, const char *name, const float *t, int ntaps, const float *ordered, size_t nordered,
                  int H_, int nch_);
    int reset(sddc_ddc *h);   // the tails back to zeros
    // One launch on s, fn(tail_in, tail_out): it reads the current tails and writes the other
    // buffer, so it runs after every earlier launch of the handle, whatever its stream; the buffers
    // swap once it is enqueued.
    template <class F> int launch(hipStream_t s, F fn)
    {
        HIP_TRY(readers.order_before(s));
        const hipError_t e = fn(d_tail[cur], d_tail[cur ^ 1]);
        const hipError_t er = readers.record(s);   // whatever was enqueued stays ordered
        HIP_TRY(e);
        if (H > 0) cur ^= 1;
        HIP_TRY(er);
        return SDDC_OK;
    }
};

// The state of the channel demodulator (sddc_ddc_channel_demodulate_*): each channel's mode, gain and
// BFO word (empty = off) with their device copy, the output format, the stream position mod 2^32
// (host) and each channel's last sample value as float2 in two device buffers that swap per launch,
// as ChannelStream's tails do.  d_partial holds the power's tile sums of one call (grown on demand,
// after a wait for the launches that may still use it).  A CPU handle keeps the last samples in
// last_h.  d_in / d_out / d_pow are the host call's device buffers.  All under the handle's mu.
struct ChannelDemod {
    std::vector<sddc::ChDemChannel> chan;
    int nch = 0, out_fmt = 0;
    uint32_t pos = 0;
    sddc::ChDemChannel *d_chan = nullptr;
    float2 *d_last[2] = {};                // [nch] each
    int cur = 0;
    std::vector<float> last_h;             // CPU handle: [nch][2]
    float *d_partial = nullptr;
    size_t partial_cap = 0;                // floats
    Readers readers;
    int max_wgs = 0;
    void *d_in = nullptr, *d_out = nullptr;
    float *d_pow = nullptr;
    size_t in_cap = 0, out_cap = 0, pow_cap = 0;   // bytes, bytes, floats

    void clear()
    {
        chan.clear();
        nch = out_fmt = 0;
        pos = 0;
        last_h.clear();
        if (d_chan) (void)hipFree(d_chan);
        d_chan = nullptr;
        for (float2 *&p : d_last) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_partial) (void)hipFree(d_partial);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_pow) (void)hipFree(d_pow);
        d_partial = d_pow = nullptr;
        d_in = d_out = nullptr;
        partial_cap = in_cap = out_cap = pow_cap = 0;
        readers.clear();
    }
};

// The state of the channel audio filter (sddc_ddc_channel_audio_filter_*; audio_iir_math.h): the
// sections [nch][nsec][5] (empty = off) and the block matrices [nch][2 nsec][2 nsec] with their device
// copies, the formats, the stream position (host) and each channel's (E, R, Zr) as [nch][3][2 nsec]
// floats in two device buffers that swap per run, as ChannelDemod's last samples do per launch.
// d_scratch holds 2 nsec floats per (channel, full block) of one run (grown on demand, after a wait
// for the launches that may still use it).  A CPU handle keeps the state in state_h.  d_in / d_out are
// the host call's device buffers.  All under the handle's mu.
struct ChannelAudio {
    std::vector<float> coef, mat;
    int nch = 0, nsec = 0, in_fmt = 0, out_fmt = 0;
    uint64_t pos = 0;
    float *d_coef = nullptr, *d_mat = nullptr;
    float *d_state[2] = {};
    int cur = 0;
    std::vector<float> state_h;
    float *d_scratch = nullptr;
    size_t scratch_cap = 0;                // floats
    Readers readers;
    int max_wgs = 0, run_blocks = 0;       // SDDC_DDC_PARAM_CHAUD_MAX_WGS, _RUN_BLOCKS (0: kDefaultRunBlocks)
    void *d_in = nullptr, *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;        // bytes
    static constexpr int kDefaultRunBlocks = 512;   // measured: 8 % faster than 2048 on 1024 x 524288

    size_t state_floats() const { return (size_t)nch * 6 * (size_t)nsec; }
    void clear()
    {
        coef.clear();
        mat.clear();
        nch = nsec = in_fmt = out_fmt = 0;
        pos = 0;
        state_h.clear();
        for (float **p : {&d_coef, &d_mat, &d_state[0], &d_state[1]}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_scratch) (void)hipFree(d_scratch);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        d_scratch = nullptr;
        d_in = d_out = nullptr;
        scratch_cap = in_cap = out_cap = 0;
        readers.clear();
    }
};

// The state of the channel AGC (sddc_ddc_channel_agc_*; agc_math.h): the parameters [nch][4] = (T, d,
// F, dB) (empty = off) with their device copy, the formats, the stream position (host) and each
// channel's (E, R, Zr) as [nch][3] floats in two device buffers that swap per run, as ChannelAudio's
// do.  d_scratch holds one float per (channel, full block) of one run (grown on demand, after a wait
// for the launches that may still use it).  A CPU handle keeps the state in state_h.  d_in / d_out /
// d_env are the host call's device buffers.  All under the handle's mu.
struct ChannelAgc {
    std::vector<float> par;
    int nch = 0, in_fmt = 0, out_fmt = 0;
    uint64_t pos = 0;
    float *d_par = nullptr;
    float *d_state[2] = {};
    int cur = 0;
    std::vector<float> state_h;
    float *d_scratch = nullptr;
    size_t scratch_cap = 0;                // floats
    Readers readers;
    int max_wgs = 0, run_blocks = 0;       // SDDC_DDC_PARAM_CHAGC_MAX_WGS, _RUN_BLOCKS (0: kDefaultRunBlocks)
    void *d_in = nullptr, *d_out = nullptr;
    float *d_env = nullptr;
    size_t in_cap = 0, out_cap = 0, env_cap = 0;   // bytes, bytes, floats
    static constexpr int kDefaultRunBlocks = 2048;   // measured: 3.5 % faster than 512 on 1024 x 524288

    size_t state_floats() const { return (size_t)nch * 3; }
    void clear()
    {
        par.clear();
        nch = in_fmt = out_fmt = 0;
        pos = 0;
        state_h.clear();
        for (float **p : {&d_par, &d_state[0], &d_state[1]}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_scratch) (void)hipFree(d_scratch);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_env) (void)hipFree(d_env);
        d_scratch = d_env = nullptr;
        d_in = d_out = nullptr;
        scratch_cap = in_cap = out_cap = env_cap = 0;
        readers.clear();
    }
};

// The state of the channel noise blanker (sddc_ddc_channel_blank_*; blanker_math.h): the parameters
// [nch][2] = (thr, qmin) (empty = off) with their device copy, the guard, the reference and the format,
// the stream position (host) and each channel's state (block powers, unfinished block, last g samples,
// last hit) as [nch][kBlankStateWords] words in two device buffers that swap per launch, as ChannelAgc's
// do.  A CPU handle keeps the state in state_h.  d_in / d_out / d_count are the host call's device
// buffers.  All under the handle's mu.
struct ChannelBlanker {
    std::vector<float> par;
    int nch = 0, guard = 0, ref_blocks = 0, ref_mode = 0, fmt = 0;
    uint64_t pos = 0;
    float *d_par = nullptr;
    uint32_t *d_state[2] = {};
    int cur = 0;
    std::vector<sddc::cpu::R2iq::BlankerChannel> state_h;
    Readers readers;
    int max_wgs = 0, run_blocks = 0;   // SDDC_DDC_PARAM_CHNB_MAX_WGS, _RUN_BLOCKS (0: chosen from the size)
    void *d_in = nullptr, *d_out = nullptr;
    uint32_t *d_count = nullptr;
    size_t in_cap = 0, out_cap = 0, count_cap = 0;   // bytes, bytes, counters

    size_t state_words() const { return (size_t)nch * sddc::kBlankStateWords; }
    void clear()
    {
        par.clear();
        nch = guard = ref_blocks = ref_mode = fmt = 0;
        pos = 0;
        state_h.clear();
        if (d_par) (void)hipFree(d_par);
        d_par = nullptr;
        for (uint32_t *&p : d_state) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_count) (void)hipFree(d_count);
        d_in = d_out = nullptr;
        d_count = nullptr;
        in_cap = out_cap = count_cap = 0;
        readers.clear();
    }
};

// The state of the channel squelch (sddc_ddc_channel_squelch_*; squelch_math.h): the modes [nch] and the
// thresholds [nch][2] = (256 To, 256 Tc) (empty = off) with their device copies, the handle's attack, hang,
// fade, sense kind and formats, the stream position (host) and each channel's state (the state machine, the
// last level, the unfinished block) as [nch][kSquelchStateWords] words in two device buffers that swap per
// launch set, as ChannelBlanker's do; d_words is the scratch of one word per channel and block of a launch
// set, grown on demand.  A CPU handle keeps the state in state_h.  d_in / d_sense / d_out / d_side are the
// host call's device buffers.  All under the handle's mu.
struct ChannelSquelch {
    static constexpr int kDefaultRunBlocks = 4096;
    std::vector<int> modes;
    std::vector<float> thr;
    int nch = 0, attack = 0, hang = 0, fade = 0, sense = 0, in_fmt = 0, out_fmt = 0;
    uint64_t pos = 0;
    int *d_modes = nullptr;
    float *d_thr = nullptr;
    uint32_t *d_state[2] = {};
    int cur = 0;
    uint32_t *d_words = nullptr;
    size_t words_cap = 0;
    std::vector<sddc::cpu::R2iq::SquelchChannel> state_h;
    Readers readers;
    int max_wgs = 0, run_blocks = 0;   // SDDC_DDC_PARAM_CHSQ_MAX_WGS, _RUN_BLOCKS (0: kDefaultRunBlocks)
    void *d_in = nullptr, *d_sense = nullptr, *d_out = nullptr;
    uint32_t *d_side = nullptr;        // [3][nch]: open, count, level
    size_t in_cap = 0, sense_cap = 0, out_cap = 0, side_cap = 0;   // bytes, bytes, bytes, words

    size_t state_words() const { return (size_t)nch * sddc::kSquelchStateWords; }
    void clear()
    {
        modes.clear();
        thr.clear();
        nch = attack = hang = fade = sense = in_fmt = out_fmt = 0;
        pos = 0;
        state_h.clear();
        if (d_modes) (void)hipFree(d_modes);
        if (d_thr) (void)hipFree(d_thr);
        d_modes = nullptr;
        d_thr = nullptr;
        for (uint32_t *&p : d_state) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_words) (void)hipFree(d_words);
        if (d_in) (void)hipFree(d_in);
        if (d_sense) (void)hipFree(d_sense);
        if (d_out) (void)hipFree(d_out);
        if (d_side) (void)hipFree(d_side);
        d_words = d_side = nullptr;
        d_in = d_sense = d_out = nullptr;
        words_cap = in_cap = sense_cap = out_cap = side_cap = 0;
        readers.clear();
    }
};

// The state of the channel tone detector (sddc_ddc_channel_tone_*; tone_math.h): the tone words [ntones],
// the masks [nch] and the scaled thresholds [nch][3] = (To, Tc, Emin) (empty = off) with their device copies,
// the handle's window, attack, hang and formats, the stream position (host) and each channel's state as
// [nch][kToneStateWords] words in two device buffers that swap per launch set, as ChannelSquelch's do;
// d_scratch holds four words per channel and window of a launch set, grown on demand.  A CPU handle keeps
// the state in state_h.  d_sense / d_in / d_out / d_side are the host call's device buffers.  All under the
// handle's mu.
struct ChannelTone {
    static constexpr int kDefaultRunBlocks = 4096;
    std::vector<uint32_t> words;
    std::vector<uint64_t> masks;
    std::vector<float> thr;
    int nch = 0, ntones = 0, window = 0, attack = 0, hang = 0, sense_fmt = 0, in_fmt = 0, out_fmt = 0;
    int max_mask_tones = 0;   // the most tones any channel's mask has
    uint64_t pos = 0;
    uint32_t *d_tones = nullptr;
    uint64_t *d_masks = nullptr;
    float *d_thr = nullptr;
    uint32_t *d_state[2] = {};
    int cur = 0;
    uint32_t *d_scratch = nullptr;
    size_t scratch_cap = 0;
    std::vector<sddc::cpu::R2iq::ToneChannel> state_h;
    Readers readers;
    int max_wgs = 0, run_blocks = 0;   // SDDC_DDC_PARAM_CHTONE_MAX_WGS, _RUN_BLOCKS (0: kDefaultRunBlocks)
    void *d_sense = nullptr, *d_in = nullptr, *d_out = nullptr;
    uint32_t *d_side = nullptr;        // [nch] tone, [nch] open, [nch] count, [nch][2] level, [nch][ntones] powers
    size_t sense_cap = 0, in_cap = 0, out_cap = 0, side_cap = 0;   // bytes, bytes, bytes, words

    size_t state_words() const { return (size_t)nch * sddc::kToneStateWords; }
    void clear()
    {
        words.clear();
        masks.clear();
        thr.clear();
        nch = ntones = window = attack = hang = sense_fmt = in_fmt = out_fmt = max_mask_tones = 0;
        pos = 0;
        state_h.clear();
        if (d_tones) (void)hipFree(d_tones);
        if (d_masks) (void)hipFree(d_masks);
        if (d_thr) (void)hipFree(d_thr);
        d_tones = nullptr;
        d_masks = nullptr;
        d_thr = nullptr;
        for (uint32_t *&p : d_state) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_scratch) (void)hipFree(d_scratch);
        if (d_sense) (void)hipFree(d_sense);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_side) (void)hipFree(d_side);
        d_scratch = d_side = nullptr;
        d_sense = d_in = d_out = nullptr;
        scratch_cap = sense_cap = in_cap = out_cap = side_cap = 0;
        readers.clear();
    }
};

// The state of the channel DCS decoder (sddc_ddc_channel_dcs_*; dcs_math.h): the codewords [ncodes] and the
// per-channel (code, invert, eye) [nch][3] (empty = off) with their device copies, the handle's phase word,
// window, N[t], error limits, attack, hang and formats, the stream position (host) and each channel's state as
// [nch][kDcsStateWords] words in two device buffers that swap per launch set, as ChannelTone's do; d_scratch
// holds four words per channel and window of a launch set, grown on demand.  A CPU handle keeps the state in
// state_h.  d_sense / d_in / d_out / d_side are the host call's device buffers.  All under the handle's mu.
struct ChannelDcs {
    static constexpr int kDefaultRunBlocks = 4096;
    std::vector<uint32_t> cws;
    std::vector<int32_t> params;
    uint32_t word = 0, counts[sddc::dcs::kDcsPhases] = {};
    int nch = 0, ncodes = 0, window = 0, e_open = 0, e_close = 0, attack = 0, hang = 0, sense_fmt = 0, in_fmt = 0, out_fmt = 0;
    uint64_t pos = 0;
    uint32_t *d_cws = nullptr;
    int32_t *d_params = nullptr;
    uint32_t *d_state[2] = {};
    int cur = 0;
    uint32_t *d_scratch = nullptr;
    size_t scratch_cap = 0;
    std::vector<sddc::cpu::R2iq::DcsChannel> state_h;
    Readers readers;
    int max_wgs = 0, run_blocks = 0;   // SDDC_DDC_PARAM_CHDCS_MAX_WGS, _RUN_BLOCKS (0: kDefaultRunBlocks)
    int ballot = 0;                    // SDDC_DDC_PARAM_CHDCS_BALLOT
    void *d_sense = nullptr, *d_in = nullptr, *d_out = nullptr;
    uint32_t *d_side = nullptr;        // [nch] code, [nch] open, [nch] count, [nch][4] info
    size_t sense_cap = 0, in_cap = 0, out_cap = 0, side_cap = 0;   // bytes, bytes, bytes, words

    size_t state_words() const { return (size_t)nch * sddc::kDcsStateWords; }
    void clear()
    {
        cws.clear();
        params.clear();
        word = 0;
        nch = ncodes = window = e_open = e_close = attack = hang = sense_fmt = in_fmt = out_fmt = 0;
        pos = 0;
        state_h.clear();
        if (d_cws) (void)hipFree(d_cws);
        if (d_params) (void)hipFree(d_params);
        d_cws = nullptr;
        d_params = nullptr;
        for (uint32_t *&p : d_state) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_scratch) (void)hipFree(d_scratch);
        if (d_sense) (void)hipFree(d_sense);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_side) (void)hipFree(d_side);
        d_scratch = d_side = nullptr;
        d_sense = d_in = d_out = nullptr;
        scratch_cap = sense_cap = in_cap = out_cap = side_cap = 0;
        readers.clear();
    }
};

// The state of the channel stereo decoder (sddc_ddc_channel_stereo_*; stereo_math.h): the modes [nch] and the
// scaled parameters [nch][4] = (To, Tc, Emin, g2) (empty = off) with their device copies, the handle's pilot
// word, window, attack, hang and formats, the stream position (host) and each channel's state as
// [nch][kStereoStateWords] words in two device buffers that swap per launch set, as ChannelTone's do (init: a
// new stream's, with q = (1, 0)); d_scratch holds kStereoScratchWords of a launch set, grown on demand.  A CPU
// handle keeps the state in state_h.  d_in / d_out / d_side are the host call's device buffers.  All under the
// handle's mu.
struct ChannelStereo {
    static constexpr int kDefaultRunBlocks = 4096;
    std::vector<uint8_t> modes;
    std::vector<float> thr;
    std::vector<uint32_t> init;
    uint32_t word = 0;
    int nch = 0, window = 0, attack = 0, hang = 0, in_fmt = 0, out_fmt = 0;
    uint64_t pos = 0;
    uint32_t *d_modes = nullptr;
    float *d_thr = nullptr;
    uint32_t *d_state[2] = {};
    int cur = 0;
    uint32_t *d_scratch = nullptr;
    size_t scratch_cap = 0;
    std::vector<sddc::cpu::R2iq::StereoChannel> state_h;
    Readers readers;
    int max_wgs = 0, run_blocks = 0;   // SDDC_DDC_PARAM_CHST_MAX_WGS, _RUN_BLOCKS (0: kDefaultRunBlocks)
    void *d_in = nullptr, *d_out = nullptr;   // d_out: the left streams, then the right ones
    uint32_t *d_side = nullptr;               // [nch] stereo, [nch] count, [nch][2] level, [nch][2] phase
    size_t in_cap = 0, out_cap = 0, side_cap = 0;   // bytes, bytes, words

    size_t state_words() const { return (size_t)nch * sddc::kStereoStateWords; }
    void clear()
    {
        modes.clear();
        thr.clear();
        init.clear();
        word = 0;
        nch = window = attack = hang = in_fmt = out_fmt = 0;
        pos = 0;
        state_h.clear();
        if (d_modes) (void)hipFree(d_modes);
        if (d_thr) (void)hipFree(d_thr);
        d_modes = nullptr;
        d_thr = nullptr;
        for (uint32_t *&p : d_state) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        cur = 0;
    }
    void free_all()
    {
        clear();
        if (d_scratch) (void)hipFree(d_scratch);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_side) (void)hipFree(d_side);
        d_scratch = d_side = nullptr;
        d_in = d_out = nullptr;
        scratch_cap = in_cap = out_cap = side_cap = 0;
        readers.clear();
    }
};

}  // namespace

struct sddc_ddc {
    int device = 0;
    float gain = 0.f;
    int d = 0, lsb = 0, rand = 0, tunebin = SDDC_DDC_HALF_FFT / 4;   // ctor: mtunebin = halfFft/4
    int out_fmt = SDDC_DDC_FMT_CF32;       // output stage format
    float cs16_scale = 1.f;
    sddc::KernelTables tables;
    sddc::LaunchCache launch_cache;        // per-kernel resident workgroups and CUs of this device
    float2 *d_tables = nullptr;

    mutable std::mutex mu;                 // serialises the host path and buffer growth
    hipStream_t stream = nullptr;          // host path: compute stream

    // host path pipeline (process_host / process_blocks): two chunk slots; H2D on s_in,
    // kernel on `stream`, D2H on s_out, ordered by events.  The stream history (last 4096
    // input samples) stays on the device: the tail of the newest slot's input.
    struct HostSlot {
        int16_t *d_in = nullptr;           // [history | kHostChunk blocks]
        void *d_out = nullptr;
        int16_t *h_in = nullptr;           // pinned staging, used for unregistered callers
        void *h_out = nullptr;
        hipEvent_t e_h2d = nullptr, e_k = nullptr, e_d2h = nullptr;
    } hs[2];
    hipStream_t s_in = nullptr, s_out = nullptr;
    bool host_ready = false;
    int last_slot = -1, last_n = 0;        // where the history lives; -1 = zeros (create/reset)
    std::vector<std::pair<const char *, size_t>> regions;   // sddc_ddc_register_host

    int *d_tunebins = nullptr;             // channel tune bins (device)
    std::vector<int> tunebins_cached;
    int2 *d_windows = nullptr;             // per-chunk compact forward-bin windows (channels v2)
    int windows_d = -1;                    // d they were computed for; -2 = do not fit
    float2 *d_chscratch = nullptr;         // channels v2: per-workgroup split-spectrum rows
    int chscratch_rows = 0;
    Readers ch_readers;                    // streams of many-channel launches (tune bins, windows, scratch)

    // split x filter coefficients of the current (d, tunebin), rebuilt on device when either
    // changes; readers = the streams of single-channel launches that read them (and d_nco)
    // Each table set remembers the stream its last rebuild ran on (pq_s, fs_s): a launch
    // on another stream first waits for that stream's last recorded launch (Readers::order_after),
    // which is behind the rebuild (a rebuild is recorded like a launch).
    float4 *d_pq = nullptr;
    int pq_d = -1, pq_tb = -1;
    hipStream_t pq_s = nullptr;
    // the d = 0 wave kernel's per-tunebin tables: pqW (4096 float4) then twI (4096 float2)
    // the d = 0 fused-split kernel's per-tunebin tables: pqf (4096 float4) then fsl (768 float2)
    float4 *d_fs = nullptr;
    int fs_tb = -1;
    hipStream_t fs_s = nullptr;
    // the single-channel kernels' dynamic frame queues: a ring of kQueueSlots slots, one per launch
    // in turn.  A slot is zero when its launch starts and its last workgroup zeroes it again, so
    // the slot's next launch must start after that launch has finished: on the same stream that
    // is stream order; on another stream it waits for the slot's stream (q_s).  A slot whose
    // launch failed, or every slot after a HIP error, is zeroed stream-ordered before its next use.
    static constexpr int kQueueSlots = 64;
    unsigned *d_queue = nullptr;
    int queue_slot = 0;
    int slot_weights = sddc::kSlotWeighting;    // the persistent kernel's slot-weighted split (ddc_queue.hpp)
    sddc::FsSched fs_sched;                    // the d = 0 kernel's frame schedule (ddc_kernels.h)
    hipStream_t q_s[kQueueSlots] = {};

    // The d = 0 kernel's adaptive static split (fs_split_controller.hpp), all under mu.  Each
    // full-residency launch of the static schedule takes a slot of a ring in host-mapped pinned
    // memory, where its workgroups write {start, end, tag, check} as they exit, and the share table
    // the controller built from the launches measured so far (in the kernel arguments: no device
    // table, no stream operation).  The next such launch picks up whatever slots are complete: an
    // entry counts only with its launch's tag and check word, so a slot that is stale, partly
    // written or overwritten by a launch that ran late is simply not complete (and is dropped when
    // its turn in the ring comes again).  A launch on another stream than the one before it may
    // overlap it: it, the one before it and the next kTaint launches are not used.
    struct FsAdapt {
        static constexpr int kRing = 16;
        static constexpr int kTaint = 4;
        static constexpr int kEager = 32;    // measurements taken one per launch; then one in kEvery launches
        static constexpr int kEvery = 8;
        bool on = true;                      // SDDC_DDC_PARAM_FS_ADAPTIVE_SPLIT
        sddc::FsSplitController ctl;
        std::vector<float> forced;           // sddc_ddc_internal_fs_set_shares
        unsigned *h_ring = nullptr, *d_ring = nullptr;   // [kRing][kFsShareMaxG][4]
        bool ring_failed = false;
        struct Pending {
            unsigned tag = 0u;
            int G = 0, ns = 0;
            bool live = false, tainted = false;
            std::vector<int> n;              // frames per workgroup of that launch
        } pend[kRing];
        int next = 0, last_pending = -1;
        unsigned seq = 0u;
        sddc::FsShares tab = {};             // the current table, its batch size and frames per workgroup
        std::vector<int> tab_n, base_n;
        int tab_ns = -1, base_ns = -1;
        hipStream_t cur_s = nullptr, last_s = nullptr;
        bool have_last = false;
        int taint_left = 0;
        long launches = 0, skipped = 0;
        int last_table = 0, last_logged = 0; // the last d = 0 launch: took a table / was measured
    } fsa;
    bool q_used[kQueueSlots] = {};
    bool q_dirty[kQueueSlots] = {};
    Readers readers{{}, true};   // lazy: no event marker between the single-channel launches of one stream

    // fused fine-tune NCO: host chain + per-launch [T | lane starts] staged through a
    // pinned 3-slot ring into d_nco (stream-ordered copy before each launch)
    float nco_fc = 0.f;
    sddc::FineTune nco;
    static constexpr int kNcoSlots = 3;
    float2 *h_nco[kNcoSlots] = {};
    hipEvent_t nco_ev[kNcoSlots] = {};
    size_t h_nco_cap = 0;                  // float2 per slot
    int nco_slot = 0;
    float2 *d_nco = nullptr;
    size_t d_nco_cap = 0;

    // per-channel fine-tune NCO of the many-channel path (sddc_ddc_set_channel_fine_tune): T, fc and
    // the lane-start state per channel on the device (the chain kernel advances the state, so a
    // call needs no host round trip), and the lane-start table of one run of a call.  All are per
    // handle: ch_readers orders the launches that touch them, a change of the fc array synchronises.
    std::vector<float> chnco_fc;           // empty = off
    float2 *d_chnco_trig = nullptr;        // [1024][32]
    float2 *d_chnco_state = nullptr;       // [1024][4]
    float *d_chnco_fc = nullptr;           // [1024]
    float2 *d_chnco_starts = nullptr;      // [nch][run's 128-sample blocks][4]
    size_t chnco_starts_cap = 0;           // bytes
    int chnco_run_blocks = 0;              // SDDC_DDC_PARAM_CH_NCO_RUN_BLOCKS

    // history to start the next host-path call from (sddc_ddc_set_history)
    std::vector<int16_t> hist_override;

    // wideband spectrum (sddc_ddc_spectrum_*): the window (empty = rectangular) with its sum, its
    // device copy, the partial rows [blocks][4096] of calls with more than one block per row
    // (grown on demand) and the host call's device buffers.  sp_readers holds the streams of the
    // spectrum launches: a launch that uses the partial rows waits for the other streams' last
    // launches, a change of the window or a regrowth for all of them.
    std::vector<float> sp_win;
    double sp_wsum = (double)SDDC_DDC_FFTN;
    float *d_sp_win = nullptr;             // [8192]
    float *d_sp_partial = nullptr;
    size_t sp_partial_cap = 0;             // blocks
    int16_t *d_sp_in = nullptr;            // spectrum_host: [4096 + sp_host_cap * 65536]
    float *d_sp_out = nullptr;             // spectrum_host: [sp_host_cap][4096]
    size_t sp_host_cap = 0;                // blocks
    Readers sp_readers;
    int sp_max_wgs = 0;                    // SDDC_DDC_PARAM_SPECTRUM_MAX_WGS

    // channel spectrum (sddc_ddc_channel_spectrum_*): the window with its length (chsp_n == 0:
    // rectangular) and its sum, its device copy, and the host call's device buffers (grown on
    // demand).  The launches keep no other state; chsp_readers holds their streams, and a change of
    // the window waits for all of them.
    std::vector<float> chsp_win;
    int chsp_n = 0;
    double chsp_wsum = 0.0;
    float *d_chsp_win = nullptr;           // [4096]
    void *d_chsp_in = nullptr;             // channel_spectrum_host
    float *d_chsp_out = nullptr;
    size_t chsp_in_cap = 0, chsp_out_cap = 0;   // bytes, floats
    Readers chsp_readers;
    int chsp_max_wgs = 0;                  // SDDC_DDC_PARAM_CHSPEC_MAX_WGS

    // channel decimator and channel resampler (sddc_ddc_channel_{decimate,resample}_*): one
    // ChannelStream each, with H = ntaps - 1 and H = K - 1 = ceil(ntaps / up) - 1 kept values per
    // channel, and what the stage alone owns.  The resampler's stream position is reduced to chres_e
    // = m0 down - N up (0 <= chres_e < down) for N samples consumed and m0 = ceil(N up / down)
    // outputs produced: all a call needs, and no product overflows at any stream length.
    ChannelStream chdec, chres;            // max_wgs: SDDC_DDC_PARAM_CH{DEC,RES}_MAX_WGS
    int chdec_R = 0;
    int chres_L = 0, chres_M = 0, chres_e = 0;
    // channel audio resampler (sddc_ddc_channel_audio_resample_*): a ChannelStream whose tails hold
    // REAL sample values, [nch][K - 1] floats at the start of its float2 buffers, which are sized
    // ceil((K - 1) / 2) float2 per channel; d_out holds output samples of either format.  The
    // position is reduced as the resampler's (audio_resample_math.h).
    ChannelStream chars;                   // max_wgs: SDDC_DDC_PARAM_CHARS_MAX_WGS
    int chars_L = 0, chars_M = 0, chars_e = 0, chars_in_fmt = 0, chars_out_fmt = 0;
    ChannelDemod chdem;                    // max_wgs: SDDC_DDC_PARAM_CHDEM_MAX_WGS
    ChannelAudio chaud;
    ChannelAgc chagc;
    ChannelBlanker chnb;
    ChannelSquelch chsq;
    ChannelTone chtone;
    ChannelDcs chdcs;
    ChannelStereo chst;

    // CPU handle (device SDDC_DDC_DEVICE_CPU): the AVX2 backend; no HIP object above exists
    std::unique_ptr<sddc::cpu::R2iq> cpu;

    // fault injection for failover tests (GPU handles): environment SDDC_DDC_INJECT_FAIL=N
    // makes the (N+1)-th process_* call fail with SDDC_ERR_HIP before any device work
    long inject_fail = -1;
    long inject_late = -1;   // SDDC_DDC_INJECT_FAIL_AFTER_D2H
};

// setFreqOffset's arithmetic (fft_mt_r2iq.cpp:104-106): the tune bin, clamped into [0, 4092],
// and the residual tunebin/4096 - offset of the unclamped bin
static int tuning_of(float offset, float *delta)
{
    const int tb = (int)(offset * SDDC_DDC_HALF_FFT / 4) * 4;
    *delta = ((float)tb / SDDC_DDC_HALF_FFT) - offset;
    return std::min(std::max(tb, 0), SDDC_DDC_HALF_FFT - 4);
}

static bool injected_failure(sddc_ddc_t *h)
{
    if (h->inject_fail < 0) return false;
    return h->inject_fail-- == 0;
}
// SDDC_DDC_INJECT_FAIL_AFTER_D2H=N: the (N+1)-th host call fails after its first chunk's kernel and
// D2H were issued, i.e. with device work in flight and the output partly written (a mid-stream
// HIP error as the drop-in's failover meets it)
static bool injected_late_failure(sddc_ddc_t *h)
{
    if (h->inject_late < 0) return false;
    return h->inject_late-- == 0;
}

// A host call's device buffer of at least `need` elements (bytes for a void buffer).  The earlier
// host calls were synchronous: nothing reads the old buffer.
template <class T>
static int grow_device_buffer(T **ptr, size_t *cap, size_t need, const char *who, const char *what)
{
    if (need <= *cap) return SDDC_OK;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    constexpr size_t elem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    if (hipMalloc(ptr, need * elem) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SDDC_ERR_NOMEM, "%s: no device memory for %zu %s", who, need, what);
    }
    *cap = need;
    return SDDC_OK;
}

/* ---- the channel stream stages' shared state machine (ChannelStream) ---------------------- */
int ChannelStream::configure(sddc_ddc_t *h, const char *name, const float *t, int ntaps, const float *ordered,
                             size_t nordered, int H_, int nch_)
{
    const bool off = !t || ntaps == 0;
    const size_t tail = off ? 0 : (size_t)nch_ * (size_t)H_;   // complex values
    if (h->cpu) {
        clear();
        if (off) return SDDC_OK;
        try {
            tail_h.assign(2 * tail, 0.f);
            taps.assign(t, t + ntaps);
        } catch (const std::exception &ex) {
            clear();
            return fail(SDDC_ERR_NOMEM, "%s: %s", name, ex.what());
        }
        H = H_;
        nch = nch_;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    HIP_TRY(readers.sync());   // earlier launches, on any stream, may still use the taps and the tails
    clear();                   // a failed upload leaves the stage off
    if (off) return SDDC_OK;
    if (nordered > taps_cap) {
        if (d_taps) (void)hipFree(d_taps);
        d_taps = nullptr;
        taps_cap = 0;
        HIP_TRY(hipMalloc(&d_taps, nordered * sizeof(float)));
        taps_cap = nordered;
    }
    HIP_TRY(hipMemcpy(d_taps, ordered, nordered * sizeof(float), hipMemcpyHostToDevice));
    if (tail) {
        for (float2 *&p : d_tail) {
            if (hipMalloc(&p, tail * sizeof(float2)) != hipSuccess) {
                (void)hipGetLastError();
                p = nullptr;
                clear();
                return fail(SDDC_ERR_NOMEM, "%s: no device memory for %zu tail values", name, tail);
            }
        }
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        hipError_t e = hipMemsetAsync(d_tail[0], 0, tail * sizeof(float2), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            clear();
            HIP_TRY(e);
        }
    }
    taps.assign(t, t + ntaps);
    H = H_;
    nch = nch_;
    return SDDC_OK;
}

int ChannelStream::reset(sddc_ddc_t *h)
{
    if (h->cpu) {
        std::fill(tail_h.begin(), tail_h.end(), 0.f);
        return SDDC_OK;
    }
    const size_t tail = (size_t)nch * (size_t)H;
    if (!tail) return SDDC_OK;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    HIP_TRY(readers.sync());   // earlier launches, on any stream, may still use the tails
    HIP_TRY(hipMemsetAsync(d_tail[cur], 0, tail * sizeof(float2), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    return SDDC_OK;
}

// The stride, null and alignment checks of a stage's call (under h->mu: the format is read here);
// out_need names 2 nout in the stage's terms.
static int check_channel_io(const sddc_ddc_t *h, const char *out_need, const void *iq, int nch, size_t nsamp,
                            size_t in_stride, const float *out, size_t out_stride, size_t nout)
{
    if (nch > 1 && (in_stride < 2 * nsamp || (in_stride & 1) != 0))
        return fail(SDDC_ERR_ARG, "in_stride must be even and >= 2 nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && (out_stride < 2 * nout || (out_stride & 1) != 0))
        return fail(SDDC_ERR_ARG, "out_stride must be even and >= %s (got %zu, need %zu)", out_need, out_stride, 2 * nout);
    if (!iq || !out) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t sample = h->out_fmt == SDDC_DDC_FMT_CS16 ? 4 : 8;
    if (((uintptr_t)iq & (sample - 1)) != 0) return fail(SDDC_ERR_ARG, "iq must be %d-byte aligned", (int)sample);
    if (((uintptr_t)out & 7) != 0) return fail(SDDC_ERR_ARG, "the output must be 8-byte aligned");
    return SDDC_OK;
}

// A stage's host call on a GPU handle: the channels' samples to the device, launch(d_in, d_out) on
// the handle's stream, the nout outputs of every channel back, and a wait for all of it.
template <class F>
static int channel_host_roundtrip(sddc_ddc_t *h, ChannelStream &st, const char *who, const void *iq, int nch,
                                  size_t nsamp, size_t in_stride, float *out, size_t out_stride, size_t nout, F launch)
{
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs (one float2 at least: a call without an output)
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + 2 * nsamp) *
                            (h->out_fmt == SDDC_DDC_FMT_CS16 ? 2 : 4);
    const size_t out_floats = (size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + 2 * nout;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, who, "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_floats ? out_floats : 2, who, "output floats")) return rc;
    HIP_TRY(hipMemcpyAsync(st.d_in, iq, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = launch(st.d_in, st.d_out);
    if (rc == SDDC_OK && nout) {   // the streams alone: the caller's memory between them stays as it is
        if (nch == 1 || out_stride == 2 * nout)
            HIP_TRY(hipMemcpyAsync(out, st.d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, out_stride * sizeof(float), st.d_out, out_stride * sizeof(float),
                                     2 * nout * sizeof(float), (size_t)nch, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

extern "C" {

int sddc_ddc_abi_version(void) { return SDDC_DDC_ABI_VERSION; }

const char *sddc_ddc_last_error(void) { return g_last_error.c_str(); }

int sddc_ddc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sddc_ddc_kaiser(int ntaps, float astop, float fpass, float fstop, float *coef)
{
    return sddc::kaiser_window(ntaps, astop, fpass, fstop, coef);
}

int sddc_ddc_filter_taps(int d, float *taps)
{
    if (d < 0 || d >= SDDC_DDC_NDEC || !taps) return fail(SDDC_ERR_ARG, "filter_taps: bad d=%d or null", d);
    sddc::filter_taps(d, taps);
    return SDDC_OK;
}

int sddc_ddc_filter_response(float gain, int d, float *H)
{
    if (d < 0 || d >= SDDC_DDC_NDEC || !H) return fail(SDDC_ERR_ARG, "filter_response: bad d=%d or null", d);
    std::vector<std::complex<double>> h(SDDC_DDC_HALF_FFT);
    sddc::filter_response(gain, d, h.data());
    for (int i = 0; i < SDDC_DDC_HALF_FFT; i++) {
        H[2 * i] = (float)h[i].real();
        H[2 * i + 1] = (float)h[i].imag();
    }
    return SDDC_OK;
}

size_t sddc_ddc_output_samples(int d, int nblk)
{
    if (d < 0 || d >= SDDC_DDC_NDEC || nblk < 0) return 0;
    return (size_t)nblk * (size_t)(SDDC_DDC_OUT_BLOCK >> d);
}

int sddc_ddc_create(float gain, int device, sddc_ddc_t **out)
{
    if (!out) return fail(SDDC_ERR_ARG, "create: null out");
    *out = nullptr;
    if (device == SDDC_DDC_DEVICE_CPU) {
        if (!sddc::cpu::supported()) return fail(SDDC_ERR_NODEV, "create: the CPU backend needs AVX2 and FMA");
        auto *h = new (std::nothrow) sddc_ddc();
        if (!h) return fail(SDDC_ERR_NOMEM, "create: out of host memory");
        h->device = SDDC_DDC_DEVICE_CPU;
        h->gain = gain;
        try {
            std::vector<std::complex<double>> H((size_t)SDDC_DDC_NDEC * SDDC_DDC_HALF_FFT);
            for (int d = 0; d < SDDC_DDC_NDEC; d++) sddc::filter_response(gain, d, H.data() + (size_t)d * SDDC_DDC_HALF_FFT);
            h->cpu.reset(new sddc::cpu::R2iq(H.data()));
        } catch (const std::exception &ex) {
            delete h;
            return fail(SDDC_ERR_NOMEM, "create: %s", ex.what());
        }
        *out = h;
        return SDDC_OK;
    }
    if (device < 0) return fail(SDDC_ERR_ARG, "create: device %d (>= 0, or SDDC_DDC_DEVICE_CPU)", device);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SDDC_ERR_NODEV, "create: no HIP device visible");
    if (device < 0 || device >= ndev) return fail(SDDC_ERR_NODEV, "create: device %d of %d", device, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SDDC_ERR_NODEV, "create: device %d is %s, the kernels are built for gfx950", device,
                    prop.gcnArchName);

    DeviceGuard g(device);
    HIP_TRY(g.err);

    auto *h = new (std::nothrow) sddc_ddc();
    if (!h) return fail(SDDC_ERR_NOMEM, "create: out of host memory");
    h->device = device;
    h->gain = gain;
    if (const char *inj = std::getenv("SDDC_DDC_INJECT_FAIL")) h->inject_fail = std::atol(inj);
    if (const char *inj = std::getenv("SDDC_DDC_INJECT_FAIL_AFTER_D2H")) h->inject_late = std::atol(inj);

    // ---- constant tables (one device allocation) ----
    auto W = [](double num, double den) {   // e^{-2 pi i num/den}, double -> float once
        const double a = -2.0 * M_PI * num / den;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    std::vector<float2> host;
    auto put = [&](size_t n) { size_t o = host.size(); host.resize(o + n, make_float2(0.f, 0.f)); return o; };
    const size_t o_tw4096 = put(4096), o_post = put(8192), o_p1 = put(15 * 16), o_recf = put(2 * 256);
    for (int k = 0; k < 4096; k++) host[o_tw4096 + k] = W(k, 4096);
    for (int k = 0; k < 8192; k++) host[o_post + k] = W(k, 8192);
    for (int r = 1; r < 16; r++)
        for (int s = 0; s < 16; s++) host[o_p1 + (r - 1) * 16 + s] = W((double)s * r, 256);
    for (int j = 0; j < 256; j++) {
        host[o_recf + j] = W(j, 4096);
        host[o_recf + 256 + j] = W(4.0 * j, 4096);
    }
    size_t o_hsel[SDDC_DDC_NDEC], o_q1[SDDC_DDC_NDEC], o_reci[SDDC_DDC_NDEC];
    std::vector<std::complex<double>> H(SDDC_DDC_HALF_FFT);
    for (int d = 0; d < SDDC_DDC_NDEC; d++) {
        const int mfft = SDDC_DDC_HALF_FFT >> d;
        sddc::filter_response(gain, d, H.data());
        o_hsel[d] = put(mfft);
        for (int m = 0; m < mfft; m++) {
            // inverse-input position m: H[m] (m < mfft/2), H[4096 - mfft + m] otherwise
            // (impl.hpp:90,94 with filter2 = filter + halfFft - mfft/2, impl.hpp:7)
            const std::complex<double> v = H[m < mfft / 2 ? m : SDDC_DDC_HALF_FFT - mfft + m];
            host[o_hsel[d] + m] = make_float2((float)(0.5 * v.real()), (float)(0.5 * v.imag()));
        }
        // inverse pass-1 table W_{16S}^{s r}, S = mfft/256 (mfft >= 512) or mfft/16
        const int S = mfft >= 512 ? mfft / 256 : mfft / 16;
        o_q1[d] = put(15 * (size_t)S);
        for (int r = 1; r < 16; r++)
            for (int s = 0; s < S; s++) host[o_q1[d] + (r - 1) * S + s] = W((double)s * r, 16.0 * S);
        // inverse pass-2 recurrence bases W_N^j, W_N^{4j}, j < N/16 (mfft >= 512)
        o_reci[d] = put(2 * 256);
        if (mfft >= 512) {
            for (int j = 0; j < mfft / 16; j++) {
                host[o_reci[d] + j] = W(j, mfft);
                host[o_reci[d] + 256 + j] = W(4.0 * j, mfft);
            }
        }
    }
    const size_t ntab = host.size();
    hipError_t e = hipMalloc(&h->d_tables, ntab * sizeof(float2));
    if (e == hipSuccess) e = hipMemcpy(h->d_tables, host.data(), ntab * sizeof(float2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&h->d_pq, SDDC_DDC_HALF_FFT * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc(&h->d_fs, 4096 * sizeof(float4) + 768 * sizeof(float2));
    if (e == hipSuccess)
        e = hipMalloc(&h->d_queue, (size_t)sddc_ddc::kQueueSlots * sddc::kFsQueueWords * sizeof(unsigned));
    if (e == hipSuccess)   // zeroed on the handle's stream and waited for: the first launch may be on any stream
        e = hipMemsetAsync(h->d_queue, 0, (size_t)sddc_ddc::kQueueSlots * sddc::kFsQueueWords * sizeof(unsigned),
                           h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        sddc_ddc_destroy(h);
        return fail(SDDC_ERR_HIP, "create: %s", hipGetErrorString(e));
    }
    const float2 *T = h->d_tables;
    h->tables.tw4096 = T + o_tw4096;
    h->tables.post8192 = T + o_post;
    h->tables.tw_p1 = T + o_p1;
    h->tables.rec_f = T + o_recf;
    h->tables.lc = &h->launch_cache;
    for (int d = 0; d < SDDC_DDC_NDEC; d++) {
        h->tables.hsel[d] = T + o_hsel[d];
        h->tables.tw_q1[d] = T + o_q1[d];
        h->tables.rec_i[d] = T + o_reci[d];
    }
    *out = h;
    return SDDC_OK;
}

int sddc_ddc_backend(const sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    return h->cpu ? SDDC_DDC_BACKEND_CPU : SDDC_DDC_BACKEND_HIP;
}

int sddc_ddc_destroy(sddc_ddc_t *h)
{
    if (!h) return SDDC_OK;
    if (h->cpu) {
        delete h;
        return SDDC_OK;
    }
    {
        DeviceGuard g(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        // copies a failed call left in flight (host_pipeline returns on the first error) finish
        // before their buffers and registrations go
        if (h->s_in) (void)hipStreamSynchronize(h->s_in);
        if (h->s_out) (void)hipStreamSynchronize(h->s_out);
        // launches on the callers' streams may still read the tables below: wait for them first
        (void)h->readers.sync();
        (void)h->ch_readers.sync();
        (void)h->sp_readers.sync();
        (void)h->chsp_readers.sync();
        (void)h->chdec.readers.sync();
        (void)h->chres.readers.sync();
        (void)h->chars.readers.sync();
        (void)h->chdem.readers.sync();
        (void)h->chaud.readers.sync();
        (void)h->chagc.readers.sync();
        (void)h->chnb.readers.sync();
        (void)h->chsq.readers.sync();
        (void)h->chtone.readers.sync();
        (void)h->chdcs.readers.sync();
        (void)h->chst.readers.sync();
        if (h->d_tables) (void)hipFree(h->d_tables);
        for (auto &sl : h->hs) {
            if (sl.d_in) (void)hipFree(sl.d_in);
            if (sl.d_out) (void)hipFree(sl.d_out);
            if (sl.h_in) (void)hipHostFree(sl.h_in);
            if (sl.h_out) (void)hipHostFree(sl.h_out);
            for (hipEvent_t ev : {sl.e_h2d, sl.e_k, sl.e_d2h})
                if (ev) (void)hipEventDestroy(ev);
        }
        if (h->s_in) (void)hipStreamDestroy(h->s_in);
        if (h->s_out) (void)hipStreamDestroy(h->s_out);
        for (auto &r : h->regions) (void)hipHostUnregister(const_cast<char *>(r.first));
        if (h->d_tunebins) (void)hipFree(h->d_tunebins);
        if (h->d_windows) (void)hipFree(h->d_windows);
        if (h->d_chscratch) (void)hipFree(h->d_chscratch);
        if (h->d_chnco_trig) (void)hipFree(h->d_chnco_trig);
        if (h->d_chnco_state) (void)hipFree(h->d_chnco_state);
        if (h->d_chnco_fc) (void)hipFree(h->d_chnco_fc);
        if (h->d_chnco_starts) (void)hipFree(h->d_chnco_starts);
        if (h->d_pq) (void)hipFree(h->d_pq);
        if (h->d_fs) (void)hipFree(h->d_fs);
        if (h->d_queue) (void)hipFree(h->d_queue);
        if (h->d_sp_win) (void)hipFree(h->d_sp_win);
        if (h->d_sp_partial) (void)hipFree(h->d_sp_partial);
        if (h->d_sp_in) (void)hipFree(h->d_sp_in);
        if (h->d_sp_out) (void)hipFree(h->d_sp_out);
        h->sp_readers.clear();
        if (h->d_chsp_win) (void)hipFree(h->d_chsp_win);
        if (h->d_chsp_in) (void)hipFree(h->d_chsp_in);
        if (h->d_chsp_out) (void)hipFree(h->d_chsp_out);
        h->chsp_readers.clear();
        h->chdec.free_all();
        h->chres.free_all();
        h->chars.free_all();
        h->chdem.free_all();
        h->chaud.free_all();
        h->chagc.free_all();
        h->chnb.free_all();
        h->chsq.free_all();
        h->chtone.free_all();
        h->chdcs.free_all();
        h->chst.free_all();
        if (h->fsa.h_ring) (void)hipHostFree(h->fsa.h_ring);   // its writers were waited for above
        h->readers.clear();
        h->ch_readers.clear();
        for (int i = 0; i < sddc_ddc::kNcoSlots; i++) {
            if (h->h_nco[i]) (void)hipHostFree(h->h_nco[i]);
            if (h->nco_ev[i]) (void)hipEventDestroy(h->nco_ev[i]);
        }
        if (h->d_nco) (void)hipFree(h->d_nco);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return SDDC_OK;
}

int sddc_ddc_set_decimation(sddc_ddc_t *h, int d)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (d < 0 || d >= SDDC_DDC_NDEC) return fail(SDDC_ERR_ARG, "decimation index %d outside 0..6", d);
    std::lock_guard<std::mutex> lk(h->mu);
    h->d = d;
    return SDDC_OK;
}

int sddc_ddc_set_sideband(sddc_ddc_t *h, int lsb)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->lsb = lsb ? 1 : 0;
    return SDDC_OK;
}

int sddc_ddc_set_rand(sddc_ddc_t *h, int rand)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->rand = rand ? 1 : 0;
    return SDDC_OK;
}

int sddc_ddc_set_tunebin(sddc_ddc_t *h, int tunebin)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (tunebin < 0 || tunebin >= SDDC_DDC_HALF_FFT)
        return fail(SDDC_ERR_ARG, "tune bin %d outside [0,4096)", tunebin);
    std::lock_guard<std::mutex> lk(h->mu);
    h->tunebin = tunebin;
    return SDDC_OK;
}

int sddc_ddc_get_tunebin(const sddc_ddc_t *h)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->tunebin;
}

float sddc_ddc_set_freq_offset(sddc_ddc_t *h, float offset)
{
    if (!h) {
        fail(SDDC_ERR_ARG, "null handle");
        return 0.f;
    }
    float delta;
    const int tb = tuning_of(offset, &delta);
    std::lock_guard<std::mutex> lk(h->mu);
    const float ret = delta * (float)(1 << h->d);
    h->tunebin = tb;
    return ret;
}

int sddc_ddc_channel_tuning(float offset, int d, int *tunebin, float *relative_freq)
{
    if (!std::isfinite(offset)) return fail(SDDC_ERR_ARG, "channel_tuning: non-finite offset");
    if (d < 0 || d >= SDDC_DDC_NDEC) return fail(SDDC_ERR_ARG, "channel_tuning: decimation index %d outside 0..6", d);
    if (!tunebin || !relative_freq) return fail(SDDC_ERR_ARG, "channel_tuning: null result pointer");
    float delta;
    *tunebin = tuning_of(offset, &delta);
    *relative_freq = delta * (float)(1 << d);
    return SDDC_OK;
}

int sddc_ddc_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->last_slot = -1;   // the next host-path chunk starts from a zero history
    h->hist_override.clear();
    if (h->cpu) h->cpu->reset();
    return SDDC_OK;
}

int sddc_ddc_set_history(sddc_ddc_t *h, const int16_t *last4096)
{
    if (!h || !last4096) return fail(SDDC_ERR_ARG, "set_history: null handle or samples");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) {
        h->cpu->set_history(last4096);
        return SDDC_OK;
    }
    h->hist_override.assign(last4096, last4096 + kHistory);
    return SDDC_OK;
}

// Stage [T | lane starts of this launch's 128-sample blocks] for the fused NCO.
static hipError_t stage_nco(sddc_ddc_t *h, int nblk, hipStream_t s)
{
    using sddc::FineTune;
    const long nb = (long)nblk * (SDDC_DDC_BLOCK / 2 >> h->d) / FineTune::kBlock;
    const size_t n = FineTune::kTable + (size_t)nb * FineTune::kLanes;
    hipError_t e;
    if (n > h->h_nco_cap) {
        for (int i = 0; i < sddc_ddc::kNcoSlots; i++) {
            if (h->nco_ev[i] && (e = hipEventSynchronize(h->nco_ev[i])) != hipSuccess) return e;
            if (h->h_nco[i]) (void)hipHostFree(h->h_nco[i]);
            h->h_nco[i] = nullptr;
        }
        h->h_nco_cap = 0;
        for (int i = 0; i < sddc_ddc::kNcoSlots; i++) {
            if ((e = hipHostMalloc(&h->h_nco[i], n * sizeof(float2), hipHostMallocDefault)) != hipSuccess) return e;
            if (!h->nco_ev[i] && (e = hipEventCreateWithFlags(&h->nco_ev[i], hipEventDisableTiming)) != hipSuccess)
                return e;
        }
        h->h_nco_cap = n;
    }
    if (n > h->d_nco_cap) {   // the previous launches may still read the old buffer
        if ((e = h->readers.sync()) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (h->d_nco) (void)hipFree(h->d_nco);
        h->d_nco = nullptr;
        h->d_nco_cap = 0;
        if ((e = hipMalloc(&h->d_nco, n * sizeof(float2))) != hipSuccess) return e;
        h->d_nco_cap = n;
    } else if ((e = h->readers.order_before(s)) != hipSuccess) {   // launches on other streams may still read d_nco
        return e;
    }
    const int slot = h->nco_slot;
    h->nco_slot = (slot + 1) % sddc_ddc::kNcoSlots;
    if ((e = hipEventSynchronize(h->nco_ev[slot])) != hipSuccess) return e;   // its last copy is done
    float2 *buf = h->h_nco[slot];
    std::memcpy(buf, h->nco.table(), FineTune::kTable * sizeof(float2));
    h->nco.starts(nb, buf + FineTune::kTable);
    if ((e = hipMemcpyAsync(h->d_nco, buf, n * sizeof(float2), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    return hipEventRecord(h->nco_ev[slot], s);
}

// The next slot of the handle's dynamic-frame-queue ring for a launch on s (under h->mu, like
// every launch): ordered after the slot's previous launch, or zeroed first if that launch failed.
// *slot receives its index for queue_slot_launched.
static hipError_t next_queue_slot(sddc_ddc_t *h, hipStream_t s, unsigned **wq, int *slot)
{
    const int i = h->queue_slot;
    h->queue_slot = (i + 1) % sddc_ddc::kQueueSlots;
    *slot = i;
    *wq = h->d_queue + (size_t)i * sddc::kFsQueueWords;
    hipError_t e = hipSuccess;
    if (h->q_dirty[i]) {
        if (h->q_used[i]) e = h->readers.order_after(h->q_s[i], s);   // the failed launch may still run
        if (e == hipSuccess) e = hipMemsetAsync(*wq, 0, sddc::kFsQueueWords * sizeof(unsigned), s);
        if (e == hipSuccess) h->q_dirty[i] = false;
    } else if (h->q_used[i]) {
        e = h->readers.order_after(h->q_s[i], s);
    }
    return e;
}

// after the launch that took slot i: on success the slot's last user is s (the launch is recorded
// in readers right after); on failure the slot is zeroed before its next use, on a stream ordered
// after an event recorded on s here: hipGetLastError may report a sticky or earlier error for a
// kernel that was enqueued and still runs (readers.record of the success path is skipped then)
static void queue_slot_launched(sddc_ddc_t *h, int i, hipStream_t s, hipError_t e)
{
    h->q_s[i] = s;
    h->q_used[i] = true;
    if (e != hipSuccess) {
        h->q_dirty[i] = true;
        (void)h->readers.record(s);
    }
}

// a HIP error on a launch path: the state of every in-flight launch is unknown, so every queue
// slot is zeroed (stream-ordered) before its next use
static void queue_mark_all_dirty(sddc_ddc_t *h)
{
    for (int i = 0; i < sddc_ddc::kQueueSlots; i++) h->q_dirty[i] = true;
}

// a launch on s reads a table set last rebuilt on `built`: wait for that rebuild
static hipError_t order_after_build(sddc_ddc_t *h, hipStream_t built, hipStream_t s)
{
    return h->readers.order_after(built, s);
}

// The adaptive split's hook of a d = 0 launch (ddc_kernels.h FsSched::adapt), under h->mu.
static bool fs_adapt_prepare(void *ctx, int G, int ns, const sddc::FsShares **tab, unsigned **tlog, unsigned *tag)
{
    using sddc::kFsShareMaxG;
    sddc_ddc_t *h = static_cast<sddc_ddc_t *>(ctx);
    sddc_ddc::FsAdapt &a = h->fsa;
    const bool want_forced = (int)a.forced.size() == G;
    if (!a.on && !want_forced) return false;
    if (a.ctl.groups() != G) a.ctl.reset(G, sddc::kFsSlotWeights);
    if (want_forced && !a.ctl.forced()) a.ctl.load(a.forced.data(), G);
    if (!want_forced && a.ctl.forced()) a.ctl.unload();
    a.ctl.set_frames(ns);
    const bool learn = a.on && !a.ctl.forced();
    bool changed = false;
    if (learn && a.h_ring) {
        // pick up what has completed, oldest first
        const bool take = a.ctl.measured() < sddc_ddc::FsAdapt::kEager || a.launches % sddc_ddc::FsAdapt::kEvery == 0;
        for (int k = 0; k < sddc_ddc::FsAdapt::kRing && take; k++) {
            auto &p = a.pend[(a.next + k) % sddc_ddc::FsAdapt::kRing];
            if (!p.live) continue;
            const volatile unsigned *e = a.h_ring + (size_t)((a.next + k) % sddc_ddc::FsAdapt::kRing) * kFsShareMaxG * 4;
            bool done = true;
            for (int w = 0; w < p.G && done; w++)
                done = e[4 * w + 2] == p.tag && (e[4 * w] ^ e[4 * w + 1] ^ p.tag) == e[4 * w + 3];
            if (!done) continue;
            p.live = false;
            if (p.tainted || p.G != G || p.ns != ns) {
                a.skipped++;
                continue;
            }
            uint32_t st[kFsShareMaxG], en[kFsShareMaxG];
            for (int w = 0; w < G; w++) {
                st[w] = e[4 * w];
                en[w] = e[4 * w + 1];
            }
            // read while the next launch of the slot cannot have started (it is enqueued below at
            // the earliest); a torn copy would fail nothing worse than the controller's bounds
            if (a.ctl.update(p.n.data(), st, en)) changed = true;
            else a.skipped++;
        }
    }
    a.launches++;
    const std::vector<int> *n = nullptr;
    if (a.ctl.warm()) {
        if (changed || a.tab_ns != ns) {
            a.tab_n.resize((size_t)G);
            a.ctl.table(ns, &a.tab, a.tab_n.data());
            a.tab_ns = ns;
        }
        *tab = &a.tab;
        n = &a.tab_n;
        a.last_table = 1;
    } else {
        if (a.base_ns != ns || (int)a.base_n.size() != G) {
            a.base_n.resize((size_t)G);
            for (int w = 0; w < G; w++)
                a.base_n[(size_t)w] = sddc::fs_slot_split_host(ns, G, w + 1, sddc::kFsSlotWeights) -
                                      sddc::fs_slot_split_host(ns, G, w, sddc::kFsSlotWeights);
            a.base_ns = ns;
        }
        *tab = nullptr;
        n = &a.base_n;
    }
    *tlog = nullptr;
    *tag = 0u;
    if (!learn) return true;
    if (!a.h_ring && !a.ring_failed) {
        const size_t bytes = (size_t)sddc_ddc::FsAdapt::kRing * kFsShareMaxG * 4 * sizeof(unsigned);
        void *hp = nullptr, *dp = nullptr;
        if (hipHostMalloc(&hp, bytes, hipHostMallocMapped) == hipSuccess) {
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
                std::memset(hp, 0, bytes);
                a.h_ring = static_cast<unsigned *>(hp);
                a.d_ring = static_cast<unsigned *>(dp);
            } else {
                (void)hipHostFree(hp);
            }
        }
        if (!a.h_ring) {
            a.ring_failed = true;   // no measurements: the launches keep the built-in split
            (void)hipGetLastError();
        }
    }
    if (!a.h_ring) return true;
    const int i = a.next;
    a.next = (i + 1) % sddc_ddc::FsAdapt::kRing;
    if (++a.seq == 0u) a.seq = 1u;
    auto &p = a.pend[i];
    p.tag = a.seq;
    p.G = G;
    p.ns = ns;
    p.live = true;
    p.tainted = a.taint_left > 0;
    p.n = *n;
    a.last_pending = i;
    a.last_logged = 1;
    *tlog = a.d_ring + (size_t)i * kFsShareMaxG * 4;
    *tag = p.tag;
    return true;
}

static hipError_t launch_single_impl(sddc_ddc_t *h, const int16_t *d_in, int nblk, void *d_out, hipStream_t s);

static hipError_t launch_single(sddc_ddc_t *h, const int16_t *d_in, int nblk, void *d_out, hipStream_t s)
{
    const hipError_t e = launch_single_impl(h, d_in, nblk, d_out, s);
    if (e != hipSuccess) queue_mark_all_dirty(h);
    return e;
}

static hipError_t launch_single_impl(sddc_ddc_t *h, const int16_t *d_in, int nblk, void *d_out, hipStream_t s)
{
    {
        // a launch on another stream than the handle's last one may overlap it (and what follows)
        sddc_ddc::FsAdapt &a = h->fsa;
        if (a.have_last && a.last_s != s) {
            a.taint_left = sddc_ddc::FsAdapt::kTaint + 1;
            if (a.last_pending >= 0) a.pend[a.last_pending].tainted = true;
        } else if (a.taint_left > 0) {
            a.taint_left--;
        }
        a.last_s = s;
        a.have_last = true;
        a.last_pending = -1;
        a.last_table = a.last_logged = 0;
    }
    const bool nco = h->nco_fc != 0.f;
    if (nco) {
        hipError_t e = stage_nco(h, nblk, s);
        if (e != hipSuccess) return e;
    }
    const float2 *nco_starts = nco ? h->d_nco + sddc::FineTune::kTable : nullptr, *nco_trig = nco ? h->d_nco : nullptr;
    if (sddc::fs_path(h->d, h->tunebin)) {
        // d = 0 fused-split kernel: its (P, Q) by bin and output-modulation lane factors
        float4 *pqf = h->d_fs;
        float2 *fsl = reinterpret_cast<float2 *>(h->d_fs + 4096);
        if (h->fs_tb != h->tunebin) {
            hipError_t e = h->readers.order_before(s);   // launches on other streams may still read them
            if (e != hipSuccess) return e;
            h->fs_tb = -1;   // a failed rebuild leaves the tables unknown
            e = sddc::launch_build_fs_tables(h->tables, h->tunebin, pqf, fsl, s);
            if (e == hipSuccess) e = h->readers.record(s);
            if (e != hipSuccess) return e;
            h->fs_tb = h->tunebin;
            h->fs_s = s;
        } else if (hipError_t e = order_after_build(h, h->fs_s, s); e != hipSuccess) {
            return e;
        }
        // the default static schedule uses no queue slot; the queue and stealing schedules (A/B)
        // take one of the ring's slots per launch
        unsigned *wq = nullptr;
        int qi = -1;
        hipError_t e = hipSuccess;
        if (h->fs_sched.sched != 0 && (e = next_queue_slot(h, s, &wq, &qi)) != hipSuccess) return e;
        h->fs_sched.adapt = fs_adapt_prepare;
        h->fs_sched.adapt_ctx = h;
        e = sddc::launch_frames_fs(h->tables, d_in, nblk, d_out, pqf, fsl, h->tunebin, h->lsb, h->rand,
                                   h->out_fmt == SDDC_DDC_FMT_CS16, h->cs16_scale, nco_starts, nco_trig, wq,
                                   h->fs_sched, h->device, s);
        if (qi >= 0) queue_slot_launched(h, qi, s, e);
        if (e != hipSuccess) return e;
        return h->readers.record(s);
    }
    if (h->pq_d != h->d || h->pq_tb != h->tunebin) {
        hipError_t e = h->readers.order_before(s);   // launches on other streams may still read d_pq
        if (e != hipSuccess) return e;
        h->pq_d = h->pq_tb = -1;
        e = sddc::launch_build_split_filter(h->tables, h->d, h->tunebin, h->d_pq, s);
        if (e == hipSuccess) e = h->readers.record(s);
        if (e != hipSuccess) return e;
        h->pq_d = h->d;
        h->pq_tb = h->tunebin;
        h->pq_s = s;
    } else if (hipError_t e = order_after_build(h, h->pq_s, s); e != hipSuccess) {
        return e;
    }
    hipError_t e = sddc::launch_frames_persistent(h->tables, h->d, d_in, nblk, d_out, h->d_pq, h->tunebin, h->lsb, h->rand,
                                         h->out_fmt == SDDC_DDC_FMT_CS16, h->cs16_scale, nco_starts, nco_trig,
                                         h->slot_weights, h->device, s);
    if (e != hipSuccess) return e;
    return h->readers.record(s);
}

int sddc_ddc_set_output_format(sddc_ddc_t *h, int format, float cs16_scale)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (format != SDDC_DDC_FMT_CF32 && format != SDDC_DDC_FMT_CS16)
        return fail(SDDC_ERR_ARG, "unknown output format %d", format);
    if (format == SDDC_DDC_FMT_CS16 && !(std::isfinite(cs16_scale) && cs16_scale > 0.f))
        return fail(SDDC_ERR_ARG, "CS16 scale must be finite and > 0");
    std::lock_guard<std::mutex> lk(h->mu);
    h->out_fmt = format;
    h->cs16_scale = format == SDDC_DDC_FMT_CS16 ? cs16_scale : 1.f;
    return SDDC_OK;
}

int sddc_ddc_set_fine_tune(sddc_ddc_t *h, float relative_freq)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (!std::isfinite(relative_freq)) return fail(SDDC_ERR_ARG, "fine tune: non-finite frequency");
    std::lock_guard<std::mutex> lk(h->mu);
    if (relative_freq != h->nco_fc) {   // RadioHandler.cpp:291-296: re-init only on change
        h->nco_fc = relative_freq;
        if (relative_freq != 0.f) h->nco.init(relative_freq, 0.0f);
    }
    return SDDC_OK;
}

int sddc_ddc_set_channel_fine_tune(sddc_ddc_t *h, const float *relative_freqs, int nch)
{
    using sddc::FineTune;
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (nch < 0 || nch > SDDC_DDC_MAX_CHANNELS)
        return fail(SDDC_ERR_ARG, "channel fine tune: channel count %d outside 0..%d", nch, SDDC_DDC_MAX_CHANNELS);
    if (!relative_freqs) nch = 0;
    for (int c = 0; c < nch; c++)
        if (!std::isfinite(relative_freqs[c]))
            return fail(SDDC_ERR_ARG, "channel fine tune: non-finite frequency of channel %d", c);
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel fine tune: a CPU handle has no many-channel path");
    if (nch == 0) {   // off; the next array, of any length, starts every channel at phase 0
        h->chnco_fc.clear();
        return SDDC_OK;
    }
    // RadioHandler.cpp:291-296 per channel index: re-init only on change; another nch restarts all
    const bool all = h->chnco_fc.size() != (size_t)nch;
    std::vector<char> changed((size_t)nch);
    bool any = false;
    for (int c = 0; c < nch; c++) any |= (changed[c] = all || relative_freqs[c] != h->chnco_fc[c]) != 0;
    if (!any) return SDDC_OK;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // earlier launches, on any stream, may still read the tables and advance the state
    HIP_TRY(h->ch_readers.sync());
    if (!h->d_chnco_trig) HIP_TRY(hipMalloc(&h->d_chnco_trig, SDDC_DDC_MAX_CHANNELS * FineTune::kTable * sizeof(float2)));
    if (!h->d_chnco_state) HIP_TRY(hipMalloc(&h->d_chnco_state, SDDC_DDC_MAX_CHANNELS * FineTune::kLanes * sizeof(float2)));
    if (!h->d_chnco_fc) HIP_TRY(hipMalloc(&h->d_chnco_fc, SDDC_DDC_MAX_CHANNELS * sizeof(float)));
    h->chnco_fc.clear();   // a failed upload leaves the NCO off
    std::vector<float2> trig((size_t)nch * FineTune::kTable), state((size_t)nch * FineTune::kLanes);
    for (int c = 0; c < nch; c++) {
        if (!changed[c]) continue;
        FineTune ft;
        ft.init(relative_freqs[c], 0.0f);
        std::memcpy(&trig[(size_t)c * FineTune::kTable], ft.table(), FineTune::kTable * sizeof(float2));
        ft.starts(1, &state[(size_t)c * FineTune::kLanes]);   // block 0's lane starts = the initial state
    }
    // synchronous copies of each run [c0, c1) of changed channels (unchanged ones keep their phase)
    for (int c0 = 0; c0 < nch;) {
        if (!changed[c0]) {
            c0++;
            continue;
        }
        int c1 = c0 + 1;
        while (c1 < nch && changed[c1]) c1++;
        const size_t n = (size_t)(c1 - c0);
        HIP_TRY(hipMemcpy(h->d_chnco_trig + (size_t)c0 * FineTune::kTable, &trig[(size_t)c0 * FineTune::kTable],
                          n * FineTune::kTable * sizeof(float2), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_chnco_state + (size_t)c0 * FineTune::kLanes, &state[(size_t)c0 * FineTune::kLanes],
                          n * FineTune::kLanes * sizeof(float2), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_chnco_fc + c0, relative_freqs + c0, n * sizeof(float), hipMemcpyHostToDevice));
        c0 = c1;
    }
    h->chnco_fc.assign(relative_freqs, relative_freqs + nch);
    return SDDC_OK;
}

/* internal (sddc_ddc_internal.h): a tuning parameter of the kernels, for A/B timing */
int sddc_ddc_internal_set_param(sddc_ddc_t *h, int param, int value)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    switch (param) {
    case SDDC_DDC_PARAM_SLOT_WEIGHTS:
        h->slot_weights = value != 0;
        return SDDC_OK;
    case SDDC_DDC_PARAM_FS_STATIC_PCT:
        if (value < 0 || value > 100) return fail(SDDC_ERR_ARG, "static share %d outside 0..100", value);
        h->fs_sched.static_pct = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_FS_FRAMES_PER_WG:
        if (value < 0 || value > 1024) return fail(SDDC_ERR_ARG, "frames per workgroup %d outside 0..1024", value);
        h->fs_sched.fpw = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_FS_SCHEDULE:
        if (value < 0 || value > 2) return fail(SDDC_ERR_ARG, "FS schedule %d outside 0..2", value);
        h->fs_sched.sched = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_FS_STEAL_MINREM:
        if (value < 0 || value > 64) return fail(SDDC_ERR_ARG, "steal threshold %d outside 0..64", value);
        h->fs_sched.minrem = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_FS_ZERO_ROWS:
        h->fs_sched.zr = value != 0;
        return SDDC_OK;
    case SDDC_DDC_PARAM_LAZY_RECORD:
        h->readers.lazy = value != 0;
        return SDDC_OK;
    case SDDC_DDC_PARAM_FS_SLOT_WEIGHTS: {
        for (int k = 0; k < 4 && value != 0; k++) {
            const int wk = (value >> (8 * k)) & 0xff;
            if (wk < 1 || wk > 127) return fail(SDDC_ERR_ARG, "slot weight %d of slot %d outside 1..127", wk, k);
        }
        h->fs_sched.slotw = (unsigned)value;
        return SDDC_OK;
    }
    case SDDC_DDC_PARAM_FS_STEAL_PUBLIC:
        if (value < 0 || value > 1024) return fail(SDDC_ERR_ARG, "public frames %d outside 0..1024", value);
        h->fs_sched.pub = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_FS_ADAPTIVE_SPLIT:
        h->fsa.on = value != 0;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CH_NCO_RUN_BLOCKS:
        if (value < 0 || value > SDDC_DDC_MAX_BLOCKS)
            return fail(SDDC_ERR_ARG, "run blocks %d outside 0..%d", value, SDDC_DDC_MAX_BLOCKS);
        h->chnco_run_blocks = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_SPECTRUM_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "spectrum workgroup cap %d is negative", value);
        h->sp_max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHSPEC_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel spectrum workgroup cap %d is negative", value);
        h->chsp_max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHDEC_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel decimator workgroup cap %d is negative", value);
        h->chdec.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHRES_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel resampler workgroup cap %d is negative", value);
        h->chres.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHDEM_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel demodulator workgroup cap %d is negative", value);
        h->chdem.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHAUD_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel audio filter workgroup cap %d is negative", value);
        h->chaud.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHAUD_RUN_BLOCKS:
        if (value < 0 || value > (1 << 20))
            return fail(SDDC_ERR_ARG, "channel audio filter run length %d outside 0..2^20 blocks", value);
        h->chaud.run_blocks = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHAGC_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel AGC workgroup cap %d is negative", value);
        h->chagc.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHAGC_RUN_BLOCKS:
        if (value < 0 || value > (1 << 20))
            return fail(SDDC_ERR_ARG, "channel AGC run length %d outside 0..2^20 blocks", value);
        h->chagc.run_blocks = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHNB_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel blanker workgroup cap %d is negative", value);
        h->chnb.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHNB_RUN_BLOCKS:
        if (value < 0 || value > (1 << 20))
            return fail(SDDC_ERR_ARG, "channel blanker run length %d outside 0..2^20 blocks", value);
        h->chnb.run_blocks = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHSQ_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel squelch workgroup cap %d is negative", value);
        h->chsq.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHSQ_RUN_BLOCKS:
        if (value < 0 || value > (1 << 20))
            return fail(SDDC_ERR_ARG, "channel squelch run length %d outside 0..2^20 blocks", value);
        h->chsq.run_blocks = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHTONE_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel tone detector workgroup cap %d is negative", value);
        h->chtone.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHTONE_RUN_BLOCKS:
        if (value < 0 || value > (1 << 20))
            return fail(SDDC_ERR_ARG, "channel tone detector run length %d outside 0..2^20 blocks", value);
        h->chtone.run_blocks = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHDCS_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel DCS decoder workgroup cap %d is negative", value);
        h->chdcs.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHDCS_RUN_BLOCKS:
        if (value < 0 || value > (1 << 20))
            return fail(SDDC_ERR_ARG, "channel DCS decoder run length %d outside 0..2^20 blocks", value);
        h->chdcs.run_blocks = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHDCS_BALLOT:
        if (value != 0 && value != 1) return fail(SDDC_ERR_ARG, "channel DCS decoder ballot route %d is not 0 or 1", value);
        h->chdcs.ballot = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHARS_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel audio resampler workgroup cap %d is negative", value);
        h->chars.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHST_MAX_WGS:
        if (value < 0) return fail(SDDC_ERR_ARG, "channel stereo decoder workgroup cap %d is negative", value);
        h->chst.max_wgs = value;
        return SDDC_OK;
    case SDDC_DDC_PARAM_CHST_RUN_BLOCKS:
        if (value < 0 || value > (1 << 20))
            return fail(SDDC_ERR_ARG, "channel stereo decoder run length %d outside 0..2^20 blocks", value);
        h->chst.run_blocks = value;
        return SDDC_OK;
    default:
        return fail(SDDC_ERR_ARG, "unknown parameter %d", param);
    }
}

/* internal: a given table of relative shares for the d = 0 kernel's full-residency launches
 * (n = the grid, 4 x CUs), used as it is until n = 0 clears it; no measurements are taken meanwhile */
int sddc_ddc_internal_fs_set_shares(sddc_ddc_t *h, const float *shares, int n)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (n < 0 || n > sddc::kFsShareMaxG || (n > 0 && !shares)) return fail(SDDC_ERR_ARG, "shares: n %d outside 0..%d", n, sddc::kFsShareMaxG);
    double sum = 0.0;
    for (int w = 0; w < n; w++) {
        if (!(shares[w] >= 0.f) || !std::isfinite(shares[w])) return fail(SDDC_ERR_ARG, "share %d is negative or not finite", w);
        sum += shares[w];
    }
    if (n > 0 && !(sum > 0.0)) return fail(SDDC_ERR_ARG, "shares: all zero");
    std::lock_guard<std::mutex> lk(h->mu);
    h->fsa.forced.assign(shares, shares + n);
    if (h->fsa.ctl.forced()) h->fsa.ctl.unload();
    h->fsa.tab_ns = -1;
    return SDDC_OK;
}

/* internal: the adaptive split's state: info = {grid of the controller, measurements used,
 * measurements skipped, the last d = 0 launch took a share table, the last d = 0 launch was
 * measured}; counts (ncounts >= grid, or null) receives the current table's frames per workgroup
 * when it has one.  Returns the number of counts written. */
int sddc_ddc_internal_fs_split_state(sddc_ddc_t *h, long *info, int *counts, int ncounts)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    const sddc_ddc::FsAdapt &a = h->fsa;
    if (info) {
        info[0] = a.ctl.groups();
        info[1] = a.ctl.measured();
        info[2] = a.skipped;
        info[3] = a.last_table;
        info[4] = a.last_logged;
    }
    int nw = 0;
    if (counts && a.tab_ns >= 0 && ncounts >= (int)a.tab_n.size()) {
        nw = (int)a.tab_n.size();
        std::copy(a.tab_n.begin(), a.tab_n.end(), counts);
    }
    return nw;
}

/* internal: the controller alone, without a handle or a device (tests/test_adaptive_split.py) */
void *sddc_fs_split_create(int G, unsigned slot_weights)
{
    if (G < 1 || G > sddc::kFsShareMaxG) return nullptr;
    auto *c = new (std::nothrow) sddc::FsSplitController;
    if (c) c->reset(G, slot_weights);
    return c;
}
void sddc_fs_split_destroy(void *c) { delete static_cast<sddc::FsSplitController *>(c); }
int sddc_fs_split_load(void *c, const float *shares, int n)
{
    auto *k = static_cast<sddc::FsSplitController *>(c);
    if (n == 0) {
        k->unload();
        return 0;
    }
    return k->load(shares, n) ? 0 : -1;
}
/* the table of a launch of ns frames: p (G + 1 entries: the 15-bit shares, then 32768) and the
 * first frame of every workgroup as the kernel computes it (first: G + 1 entries, the last ns) */
int sddc_fs_split_table(void *c, int ns, unsigned *p, int *first)
{
    auto *k = static_cast<sddc::FsSplitController *>(c);
    const int G = k->groups();
    if (ns < 0) return -1;
    sddc::FsShares t;
    std::vector<int> n((size_t)G);
    k->table(ns, &t, n.data());
    if (!sddc::fs_shares_valid(t, G)) return -2;
    for (int w = 0; w <= G; w++) {
        if (p) p[w] = w < G ? sddc::fs_share_get(t, w) : sddc::kFsShareOne;
        if (first) first[w] = sddc::fs_share_start(ns, G, w, t);
    }
    return 0;
}
int sddc_fs_split_update(void *c, const int *n, const unsigned *start, const unsigned *end)
{
    return static_cast<sddc::FsSplitController *>(c)->update(n, start, end) ? 1 : 0;
}
int sddc_fs_split_model(void *c, double *cost, double *offset)
{
    auto *k = static_cast<sddc::FsSplitController *>(c);
    for (int w = 0; w < k->groups(); w++) {
        if (cost) cost[w] = k->cost()[(size_t)w];
        if (offset) offset[w] = k->offset()[(size_t)w];
    }
    return k->groups();
}

static int check_process_args(sddc_ddc_t *h, const int16_t *in, int nblk, const void *out)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (nblk <= 0 || nblk > SDDC_DDC_MAX_BLOCKS)
        return fail(SDDC_ERR_ARG, "nblk must be in 1..%d (got %d)", SDDC_DDC_MAX_BLOCKS, nblk);
    if (!in || !out) return fail(SDDC_ERR_ARG, "null buffer");
    if (((uintptr_t)in & 3) != 0) return fail(SDDC_ERR_ARG, "input must be 4-byte aligned");
    const unsigned oal = h->out_fmt == SDDC_DDC_FMT_CS16 ? 4 : 8;
    if (((uintptr_t)out & (oal - 1)) != 0) return fail(SDDC_ERR_ARG, "output must be %u-byte aligned", oal);
    return SDDC_OK;
}

int sddc_ddc_process_device(sddc_ddc_t *h, const int16_t *d_in, int nblk, void *d_out, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // the call reads d, format, tune bin: one consistent set
    if (h->cpu) return fail(SDDC_ERR_STATE, "process_device: a CPU handle has no device path");
    int rc = check_process_args(h, d_in, nblk, d_out);
    if (rc) return rc;
    if (injected_failure(h)) return fail(SDDC_ERR_HIP, "injected failure (SDDC_DDC_INJECT_FAIL)");
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    HIP_TRY(launch_single(h, d_in, nblk, d_out, (hipStream_t)hip_stream));
    return SDDC_OK;
}

int sddc_ddc_process_channels_device(sddc_ddc_t *h, const int16_t *d_in, int nblk, const int *tunebins,
                                     int nch, void *d_out, size_t out_stride, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // d, format and NCO state are read below
    if (h->cpu) return fail(SDDC_ERR_STATE, "process_channels_device: a CPU handle has no device path");
    int rc = check_process_args(h, d_in, nblk, d_out);
    if (rc) return rc;
    if (!tunebins || nch <= 0 || nch > SDDC_DDC_MAX_CHANNELS)
        return fail(SDDC_ERR_ARG, "channel count %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
    for (int c = 0; c < nch; c++)
        if (tunebins[c] < 0 || tunebins[c] >= SDDC_DDC_HALF_FFT)
            return fail(SDDC_ERR_ARG, "channel %d tune bin %d outside [0,4096)", c, tunebins[c]);
    if (h->nco_fc != 0.f)
        return fail(SDDC_ERR_STATE, "set_fine_tune's NCO is single-channel; set it to 0 first "
                                    "(channels: sddc_ddc_set_channel_fine_tune)");
    const bool nco = !h->chnco_fc.empty();
    if (nco && h->chnco_fc.size() != (size_t)nch)
        return fail(SDDC_ERR_STATE, "per-channel fine tune is set for %zu channels, the call has %d",
                    h->chnco_fc.size(), nch);
    const size_t need = (size_t)nblk * (size_t)(SDDC_DDC_OUT_BLOCK >> h->d) * 2;
    if (nch > 1 && out_stride < need)
        return fail(SDDC_ERR_ARG, "out_stride %zu < %zu components per channel", out_stride, need);
    if (nch > 1 && (out_stride & 1))   // channels start on whole complex samples
        return fail(SDDC_ERR_ARG, "out_stride %zu must be even (components, 2 per complex sample)", out_stride);
    const int cs16 = h->out_fmt == SDDC_DDC_FMT_CS16;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    hipStream_t s = (hipStream_t)hip_stream;
    const bool v2 = h->d >= 4;
    const bool changed = h->tunebins_cached.size() != (size_t)nch ||
                         !std::equal(h->tunebins_cached.begin(), h->tunebins_cached.end(), tunebins);
    if (changed || (v2 && h->windows_d != h->d && h->windows_d != -2 - 8 * h->d)) {
        // earlier launches, on any stream, may still read the device copies
        HIP_TRY(h->ch_readers.sync());
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (changed) {
        if (!h->d_tunebins) HIP_TRY(hipMalloc(&h->d_tunebins, SDDC_DDC_MAX_CHANNELS * sizeof(int)));
        h->tunebins_cached.assign(tunebins, tunebins + nch);
        h->windows_d = -1;
        // synchronous: the host array may go away after we return
        HIP_TRY(hipMemcpy(h->d_tunebins, tunebins, nch * sizeof(int), hipMemcpyHostToDevice));
    }
    const int2 *windows = nullptr;
    if (v2) {
        if (h->windows_d != h->d && h->windows_d != -2 - 8 * h->d) {
            std::vector<int2> w((SDDC_DDC_MAX_CHANNELS + 127) / 128);
            if (sddc::channel_windows(h->d, tunebins, nch, w.data())) {
                if (!h->d_windows) HIP_TRY(hipMalloc(&h->d_windows, w.size() * sizeof(int2)));
                HIP_TRY(hipMemcpy(h->d_windows, w.data(), w.size() * sizeof(int2), hipMemcpyHostToDevice));
                h->windows_d = h->d;
            } else {
                h->windows_d = -2 - 8 * h->d;   // spread-out tune bins: the full-spectrum form
            }
        }
        if (h->windows_d == h->d) windows = h->d_windows;
    }
    if (((v2 && windows && nch > 128) || !v2) && !h->d_chscratch) {
        // one 4096-bin row per resident workgroup (<= 4 per CU), 32 KB each
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        HIP_TRY(hipMalloc(&h->d_chscratch, (size_t)cus * 4 * SDDC_DDC_HALF_FFT * sizeof(float2)));
        h->chscratch_rows = cus * 4;
    }
    // the scratch rows are per handle: a launch must not overlap one on another stream
    // (so are the per-channel NCO's state and tables)
    if (h->d_chscratch || nco) HIP_TRY(h->ch_readers.order_before(s));
    auto launch = [&](const int16_t *in, int n, void *out, const sddc::ChNco *cn) {
        if (v2)
            return sddc::launch_channels_v2(h->tables, h->d, in, n, h->d_tunebins, nch, out, out_stride, h->lsb,
                                            h->rand, cs16, h->cs16_scale, windows, h->d_chscratch,
                                            h->chscratch_rows, h->device, s, cn);
        return sddc::launch_channels_p(h->tables, h->d, in, n, h->d_tunebins, nch, out, out_stride, h->lsb, h->rand,
                                       cs16, h->cs16_scale, h->d_chscratch, h->chscratch_rows, h->device, s, cn);
    };
    if (!nco) {
        HIP_TRY(launch(d_in, nblk, d_out, nullptr));
        HIP_TRY(h->ch_readers.record(s));
        return SDDC_OK;
    }
    // Per-channel NCO: runs of whole blocks, each a chain launch (the run's lane starts, the state
    // advanced on the device) and a channels launch over the run's blocks with their 4096-sample
    // halo.  The channels kernels are stateless per (frame, chunk), so the cut changes no bit.
    const size_t blk_bytes = (size_t)nch * (size_t)(kChNcoBlockBytes >> h->d);   // table bytes per input block
    int run = (int)std::min<size_t>((size_t)nblk, std::max<size_t>(1, kChNcoTableCap / blk_bytes));
    if (h->chnco_run_blocks > 0) run = std::min(run, h->chnco_run_blocks);
    if ((size_t)run * blk_bytes > h->chnco_starts_cap) {   // earlier launches may still read the old table
        HIP_TRY(h->ch_readers.sync());
        HIP_TRY(hipStreamSynchronize(s));
        if (h->d_chnco_starts) (void)hipFree(h->d_chnco_starts);
        h->d_chnco_starts = nullptr;
        h->chnco_starts_cap = 0;
        HIP_TRY(hipMalloc(&h->d_chnco_starts, (size_t)run * blk_bytes));
        h->chnco_starts_cap = (size_t)run * blk_bytes;
    }
    const int per_blk = SDDC_DDC_OUT_BLOCK >> h->d;                      // complex samples per block
    const int nb_blk = per_blk / sddc::FineTune::kBlock;                 // 128-sample blocks per block
    const size_t out_blk = (size_t)per_blk * (cs16 ? 4 : 8);             // bytes per channel and block
    for (int b0 = 0; b0 < nblk; b0 += run) {
        const int n = std::min(run, nblk - b0);
        const sddc::ChNco cn{h->d_chnco_starts, h->d_chnco_trig, h->d_chnco_fc, n * nb_blk};
        hipError_t e = sddc::launch_channel_nco_chain(h->d_chnco_state, h->d_chnco_trig, h->d_chnco_starts, nch,
                                                      cn.nb, s);
        if (e == hipSuccess) e = launch(d_in + (size_t)b0 * kBlock, n, static_cast<char *>(d_out) + (size_t)b0 * out_blk, &cn);
        // the launches so far stay ordered against other streams and the next fc change
        const hipError_t er = h->ch_readers.record(s);
        HIP_TRY(e);
        HIP_TRY(er);
    }
    return SDDC_OK;
}

/* ---- wideband averaged power spectrum --------------------------------------------------- */
// periodic (DFT-even) cosine-sum windows over n points, evaluated in double and rounded once
static int cosine_window(const char *who, int kind, int n, float *w)
{
    if (!w) return fail(SDDC_ERR_ARG, "%s: null array", who);
    static const double kRect[] = {1.0}, kHann[] = {0.5, 0.5}, kBh[] = {0.35875, 0.48829, 0.14128, 0.01168};
    const double *a;
    int na;
    switch (kind) {
    case SDDC_DDC_WINDOW_RECT: a = kRect, na = 1; break;
    case SDDC_DDC_WINDOW_HANN: a = kHann, na = 2; break;
    case SDDC_DDC_WINDOW_BLACKMAN_HARRIS: a = kBh, na = 4; break;
    default: return fail(SDDC_ERR_ARG, "%s: unknown window %d", who, kind);
    }
    for (int j = 0; j < n; j++) {
        double v = 0.0;
        for (int m = 0; m < na; m++) v += ((m & 1) ? -a[m] : a[m]) * std::cos(2.0 * M_PI * m * j / n);
        w[j] = (float)v;
    }
    return SDDC_OK;
}

int sddc_ddc_spectrum_window(int kind, float *w) { return cosine_window("spectrum_window", kind, SDDC_DDC_FFTN, w); }

int sddc_ddc_window(int kind, int n, float *w)
{
    if (n < 32 || n > 8192 || (n & (n - 1)) != 0)
        return fail(SDDC_ERR_ARG, "window: n must be a power of two in 32..8192 (got %d)", n);
    return cosine_window("window", kind, n, w);
}

int sddc_ddc_set_spectrum_window(sddc_ddc_t *h, const float *w)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    double sum = (double)SDDC_DDC_FFTN;
    if (w) {
        sum = 0.0;
        for (int j = 0; j < SDDC_DDC_FFTN; j++) {
            if (!std::isfinite(w[j])) return fail(SDDC_ERR_ARG, "spectrum window: value %d is not finite", j);
            sum += w[j];
        }
        if (!(sum > 0.0)) return fail(SDDC_ERR_ARG, "spectrum window: the sum of the window must be > 0");
    }
    std::lock_guard<std::mutex> lk(h->mu);
    if (w && !h->cpu) {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(h->sp_readers.sync());   // earlier launches, on any stream, may still read the device copy
        if (!h->d_sp_win) HIP_TRY(hipMalloc(&h->d_sp_win, SDDC_DDC_FFTN * sizeof(float)));
        h->sp_win.clear();               // a failed upload leaves the rectangular window
        h->sp_wsum = (double)SDDC_DDC_FFTN;
        HIP_TRY(hipMemcpy(h->d_sp_win, w, SDDC_DDC_FFTN * sizeof(float), hipMemcpyHostToDevice));
    }
    if (w) h->sp_win.assign(w, w + SDDC_DDC_FFTN);
    else h->sp_win.clear();
    h->sp_wsum = sum;
    return SDDC_OK;
}

static int check_spectrum_args(const int16_t *in, int nblk, int bpr, const float *psd)
{
    if (nblk <= 0 || nblk > SDDC_DDC_MAX_BLOCKS)
        return fail(SDDC_ERR_ARG, "nblk must be in 1..%d (got %d)", SDDC_DDC_MAX_BLOCKS, nblk);
    if (bpr < 1 || nblk % bpr != 0)
        return fail(SDDC_ERR_ARG, "blocks_per_row must be >= 1 and divide nblk (got %d, nblk %d)", bpr, nblk);
    if (!in || !psd) return fail(SDDC_ERR_ARG, "null buffer");
    if (((uintptr_t)in & 3) != 0) return fail(SDDC_ERR_ARG, "input must be 4-byte aligned");
    if (((uintptr_t)psd & 3) != 0) return fail(SDDC_ERR_ARG, "psd must be 4-byte aligned");
    return SDDC_OK;
}

// 1 / (11 bpr (sum w)^2), in double
static double spectrum_scale(const sddc_ddc_t *h, int bpr)
{
    return 1.0 / ((double)SDDC_DDC_FRAMES * (double)bpr * h->sp_wsum * h->sp_wsum);
}

// the spectrum launches of one call on s (under h->mu)
static int spectrum_launch(sddc_ddc_t *h, const int16_t *d_in, int nblk, int bpr, float *d_psd, hipStream_t s)
{
    const float *win = h->sp_win.empty() ? nullptr : h->d_sp_win;
    // the kernel sums 4 |X|^2 (it leaves out the split's 1/2)
    const float scale = (float)(0.25 * spectrum_scale(h, bpr));
    if (bpr == 1) {
        HIP_TRY(sddc::launch_spectrum(h->tables, d_in, nblk, d_psd, win, scale, h->rand, h->sp_max_wgs, h->device, s));
        HIP_TRY(h->sp_readers.record(s));
        return SDDC_OK;
    }
    if ((size_t)nblk > h->sp_partial_cap) {   // earlier launches may still use the old rows
        HIP_TRY(h->sp_readers.sync());
        if (h->d_sp_partial) (void)hipFree(h->d_sp_partial);
        h->d_sp_partial = nullptr;
        h->sp_partial_cap = 0;
        HIP_TRY(hipMalloc(&h->d_sp_partial, (size_t)nblk * SDDC_DDC_SPECTRUM_BINS * sizeof(float)));
        h->sp_partial_cap = (size_t)nblk;
    } else {
        // the partial rows are per handle: this launch must not overlap one on another stream
        HIP_TRY(h->sp_readers.order_before(s));
    }
    hipError_t e = sddc::launch_spectrum(h->tables, d_in, nblk, h->d_sp_partial, win, 1.f, h->rand, h->sp_max_wgs,
                                         h->device, s);
    if (e == hipSuccess) e = sddc::launch_spectrum_reduce(h->d_sp_partial, nblk / bpr, bpr, scale, d_psd, s);
    const hipError_t er = h->sp_readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_spectrum_device(sddc_ddc_t *h, const int16_t *d_in, int nblk, int blocks_per_row, float *d_psd,
                             void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // the call reads rand and the window: one consistent set
    if (h->cpu) return fail(SDDC_ERR_STATE, "spectrum_device: a CPU handle has no device path");
    if (int rc = check_spectrum_args(d_in, nblk, blocks_per_row, d_psd)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return spectrum_launch(h, d_in, nblk, blocks_per_row, d_psd, (hipStream_t)hip_stream);
}

int sddc_ddc_spectrum_host(sddc_ddc_t *h, const int16_t *in, int nblk, int blocks_per_row, float *psd)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_spectrum_args(in, nblk, blocks_per_row, psd)) return rc;
    if (h->cpu) {
        try {
            h->cpu->spectrum(in, nblk, blocks_per_row, h->sp_win.empty() ? nullptr : h->sp_win.data(),
                             (float)spectrum_scale(h, blocks_per_row), h->rand != 0, psd);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "cpu backend: %s", ex.what());
        }
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    if ((size_t)nblk > h->sp_host_cap) {   // the earlier host calls were synchronous: nothing reads the old buffers
        if (h->d_sp_in) (void)hipFree(h->d_sp_in);
        if (h->d_sp_out) (void)hipFree(h->d_sp_out);
        h->d_sp_in = nullptr;
        h->d_sp_out = nullptr;
        h->sp_host_cap = 0;
        if (hipMalloc(&h->d_sp_in, (kHistory + (size_t)nblk * kBlock) * sizeof(int16_t)) != hipSuccess ||
            hipMalloc(&h->d_sp_out, (size_t)nblk * SDDC_DDC_SPECTRUM_BINS * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            if (h->d_sp_in) (void)hipFree(h->d_sp_in);
            h->d_sp_in = nullptr;
            return fail(SDDC_ERR_NOMEM, "spectrum_host: no device memory for %d blocks", nblk);
        }
        h->sp_host_cap = (size_t)nblk;
    }
    const int rows = nblk / blocks_per_row;
    HIP_TRY(hipMemcpyAsync(h->d_sp_in, in, (kHistory + (size_t)nblk * kBlock) * sizeof(int16_t), hipMemcpyHostToDevice,
                           h->stream));
    const int rc = spectrum_launch(h, h->d_sp_in, nblk, blocks_per_row, h->d_sp_out, h->stream);
    if (rc == SDDC_OK)
        HIP_TRY(hipMemcpyAsync(psd, h->d_sp_out, (size_t)rows * SDDC_DDC_SPECTRUM_BINS * sizeof(float),
                               hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel spectrum: the averaged power spectrum of the DDC's IQ output ----------------- */
static bool chsp_size(int n) { return n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096; }

int sddc_ddc_set_channel_spectrum_window(sddc_ddc_t *h, const float *w, int n)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    double sum = 0.0;
    if (w) {
        if (!chsp_size(n)) return fail(SDDC_ERR_ARG, "channel spectrum window: n must be 256, 512, 1024, 2048 or 4096 (got %d)", n);
        for (int j = 0; j < n; j++) {
            if (!std::isfinite(w[j])) return fail(SDDC_ERR_ARG, "channel spectrum window: value %d is not finite", j);
            sum += w[j];
        }
        if (!(sum > 0.0)) return fail(SDDC_ERR_ARG, "channel spectrum window: the sum of the window must be > 0");
    }
    std::lock_guard<std::mutex> lk(h->mu);
    if (w && !h->cpu) {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(h->chsp_readers.sync());   // earlier launches, on any stream, may still read the device copy
        if (!h->d_chsp_win) HIP_TRY(hipMalloc(&h->d_chsp_win, 4096 * sizeof(float)));
        h->chsp_win.clear();               // a failed upload leaves the rectangular window
        h->chsp_n = 0;
        HIP_TRY(hipMemcpy(h->d_chsp_win, w, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    }
    if (w) h->chsp_win.assign(w, w + n);
    else h->chsp_win.clear();
    h->chsp_n = w ? n : 0;
    h->chsp_wsum = sum;
    return SDDC_OK;
}

// the checks both calls share (under h->mu: the format and the window are read here)
static int check_chsp_args(const sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, int n,
                           int hop, int fpr, int nrows, const float *psd)
{
    if (!chsp_size(n)) return fail(SDDC_ERR_ARG, "channel spectrum: n must be 256, 512, 1024, 2048 or 4096 (got %d)", n);
    if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
        return fail(SDDC_ERR_ARG, "nch must be in 1..%d (got %d)", SDDC_DDC_MAX_CHANNELS, nch);
    if (hop < 1 || fpr < 1 || nrows < 1)
        return fail(SDDC_ERR_ARG, "hop, frames_per_row and nrows must be >= 1 (got %d, %d, %d)", hop, fpr, nrows);
    if ((unsigned long long)nch * (unsigned long long)nrows > 0x7fffffffULL || nsamp > ((size_t)1 << 48))
        return fail(SDDC_ERR_ARG, "nch * nrows must be below 2^31 and nsamp at most 2^48");
    // (nrows fpr - 1) hop + n <= nsamp, without overflow
    const unsigned long long frames = (unsigned long long)nrows * (unsigned long long)fpr;
    if (nsamp < (size_t)n || (frames - 1) > (unsigned long long)(nsamp - (size_t)n) / (unsigned long long)hop)
        return fail(SDDC_ERR_ARG, "%d rows of %d frames at hop %d need more than the %zu samples given", nrows, fpr,
                    hop, nsamp);
    if (nch > 1 && (in_stride < 2 * nsamp || (in_stride & 1) != 0))
        return fail(SDDC_ERR_ARG, "in_stride must be even and >= 2 nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (!iq || !psd) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t sample = h->out_fmt == SDDC_DDC_FMT_CS16 ? 4 : 8;
    if (((uintptr_t)iq & (sample - 1)) != 0) return fail(SDDC_ERR_ARG, "iq must be %d-byte aligned", (int)sample);
    if (((uintptr_t)psd & 3) != 0) return fail(SDDC_ERR_ARG, "psd must be 4-byte aligned");
    if (h->chsp_n != 0 && h->chsp_n != n)
        return fail(SDDC_ERR_STATE, "the channel spectrum window has %d points, the call asks for n = %d", h->chsp_n, n);
    return SDDC_OK;
}

// 1 / (fpr (sum w)^2 s^2) in double; s = cs16_scale under CS16 (the samples enter as integers)
static double chsp_scale(const sddc_ddc_t *h, int n, int fpr)
{
    const double wsum = h->chsp_n ? h->chsp_wsum : (double)n;
    const double s = h->out_fmt == SDDC_DDC_FMT_CS16 ? (double)h->cs16_scale : 1.0;
    return 1.0 / ((double)fpr * wsum * wsum * s * s);
}

static int chsp_launch(sddc_ddc_t *h, const void *d_iq, int nch, size_t in_stride, int n, int hop, int fpr, int nrows,
                       float *d_psd, hipStream_t s)
{
    const hipError_t e = sddc::launch_channel_spectrum(h->tables, d_iq, h->out_fmt == SDDC_DDC_FMT_CS16, nch, nrows,
                                                       in_stride / 2, n, hop, fpr, d_psd,
                                                       h->chsp_n ? h->d_chsp_win : nullptr, (float)chsp_scale(h, n, fpr),
                                                       h->chsp_max_wgs, h->device, s);
    const hipError_t er = h->chsp_readers.record(s);   // whatever was enqueued stays ordered before a window change
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_spectrum_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride, int n,
                                     int hop, int frames_per_row, int nrows, float *d_psd, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // the call reads the format and the window: one consistent set
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_spectrum_device: a CPU handle has no device path");
    if (int rc = check_chsp_args(h, d_iq, nch, nsamp, in_stride, n, hop, frames_per_row, nrows, d_psd)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chsp_launch(h, d_iq, nch, in_stride, n, hop, frames_per_row, nrows, d_psd, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_spectrum_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, int n,
                                   int hop, int frames_per_row, int nrows, float *psd)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chsp_args(h, iq, nch, nsamp, in_stride, n, hop, frames_per_row, nrows, psd)) return rc;
    const bool cs16 = h->out_fmt == SDDC_DDC_FMT_CS16;
    if (h->cpu) {
        try {
            h->cpu->channel_spectrum(iq, cs16, nch, nch > 1 ? in_stride / 2 : 0, n, hop, frames_per_row, nrows,
                                     h->chsp_n ? h->chsp_win.data() : nullptr,
                                     (float)chsp_scale(h, n, frames_per_row), psd);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "cpu backend: %s", ex.what());
        }
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the span that holds every channel's nsamp samples, and the rows
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + 2 * nsamp) * (cs16 ? 2 : 4);
    const size_t out_floats = (size_t)nch * (size_t)nrows * (size_t)n;
    if (int rc = grow_device_buffer(&h->d_chsp_in, &h->chsp_in_cap, in_bytes, "channel_spectrum_host", "input bytes"))
        return rc;
    if (int rc = grow_device_buffer(&h->d_chsp_out, &h->chsp_out_cap, out_floats, "channel_spectrum_host", "output floats"))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->d_chsp_in, iq, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chsp_launch(h, h->d_chsp_in, nch, in_stride, n, hop, frames_per_row, nrows, h->d_chsp_out, h->stream);
    if (rc == SDDC_OK)
        HIP_TRY(hipMemcpyAsync(psd, h->d_chsp_out, out_floats * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel decimator: a streaming decimating FIR on the DDC's IQ output ----------------- */
static_assert(SDDC_DDC_DECIM_MAX_TAPS == sddc::kChDecMaxTaps && SDDC_DDC_DECIM_MAX_FACTOR == sddc::kChDecMaxFactor,
              "the kernel's limits are the ABI's");

/* internal (sddc_ddc_internal.h): the kernel's tile of (factor, ntaps, format) */
int sddc_ddc_internal_chdec_layout(int factor, int ntaps, int cs16, int *tile, int *pitch, int *store_conflicts)
{
    if (factor < 2 || factor > SDDC_DDC_DECIM_MAX_FACTOR || ntaps < 1 || ntaps > SDDC_DDC_DECIM_MAX_TAPS || !tile ||
        !pitch || !store_conflicts)
        return fail(SDDC_ERR_ARG, "chdec layout: factor %d, ntaps %d or a null pointer", factor, ntaps);
    const sddc::ChDecLayout g = sddc::channel_decimate_layout(factor, ntaps, cs16);
    *tile = g.tile;
    *pitch = g.pitch;
    *store_conflicts = g.store_conflicts;
    return SDDC_OK;
}

int sddc_ddc_set_channel_decimator(sddc_ddc_t *h, const float *taps, int ntaps, int factor, int nch)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !taps || ntaps == 0;
    float ordered[SDDC_DDC_DECIM_MAX_TAPS];   // the device copy is in the kernel's order
    if (!off) {
        if (ntaps < 1 || ntaps > SDDC_DDC_DECIM_MAX_TAPS)
            return fail(SDDC_ERR_ARG, "channel decimator: ntaps %d outside 1..%d", ntaps, SDDC_DDC_DECIM_MAX_TAPS);
        if (factor < 2 || factor > SDDC_DDC_DECIM_MAX_FACTOR)
            return fail(SDDC_ERR_ARG, "channel decimator: factor %d outside 2..%d", factor, SDDC_DDC_DECIM_MAX_FACTOR);
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel decimator: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        for (int j = 0; j < ntaps; j++)
            if (!std::isfinite(taps[j])) return fail(SDDC_ERR_ARG, "channel decimator: tap %d is not finite", j);
        sddc::channel_decimate_order_taps(taps, ntaps, factor, ordered);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = h->chdec.configure(h, "channel decimator", taps, ntaps, ordered, (size_t)ntaps, ntaps - 1, nch)) return rc;
    h->chdec_R = off ? 0 : factor;
    return SDDC_OK;
}

int sddc_ddc_channel_decimator_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chdec.taps.empty()) return fail(SDDC_ERR_STATE, "channel decimator reset: no decimator set");
    return h->chdec.reset(h);
}

size_t sddc_ddc_channel_decimate_samples(int factor, size_t nsamp)
{
    if (factor < 2 || factor > SDDC_DDC_DECIM_MAX_FACTOR || nsamp % (size_t)factor != 0) return 0;
    return nsamp / (size_t)factor;
}

// the checks both calls share (under h->mu: the format and the decimator are read here)
static int check_chdec_args(const sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride,
                            const float *out, size_t out_stride)
{
    if (h->chdec.taps.empty()) return fail(SDDC_ERR_STATE, "channel decimate: no decimator set");
    if (nch != h->chdec.nch)
        return fail(SDDC_ERR_STATE, "channel decimate: the decimator is set for %d channels, the call has %d",
                    h->chdec.nch, nch);
    const size_t R = (size_t)h->chdec_R;
    if (nsamp == 0 || nsamp % R != 0 || nsamp > ((size_t)1 << 40))
        return fail(SDDC_ERR_ARG, "nsamp must be a positive multiple of the factor %zu, at most 2^40 (got %zu)", R, nsamp);
    return check_channel_io(h, "2 nsamp / factor", iq, nch, nsamp, in_stride, out, out_stride, nsamp / R);
}

static int chdec_launch(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride, float *d_out,
                        size_t out_stride, hipStream_t s)
{
    return h->chdec.launch(s, [&](const float2 *tail_in, float2 *tail_out) {
        return sddc::launch_channel_decimate(h->tables, d_iq, h->out_fmt == SDDC_DDC_FMT_CS16, h->cs16_scale, nch, nsamp,
                                             in_stride, h->chdec.d_taps, (int)h->chdec.taps.size(), h->chdec_R, tail_in,
                                             tail_out, d_out, out_stride, h->chdec.max_wgs, h->device, s);
    });
}

int sddc_ddc_channel_decimate_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride,
                                     float *d_out, size_t out_stride, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // the call reads the format and the decimator: one consistent set
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_decimate_device: a CPU handle has no device path");
    if (int rc = check_chdec_args(h, d_iq, nch, nsamp, in_stride, d_out, out_stride)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chdec_launch(h, d_iq, nch, nsamp, in_stride, d_out, out_stride, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_decimate_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, float *out,
                                   size_t out_stride)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chdec_args(h, iq, nch, nsamp, in_stride, out, out_stride)) return rc;
    if (h->cpu) {
        try {
            sddc::cpu::R2iq::channel_decimate(iq, h->out_fmt == SDDC_DDC_FMT_CS16, (float)(1.0 / (double)h->cs16_scale),
                                              nch, nsamp, nch > 1 ? in_stride : 0, h->chdec.taps.data(),
                                              (int)h->chdec.taps.size(), h->chdec_R, h->chdec.tail_h.data(), out,
                                              nch > 1 ? out_stride : 0);
        } catch (const std::exception &ex) {   // thrown before any output or tail is written
            return fail(SDDC_ERR_NOMEM, "cpu backend: %s", ex.what());
        }
        return SDDC_OK;
    }
    return channel_host_roundtrip(h, h->chdec, "channel_decimate_host", iq, nch, nsamp, in_stride, out, out_stride,
                                  nsamp / (size_t)h->chdec_R, [&](const void *d_in, float *d_out) {
                                      return chdec_launch(h, d_in, nch, nsamp, in_stride, d_out, out_stride, h->stream);
                                  });
}

/* ---- channel resampler: a streaming rational L/M polyphase FIR on the DDC's IQ output ------ */
static_assert(SDDC_DDC_RESAMPLE_MAX_TAPS == sddc::kChResMaxTaps && SDDC_DDC_RESAMPLE_MAX_UP == sddc::kChResMaxUp &&
                  SDDC_DDC_RESAMPLE_MAX_DOWN == sddc::kChResMaxDown && SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS == sddc::kChResMaxK,
              "the kernel's limits are the ABI's");

static int chres_gcd(int a, int b)
{
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// the factors of the ABI: ranges, coprime, not the identity
static bool chres_factors_ok(int up, int down)
{
    return up >= 1 && up <= SDDC_DDC_RESAMPLE_MAX_UP && down >= 1 && down <= SDDC_DDC_RESAMPLE_MAX_DOWN &&
           chres_gcd(up, down) == 1 && !(up == 1 && down == 1);
}

// The reduced position of N samples consumed: e = ceil(N up / down) down - N up = (-N up) mod down.
static int chres_position(int up, int down, uint64_t pos)
{
    const int r = (int)((pos % (uint64_t)down) * (uint64_t)up % (uint64_t)down);
    return r ? down - r : 0;
}

// Outputs of nsamp <= 2^40 samples at the reduced position e: the k >= 0 with e + k down < nsamp up.
static size_t chres_count(int up, int down, int e, size_t nsamp)
{
    const uint64_t span = (uint64_t)nsamp * (uint64_t)up;
    return span > (uint64_t)e ? (size_t)((span - (uint64_t)e + (uint64_t)down - 1) / (uint64_t)down) : 0;
}

// the position after that call: e + nout down - nsamp up
static int chres_advance(int up, int down, int e, size_t nsamp, size_t nout)
{
    return (int)((int64_t)e + (int64_t)nout * down - (int64_t)nsamp * up);
}

/* internal (sddc_ddc_internal.h): the kernel's tile of (up, down, ntaps, format) */
int sddc_ddc_internal_chres_layout(int up, int down, int ntaps, int cs16, int *tile_outputs, int *pitch,
                                   int *store_conflicts)
{
    if (!chres_factors_ok(up, down) || ntaps < 1 || ntaps > SDDC_DDC_RESAMPLE_MAX_TAPS ||
        (ntaps + up - 1) / up > SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS || !tile_outputs || !pitch || !store_conflicts)
        return fail(SDDC_ERR_ARG, "chres layout: up %d, down %d, ntaps %d or a null pointer", up, down, ntaps);
    const sddc::ChResLayout g = sddc::channel_resample_layout(up, down, ntaps, cs16);
    *tile_outputs = g.ta * up;
    *pitch = g.pitch;
    *store_conflicts = g.store_conflicts;
    return SDDC_OK;
}

/* internal: the stream position, the tails left as they are */
int sddc_ddc_internal_chres_set_position(sddc_ddc_t *h, uint64_t pos)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chres.taps.empty()) return fail(SDDC_ERR_STATE, "chres set position: no resampler set");
    h->chres_e = chres_position(h->chres_L, h->chres_M, pos);   // host state: a launch in flight has its own copy
    return SDDC_OK;
}

int sddc_ddc_set_channel_resampler(sddc_ddc_t *h, const float *taps, int ntaps, int up, int down, int nch)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !taps || ntaps == 0;
    int K = 0;
    float ordered[SDDC_DDC_RESAMPLE_MAX_TAPS + SDDC_DDC_RESAMPLE_MAX_UP];   // the kernel's order: up K < ntaps + up
    if (!off) {
        if (ntaps < 1 || ntaps > SDDC_DDC_RESAMPLE_MAX_TAPS)
            return fail(SDDC_ERR_ARG, "channel resampler: ntaps %d outside 1..%d", ntaps, SDDC_DDC_RESAMPLE_MAX_TAPS);
        if (!chres_factors_ok(up, down))
            return fail(SDDC_ERR_ARG, "channel resampler: up %d (1..%d) and down %d (1..%d) must be coprime and not both 1",
                        up, SDDC_DDC_RESAMPLE_MAX_UP, down, SDDC_DDC_RESAMPLE_MAX_DOWN);
        K = (ntaps + up - 1) / up;
        if (K > SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS)
            return fail(SDDC_ERR_ARG, "channel resampler: ceil(ntaps / up) = %d is above %d", K,
                        SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS);
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel resampler: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        for (int j = 0; j < ntaps; j++)
            if (!std::isfinite(taps[j])) return fail(SDDC_ERR_ARG, "channel resampler: tap %d is not finite", j);
        sddc::channel_resample_order_taps(taps, ntaps, up, ordered);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = h->chres.configure(h, "channel resampler", taps, ntaps, ordered, (size_t)up * (size_t)K, K - 1, nch))
        return rc;
    h->chres_L = off ? 0 : up;
    h->chres_M = off ? 0 : down;
    h->chres_e = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_resampler_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chres.taps.empty()) return fail(SDDC_ERR_STATE, "channel resampler reset: no resampler set");
    if (int rc = h->chres.reset(h)) return rc;
    h->chres_e = 0;
    return SDDC_OK;
}

size_t sddc_ddc_resample_count(int up, int down, uint64_t pos, size_t nsamp)
{
    if (!chres_factors_ok(up, down) || nsamp > ((size_t)1 << 40)) return 0;
    return chres_count(up, down, chres_position(up, down, pos), nsamp);
}

size_t sddc_ddc_channel_resample_samples(sddc_ddc_t *h, size_t nsamp)
{
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chres.taps.empty() || nsamp > ((size_t)1 << 40)) return 0;
    return chres_count(h->chres_L, h->chres_M, h->chres_e, nsamp);
}

// the checks both calls share (under h->mu: the format, the resampler and the position are read here)
static int check_chres_args(const sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride,
                            const float *out, size_t out_stride, size_t *nout)
{
    if (h->chres.taps.empty()) return fail(SDDC_ERR_STATE, "channel resample: no resampler set");
    if (nch != h->chres.nch)
        return fail(SDDC_ERR_STATE, "channel resample: the resampler is set for %d channels, the call has %d",
                    h->chres.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40))
        return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    *nout = chres_count(h->chres_L, h->chres_M, h->chres_e, nsamp);
    return check_channel_io(h, "2 nout", iq, nch, nsamp, in_stride, out, out_stride, *nout);
}

// the position advances once the launch is enqueued
static int chres_launch(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride, float *d_out,
                        size_t out_stride, size_t nout, hipStream_t s)
{
    return h->chres.launch(s, [&](const float2 *tail_in, float2 *tail_out) {
        const hipError_t e = sddc::launch_channel_resample(
            h->tables, d_iq, h->out_fmt == SDDC_DDC_FMT_CS16, h->cs16_scale, nch, nsamp, in_stride, h->chres.d_taps,
            (int)h->chres.taps.size(), h->chres_L, h->chres_M, h->chres_e, nout, tail_in, tail_out, d_out, out_stride,
            h->chres.max_wgs, h->device, s);
        if (e == hipSuccess) h->chres_e = chres_advance(h->chres_L, h->chres_M, h->chres_e, nsamp, nout);
        return e;
    });
}

int sddc_ddc_channel_resample_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride,
                                     float *d_out, size_t out_stride, size_t *nout, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // the call reads the format and the resampler: one consistent set
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_resample_device: a CPU handle has no device path");
    size_t n = 0;
    if (int rc = check_chres_args(h, d_iq, nch, nsamp, in_stride, d_out, out_stride, &n)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    if (int rc = chres_launch(h, d_iq, nch, nsamp, in_stride, d_out, out_stride, n, (hipStream_t)hip_stream)) return rc;
    if (nout) *nout = n;
    return SDDC_OK;
}

int sddc_ddc_channel_resample_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, float *out,
                                   size_t out_stride, size_t *nout_p)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    size_t nout = 0;
    if (int rc = check_chres_args(h, iq, nch, nsamp, in_stride, out, out_stride, &nout)) return rc;
    if (h->cpu) {
        try {
            sddc::cpu::R2iq::channel_resample(iq, h->out_fmt == SDDC_DDC_FMT_CS16, (float)(1.0 / (double)h->cs16_scale),
                                              nch, nsamp, nch > 1 ? in_stride : 0, h->chres.taps.data(),
                                              (int)h->chres.taps.size(), h->chres_L, h->chres_M, h->chres_e, nout,
                                              h->chres.tail_h.data(), out, nch > 1 ? out_stride : 0);
        } catch (const std::exception &ex) {   // thrown before any output or tail is written
            return fail(SDDC_ERR_NOMEM, "cpu backend: %s", ex.what());
        }
        h->chres_e = chres_advance(h->chres_L, h->chres_M, h->chres_e, nsamp, nout);
        if (nout_p) *nout_p = nout;
        return SDDC_OK;
    }
    const int rc = channel_host_roundtrip(h, h->chres, "channel_resample_host", iq, nch, nsamp, in_stride, out, out_stride,
                                          nout, [&](const void *d_in, float *d_out) {
                                              return chres_launch(h, d_in, nch, nsamp, in_stride, d_out, out_stride, nout,
                                                                  h->stream);
                                          });
    if (rc == SDDC_OK && nout_p) *nout_p = nout;
    return rc;
}

/* ---- channel audio resampler: a streaming rational L/M polyphase FIR on real audio ---------- */
/* internal (sddc_ddc_internal.h): the kernel's tile of (up, down, ntaps, input format) */
int sddc_ddc_internal_chars_layout(int up, int down, int ntaps, int in_s16, int *tile_a, int *lds, int *pitch,
                                   int *store_conflicts)
{
    if (!chres_factors_ok(up, down) || ntaps < 1 || ntaps > SDDC_DDC_RESAMPLE_MAX_TAPS ||
        (ntaps + up - 1) / up > SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS || !tile_a || !lds || !pitch || !store_conflicts)
        return fail(SDDC_ERR_ARG, "chars layout: up %d, down %d, ntaps %d or a null pointer", up, down, ntaps);
    const sddc::ChArsLayout g = sddc::channel_audio_resample_layout(up, down, ntaps, in_s16);
    *tile_a = g.ta;
    *lds = g.lds;
    *pitch = g.pitch;
    *store_conflicts = g.store_conflicts;
    return SDDC_OK;
}

/* internal: the pitch search alone (tools/channel_audio_resample_banks.py) */
int sddc_ddc_internal_chars_pitch(int mod, int need, int max_pitch, int V, int *store_conflicts)
{
    if (mod < 1 || need < 1 || max_pitch < need || (V != 4 && V != 8) || !store_conflicts)
        return fail(SDDC_ERR_ARG, "chars pitch: mod %d, need %d, max %d, V %d or a null pointer", mod, need, max_pitch, V);
    return sddc::channel_audio_resample_pitch(mod, need, max_pitch, V, store_conflicts);
}

/* internal: the stream position, the tails left as they are */
int sddc_ddc_internal_chars_set_position(sddc_ddc_t *h, uint64_t pos)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chars.taps.empty()) return fail(SDDC_ERR_STATE, "chars set position: no audio resampler set");
    h->chars_e = sddc::ars::ars_position(h->chars_L, h->chars_M, pos);   // host state: a launch in flight has its own copy
    return SDDC_OK;
}

int sddc_ddc_set_channel_audio_resampler(sddc_ddc_t *h, const float *taps, int ntaps, int up, int down, int nch,
                                         int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !taps || ntaps == 0;
    int K = 0;
    float ordered[SDDC_DDC_RESAMPLE_MAX_TAPS + SDDC_DDC_RESAMPLE_MAX_UP];   // the kernel's order: up K < ntaps + up
    if (!off) {
        if (ntaps < 1 || ntaps > SDDC_DDC_RESAMPLE_MAX_TAPS)
            return fail(SDDC_ERR_ARG, "channel audio resampler: ntaps %d outside 1..%d", ntaps, SDDC_DDC_RESAMPLE_MAX_TAPS);
        if (!chres_factors_ok(up, down))
            return fail(SDDC_ERR_ARG, "channel audio resampler: up %d (1..%d) and down %d (1..%d) must be coprime and not both 1",
                        up, SDDC_DDC_RESAMPLE_MAX_UP, down, SDDC_DDC_RESAMPLE_MAX_DOWN);
        K = (ntaps + up - 1) / up;
        if (K > SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS)
            return fail(SDDC_ERR_ARG, "channel audio resampler: ceil(ntaps / up) = %d is above %d", K,
                        SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS);
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel audio resampler: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        for (int fmt : {in_format, out_format})
            if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
                return fail(SDDC_ERR_ARG, "channel audio resampler: unknown sample format %d", fmt);
        for (int j = 0; j < ntaps; j++)
            if (!std::isfinite(taps[j])) return fail(SDDC_ERR_ARG, "channel audio resampler: tap %d is not finite", j);
        sddc::ars::ars_order_taps(taps, ntaps, up, ordered);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    // K - 1 floats per channel in ceil((K - 1) / 2) float2
    if (int rc = h->chars.configure(h, "channel audio resampler", taps, ntaps, ordered, (size_t)up * (size_t)K, K / 2, nch))
        return rc;
    h->chars_L = off ? 0 : up;
    h->chars_M = off ? 0 : down;
    h->chars_e = 0;
    h->chars_in_fmt = off ? 0 : in_format;
    h->chars_out_fmt = off ? 0 : out_format;
    return SDDC_OK;
}

int sddc_ddc_channel_audio_resampler_formats(sddc_ddc_t *h, int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    for (int fmt : {in_format, out_format})
        if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
            return fail(SDDC_ERR_ARG, "channel audio resampler: unknown sample format %d", fmt);
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chars.taps.empty()) return fail(SDDC_ERR_STATE, "channel audio resampler formats: no audio resampler set");
    h->chars_in_fmt = in_format;   // host state: a launch in flight has its own copy
    h->chars_out_fmt = out_format;
    return SDDC_OK;
}

int sddc_ddc_channel_audio_resampler_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chars.taps.empty()) return fail(SDDC_ERR_STATE, "channel audio resampler reset: no audio resampler set");
    if (int rc = h->chars.reset(h)) return rc;
    h->chars_e = 0;
    return SDDC_OK;
}

size_t sddc_ddc_channel_audio_resample_samples(sddc_ddc_t *h, size_t nsamp)
{
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chars.taps.empty() || nsamp > ((size_t)1 << 40)) return 0;
    return (size_t)sddc::ars::ars_count(h->chars_L, h->chars_M, h->chars_e, nsamp);
}

// the checks both calls share (under h->mu: the formats, the resampler and the position are read here)
static int check_chars_args(const sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, const void *out,
                            size_t out_stride, size_t *nout)
{
    if (h->chars.taps.empty()) return fail(SDDC_ERR_STATE, "channel audio resample: no audio resampler set");
    if (nch != h->chars.nch)
        return fail(SDDC_ERR_STATE, "channel audio resample: the resampler is set for %d channels, the call has %d",
                    h->chars.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    *nout = (size_t)sddc::ars::ars_count(h->chars_L, h->chars_M, h->chars_e, nsamp);
    if (nch > 1 && in_stride < nsamp) return fail(SDDC_ERR_ARG, "in_stride must be >= nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < *nout)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nout (got %zu, nout %zu)", out_stride, *nout);
    if (!in || !out) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t is = h->chars_in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = h->chars_out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)in & (is - 1)) != 0) return fail(SDDC_ERR_ARG, "the input must be %d-byte aligned", (int)is);
    if (((uintptr_t)out & (os - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)os);
    return SDDC_OK;
}

// the position advances once the launch is enqueued
static int chars_launch(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride, void *d_out,
                        size_t out_stride, size_t nout, hipStream_t s)
{
    return h->chars.launch(s, [&](const float2 *tail_in, float2 *tail_out) {
        const hipError_t e = sddc::launch_channel_audio_resample(
            h->tables, d_in, h->chars_in_fmt == SDDC_DDC_AUDIO_S16, nch, nsamp, in_stride, h->chars.d_taps,
            (int)h->chars.taps.size(), h->chars_L, h->chars_M, h->chars_e, nout, reinterpret_cast<const float *>(tail_in),
            reinterpret_cast<float *>(tail_out), d_out, h->chars_out_fmt == SDDC_DDC_AUDIO_S16, out_stride, h->chars.max_wgs,
            h->device, s);
        if (e == hipSuccess) h->chars_e = sddc::ars::ars_advance(h->chars_L, h->chars_M, h->chars_e, nsamp, nout);
        return e;
    });
}

int sddc_ddc_channel_audio_resample_device(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride,
                                           void *d_out, size_t out_stride, size_t *nout, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // the call reads the formats and the resampler: one consistent set
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_audio_resample_device: a CPU handle has no device path");
    size_t n = 0;
    if (int rc = check_chars_args(h, d_in, nch, nsamp, in_stride, d_out, out_stride, &n)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    if (int rc = chars_launch(h, d_in, nch, nsamp, in_stride, d_out, out_stride, n, (hipStream_t)hip_stream)) return rc;
    if (nout) *nout = n;
    return SDDC_OK;
}

int sddc_ddc_channel_audio_resample_host(sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, void *out,
                                         size_t out_stride, size_t *nout_p)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    size_t nout = 0;
    if (int rc = check_chars_args(h, in, nch, nsamp, in_stride, out, out_stride, &nout)) return rc;
    ChannelStream &st = h->chars;
    const bool in16 = h->chars_in_fmt == SDDC_DDC_AUDIO_S16, out16 = h->chars_out_fmt == SDDC_DDC_AUDIO_S16;
    if (h->cpu) {
        try {
            sddc::cpu::R2iq::channel_audio_resample(in, in16, nch, nsamp, nch > 1 ? in_stride : 0, st.taps.data(),
                                                    (int)st.taps.size(), h->chars_L, h->chars_M, h->chars_e, nout,
                                                    st.tail_h.data(), out, out16, nch > 1 ? out_stride : 0);
        } catch (const std::exception &ex) {   // thrown before any output or tail is written
            return fail(SDDC_ERR_NOMEM, "cpu backend: %s", ex.what());
        }
        h->chars_e = sddc::ars::ars_advance(h->chars_L, h->chars_M, h->chars_e, nsamp, nout);
        if (nout_p) *nout_p = nout;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs (one float at least: a call without an output)
    const size_t is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const size_t out_bytes = ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nout) * os;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_audio_resample_host", "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes / 4 + 1, "channel_audio_resample_host", "output floats"))
        return rc;
    HIP_TRY(hipMemcpyAsync(st.d_in, in, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chars_launch(h, st.d_in, nch, nsamp, in_stride, st.d_out, out_stride, nout, h->stream);
    if (rc == SDDC_OK && nout) {   // the streams alone: the caller's memory between them stays as it is
        if (nch == 1 || out_stride == nout)
            HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, out_stride * os, st.d_out, out_stride * os, nout * os, (size_t)nch,
                                     hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    if (rc == SDDC_OK && nout_p) *nout_p = nout;
    return rc;
}

/* ---- channel demodulator: streaming AM / FM / BFO audio from the channel streams ---------- */
uint32_t sddc_ddc_bfo_word(double relative_freq)
{
    if (!std::isfinite(relative_freq)) return 0u;
    const double r = relative_freq - std::floor(relative_freq + 0.5);   // [-0.5, 0.5)
    return (uint32_t)(int64_t)std::llround(r * 4294967296.0);
}

/* internal (sddc_ddc_internal.h): demod_math.h's two routines as the CPU backend compiles them */
int sddc_ddc_internal_demod_angle(const float *im, const float *re, size_t n, float *out)
{
    if (!im || !re || !out) return fail(SDDC_ERR_ARG, "demod angle: null pointer");
    sddc::cpu::R2iq::demod_angle_n(im, re, n, out);
    return SDDC_OK;
}

int sddc_ddc_internal_demod_sincos(const uint32_t *words, size_t n, float *c, float *s)
{
    if (!words || !c || !s) return fail(SDDC_ERR_ARG, "demod sincos: null pointer");
    sddc::cpu::R2iq::demod_sincos_n(words, n, c, s);
    return SDDC_OK;
}

/* internal: the stream position, the last samples left as they are */
int sddc_ddc_internal_chdem_set_position(sddc_ddc_t *h, uint32_t pos)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chdem.chan.empty()) return fail(SDDC_ERR_STATE, "chdem set position: no demodulator set");
    h->chdem.pos = pos;   // host state: a launch in flight has its own copy
    return SDDC_OK;
}

int sddc_ddc_set_channel_demodulator(sddc_ddc_t *h, const int *modes, const float *gains, const uint32_t *bfo_words,
                                     int nch, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !modes || nch == 0;
    std::vector<sddc::ChDemChannel> chan;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel demodulator: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        if (out_format != SDDC_DDC_AUDIO_F32 && out_format != SDDC_DDC_AUDIO_S16)
            return fail(SDDC_ERR_ARG, "channel demodulator: unknown output format %d", out_format);
        try {
            chan.resize((size_t)nch);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel demodulator: %s", ex.what());
        }
        for (int c = 0; c < nch; c++) {
            if (modes[c] < SDDC_DDC_DEMOD_AM || modes[c] > SDDC_DDC_DEMOD_BFO)
                return fail(SDDC_ERR_ARG, "channel demodulator: mode %d of channel %d outside 0..2", modes[c], c);
            const float g = gains ? gains[c] : 1.f;
            if (!std::isfinite(g)) return fail(SDDC_ERR_ARG, "channel demodulator: the gain of channel %d is not finite", c);
            chan[(size_t)c] = sddc::ChDemChannel{modes[c], g, bfo_words ? bfo_words[c] : 0u, 0u};
        }
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelDemod &st = h->chdem;
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.last_h.assign(2 * (size_t)nch, 0.f);
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel demodulator: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the demodulator off
        if (off) return SDDC_OK;
        hipError_t e = hipMalloc(&st.d_chan, (size_t)nch * sizeof(sddc::ChDemChannel));
        for (float2 *&p : st.d_last)
            if (e == hipSuccess) e = hipMalloc(&p, (size_t)nch * sizeof(float2));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel demodulator: no device memory for %d channels", nch);
        }
        e = hipMemcpy(st.d_chan, chan.data(), (size_t)nch * sizeof(sddc::ChDemChannel), hipMemcpyHostToDevice);
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        if (e == hipSuccess) e = hipMemsetAsync(st.d_last[0], 0, (size_t)nch * sizeof(float2), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.chan = std::move(chan);
    st.nch = nch;
    st.out_fmt = out_format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_demodulator_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelDemod &st = h->chdem;
    if (st.chan.empty()) return fail(SDDC_ERR_STATE, "channel demodulator reset: no demodulator set");
    if (h->cpu) {
        std::fill(st.last_h.begin(), st.last_h.end(), 0.f);
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the last samples
        HIP_TRY(hipMemsetAsync(st.d_last[st.cur], 0, (size_t)st.nch * sizeof(float2), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

// the checks both calls share (under h->mu: the formats and the demodulator are read here)
static int check_chdem_args(const sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride,
                            const void *out, size_t out_stride, const float *power)
{
    const ChannelDemod &st = h->chdem;
    if (st.chan.empty()) return fail(SDDC_ERR_STATE, "channel demodulate: no demodulator set");
    if (nch != st.nch)
        return fail(SDDC_ERR_STATE, "channel demodulate: the demodulator is set for %d channels, the call has %d", st.nch,
                    nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (nch > 1 && (in_stride < 2 * nsamp || (in_stride & 1) != 0))
        return fail(SDDC_ERR_ARG, "in_stride must be even and >= 2 nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < nsamp)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    if (!iq || !out) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t sample = h->out_fmt == SDDC_DDC_FMT_CS16 ? 4 : 8;
    if (((uintptr_t)iq & (sample - 1)) != 0) return fail(SDDC_ERR_ARG, "iq must be %d-byte aligned", (int)sample);
    const uintptr_t es = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)out & (es - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)es);
    if (((uintptr_t)power & 3) != 0) return fail(SDDC_ERR_ARG, "the power array must be 4-byte aligned");
    return SDDC_OK;
}

// One launch on s: it reads the current last samples and writes the other buffer, so it runs after
// every earlier launch of the handle, whatever its stream; the buffers swap and the position
// advances once it is enqueued.
static int chdem_launch(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride, void *d_out,
                        size_t out_stride, float *d_power, hipStream_t s)
{
    ChannelDemod &st = h->chdem;
    if (d_power) {
        const size_t need = (size_t)nch * sddc::channel_demod_tiles(nsamp);
        if (need > st.partial_cap) {
            HIP_TRY(st.readers.sync());   // an earlier launch may still add its tile sums
            if (int rc = grow_device_buffer(&st.d_partial, &st.partial_cap, need, "channel demodulate", "tile sums")) return rc;
        }
    }
    HIP_TRY(st.readers.order_before(s));
    const hipError_t e = sddc::launch_channel_demod(h->tables, d_iq, h->out_fmt == SDDC_DDC_FMT_CS16, h->cs16_scale, nch,
                                                    nsamp, in_stride, st.d_chan, st.pos, st.d_last[st.cur],
                                                    st.d_last[st.cur ^ 1], d_out, st.out_fmt == SDDC_DDC_AUDIO_S16,
                                                    out_stride, d_power, st.d_partial, st.max_wgs, h->device, s);
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    st.cur ^= 1;
    st.pos += (uint32_t)nsamp;
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_demodulate_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride,
                                       void *d_out, size_t out_stride, float *d_power, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);   // the call reads the formats and the demodulator: one consistent set
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_demodulate_device: a CPU handle has no device path");
    if (int rc = check_chdem_args(h, d_iq, nch, nsamp, in_stride, d_out, out_stride, d_power)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chdem_launch(h, d_iq, nch, nsamp, in_stride, d_out, out_stride, d_power, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_demodulate_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, void *out,
                                     size_t out_stride, float *power)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chdem_args(h, iq, nch, nsamp, in_stride, out, out_stride, power)) return rc;
    ChannelDemod &st = h->chdem;
    const bool cs16 = h->out_fmt == SDDC_DDC_FMT_CS16, s16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_demodulate(iq, cs16, (float)(1.0 / (double)h->cs16_scale), nch, nsamp,
                                            nch > 1 ? in_stride : 0, st.chan.data(), st.pos, st.last_h.data(), out, s16,
                                            nch > 1 ? out_stride : 0, power);
        st.pos += (uint32_t)nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs
    const size_t es = s16 ? 2 : 4;
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + 2 * nsamp) * (cs16 ? 2 : 4);
    const size_t out_bytes = ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * es;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_demodulate_host", "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes, "channel_demodulate_host", "output bytes")) return rc;
    if (power)
        if (int rc = grow_device_buffer(&st.d_pow, &st.pow_cap, (size_t)nch, "channel_demodulate_host", "powers")) return rc;
    HIP_TRY(hipMemcpyAsync(st.d_in, iq, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chdem_launch(h, st.d_in, nch, nsamp, in_stride, st.d_out, out_stride, power ? st.d_pow : nullptr, h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        if (nch == 1 || out_stride == nsamp)
            HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, out_stride * es, st.d_out, out_stride * es, nsamp * es, (size_t)nch,
                                     hipMemcpyDeviceToHost, h->stream));
        if (power) HIP_TRY(hipMemcpyAsync(power, st.d_pow, (size_t)nch * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel audio filter: a streaming biquad cascade per channel --------------------------- */
int sddc_ddc_biquad(int kind, double f, double q, float coeffs[5])
{
    if (!coeffs) return fail(SDDC_ERR_ARG, "biquad: null coeffs");
    if (kind < SDDC_DDC_BIQUAD_IDENTITY || kind > SDDC_DDC_BIQUAD_NOTCH) return fail(SDDC_ERR_ARG, "biquad: unknown kind %d", kind);
    float c[5] = {1.f, 0.f, 0.f, 0.f, 0.f};
    if (kind != SDDC_DDC_BIQUAD_IDENTITY) {
        if (!(f > 0.0 && f < 0.5)) return fail(SDDC_ERR_ARG, "biquad: f %g outside (0, 0.5)", f);
        const double w = 2.0 * 3.14159265358979323846 * f;
        if (kind == SDDC_DDC_BIQUAD_DC_BLOCK) {
            const double r = std::exp(-w);
            c[0] = (float)((1.0 + r) / 2.0);
            c[1] = -c[0];
            c[3] = (float)-r;
        } else if (kind == SDDC_DDC_BIQUAD_ONE_POLE_LP) {
            const double al = std::exp(-w);
            c[0] = (float)(1.0 - al);
            c[3] = (float)-al;
        } else {
            if (!(q > 0.0) || !std::isfinite(q)) return fail(SDDC_ERR_ARG, "biquad: q %g is not a positive finite number", q);
            const double cw = std::cos(w), alpha = std::sin(w) / (2.0 * q), a0 = 1.0 + alpha;
            c[3] = (float)(-2.0 * cw / a0);
            c[4] = (float)((1.0 - alpha) / a0);
            if (kind == SDDC_DDC_BIQUAD_LOWPASS) {
                c[0] = c[2] = (float)((1.0 - cw) / (2.0 * a0));
                c[1] = 2.f * c[0];
            } else if (kind == SDDC_DDC_BIQUAD_HIGHPASS) {
                c[0] = c[2] = (float)((1.0 + cw) / (2.0 * a0));
                c[1] = -2.f * c[0];
            } else {
                c[0] = c[2] = (float)(1.0 / a0);
                c[1] = c[3];
            }
        }
    }
    for (int i = 0; i < 5; i++) coeffs[i] = c[i];
    return SDDC_OK;
}

/* internal: the stream position, the states left as they are */
int sddc_ddc_internal_chaud_set_position(sddc_ddc_t *h, uint64_t pos)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chaud.coef.empty()) return fail(SDDC_ERR_STATE, "chaud set position: no audio filter set");
    h->chaud.pos = pos;   // host state: a launch in flight has its own copy
    return SDDC_OK;
}

int sddc_ddc_set_channel_audio_filter(sddc_ddc_t *h, const float *coeffs, int nsec, int nch, int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !coeffs || nch == 0;
    std::vector<float> coef, mat;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel audio filter: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        if (nsec < 1 || nsec > SDDC_DDC_AUDIO_MAX_SECTIONS)
            return fail(SDDC_ERR_ARG, "channel audio filter: nsec %d outside 1..%d", nsec, SDDC_DDC_AUDIO_MAX_SECTIONS);
        for (int fmt : {in_format, out_format})
            if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
                return fail(SDDC_ERR_ARG, "channel audio filter: unknown sample format %d", fmt);
        const size_t n = (size_t)nch * (size_t)nsec;
        for (size_t k = 0; k < n; k++) {
            const float *c = coeffs + 5 * k;
            for (int i = 0; i < 5; i++)
                if (!std::isfinite(c[i]))
                    return fail(SDDC_ERR_ARG, "channel audio filter: a coefficient of channel %zu, section %zu is not finite",
                                k / (size_t)nsec, k % (size_t)nsec);
            if (!(std::fabs(c[4]) < 1.f) || !(std::fabs((double)c[3]) < 1.0 + (double)c[4]))
                return fail(SDDC_ERR_ARG, "channel audio filter: section %zu of channel %zu is not stable (a1 %g, a2 %g)",
                            k % (size_t)nsec, k / (size_t)nsec, (double)c[3], (double)c[4]);
        }
        try {
            coef.assign(coeffs, coeffs + 5 * n);
            mat.resize((size_t)nch * 4 * (size_t)nsec * (size_t)nsec);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel audio filter: %s", ex.what());
        }
        for (int c = 0; c < nch; c++)
            sddc::audio::audio_block_matrix(coef.data() + (size_t)c * 5 * nsec, nsec, mat.data() + (size_t)c * 4 * nsec * nsec);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelAudio &st = h->chaud;
    const size_t nstate = (size_t)nch * 6 * (size_t)(off ? 0 : nsec);
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.state_h.assign(nstate, 0.f);
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel audio filter: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the stage off
        if (off) return SDDC_OK;
        hipError_t e = hipMalloc(&st.d_coef, coef.size() * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&st.d_mat, mat.size() * sizeof(float));
        for (float *&p : st.d_state)
            if (e == hipSuccess) e = hipMalloc(&p, nstate * sizeof(float));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel audio filter: no device memory for %d channels", nch);
        }
        e = hipMemcpy(st.d_coef, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(st.d_mat, mat.data(), mat.size() * sizeof(float), hipMemcpyHostToDevice);
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        if (e == hipSuccess) e = hipMemsetAsync(st.d_state[0], 0, nstate * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.coef = std::move(coef);
    st.mat = std::move(mat);
    st.nch = nch;
    st.nsec = nsec;
    st.in_fmt = in_format;
    st.out_fmt = out_format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_audio_filter_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelAudio &st = h->chaud;
    if (st.coef.empty()) return fail(SDDC_ERR_STATE, "channel audio filter reset: no filter set");
    if (h->cpu) {
        std::fill(st.state_h.begin(), st.state_h.end(), 0.f);
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        HIP_TRY(hipMemsetAsync(st.d_state[st.cur], 0, st.state_floats() * sizeof(float), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

// the checks both calls share (under h->mu)
static int check_chaud_args(const sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, const void *out,
                            size_t out_stride)
{
    const ChannelAudio &st = h->chaud;
    if (st.coef.empty()) return fail(SDDC_ERR_STATE, "channel audio filter: no filter set");
    if (nch != st.nch)
        return fail(SDDC_ERR_STATE, "channel audio filter: the filter is set for %d channels, the call has %d", st.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (nch > 1 && in_stride < nsamp) return fail(SDDC_ERR_ARG, "in_stride must be >= nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < nsamp)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    if (!in || !out) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)in & (is - 1)) != 0) return fail(SDDC_ERR_ARG, "the input must be %d-byte aligned", (int)is);
    if (((uintptr_t)out & (os - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)os);
    return SDDC_OK;
}

// The call in runs of at most run_blocks full blocks, each three launches on s.  A run reads the
// current state buffer and writes the other one, so it runs after every earlier launch of the handle,
// whatever its stream; the buffers swap and the position advances once a run is enqueued.
static int chaud_launch(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride, void *d_out,
                        size_t out_stride, hipStream_t s)
{
    ChannelAudio &st = h->chaud;
    const size_t B = SDDC_DDC_AUDIO_BLOCK, run_blocks = (size_t)(st.run_blocks > 0 ? st.run_blocks : ChannelAudio::kDefaultRunBlocks);
    const size_t blocks = sddc::channel_audio_blocks((unsigned)(st.pos % B), nsamp);
    const size_t need = (size_t)nch * 2 * (size_t)st.nsec * (blocks < run_blocks ? blocks : run_blocks);
    if (need > st.scratch_cap) {
        HIP_TRY(st.readers.sync());   // an earlier launch may still use the scratch
        if (int rc = grow_device_buffer(&st.d_scratch, &st.scratch_cap, need, "channel audio filter", "scratch floats")) return rc;
    }
    HIP_TRY(st.readers.order_before(s));
    const size_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    hipError_t e = hipSuccess;
    for (size_t done = 0; done < nsamp && e == hipSuccess;) {
        // a run ends at a block boundary of the stream, run_blocks full blocks after its head
        const unsigned bp = (unsigned)(st.pos % B);
        const size_t head = (B - bp) % B;
        size_t n = nsamp - done;
        if (n > head + run_blocks * B) n = head + run_blocks * B;
        e = sddc::launch_channel_audio(h->tables, static_cast<const char *>(d_in) + done * is, st.in_fmt == SDDC_DDC_AUDIO_S16,
                                       nch, st.nsec, n, in_stride, bp, st.d_coef, st.d_mat, st.d_state[st.cur],
                                       st.d_state[st.cur ^ 1], st.d_scratch, static_cast<char *>(d_out) + done * os,
                                       st.out_fmt == SDDC_DDC_AUDIO_S16, out_stride, st.max_wgs, h->device, s);
        if (e != hipSuccess) break;
        st.cur ^= 1;
        st.pos += n;
        done += n;
    }
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_audio_filter_device(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride,
                                         void *d_out, size_t out_stride, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_audio_filter_device: a CPU handle has no device path");
    if (int rc = check_chaud_args(h, d_in, nch, nsamp, in_stride, d_out, out_stride)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chaud_launch(h, d_in, nch, nsamp, in_stride, d_out, out_stride, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_audio_filter_host(sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, void *out,
                                       size_t out_stride)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chaud_args(h, in, nch, nsamp, in_stride, out, out_stride)) return rc;
    ChannelAudio &st = h->chaud;
    const bool in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_audio_filter(in, in16, nch, st.nsec, nsamp, nch > 1 ? in_stride : 0, st.coef.data(),
                                              st.mat.data(), (unsigned)(st.pos % SDDC_DDC_AUDIO_BLOCK), st.state_h.data(),
                                              out, out16, nch > 1 ? out_stride : 0);
        st.pos += nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs
    const size_t is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const size_t out_bytes = ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_audio_filter_host", "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes, "channel_audio_filter_host", "output bytes")) return rc;
    HIP_TRY(hipMemcpyAsync(st.d_in, in, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chaud_launch(h, st.d_in, nch, nsamp, in_stride, st.d_out, out_stride, h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        if (nch == 1 || out_stride == nsamp)
            HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, out_stride * os, st.d_out, out_stride * os, nsamp * os, (size_t)nch,
                                     hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel AGC: a streaming peak AGC per channel in max-plus block form ------------------- */
int sddc_ddc_agc_decay(double tau_samples, float *decay)
{
    if (!decay) return fail(SDDC_ERR_ARG, "agc_decay: null decay");
    if (!std::isfinite(tau_samples) || !(tau_samples > 0.0))
        return fail(SDDC_ERR_ARG, "agc_decay: tau %g is not a positive finite number of samples", tau_samples);
    float d = (float)std::exp(-1.0 / tau_samples);
    if (!(d < 1.f)) d = 0.99999994f;   // 1 - 2^-24, the largest valid factor
    *decay = d;
    return SDDC_OK;
}

/* internal: the stream position, the envelopes left as they are */
int sddc_ddc_internal_chagc_set_position(sddc_ddc_t *h, uint64_t pos)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->chagc.par.empty()) return fail(SDDC_ERR_STATE, "chagc set position: no AGC set");
    h->chagc.pos = pos;   // host state: a launch in flight has its own copy
    return SDDC_OK;
}

int sddc_ddc_set_channel_agc(sddc_ddc_t *h, const float *params, int nch, int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !params || nch == 0;
    std::vector<float> par;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel AGC: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        for (int fmt : {in_format, out_format})
            if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
                return fail(SDDC_ERR_ARG, "channel AGC: unknown sample format %d", fmt);
        const float lo = 8.6736173798840355e-19f, hi = 1152921504606846976.f;   // 2^-60, 2^60
        for (int c = 0; c < nch; c++) {
            const float T = params[3 * c], d = params[3 * c + 1], F = params[3 * c + 2];
            if (!std::isfinite(T) || !std::isfinite(d) || !std::isfinite(F))
                return fail(SDDC_ERR_ARG, "channel AGC: a parameter of channel %d is not finite", c);
            if (!(T == 0.f || (T >= lo && T <= hi)))
                return fail(SDDC_ERR_ARG, "channel AGC: the target %g of channel %d is neither 0 nor in [2^-60, 2^60]", (double)T, c);
            if (!(F >= lo && F <= hi))
                return fail(SDDC_ERR_ARG, "channel AGC: the floor %g of channel %d is outside [2^-60, 2^60]", (double)F, c);
            if (!(d >= 0.f && d < 1.f))
                return fail(SDDC_ERR_ARG, "channel AGC: the release factor %g of channel %d is outside [0, 1)", (double)d, c);
        }
        try {
            par.resize((size_t)nch * sddc::agc::kAgcParams);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel AGC: %s", ex.what());
        }
        for (int c = 0; c < nch; c++) {
            float *p = par.data() + (size_t)c * sddc::agc::kAgcParams;
            p[0] = params[3 * c];
            p[1] = params[3 * c + 1];
            p[2] = params[3 * c + 2];
            p[3] = sddc::agc::agc_block_decay(p[1]);
        }
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelAgc &st = h->chagc;
    const size_t nstate = off ? 0 : (size_t)nch * 3;
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.state_h.assign(nstate, 0.f);
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel AGC: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the stage off
        if (off) return SDDC_OK;
        hipError_t e = hipMalloc(&st.d_par, par.size() * sizeof(float));
        for (float *&p : st.d_state)
            if (e == hipSuccess) e = hipMalloc(&p, nstate * sizeof(float));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel AGC: no device memory for %d channels", nch);
        }
        e = hipMemcpy(st.d_par, par.data(), par.size() * sizeof(float), hipMemcpyHostToDevice);
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        if (e == hipSuccess) e = hipMemsetAsync(st.d_state[0], 0, nstate * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.par = std::move(par);
    st.nch = nch;
    st.in_fmt = in_format;
    st.out_fmt = out_format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_agc_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelAgc &st = h->chagc;
    if (st.par.empty()) return fail(SDDC_ERR_STATE, "channel AGC reset: no AGC set");
    if (h->cpu) {
        std::fill(st.state_h.begin(), st.state_h.end(), 0.f);
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        HIP_TRY(hipMemsetAsync(st.d_state[st.cur], 0, st.state_floats() * sizeof(float), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

// the checks both calls share (under h->mu)
static int check_chagc_args(const sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, const void *out,
                            size_t out_stride)
{
    const ChannelAgc &st = h->chagc;
    if (st.par.empty()) return fail(SDDC_ERR_STATE, "channel AGC: no AGC set");
    if (nch != st.nch) return fail(SDDC_ERR_STATE, "channel AGC: the AGC is set for %d channels, the call has %d", st.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (nch > 1 && in_stride < nsamp) return fail(SDDC_ERR_ARG, "in_stride must be >= nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < nsamp)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    if (!in || !out) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)in & (is - 1)) != 0) return fail(SDDC_ERR_ARG, "the input must be %d-byte aligned", (int)is);
    if (((uintptr_t)out & (os - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)os);
    return SDDC_OK;
}

// The call in runs of at most run_blocks full blocks, each three launches on s, as chaud_launch; the
// last run writes d_env.
static int chagc_launch(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride, void *d_out,
                        size_t out_stride, float *d_env, hipStream_t s)
{
    ChannelAgc &st = h->chagc;
    const size_t B = SDDC_DDC_AGC_BLOCK, run_blocks = (size_t)(st.run_blocks > 0 ? st.run_blocks : ChannelAgc::kDefaultRunBlocks);
    const size_t blocks = sddc::channel_audio_blocks((unsigned)(st.pos % B), nsamp);
    const size_t need = (size_t)nch * (blocks < run_blocks ? blocks : run_blocks);
    if (need > st.scratch_cap) {
        HIP_TRY(st.readers.sync());   // an earlier launch may still use the scratch
        if (int rc = grow_device_buffer(&st.d_scratch, &st.scratch_cap, need, "channel AGC", "scratch floats")) return rc;
    }
    HIP_TRY(st.readers.order_before(s));
    const size_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    hipError_t e = hipSuccess;
    for (size_t done = 0; done < nsamp && e == hipSuccess;) {
        // a run ends at a block boundary of the stream, run_blocks full blocks after its head
        const unsigned bp = (unsigned)(st.pos % B);
        const size_t head = (B - bp) % B;
        size_t n = nsamp - done;
        if (n > head + run_blocks * B) n = head + run_blocks * B;
        e = sddc::launch_channel_agc(h->tables, static_cast<const char *>(d_in) + done * is, st.in_fmt == SDDC_DDC_AUDIO_S16,
                                     nch, n, in_stride, bp, st.d_par, st.d_state[st.cur], st.d_state[st.cur ^ 1],
                                     st.d_scratch, static_cast<char *>(d_out) + done * os, st.out_fmt == SDDC_DDC_AUDIO_S16,
                                     out_stride, done + n == nsamp ? d_env : nullptr, st.max_wgs, h->device, s);
        if (e != hipSuccess) break;
        st.cur ^= 1;
        st.pos += n;
        done += n;
    }
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_agc_device(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride, void *d_out,
                                size_t out_stride, float *d_env, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_agc_device: a CPU handle has no device path");
    if (int rc = check_chagc_args(h, d_in, nch, nsamp, in_stride, d_out, out_stride)) return rc;
    if (((uintptr_t)d_env & 3) != 0) return fail(SDDC_ERR_ARG, "d_env must be 4-byte aligned");
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chagc_launch(h, d_in, nch, nsamp, in_stride, d_out, out_stride, d_env, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_agc_host(sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, void *out,
                              size_t out_stride, float *env)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chagc_args(h, in, nch, nsamp, in_stride, out, out_stride)) return rc;
    ChannelAgc &st = h->chagc;
    const bool in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_agc(in, in16, nch, nsamp, nch > 1 ? in_stride : 0, st.par.data(),
                                     (unsigned)(st.pos % SDDC_DDC_AGC_BLOCK), st.state_h.data(), out, out16,
                                     nch > 1 ? out_stride : 0, env);
        st.pos += nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs
    const size_t is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const size_t out_bytes = ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_agc_host", "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes, "channel_agc_host", "output bytes")) return rc;
    if (env)
        if (int rc = grow_device_buffer(&st.d_env, &st.env_cap, (size_t)nch, "channel_agc_host", "envelopes")) return rc;
    HIP_TRY(hipMemcpyAsync(st.d_in, in, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chagc_launch(h, st.d_in, nch, nsamp, in_stride, st.d_out, out_stride, env ? st.d_env : nullptr, h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        if (nch == 1 || out_stride == nsamp)
            HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, out_stride * os, st.d_out, out_stride * os, nsamp * os, (size_t)nch,
                                     hipMemcpyDeviceToHost, h->stream));
        if (env) HIP_TRY(hipMemcpyAsync(env, st.d_env, (size_t)nch * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel noise blanker: a streaming per-channel impulse blanker on IQ -------------------- */
static_assert(SDDC_DDC_BLANKER_BLOCK == sddc::blank::kBlankBlock && SDDC_DDC_BLANKER_MAX_GUARD == sddc::blank::kBlankMaxGuard &&
                  SDDC_DDC_BLANKER_MAX_REF_BLOCKS == sddc::blank::kBlankMaxRef && SDDC_DDC_BLANKER_MEAN == sddc::blank::kBlankMean &&
                  SDDC_DDC_BLANKER_MEDIAN == sddc::blank::kBlankMedian,
              "the arithmetic header's constants are the ABI's");

int sddc_ddc_blanker_threshold(double db, float *k2)
{
    if (!k2) return fail(SDDC_ERR_ARG, "blanker_threshold: null k2");
    if (!std::isfinite(db) || db < 0.0 || db > 120.0)
        return fail(SDDC_ERR_ARG, "blanker_threshold: %g dB is outside 0..120", db);
    *k2 = (float)std::pow(10.0, db / 10.0);
    return SDDC_OK;
}

int sddc_ddc_set_channel_blanker(sddc_ddc_t *h, const float *params, int nch, int guard, int ref_blocks, int ref_mode,
                                 int format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !params || nch == 0;
    std::vector<float> par;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel blanker: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        if (guard < 0 || guard > SDDC_DDC_BLANKER_MAX_GUARD)
            return fail(SDDC_ERR_ARG, "channel blanker: guard %d outside 0..%d", guard, SDDC_DDC_BLANKER_MAX_GUARD);
        if (ref_blocks < 1 || ref_blocks > SDDC_DDC_BLANKER_MAX_REF_BLOCKS)
            return fail(SDDC_ERR_ARG, "channel blanker: ref_blocks %d outside 1..%d", ref_blocks, SDDC_DDC_BLANKER_MAX_REF_BLOCKS);
        if (ref_mode != SDDC_DDC_BLANKER_MEAN && ref_mode != SDDC_DDC_BLANKER_MEDIAN)
            return fail(SDDC_ERR_ARG, "channel blanker: unknown reference mode %d", ref_mode);
        if (format != SDDC_DDC_FMT_CF32 && format != SDDC_DDC_FMT_CS16)
            return fail(SDDC_ERR_ARG, "channel blanker: unknown sample format %d", format);
        const float k2max = 1099511627776.f, qmax = 1208925819614629174706176.f;   // 2^40, 2^80
        for (int c = 0; c < nch; c++) {
            const float k2 = params[2 * c], qmin = params[2 * c + 1];
            if (!std::isfinite(k2) || !std::isfinite(qmin))
                return fail(SDDC_ERR_ARG, "channel blanker: a parameter of channel %d is not finite", c);
            if (!(k2 == 0.f || (k2 >= 1.f && k2 <= k2max)))
                return fail(SDDC_ERR_ARG, "channel blanker: the threshold %g of channel %d is neither 0 nor in [1, 2^40]", (double)k2, c);
            if (!(qmin >= 0.f && qmin <= qmax))
                return fail(SDDC_ERR_ARG, "channel blanker: the floor %g of channel %d is outside [0, 2^80]", (double)qmin, c);
        }
        try {
            par.resize((size_t)nch * 2);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel blanker: %s", ex.what());
        }
        for (int c = 0; c < nch; c++) {
            par[2 * c] = sddc::blank::blank_thr(params[2 * c]);
            par[2 * c + 1] = params[2 * c + 1] == 0.f ? 0.f : params[2 * c + 1];   // -0 as +0
        }
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelBlanker &st = h->chnb;
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.state_h.assign((size_t)nch, sddc::cpu::R2iq::BlankerChannel());
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel blanker: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the stage off
        if (off) return SDDC_OK;
        const size_t nstate = (size_t)nch * sddc::kBlankStateWords;
        hipError_t e = hipMalloc(&st.d_par, par.size() * sizeof(float));
        for (uint32_t *&p : st.d_state)
            if (e == hipSuccess) e = hipMalloc(&p, nstate * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel blanker: no device memory for %d channels", nch);
        }
        e = hipMemcpy(st.d_par, par.data(), par.size() * sizeof(float), hipMemcpyHostToDevice);
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        for (uint32_t *p : st.d_state)
            if (e == hipSuccess) e = hipMemsetAsync(p, 0, nstate * sizeof(uint32_t), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.par = std::move(par);
    st.nch = nch;
    st.guard = guard;
    st.ref_blocks = ref_blocks;
    st.ref_mode = ref_mode;
    st.fmt = format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_blanker_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelBlanker &st = h->chnb;
    if (st.par.empty()) return fail(SDDC_ERR_STATE, "channel blanker reset: no blanker set");
    if (h->cpu) {
        std::fill(st.state_h.begin(), st.state_h.end(), sddc::cpu::R2iq::BlankerChannel());
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        HIP_TRY(hipMemsetAsync(st.d_state[st.cur], 0, st.state_words() * sizeof(uint32_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

// the checks both calls share (under h->mu)
static int check_chnb_args(const sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, const void *out,
                           size_t out_stride, const uint32_t *count)
{
    const ChannelBlanker &st = h->chnb;
    if (st.par.empty()) return fail(SDDC_ERR_STATE, "channel blanker: no blanker set");
    if (nch != st.nch)
        return fail(SDDC_ERR_STATE, "channel blanker: the blanker is set for %d channels, the call has %d", st.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (nch > 1 && (in_stride < 2 * nsamp || (in_stride & 1) != 0))
        return fail(SDDC_ERR_ARG, "in_stride must be even and >= 2 nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && (out_stride < 2 * nsamp || (out_stride & 1) != 0))
        return fail(SDDC_ERR_ARG, "out_stride must be even and >= 2 nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    if (!iq || !out) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t comp = st.fmt == SDDC_DDC_FMT_CS16 ? 2 : 4, sample = 2 * comp;
    if (((uintptr_t)iq & (sample - 1)) != 0) return fail(SDDC_ERR_ARG, "iq must be %d-byte aligned", (int)sample);
    if (((uintptr_t)out & (sample - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)sample);
    if (((uintptr_t)count & 3) != 0) return fail(SDDC_ERR_ARG, "the counts must be 4-byte aligned");
    // the spans from the first channel's first sample to the last channel's last one
    const uintptr_t ia = (uintptr_t)iq, oa = (uintptr_t)out;
    const uintptr_t ib = ia + ((uintptr_t)(nch - 1) * (nch > 1 ? in_stride : 0) + 2 * nsamp) * comp;
    const uintptr_t ob = oa + ((uintptr_t)(nch - 1) * (nch > 1 ? out_stride : 0) + 2 * nsamp) * comp;
    if (ia < ob && oa < ib) return fail(SDDC_ERR_ARG, "the input and the output overlap");
    return SDDC_OK;
}

// The call in launches of at most kBlankMaxLaunch samples per channel (the kernels index a launch with
// an int), two kernels each on s.  d_count, if given, is zeroed first and every launch adds to it.
static int chnb_launch(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride, void *d_out,
                       size_t out_stride, uint32_t *d_count, hipStream_t s)
{
    ChannelBlanker &st = h->chnb;
    HIP_TRY(st.readers.order_before(s));
    const bool cs16 = st.fmt == SDDC_DDC_FMT_CS16;
    const size_t sample = cs16 ? 4 : 8;
    hipError_t e = hipSuccess;
    if (d_count) e = hipMemsetAsync(d_count, 0, (size_t)nch * sizeof(uint32_t), s);
    for (size_t done = 0; done < nsamp && e == hipSuccess;) {
        size_t n = nsamp - done;
        if (n > sddc::kBlankMaxLaunch) n = sddc::kBlankMaxLaunch;
        e = sddc::launch_channel_blank(h->tables, static_cast<const char *>(d_iq) + done * sample, cs16, nch, n, in_stride,
                                       st.pos, st.d_par, st.guard, st.ref_blocks, st.ref_mode, st.d_state[st.cur],
                                       st.d_state[st.cur ^ 1], static_cast<char *>(d_out) + done * sample, out_stride,
                                       d_count, st.max_wgs, st.run_blocks, h->device, s);
        if (e != hipSuccess) break;
        st.cur ^= 1;
        st.pos += n;
        done += n;
    }
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_blank_device(sddc_ddc_t *h, const void *d_iq, int nch, size_t nsamp, size_t in_stride, void *d_out,
                                  size_t out_stride, uint32_t *d_count, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_blank_device: a CPU handle has no device path");
    if (int rc = check_chnb_args(h, d_iq, nch, nsamp, in_stride, d_out, out_stride, d_count)) return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chnb_launch(h, d_iq, nch, nsamp, in_stride, d_out, out_stride, d_count, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_blank_host(sddc_ddc_t *h, const void *iq, int nch, size_t nsamp, size_t in_stride, void *out,
                                size_t out_stride, uint32_t *count)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chnb_args(h, iq, nch, nsamp, in_stride, out, out_stride, count)) return rc;
    ChannelBlanker &st = h->chnb;
    const bool cs16 = st.fmt == SDDC_DDC_FMT_CS16;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_blank(iq, cs16, nch, nsamp, nch > 1 ? in_stride : 0, st.par.data(), st.guard, st.ref_blocks,
                                       st.ref_mode, st.pos, st.state_h.data(), out, nch > 1 ? out_stride : 0, count);
        st.pos += nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs
    const size_t comp = cs16 ? 2 : 4;
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + 2 * nsamp) * comp;
    const size_t out_bytes = ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + 2 * nsamp) * comp;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_blank_host", "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes, "channel_blank_host", "output bytes")) return rc;
    if (count)
        if (int rc = grow_device_buffer(&st.d_count, &st.count_cap, (size_t)nch, "channel_blank_host", "counters")) return rc;
    HIP_TRY(hipMemcpyAsync(st.d_in, iq, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chnb_launch(h, st.d_in, nch, nsamp, in_stride, st.d_out, out_stride, count ? st.d_count : nullptr, h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        if (nch == 1 || out_stride == 2 * nsamp)
            HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, out_stride * comp, st.d_out, out_stride * comp, 2 * nsamp * comp, (size_t)nch,
                                     hipMemcpyDeviceToHost, h->stream));
        if (count) HIP_TRY(hipMemcpyAsync(count, st.d_count, (size_t)nch * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel squelch: a streaming per-channel gate on the audio ------------------------------ */
static_assert(SDDC_DDC_SQUELCH_BLOCK == sddc::squelch::kSquelchBlock && SDDC_DDC_SQUELCH_OFF == sddc::squelch::kSquelchOff &&
                  SDDC_DDC_SQUELCH_LEVEL == sddc::squelch::kSquelchLevel && SDDC_DDC_SQUELCH_NOISE == sddc::squelch::kSquelchNoise &&
                  SDDC_DDC_SQUELCH_MUTE == sddc::squelch::kSquelchMute && SDDC_DDC_SQUELCH_SENSE_SELF == sddc::squelch::kSenseSelf &&
                  SDDC_DDC_SQUELCH_SENSE_F32 == sddc::squelch::kSenseF32 && SDDC_DDC_SQUELCH_SENSE_S16 == sddc::squelch::kSenseS16 &&
                  SDDC_DDC_SQUELCH_SENSE_CF32 == sddc::squelch::kSenseCF32 && SDDC_DDC_SQUELCH_SENSE_CS16 == sddc::squelch::kSenseCS16 &&
                  SDDC_DDC_SQUELCH_MAX_ATTACK == sddc::squelch::kSquelchMaxAttack &&
                  SDDC_DDC_SQUELCH_MAX_HANG == sddc::squelch::kSquelchMaxHang,
              "the arithmetic header's constants are the ABI's");

int sddc_ddc_squelch_blocks(double seconds, double fs, int *blocks)
{
    if (!blocks) return fail(SDDC_ERR_ARG, "squelch_blocks: null blocks");
    if (!std::isfinite(seconds) || !std::isfinite(fs) || !(fs > 0.0))
        return fail(SDDC_ERR_ARG, "squelch_blocks: %g s at %g Hz is not a finite time at a positive rate", seconds, fs);
    const double b = std::nearbyint(seconds * fs / (double)SDDC_DDC_SQUELCH_BLOCK);
    if (!(b >= 0.0 && b <= (double)SDDC_DDC_SQUELCH_MAX_HANG))
        return fail(SDDC_ERR_ARG, "squelch_blocks: %g s at %g Hz is %g blocks, outside 0..%d", seconds, fs, b,
                    SDDC_DDC_SQUELCH_MAX_HANG);
    *blocks = (int)b;
    return SDDC_OK;
}

int sddc_ddc_set_channel_squelch(sddc_ddc_t *h, const int *modes, const float *thresholds, int nch, int attack, int hang,
                                 int fade, int sense, int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !modes || !thresholds || nch == 0;
    std::vector<int> md;
    std::vector<float> thr;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel squelch: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        if (attack < 1 || attack > SDDC_DDC_SQUELCH_MAX_ATTACK)
            return fail(SDDC_ERR_ARG, "channel squelch: attack %d outside 1..%d blocks", attack, SDDC_DDC_SQUELCH_MAX_ATTACK);
        if (hang < 0 || hang > SDDC_DDC_SQUELCH_MAX_HANG)
            return fail(SDDC_ERR_ARG, "channel squelch: hang %d outside 0..%d blocks", hang, SDDC_DDC_SQUELCH_MAX_HANG);
        if (fade != 0 && fade != 1) return fail(SDDC_ERR_ARG, "channel squelch: fade %d is neither 0 nor 1", fade);
        if (sense < SDDC_DDC_SQUELCH_SENSE_SELF || sense > SDDC_DDC_SQUELCH_SENSE_CS16)
            return fail(SDDC_ERR_ARG, "channel squelch: unknown sense kind %d", sense);
        for (int fmt : {in_format, out_format})
            if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
                return fail(SDDC_ERR_ARG, "channel squelch: unknown sample format %d", fmt);
        const float tmax = 1208925819614629174706176.f;   // 2^80
        for (int c = 0; c < nch; c++) {
            const int m = modes[c];
            const float to = thresholds[2 * c], tc = thresholds[2 * c + 1];
            if (m < SDDC_DDC_SQUELCH_OFF || m > SDDC_DDC_SQUELCH_MUTE)
                return fail(SDDC_ERR_ARG, "channel squelch: unknown mode %d of channel %d", m, c);
            if (!std::isfinite(to) || !std::isfinite(tc) || !(to >= 0.f && to <= tmax) || !(tc >= 0.f && tc <= tmax))
                return fail(SDDC_ERR_ARG, "channel squelch: a threshold of channel %d is not a finite value in [0, 2^80]", c);
            if (m == SDDC_DDC_SQUELCH_LEVEL && !(tc <= to))
                return fail(SDDC_ERR_ARG, "channel squelch: LEVEL channel %d has T_close %g above T_open %g", c, (double)tc, (double)to);
            if (m == SDDC_DDC_SQUELCH_NOISE && !(tc >= to))
                return fail(SDDC_ERR_ARG, "channel squelch: NOISE channel %d has T_close %g below T_open %g", c, (double)tc, (double)to);
        }
        try {
            md.assign(modes, modes + nch);
            thr.resize((size_t)nch * 2);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel squelch: %s", ex.what());
        }
        for (size_t i = 0; i < thr.size(); i++) thr[i] = sddc::squelch::squelch_scale(thresholds[i] == 0.f ? 0.f : thresholds[i]);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelSquelch &st = h->chsq;
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.state_h.assign((size_t)nch, sddc::cpu::R2iq::SquelchChannel());
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel squelch: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the stage off
        if (off) return SDDC_OK;
        const size_t nstate = (size_t)nch * sddc::kSquelchStateWords;
        hipError_t e = hipMalloc(&st.d_modes, md.size() * sizeof(int));
        if (e == hipSuccess) e = hipMalloc(&st.d_thr, thr.size() * sizeof(float));
        for (uint32_t *&p : st.d_state)
            if (e == hipSuccess) e = hipMalloc(&p, nstate * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel squelch: no device memory for %d channels", nch);
        }
        e = hipMemcpy(st.d_modes, md.data(), md.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(st.d_thr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice);
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        for (uint32_t *p : st.d_state)
            if (e == hipSuccess) e = hipMemsetAsync(p, 0, nstate * sizeof(uint32_t), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.modes = std::move(md);
    st.thr = std::move(thr);
    st.nch = nch;
    st.attack = attack;
    st.hang = hang;
    st.fade = fade;
    st.sense = sense;
    st.in_fmt = in_format;
    st.out_fmt = out_format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_squelch_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelSquelch &st = h->chsq;
    if (st.modes.empty()) return fail(SDDC_ERR_STATE, "channel squelch reset: no squelch set");
    if (h->cpu) {
        std::fill(st.state_h.begin(), st.state_h.end(), sddc::cpu::R2iq::SquelchChannel());
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        HIP_TRY(hipMemsetAsync(st.d_state[st.cur], 0, st.state_words() * sizeof(uint32_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

namespace {
// the bytes of a sense sample (SELF: 0) and the components per sample
struct SenseShape {
    size_t comp, per;
};
SenseShape sense_shape(int kind)
{
    switch (kind) {
    case SDDC_DDC_SQUELCH_SENSE_F32: return {4, 1};
    case SDDC_DDC_SQUELCH_SENSE_S16: return {2, 1};
    case SDDC_DDC_SQUELCH_SENSE_CF32: return {4, 2};
    case SDDC_DDC_SQUELCH_SENSE_CS16: return {2, 2};
    default: return {0, 1};
    }
}
}  // namespace

// the checks both calls share (under h->mu)
static int check_chsq_args(const sddc_ddc_t *h, const void *in, const void *sense, int nch, size_t nsamp, size_t in_stride,
                           size_t sense_stride, const void *out, size_t out_stride, const void *open, const void *count,
                           const void *level)
{
    const ChannelSquelch &st = h->chsq;
    if (st.modes.empty()) return fail(SDDC_ERR_STATE, "channel squelch: no squelch set");
    if (nch != st.nch)
        return fail(SDDC_ERR_STATE, "channel squelch: the squelch is set for %d channels, the call has %d", st.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (nch > 1 && in_stride < nsamp) return fail(SDDC_ERR_ARG, "in_stride must be >= nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < nsamp)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    if (!in || !out) return fail(SDDC_ERR_ARG, "null buffer");
    const uintptr_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)in & (is - 1)) != 0) return fail(SDDC_ERR_ARG, "the input must be %d-byte aligned", (int)is);
    if (((uintptr_t)out & (os - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)os);
    if ((((uintptr_t)open | (uintptr_t)count | (uintptr_t)level) & 3) != 0)
        return fail(SDDC_ERR_ARG, "the side outputs must be 4-byte aligned");
    const uintptr_t ia = (uintptr_t)in, oa = (uintptr_t)out;
    const uintptr_t ib = ia + ((uintptr_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const uintptr_t ob = oa + ((uintptr_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os;
    if (ia < ob && oa < ib) return fail(SDDC_ERR_ARG, "the input and the output overlap");
    if (st.sense != SDDC_DDC_SQUELCH_SENSE_SELF) {
        const SenseShape sh = sense_shape(st.sense);
        if (!sense) return fail(SDDC_ERR_ARG, "null sense buffer with a sense kind other than SELF");
        if (nch > 1 && (sense_stride < sh.per * nsamp || (sense_stride & (sh.per - 1)) != 0))
            return fail(SDDC_ERR_ARG, "sense_stride must be %s>= %zu (got %zu)", sh.per == 2 ? "even and " : "", sh.per * nsamp,
                        sense_stride);
        if (((uintptr_t)sense & (sh.comp * sh.per - 1)) != 0)
            return fail(SDDC_ERR_ARG, "the sense buffer must be %d-byte aligned", (int)(sh.comp * sh.per));
        const uintptr_t sa = (uintptr_t)sense;
        const uintptr_t sb = sa + ((uintptr_t)(nch - 1) * (nch > 1 ? sense_stride : 0) + sh.per * nsamp) * sh.comp;
        if (sa < ob && oa < sb) return fail(SDDC_ERR_ARG, "the sense buffer and the output overlap");
    }
    return SDDC_OK;
}

// The call in launch sets of at most run_blocks blocks per channel (the scratch holds a word per channel
// and block of a set, and the kernels index a set with an int), three kernels each on s.
static int chsq_launch(sddc_ddc_t *h, const void *d_in, const void *d_sense, int nch, size_t nsamp, size_t in_stride,
                       size_t sense_stride, void *d_out, size_t out_stride, uint32_t *d_open, uint32_t *d_count, float *d_level,
                       hipStream_t s)
{
    ChannelSquelch &st = h->chsq;
    const size_t B = SDDC_DDC_SQUELCH_BLOCK, run_blocks = (size_t)(st.run_blocks > 0 ? st.run_blocks : ChannelSquelch::kDefaultRunBlocks);
    const size_t hb0 = (size_t)(st.pos % B), blocks = (hb0 + nsamp + B - 1) / B;
    const size_t need = (size_t)nch * (blocks < run_blocks ? blocks : run_blocks);
    if (need > st.words_cap) {
        HIP_TRY(st.readers.sync());   // an earlier launch may still use the scratch
        if (int rc = grow_device_buffer(&st.d_words, &st.words_cap, need, "channel squelch", "scratch words")) return rc;
    }
    HIP_TRY(st.readers.order_before(s));
    const bool in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    const size_t is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const SenseShape sh = sense_shape(st.sense);
    hipError_t e = hipSuccess;
    for (size_t done = 0; done < nsamp && e == hipSuccess;) {
        const size_t hb = (size_t)(st.pos % B);
        size_t n = nsamp - done;
        if (n > run_blocks * B - hb) n = run_blocks * B - hb;
        e = sddc::launch_channel_squelch(h->tables, static_cast<const char *>(d_in) + done * is, in16,
                                         d_sense ? static_cast<const char *>(d_sense) + done * sh.per * sh.comp : nullptr, st.sense,
                                         nch, n, in_stride, sense_stride, st.pos, st.d_modes, st.d_thr, st.attack, st.hang, st.fade,
                                         st.d_state[st.cur], st.d_state[st.cur ^ 1], st.d_words,
                                         static_cast<char *>(d_out) + done * os, out16, out_stride, d_open, d_count, d_level,
                                         done > 0, st.max_wgs, h->device, s);
        if (e != hipSuccess) break;
        st.cur ^= 1;
        st.pos += n;
        done += n;
    }
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_squelch_device(sddc_ddc_t *h, const void *d_audio, const void *d_sense, int nch, size_t nsamp,
                                    size_t in_stride, size_t sense_stride, void *d_out, size_t out_stride, uint32_t *d_open,
                                    uint32_t *d_count, float *d_level, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_squelch_device: a CPU handle has no device path");
    if (int rc = check_chsq_args(h, d_audio, d_sense, nch, nsamp, in_stride, sense_stride, d_out, out_stride, d_open, d_count, d_level))
        return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chsq_launch(h, d_audio, h->chsq.sense == SDDC_DDC_SQUELCH_SENSE_SELF ? nullptr : d_sense, nch, nsamp, in_stride,
                       sense_stride, d_out, out_stride, d_open, d_count, d_level, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_squelch_host(sddc_ddc_t *h, const void *audio, const void *sense, int nch, size_t nsamp,
                                  size_t in_stride, size_t sense_stride, void *out, size_t out_stride, uint32_t *open,
                                  uint32_t *count, float *level)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chsq_args(h, audio, sense, nch, nsamp, in_stride, sense_stride, out, out_stride, open, count, level)) return rc;
    ChannelSquelch &st = h->chsq;
    const bool in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    const bool self = st.sense == SDDC_DDC_SQUELCH_SENSE_SELF;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_squelch(audio, in16, self ? nullptr : sense, st.sense, nch, nsamp, nch > 1 ? in_stride : 0,
                                         nch > 1 ? sense_stride : 0, st.modes.data(), st.thr.data(), st.attack, st.hang, st.fade,
                                         st.pos, st.state_h.data(), out, out16, nch > 1 ? out_stride : 0, open, count, level);
        st.pos += nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs
    const size_t is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const SenseShape sh = sense_shape(st.sense);
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const size_t out_bytes = ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os;
    const size_t sense_bytes = self ? 0 : ((size_t)(nch - 1) * (nch > 1 ? sense_stride : 0) + sh.per * nsamp) * sh.comp;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_squelch_host", "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes, "channel_squelch_host", "output bytes")) return rc;
    if (!self)
        if (int rc = grow_device_buffer(&st.d_sense, &st.sense_cap, sense_bytes, "channel_squelch_host", "sense bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_side, &st.side_cap, (size_t)3 * nch, "channel_squelch_host", "side outputs")) return rc;
    uint32_t *d_open = open ? st.d_side : nullptr, *d_count = count ? st.d_side + nch : nullptr;
    float *d_level = level ? reinterpret_cast<float *>(st.d_side + 2 * (size_t)nch) : nullptr;
    HIP_TRY(hipMemcpyAsync(st.d_in, audio, in_bytes, hipMemcpyHostToDevice, h->stream));
    if (!self) HIP_TRY(hipMemcpyAsync(st.d_sense, sense, sense_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chsq_launch(h, st.d_in, self ? nullptr : st.d_sense, nch, nsamp, in_stride, sense_stride, st.d_out, out_stride,
                               d_open, d_count, d_level, h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        if (nch == 1 || out_stride == nsamp)
            HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, out_stride * os, st.d_out, out_stride * os, nsamp * os, (size_t)nch,
                                     hipMemcpyDeviceToHost, h->stream));
        if (open) HIP_TRY(hipMemcpyAsync(open, d_open, (size_t)nch * 4, hipMemcpyDeviceToHost, h->stream));
        if (count) HIP_TRY(hipMemcpyAsync(count, d_count, (size_t)nch * 4, hipMemcpyDeviceToHost, h->stream));
        if (level) HIP_TRY(hipMemcpyAsync(level, d_level, (size_t)nch * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel tone detector: streaming per-channel CTCSS / tone squelch ------------------------- */
static_assert(SDDC_DDC_TONE_BLOCK == sddc::tone::kToneBlock && SDDC_DDC_TONE_MAX_TONES == sddc::tone::kToneMaxTones &&
                  SDDC_DDC_TONE_MAX_WINDOW == sddc::tone::kToneMaxWindow && SDDC_DDC_TONE_MAX_ATTACK == sddc::tone::kToneMaxAttack &&
                  SDDC_DDC_TONE_MAX_HANG == sddc::tone::kToneMaxHang,
              "the arithmetic header's constants are the ABI's");
static_assert(sizeof(sddc::cpu::R2iq::ToneChannel) == (size_t)sddc::kToneStateWords * 4, "the CPU state holds what the device's does");

int sddc_ddc_tone_window(double seconds, double fs, int *blocks)
{
    if (!blocks) return fail(SDDC_ERR_ARG, "tone_window: null blocks");
    if (!std::isfinite(seconds) || !std::isfinite(fs) || !(fs > 0.0) || !(seconds >= 0.0))
        return fail(SDDC_ERR_ARG, "tone_window: %g s at %g Hz is not a finite time >= 0 at a positive rate", seconds, fs);
    double b = std::nearbyint(seconds * fs / (double)SDDC_DDC_TONE_BLOCK);
    if (b < 1.0) b = 1.0;
    if (!(b <= (double)SDDC_DDC_TONE_MAX_WINDOW))
        return fail(SDDC_ERR_ARG, "tone_window: %g s at %g Hz is %g blocks, above %d", seconds, fs, b, SDDC_DDC_TONE_MAX_WINDOW);
    *blocks = (int)b;
    return SDDC_OK;
}

int sddc_ddc_set_channel_tone_detector(sddc_ddc_t *h, const uint32_t *words, int ntones, const uint64_t *masks,
                                       const float *thresholds, int nch, int window, int attack, int hang, int sense_format,
                                       int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !words || !masks || !thresholds || nch == 0;
    std::vector<uint32_t> wd;
    std::vector<uint64_t> mk;
    std::vector<float> thr;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel tone detector: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        if (ntones < 1 || ntones > SDDC_DDC_TONE_MAX_TONES)
            return fail(SDDC_ERR_ARG, "channel tone detector: ntones %d outside 1..%d", ntones, SDDC_DDC_TONE_MAX_TONES);
        if (window < 1 || window > SDDC_DDC_TONE_MAX_WINDOW)
            return fail(SDDC_ERR_ARG, "channel tone detector: window %d outside 1..%d blocks", window, SDDC_DDC_TONE_MAX_WINDOW);
        if (attack < 1 || attack > SDDC_DDC_TONE_MAX_ATTACK)
            return fail(SDDC_ERR_ARG, "channel tone detector: attack %d outside 1..%d windows", attack, SDDC_DDC_TONE_MAX_ATTACK);
        if (hang < 0 || hang > SDDC_DDC_TONE_MAX_HANG)
            return fail(SDDC_ERR_ARG, "channel tone detector: hang %d outside 0..%d windows", hang, SDDC_DDC_TONE_MAX_HANG);
        for (int fmt : {sense_format, in_format, out_format})
            if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
                return fail(SDDC_ERR_ARG, "channel tone detector: unknown sample format %d", fmt);
        try {
            wd.assign(words, words + ntones);
            mk.assign(masks, masks + nch);
            thr.resize((size_t)nch * 3);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel tone detector: %s", ex.what());
        }
        for (int c = 0; c < nch; c++) {
            const float ro = thresholds[3 * c], rc = thresholds[3 * c + 1], em = thresholds[3 * c + 2];
            if (ntones < 64 && (masks[c] >> ntones) != 0)
                return fail(SDDC_ERR_ARG, "channel tone detector: the mask of channel %d has a bit at or above ntones = %d", c, ntones);
            if (!(ro > 0.f && ro <= 1.f) || !(rc > 0.f && rc <= 1.f))
                return fail(SDDC_ERR_ARG, "channel tone detector: rho_open %g or rho_close %g of channel %d is outside (0, 1]",
                            (double)ro, (double)rc, c);
            if (!(rc <= ro))
                return fail(SDDC_ERR_ARG, "channel tone detector: channel %d has rho_close %g above rho_open %g", c, (double)rc, (double)ro);
            thr[3 * (size_t)c] = sddc::tone::tone_scale(ro, window);
            thr[3 * (size_t)c + 1] = sddc::tone::tone_scale(rc, window);
            thr[3 * (size_t)c + 2] = sddc::tone::tone_scale(em == 0.f ? 0.f : em, window);
            if (!(em >= 0.f) || !std::isfinite(thr[3 * (size_t)c + 2]))
                return fail(SDDC_ERR_ARG, "channel tone detector: e_min %g of channel %d is not a value >= 0 with a finite 256 W e_min",
                            (double)em, c);
        }
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelTone &st = h->chtone;
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.state_h.assign((size_t)nch, sddc::cpu::R2iq::ToneChannel());
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel tone detector: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the stage off
        if (off) return SDDC_OK;
        const size_t nstate = (size_t)nch * sddc::kToneStateWords;
        hipError_t e = hipMalloc(&st.d_tones, wd.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&st.d_masks, mk.size() * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc(&st.d_thr, thr.size() * sizeof(float));
        for (uint32_t *&p : st.d_state)
            if (e == hipSuccess) e = hipMalloc(&p, nstate * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel tone detector: no device memory for %d channels", nch);
        }
        e = hipMemcpy(st.d_tones, wd.data(), wd.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(st.d_masks, mk.data(), mk.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(st.d_thr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice);
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        for (uint32_t *p : st.d_state)
            if (e == hipSuccess) e = hipMemsetAsync(p, 0, nstate * sizeof(uint32_t), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.words = std::move(wd);
    st.max_mask_tones = 0;
    for (uint64_t m : mk) st.max_mask_tones = std::max(st.max_mask_tones, __builtin_popcountll(m));
    st.masks = std::move(mk);
    st.thr = std::move(thr);
    st.nch = nch;
    st.ntones = ntones;
    st.window = window;
    st.attack = attack;
    st.hang = hang;
    st.sense_fmt = sense_format;
    st.in_fmt = in_format;
    st.out_fmt = out_format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_tone_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelTone &st = h->chtone;
    if (st.masks.empty()) return fail(SDDC_ERR_STATE, "channel tone reset: no detector set");
    if (h->cpu) {
        std::fill(st.state_h.begin(), st.state_h.end(), sddc::cpu::R2iq::ToneChannel());
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        HIP_TRY(hipMemsetAsync(st.d_state[st.cur], 0, st.state_words() * sizeof(uint32_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_internal_chtone_set_position(sddc_ddc_t *h, uint64_t pos)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelTone &st = h->chtone;
    if (st.masks.empty()) return fail(SDDC_ERR_STATE, "channel tone position: no detector set");
    if (pos % ((uint64_t)SDDC_DDC_TONE_BLOCK * (uint64_t)st.window) != 0)
        return fail(SDDC_ERR_ARG, "channel tone position: %llu is no multiple of 256 W = %d", (unsigned long long)pos,
                    SDDC_DDC_TONE_BLOCK * st.window);
    if (h->cpu) {
        for (auto &ch : st.state_h) {
            ch.E = 0.f;
            ch.bad = 0;
            std::fill(std::begin(ch.zr), std::end(ch.zr), 0.f);
            std::fill(std::begin(ch.zi), std::end(ch.zi), 0.f);
            std::fill(std::begin(ch.x), std::end(ch.x), 0.f);
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());
        // words 6 .. 135 of every channel: E, the bad flag, Zr and Zi (the stored block is not read at a block's start)
        HIP_TRY(hipMemset2DAsync(st.d_state[st.cur] + 6, (size_t)sddc::kToneStateWords * 4, 0, (size_t)130 * 4, (size_t)st.nch,
                                 h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    st.pos = pos;
    return SDDC_OK;
}

// the checks both calls share (under h->mu)
static int check_chtone_args(const sddc_ddc_t *h, const void *sense, size_t sense_stride, const void *in, int nch, size_t nsamp,
                             size_t in_stride, const void *out, size_t out_stride, const void *tone, const void *open,
                             const void *count, const void *level, const void *powers)
{
    const ChannelTone &st = h->chtone;
    if (st.masks.empty()) return fail(SDDC_ERR_STATE, "channel tone detector: no detector set");
    if (nch != st.nch)
        return fail(SDDC_ERR_STATE, "channel tone detector: the detector is set for %d channels, the call has %d", st.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (!sense) return fail(SDDC_ERR_ARG, "null sense buffer");
    if (nch > 1 && sense_stride < nsamp)
        return fail(SDDC_ERR_ARG, "sense_stride must be >= nsamp (got %zu, nsamp %zu)", sense_stride, nsamp);
    const uintptr_t ss = st.sense_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)sense & (ss - 1)) != 0) return fail(SDDC_ERR_ARG, "the sense buffer must be %d-byte aligned", (int)ss);
    if ((((uintptr_t)tone | (uintptr_t)open | (uintptr_t)count | (uintptr_t)level | (uintptr_t)powers) & 3) != 0)
        return fail(SDDC_ERR_ARG, "the side outputs must be 4-byte aligned");
    if (!in && out) return fail(SDDC_ERR_ARG, "an output without audio");
    if (in && !out) return fail(SDDC_ERR_ARG, "audio without an output");
    if (!in) return SDDC_OK;
    if (nch > 1 && in_stride < nsamp) return fail(SDDC_ERR_ARG, "in_stride must be >= nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < nsamp)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    const uintptr_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)in & (is - 1)) != 0) return fail(SDDC_ERR_ARG, "the input must be %d-byte aligned", (int)is);
    if (((uintptr_t)out & (os - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)os);
    const uintptr_t ia = (uintptr_t)in, oa = (uintptr_t)out, sa = (uintptr_t)sense;
    const uintptr_t ib = ia + ((uintptr_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const uintptr_t ob = oa + ((uintptr_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os;
    const uintptr_t sb = sa + ((uintptr_t)(nch - 1) * (nch > 1 ? sense_stride : 0) + nsamp) * ss;
    if (ia < ob && oa < ib) return fail(SDDC_ERR_ARG, "the input and the output overlap");
    if (sa < ob && oa < sb) return fail(SDDC_ERR_ARG, "the sense buffer and the output overlap");
    return SDDC_OK;
}

// The call in launch sets of at most run_blocks blocks per channel, rounded down to whole windows (the
// scratch holds four words per channel and window of a set, and the kernels index a set with an int).
static int chtone_launch(sddc_ddc_t *h, const void *d_sense, size_t sense_stride, const void *d_in, int nch, size_t nsamp,
                         size_t in_stride, void *d_out, size_t out_stride, int32_t *d_tone, uint32_t *d_open, uint32_t *d_count,
                         float *d_level, float *d_powers, hipStream_t s)
{
    ChannelTone &st = h->chtone;
    const size_t B = SDDC_DDC_TONE_BLOCK, W = (size_t)st.window, WB = W * B;
    const size_t run_blocks = (size_t)(st.run_blocks > 0 ? st.run_blocks : ChannelTone::kDefaultRunBlocks);
    const size_t run_windows = run_blocks / W > 0 ? run_blocks / W : 1;
    const size_t hs0 = (size_t)(st.pos % WB), windows = (hs0 + nsamp + WB - 1) / WB;
    const size_t need = (size_t)nch * (windows < run_windows ? windows : run_windows) * 4;
    if (need > st.scratch_cap) {
        HIP_TRY(st.readers.sync());   // an earlier launch may still use the scratch
        if (int rc = grow_device_buffer(&st.d_scratch, &st.scratch_cap, need, "channel tone detector", "scratch words")) return rc;
    }
    HIP_TRY(st.readers.order_before(s));
    const bool s16 = st.sense_fmt == SDDC_DDC_AUDIO_S16, in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    const size_t ss = s16 ? 2 : 4, is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    hipError_t e = hipSuccess;
    for (size_t done = 0; done < nsamp && e == hipSuccess;) {
        const size_t hs = (size_t)(st.pos % WB);
        size_t n = nsamp - done;
        if (n > run_windows * WB - hs) n = run_windows * WB - hs;
        e = sddc::launch_channel_tone(h->tables, static_cast<const char *>(d_sense) + done * ss, s16, sense_stride,
                                      d_in ? static_cast<const char *>(d_in) + done * is : nullptr, in16, nch, n, in_stride, st.pos,
                                      st.d_tones, st.ntones, st.d_masks, st.max_mask_tones, st.d_thr, st.window, st.attack, st.hang, st.d_state[st.cur],
                                      st.d_state[st.cur ^ 1], st.d_scratch, d_in ? static_cast<char *>(d_out) + done * os : nullptr,
                                      out16, out_stride, d_tone, d_open, d_count, d_level, d_powers, done > 0, st.max_wgs, h->device, s);
        if (e != hipSuccess) break;
        st.cur ^= 1;
        st.pos += n;
        done += n;
    }
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_tone_device(sddc_ddc_t *h, const void *d_sense, size_t sense_stride, const void *d_audio, int nch,
                                 size_t nsamp, size_t in_stride, void *d_out, size_t out_stride, int32_t *d_tone,
                                 uint32_t *d_open, uint32_t *d_count, float *d_level, float *d_powers, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_tone_device: a CPU handle has no device path");
    if (int rc = check_chtone_args(h, d_sense, sense_stride, d_audio, nch, nsamp, in_stride, d_out, out_stride, d_tone, d_open, d_count,
                                   d_level, d_powers))
        return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chtone_launch(h, d_sense, sense_stride, d_audio, nch, nsamp, in_stride, d_out, out_stride, d_tone, d_open, d_count, d_level,
                         d_powers, (hipStream_t)hip_stream);
}

int sddc_ddc_channel_tone_host(sddc_ddc_t *h, const void *sense, size_t sense_stride, const void *audio, int nch, size_t nsamp,
                               size_t in_stride, void *out, size_t out_stride, int32_t *tone, uint32_t *open, uint32_t *count,
                               float *level, float *powers)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chtone_args(h, sense, sense_stride, audio, nch, nsamp, in_stride, out, out_stride, tone, open, count, level, powers))
        return rc;
    ChannelTone &st = h->chtone;
    const bool s16 = st.sense_fmt == SDDC_DDC_AUDIO_S16, in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_tone(sense, s16, audio, in16, nch, nsamp, nch > 1 ? sense_stride : 0, nch > 1 ? in_stride : 0,
                                      st.words.data(), st.ntones, st.masks.data(), st.thr.data(), st.window, st.attack, st.hang, st.pos,
                                      st.state_h.data(), out, out16, nch > 1 ? out_stride : 0, tone, open, count, level, powers);
        st.pos += nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs
    const size_t ss = s16 ? 2 : 4, is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const size_t sense_bytes = ((size_t)(nch - 1) * (nch > 1 ? sense_stride : 0) + nsamp) * ss;
    const size_t in_bytes = audio ? ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is : 0;
    const size_t out_bytes = audio ? ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os : 0;
    const size_t n = (size_t)nch;
    if (int rc = grow_device_buffer(&st.d_sense, &st.sense_cap, sense_bytes, "channel_tone_host", "sense bytes")) return rc;
    if (audio) {
        if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_tone_host", "input bytes")) return rc;
        if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes, "channel_tone_host", "output bytes")) return rc;
    }
    if (int rc = grow_device_buffer(&st.d_side, &st.side_cap, n * (5 + (size_t)st.ntones), "channel_tone_host", "side outputs")) return rc;
    int32_t *d_tone = tone ? reinterpret_cast<int32_t *>(st.d_side) : nullptr;
    uint32_t *d_open = open ? st.d_side + n : nullptr, *d_count = count ? st.d_side + 2 * n : nullptr;
    float *d_level = level ? reinterpret_cast<float *>(st.d_side + 3 * n) : nullptr;
    float *d_powers = powers ? reinterpret_cast<float *>(st.d_side + 5 * n) : nullptr;
    HIP_TRY(hipMemcpyAsync(st.d_sense, sense, sense_bytes, hipMemcpyHostToDevice, h->stream));
    if (audio) HIP_TRY(hipMemcpyAsync(st.d_in, audio, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chtone_launch(h, st.d_sense, sense_stride, audio ? st.d_in : nullptr, nch, nsamp, in_stride, audio ? st.d_out : nullptr,
                                 out_stride, d_tone, d_open, d_count, d_level, d_powers, h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        if (audio) {
            if (nch == 1 || out_stride == nsamp)
                HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
            else
                HIP_TRY(hipMemcpy2DAsync(out, out_stride * os, st.d_out, out_stride * os, nsamp * os, n, hipMemcpyDeviceToHost,
                                         h->stream));
        }
        if (tone) HIP_TRY(hipMemcpyAsync(tone, d_tone, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (open) HIP_TRY(hipMemcpyAsync(open, d_open, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (count) HIP_TRY(hipMemcpyAsync(count, d_count, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (level) HIP_TRY(hipMemcpyAsync(level, d_level, n * 8, hipMemcpyDeviceToHost, h->stream));
        if (powers) HIP_TRY(hipMemcpyAsync(powers, d_powers, n * (size_t)st.ntones * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel DCS decoder: streaming per-channel digital code squelch ----------------------------- */
static_assert(SDDC_DDC_DCS_BLOCK == sddc::dcs::kDcsBlock && SDDC_DDC_DCS_MAX_CODES == sddc::dcs::kDcsMaxCodes &&
                  SDDC_DDC_DCS_MAX_WINDOW == sddc::dcs::kDcsMaxWindow && SDDC_DDC_DCS_MAX_ATTACK == sddc::dcs::kDcsMaxAttack &&
                  SDDC_DDC_DCS_MAX_HANG == sddc::dcs::kDcsMaxHang && SDDC_DDC_DCS_MAX_ERRORS == sddc::dcs::kDcsMaxErrors &&
                  SDDC_DDC_DCS_MAX_EYE == sddc::dcs::kDcsMaxEye && SDDC_DDC_DCS_ANY == sddc::dcs::kDcsAny &&
                  SDDC_DDC_DCS_OFF == sddc::dcs::kDcsOff && SDDC_DDC_DCS_MAX_WORD == sddc::dcs::kDcsMaxWord,
              "the arithmetic header's constants are the ABI's");
static_assert(sizeof(sddc::cpu::R2iq::DcsChannel) == (size_t)sddc::kDcsStateWords * 4, "the CPU state holds what the device's does");

int sddc_ddc_dcs_codeword(int code, uint32_t *cw)
{
    if (!cw) return fail(SDDC_ERR_ARG, "dcs_codeword: null cw");
    if (code < 0 || code > 511) return fail(SDDC_ERR_ARG, "dcs_codeword: code %d outside 0..511 (three octal digits)", code);
    *cw = sddc::dcs::dcs_codeword((uint32_t)code);
    return SDDC_OK;
}

int sddc_ddc_dcs_window(double fs, double bitrate, uint32_t *word, int *blocks)
{
    if (!word || !blocks) return fail(SDDC_ERR_ARG, "dcs_window: null word or blocks");
    if (!std::isfinite(fs) || !std::isfinite(bitrate) || !(fs > 0.0) || !(bitrate > 0.0))
        return fail(SDDC_ERR_ARG, "dcs_window: %g bit/s at %g Hz are not finite positive rates", bitrate, fs);
    const double w = std::nearbyint(bitrate / fs * 4294967296.0);
    if (!(w >= 1.0) || !(w <= (double)SDDC_DDC_DCS_MAX_WORD))
        return fail(SDDC_ERR_ARG, "dcs_window: %g bit/s at %g Hz is the phase word %g, outside 1..2^29", bitrate, fs, w);
    const uint64_t wi = (uint64_t)w, num = (uint64_t)24 << 32, den = (uint64_t)SDDC_DDC_DCS_BLOCK * wi;
    const uint64_t b = (num + den - 1) / den;
    if (b > (uint64_t)SDDC_DDC_DCS_MAX_WINDOW)
        return fail(SDDC_ERR_ARG, "dcs_window: %g bit/s at %g Hz needs %llu blocks, above %d", bitrate, fs, (unsigned long long)b,
                    SDDC_DDC_DCS_MAX_WINDOW);
    *word = (uint32_t)wi;
    *blocks = (int)(b < 1 ? 1 : b);
    return SDDC_OK;
}

int sddc_ddc_set_channel_dcs_decoder(sddc_ddc_t *h, const uint32_t *codewords, int ncodes, const int32_t *params, int nch,
                                     uint32_t word, int window, int e_open, int e_close, int attack, int hang, int sense_format,
                                     int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !codewords || !params || nch == 0;
    std::vector<uint32_t> cw;
    std::vector<int32_t> pr;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel DCS decoder: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        if (ncodes < 1 || ncodes > SDDC_DDC_DCS_MAX_CODES)
            return fail(SDDC_ERR_ARG, "channel DCS decoder: ncodes %d outside 1..%d", ncodes, SDDC_DDC_DCS_MAX_CODES);
        if (word < 1 || word > SDDC_DDC_DCS_MAX_WORD)
            return fail(SDDC_ERR_ARG, "channel DCS decoder: the phase word %u is outside 1..2^29", word);
        if (window < 1 || window > SDDC_DDC_DCS_MAX_WINDOW)
            return fail(SDDC_ERR_ARG, "channel DCS decoder: window %d outside 1..%d blocks", window, SDDC_DDC_DCS_MAX_WINDOW);
        if ((uint64_t)SDDC_DDC_DCS_BLOCK * (uint64_t)window * (uint64_t)word < ((uint64_t)24 << 32))
            return fail(SDDC_ERR_ARG, "channel DCS decoder: a window of %d blocks holds fewer than 24 bits at the phase word %u", window,
                        word);
        if (e_open < 0 || e_open > e_close || e_close > SDDC_DDC_DCS_MAX_ERRORS)
            return fail(SDDC_ERR_ARG, "channel DCS decoder: the error limits %d, %d are not 0 <= e_open <= e_close <= %d", e_open,
                        e_close, SDDC_DDC_DCS_MAX_ERRORS);
        if (attack < 1 || attack > SDDC_DDC_DCS_MAX_ATTACK)
            return fail(SDDC_ERR_ARG, "channel DCS decoder: attack %d outside 1..%d windows", attack, SDDC_DDC_DCS_MAX_ATTACK);
        if (hang < 0 || hang > SDDC_DDC_DCS_MAX_HANG)
            return fail(SDDC_ERR_ARG, "channel DCS decoder: hang %d outside 0..%d windows", hang, SDDC_DDC_DCS_MAX_HANG);
        for (int fmt : {sense_format, in_format, out_format})
            if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
                return fail(SDDC_ERR_ARG, "channel DCS decoder: unknown sample format %d", fmt);
        for (int i = 0; i < ncodes; i++)
            if (codewords[i] >> 23)
                return fail(SDDC_ERR_ARG, "channel DCS decoder: codeword %d = 0x%x has a bit above its 23", i, codewords[i]);
        for (int c = 0; c < nch; c++) {
            const int32_t code = params[3 * c], inv = params[3 * c + 1], eye = params[3 * c + 2];
            if (code < SDDC_DDC_DCS_OFF || code >= ncodes)
                return fail(SDDC_ERR_ARG, "channel DCS decoder: the code %d of channel %d is no index below ncodes = %d, ANY or OFF", code,
                            c, ncodes);
            if (inv != 0 && inv != 1) return fail(SDDC_ERR_ARG, "channel DCS decoder: invert %d of channel %d is not 0 or 1", inv, c);
            if (eye < 0 || eye > SDDC_DDC_DCS_MAX_EYE)
                return fail(SDDC_ERR_ARG, "channel DCS decoder: eye %d of channel %d outside 0..%d", eye, c, SDDC_DDC_DCS_MAX_EYE);
        }
        try {
            cw.assign(codewords, codewords + ncodes);
            pr.assign(params, params + 3 * (size_t)nch);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel DCS decoder: %s", ex.what());
        }
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelDcs &st = h->chdcs;
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.state_h.assign((size_t)nch, sddc::cpu::R2iq::DcsChannel());
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel DCS decoder: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the stage off
        if (off) return SDDC_OK;
        const size_t nstate = (size_t)nch * sddc::kDcsStateWords;
        hipError_t e = hipMalloc(&st.d_cws, cw.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&st.d_params, pr.size() * sizeof(int32_t));
        for (uint32_t *&p : st.d_state)
            if (e == hipSuccess) e = hipMalloc(&p, nstate * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel DCS decoder: no device memory for %d channels", nch);
        }
        e = hipMemcpy(st.d_cws, cw.data(), cw.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(st.d_params, pr.data(), pr.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        // zeroed on the handle's stream and waited for: the first launch may be on any stream
        for (uint32_t *p : st.d_state)
            if (e == hipSuccess) e = hipMemsetAsync(p, 0, nstate * sizeof(uint32_t), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.cws = std::move(cw);
    st.params = std::move(pr);
    st.word = word;
    sddc::dcs::dcs_count(word, window, st.counts);
    st.nch = nch;
    st.ncodes = ncodes;
    st.window = window;
    st.e_open = e_open;
    st.e_close = e_close;
    st.attack = attack;
    st.hang = hang;
    st.sense_fmt = sense_format;
    st.in_fmt = in_format;
    st.out_fmt = out_format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_dcs_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelDcs &st = h->chdcs;
    if (st.params.empty()) return fail(SDDC_ERR_STATE, "channel DCS reset: no decoder set");
    if (h->cpu) {
        std::fill(st.state_h.begin(), st.state_h.end(), sddc::cpu::R2iq::DcsChannel());
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        HIP_TRY(hipMemsetAsync(st.d_state[st.cur], 0, st.state_words() * sizeof(uint32_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

// the checks both calls share (under h->mu)
static int check_chdcs_args(const sddc_ddc_t *h, const void *sense, size_t sense_stride, const void *in, int nch, size_t nsamp,
                            size_t in_stride, const void *out, size_t out_stride, const void *code, const void *open,
                            const void *count, const void *info)
{
    const ChannelDcs &st = h->chdcs;
    if (st.params.empty()) return fail(SDDC_ERR_STATE, "channel DCS decoder: no decoder set");
    if (nch != st.nch)
        return fail(SDDC_ERR_STATE, "channel DCS decoder: the decoder is set for %d channels, the call has %d", st.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (!sense) return fail(SDDC_ERR_ARG, "null sense buffer");
    if (nch > 1 && sense_stride < nsamp)
        return fail(SDDC_ERR_ARG, "sense_stride must be >= nsamp (got %zu, nsamp %zu)", sense_stride, nsamp);
    const uintptr_t ss = st.sense_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)sense & (ss - 1)) != 0) return fail(SDDC_ERR_ARG, "the sense buffer must be %d-byte aligned", (int)ss);
    if ((((uintptr_t)code | (uintptr_t)open | (uintptr_t)count | (uintptr_t)info) & 3) != 0)
        return fail(SDDC_ERR_ARG, "the side outputs must be 4-byte aligned");
    if (!in && out) return fail(SDDC_ERR_ARG, "an output without audio");
    if (in && !out) return fail(SDDC_ERR_ARG, "audio without an output");
    if (!in) return SDDC_OK;
    if (nch > 1 && in_stride < nsamp) return fail(SDDC_ERR_ARG, "in_stride must be >= nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < nsamp)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    const uintptr_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)in & (is - 1)) != 0) return fail(SDDC_ERR_ARG, "the input must be %d-byte aligned", (int)is);
    if (((uintptr_t)out & (os - 1)) != 0) return fail(SDDC_ERR_ARG, "the output must be %d-byte aligned", (int)os);
    const uintptr_t ia = (uintptr_t)in, oa = (uintptr_t)out, sa = (uintptr_t)sense;
    const uintptr_t ib = ia + ((uintptr_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const uintptr_t ob = oa + ((uintptr_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os;
    const uintptr_t sb = sa + ((uintptr_t)(nch - 1) * (nch > 1 ? sense_stride : 0) + nsamp) * ss;
    if (ia < ob && oa < ib) return fail(SDDC_ERR_ARG, "the input and the output overlap");
    if (sa < ob && oa < sb) return fail(SDDC_ERR_ARG, "the sense buffer and the output overlap");
    return SDDC_OK;
}

// The call in launch sets of at most run_blocks blocks per channel, rounded down to whole windows (the
// scratch holds four words per channel and window of a set, and the kernels index a set with an int).
static int chdcs_launch(sddc_ddc_t *h, const void *d_sense, size_t sense_stride, const void *d_in, int nch, size_t nsamp,
                        size_t in_stride, void *d_out, size_t out_stride, int32_t *d_code, uint32_t *d_open, uint32_t *d_count,
                        uint32_t *d_info, hipStream_t s)
{
    ChannelDcs &st = h->chdcs;
    const size_t B = SDDC_DDC_DCS_BLOCK, W = (size_t)st.window, WB = W * B;
    const size_t run_blocks = (size_t)(st.run_blocks > 0 ? st.run_blocks : ChannelDcs::kDefaultRunBlocks);
    const size_t run_windows = run_blocks / W > 0 ? run_blocks / W : 1;
    const size_t hs0 = (size_t)(st.pos % WB), windows = (hs0 + nsamp + WB - 1) / WB;
    const size_t need = (size_t)nch * (windows < run_windows ? windows : run_windows) * 4;
    if (need > st.scratch_cap) {
        HIP_TRY(st.readers.sync());   // an earlier launch may still use the scratch
        if (int rc = grow_device_buffer(&st.d_scratch, &st.scratch_cap, need, "channel DCS decoder", "scratch words")) return rc;
    }
    HIP_TRY(st.readers.order_before(s));
    const bool s16 = st.sense_fmt == SDDC_DDC_AUDIO_S16, in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    const size_t ss = s16 ? 2 : 4, is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    hipError_t e = hipSuccess;
    for (size_t done = 0; done < nsamp && e == hipSuccess;) {
        const size_t hs = (size_t)(st.pos % WB);
        size_t n = nsamp - done;
        if (n > run_windows * WB - hs) n = run_windows * WB - hs;
        e = sddc::launch_channel_dcs(h->tables, static_cast<const char *>(d_sense) + done * ss, s16, sense_stride,
                                     d_in ? static_cast<const char *>(d_in) + done * is : nullptr, in16, nch, n, in_stride, st.pos,
                                     st.d_cws, st.ncodes, st.d_params, st.word, st.counts, st.window, st.e_open, st.e_close, st.attack,
                                     st.hang, st.d_state[st.cur], st.d_state[st.cur ^ 1], st.d_scratch,
                                     d_in ? static_cast<char *>(d_out) + done * os : nullptr, out16, out_stride, d_code, d_open, d_count,
                                     d_info, done > 0, st.ballot, st.max_wgs, h->device, s);
        if (e != hipSuccess) break;
        st.cur ^= 1;
        st.pos += n;
        done += n;
    }
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_dcs_device(sddc_ddc_t *h, const void *d_sense, size_t sense_stride, const void *d_audio, int nch,
                                size_t nsamp, size_t in_stride, void *d_out, size_t out_stride, int32_t *d_code, uint32_t *d_open,
                                uint32_t *d_count, uint32_t *d_info, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_dcs_device: a CPU handle has no device path");
    if (int rc = check_chdcs_args(h, d_sense, sense_stride, d_audio, nch, nsamp, in_stride, d_out, out_stride, d_code, d_open, d_count,
                                  d_info))
        return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chdcs_launch(h, d_sense, sense_stride, d_audio, nch, nsamp, in_stride, d_out, out_stride, d_code, d_open, d_count, d_info,
                        (hipStream_t)hip_stream);
}

int sddc_ddc_channel_dcs_host(sddc_ddc_t *h, const void *sense, size_t sense_stride, const void *audio, int nch, size_t nsamp,
                              size_t in_stride, void *out, size_t out_stride, int32_t *code, uint32_t *open, uint32_t *count,
                              uint32_t *info)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chdcs_args(h, sense, sense_stride, audio, nch, nsamp, in_stride, out, out_stride, code, open, count, info)) return rc;
    ChannelDcs &st = h->chdcs;
    const bool s16 = st.sense_fmt == SDDC_DDC_AUDIO_S16, in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_dcs(sense, s16, audio, in16, nch, nsamp, nch > 1 ? sense_stride : 0, nch > 1 ? in_stride : 0,
                                     st.cws.data(), st.ncodes, st.params.data(), st.word, st.counts, st.window, st.e_open, st.e_close,
                                     st.attack, st.hang, st.pos, st.state_h.data(), out, out16, nch > 1 ? out_stride : 0, code, open,
                                     count, info);
        st.pos += nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs
    const size_t ss = s16 ? 2 : 4, is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const size_t sense_bytes = ((size_t)(nch - 1) * (nch > 1 ? sense_stride : 0) + nsamp) * ss;
    const size_t in_bytes = audio ? ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is : 0;
    const size_t out_bytes = audio ? ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os : 0;
    const size_t n = (size_t)nch;
    if (int rc = grow_device_buffer(&st.d_sense, &st.sense_cap, sense_bytes, "channel_dcs_host", "sense bytes")) return rc;
    if (audio) {
        if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_dcs_host", "input bytes")) return rc;
        if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, out_bytes, "channel_dcs_host", "output bytes")) return rc;
    }
    if (int rc = grow_device_buffer(&st.d_side, &st.side_cap, n * 7, "channel_dcs_host", "side outputs")) return rc;
    int32_t *d_code = code ? reinterpret_cast<int32_t *>(st.d_side) : nullptr;
    uint32_t *d_open = open ? st.d_side + n : nullptr, *d_count = count ? st.d_side + 2 * n : nullptr;
    uint32_t *d_info = info ? st.d_side + 3 * n : nullptr;
    HIP_TRY(hipMemcpyAsync(st.d_sense, sense, sense_bytes, hipMemcpyHostToDevice, h->stream));
    if (audio) HIP_TRY(hipMemcpyAsync(st.d_in, audio, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chdcs_launch(h, st.d_sense, sense_stride, audio ? st.d_in : nullptr, nch, nsamp, in_stride, audio ? st.d_out : nullptr,
                                out_stride, d_code, d_open, d_count, d_info, h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        if (audio) {
            if (nch == 1 || out_stride == nsamp)
                HIP_TRY(hipMemcpyAsync(out, st.d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
            else
                HIP_TRY(hipMemcpy2DAsync(out, out_stride * os, st.d_out, out_stride * os, nsamp * os, n, hipMemcpyDeviceToHost,
                                         h->stream));
        }
        if (code) HIP_TRY(hipMemcpyAsync(code, d_code, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (open) HIP_TRY(hipMemcpyAsync(open, d_open, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (count) HIP_TRY(hipMemcpyAsync(count, d_count, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (info) HIP_TRY(hipMemcpyAsync(info, d_info, n * 16, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

/* ---- channel stereo decoder: streaming WFM stereo from the MPX -------------------------------------- */
static_assert(SDDC_DDC_STEREO_BLOCK == sddc::stereo::kStereoBlock && SDDC_DDC_STEREO_MAX_WINDOW == sddc::stereo::kStereoMaxWindow &&
                  SDDC_DDC_STEREO_MONO == sddc::stereo::kStereoMono && SDDC_DDC_STEREO_AUTO == sddc::stereo::kStereoAuto,
              "the arithmetic header's constants are the ABI's");
static_assert(sizeof(sddc::cpu::R2iq::StereoChannel) == (size_t)sddc::kStereoStateWords * 4, "the CPU state holds what the device's does");

int sddc_ddc_set_channel_stereo_decoder(sddc_ddc_t *h, uint32_t pilot_word, const uint8_t *modes, const float *params, int nch,
                                        int window, int attack, int hang, int in_format, int out_format)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    const bool off = !modes || !params || nch == 0;
    std::vector<uint8_t> md;
    std::vector<float> thr;
    std::vector<uint32_t> mw, init;
    if (!off) {
        if (nch < 1 || nch > SDDC_DDC_MAX_CHANNELS)
            return fail(SDDC_ERR_ARG, "channel stereo decoder: nch %d outside 1..%d", nch, SDDC_DDC_MAX_CHANNELS);
        if (pilot_word == 0) return fail(SDDC_ERR_ARG, "channel stereo decoder: the pilot word is 0");
        if (window < 1 || window > SDDC_DDC_STEREO_MAX_WINDOW)
            return fail(SDDC_ERR_ARG, "channel stereo decoder: window %d outside 1..%d blocks", window, SDDC_DDC_STEREO_MAX_WINDOW);
        if (attack < 1 || attack > SDDC_DDC_TONE_MAX_ATTACK)
            return fail(SDDC_ERR_ARG, "channel stereo decoder: attack %d outside 1..%d windows", attack, SDDC_DDC_TONE_MAX_ATTACK);
        if (hang < 0 || hang > SDDC_DDC_TONE_MAX_HANG)
            return fail(SDDC_ERR_ARG, "channel stereo decoder: hang %d outside 0..%d windows", hang, SDDC_DDC_TONE_MAX_HANG);
        for (int fmt : {in_format, out_format})
            if (fmt != SDDC_DDC_AUDIO_F32 && fmt != SDDC_DDC_AUDIO_S16)
                return fail(SDDC_ERR_ARG, "channel stereo decoder: unknown sample format %d", fmt);
        try {
            md.assign(modes, modes + nch);
            mw.assign(modes, modes + nch);
            thr.resize((size_t)nch * 4);
            init.assign((size_t)nch * sddc::kStereoStateWords, 0u);
        } catch (const std::exception &ex) {
            return fail(SDDC_ERR_NOMEM, "channel stereo decoder: %s", ex.what());
        }
        const sddc::cpu::R2iq::StereoChannel fresh;
        for (int c = 0; c < nch; c++) {
            const float ro = params[4 * c], rc = params[4 * c + 1], em = params[4 * c + 2], g = params[4 * c + 3];
            if (modes[c] != SDDC_DDC_STEREO_MONO && modes[c] != SDDC_DDC_STEREO_AUTO)
                return fail(SDDC_ERR_ARG, "channel stereo decoder: unknown mode %d of channel %d", (int)modes[c], c);
            if (!(ro > 0.f && ro <= 1.f) || !(rc > 0.f && rc <= 1.f))
                return fail(SDDC_ERR_ARG, "channel stereo decoder: rho_open %g or rho_close %g of channel %d is outside (0, 1]",
                            (double)ro, (double)rc, c);
            if (!(rc <= ro))
                return fail(SDDC_ERR_ARG, "channel stereo decoder: channel %d has rho_close %g above rho_open %g", c, (double)rc, (double)ro);
            thr[4 * (size_t)c] = sddc::tone::tone_scale(ro, window);
            thr[4 * (size_t)c + 1] = sddc::tone::tone_scale(rc, window);
            thr[4 * (size_t)c + 2] = sddc::tone::tone_scale(em == 0.f ? 0.f : em, window);
            thr[4 * (size_t)c + 3] = sddc::stereo::stereo_g2(g == 0.f ? 0.f : g);
            if (!(em >= 0.f) || !std::isfinite(thr[4 * (size_t)c + 2]))
                return fail(SDDC_ERR_ARG, "channel stereo decoder: e_min %g of channel %d is not a value >= 0 with a finite 256 W e_min",
                            (double)em, c);
            if (!(g >= 0.f) || !std::isfinite(thr[4 * (size_t)c + 3]))
                return fail(SDDC_ERR_ARG, "channel stereo decoder: the gain %g of channel %d is not a value >= 0 with a finite 2 g",
                            (double)g, c);
            std::memcpy(&init[(size_t)c * sddc::kStereoStateWords], &fresh, sizeof fresh);
        }
    }
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelStereo &st = h->chst;
    if (h->cpu) {
        st.clear();
        if (off) return SDDC_OK;
        try {
            st.state_h.assign((size_t)nch, sddc::cpu::R2iq::StereoChannel());
        } catch (const std::exception &ex) {
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel stereo decoder: %s", ex.what());
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        st.clear();                   // a failed upload leaves the stage off
        if (off) return SDDC_OK;
        hipError_t e = hipMalloc(&st.d_modes, mw.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&st.d_thr, thr.size() * sizeof(float));
        for (uint32_t *&p : st.d_state)
            if (e == hipSuccess) e = hipMalloc(&p, init.size() * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st.clear();
            return fail(SDDC_ERR_NOMEM, "channel stereo decoder: no device memory for %d channels", nch);
        }
        // synchronous copies from pageable memory: done when they return, so the first launch may be on any stream
        e = hipMemcpy(st.d_modes, mw.data(), mw.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(st.d_thr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice);
        for (uint32_t *p : st.d_state)
            if (e == hipSuccess) e = hipMemcpy(p, init.data(), init.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            st.clear();
            HIP_TRY(e);
        }
    }
    st.modes = std::move(md);
    st.thr = std::move(thr);
    st.init = std::move(init);
    st.word = pilot_word;
    st.nch = nch;
    st.window = window;
    st.attack = attack;
    st.hang = hang;
    st.in_fmt = in_format;
    st.out_fmt = out_format;
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_channel_stereo_reset(sddc_ddc_t *h)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelStereo &st = h->chst;
    if (st.modes.empty()) return fail(SDDC_ERR_STATE, "channel stereo reset: no decoder set");
    if (h->cpu) {
        std::fill(st.state_h.begin(), st.state_h.end(), sddc::cpu::R2iq::StereoChannel());
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());   // earlier launches, on any stream, may still use the state
        HIP_TRY(hipMemcpy(st.d_state[st.cur], st.init.data(), st.init.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipDeviceSynchronize());   // the next launch may be on any stream
    }
    st.pos = 0;
    return SDDC_OK;
}

int sddc_ddc_internal_chst_set_position(sddc_ddc_t *h, uint64_t pos)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    ChannelStereo &st = h->chst;
    if (st.modes.empty()) return fail(SDDC_ERR_STATE, "channel stereo position: no decoder set");
    if (pos % ((uint64_t)SDDC_DDC_STEREO_BLOCK * (uint64_t)st.window) != 0)
        return fail(SDDC_ERR_ARG, "channel stereo position: %llu is no multiple of 256 W = %d", (unsigned long long)pos,
                    SDDC_DDC_STEREO_BLOCK * st.window);
    if (h->cpu) {
        for (auto &ch : st.state_h) {
            ch.zr = ch.zi = ch.E = 0.f;
            ch.bad = 0;
            std::fill(std::begin(ch.x), std::end(ch.x), 0.f);
        }
    } else {
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(st.readers.sync());
        // words 7 .. 10 of every channel: Zr, Zi, E and the bad flag (the stored block is not read at a block's start)
        HIP_TRY(hipMemset2DAsync(st.d_state[st.cur] + 7, (size_t)sddc::kStereoStateWords * 4, 0, (size_t)4 * 4, (size_t)st.nch,
                                 h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    st.pos = pos;
    return SDDC_OK;
}

// the checks both calls share (under h->mu)
static int check_chst_args(const sddc_ddc_t *h, const void *in, int nch, size_t nsamp, size_t in_stride, const void *left,
                           const void *right, size_t out_stride, const void *stereo, const void *count, const void *level,
                           const void *phase)
{
    const ChannelStereo &st = h->chst;
    if (st.modes.empty()) return fail(SDDC_ERR_STATE, "channel stereo decoder: no decoder set");
    if (nch != st.nch)
        return fail(SDDC_ERR_STATE, "channel stereo decoder: the decoder is set for %d channels, the call has %d", st.nch, nch);
    if (nsamp == 0 || nsamp > ((size_t)1 << 40)) return fail(SDDC_ERR_ARG, "nsamp must be in 1..2^40 (got %zu)", nsamp);
    if (!in || !left || !right) return fail(SDDC_ERR_ARG, "null input or output buffer");
    if (nch > 1 && in_stride < nsamp) return fail(SDDC_ERR_ARG, "in_stride must be >= nsamp (got %zu, nsamp %zu)", in_stride, nsamp);
    if (nch > 1 && out_stride < nsamp)
        return fail(SDDC_ERR_ARG, "out_stride must be >= nsamp (got %zu, nsamp %zu)", out_stride, nsamp);
    const uintptr_t is = st.in_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4, os = st.out_fmt == SDDC_DDC_AUDIO_S16 ? 2 : 4;
    if (((uintptr_t)in & (is - 1)) != 0) return fail(SDDC_ERR_ARG, "the input must be %d-byte aligned", (int)is);
    if ((((uintptr_t)left | (uintptr_t)right) & (os - 1)) != 0) return fail(SDDC_ERR_ARG, "the outputs must be %d-byte aligned", (int)os);
    if ((((uintptr_t)stereo | (uintptr_t)count | (uintptr_t)level | (uintptr_t)phase) & 3) != 0)
        return fail(SDDC_ERR_ARG, "the side outputs must be 4-byte aligned");
    const uintptr_t ia = (uintptr_t)in, la = (uintptr_t)left, ra = (uintptr_t)right;
    const uintptr_t ospan = ((uintptr_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os;
    const uintptr_t ib = ia + ((uintptr_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const uintptr_t lb = la + ospan, rb = ra + ospan;
    if ((ia < lb && la < ib) || (ia < rb && ra < ib)) return fail(SDDC_ERR_ARG, "the input and an output overlap");
    if (la < rb && ra < lb) return fail(SDDC_ERR_ARG, "the two outputs overlap");
    return SDDC_OK;
}

// The call in launch sets of at most run_blocks blocks per channel (the scratch holds eight words per channel
// and block of a set, and the kernels index a set with an int).
static int chst_launch(sddc_ddc_t *h, const void *d_in, int nch, size_t nsamp, size_t in_stride, void *d_left, void *d_right,
                       size_t out_stride, uint32_t *d_stereo, uint32_t *d_count, float *d_level, float *d_phase, hipStream_t s)
{
    ChannelStereo &st = h->chst;
    const size_t B = SDDC_DDC_STEREO_BLOCK;
    const size_t run_blocks = (size_t)(st.run_blocks > 0 ? st.run_blocks : ChannelStereo::kDefaultRunBlocks);
    const size_t blocks = ((size_t)(st.pos % B) + nsamp + B - 1) / B;
    const size_t need = sddc::kStereoScratchWords((size_t)nch, blocks < run_blocks ? blocks : run_blocks);
    if (need > st.scratch_cap) {
        HIP_TRY(st.readers.sync());   // an earlier launch may still use the scratch
        if (int rc = grow_device_buffer(&st.d_scratch, &st.scratch_cap, need, "channel stereo decoder", "scratch words")) return rc;
    }
    HIP_TRY(st.readers.order_before(s));
    const bool in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    const size_t is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    hipError_t e = hipSuccess;
    for (size_t done = 0; done < nsamp && e == hipSuccess;) {
        const size_t hs = (size_t)(st.pos % B);
        size_t n = nsamp - done;
        if (n > run_blocks * B - hs) n = run_blocks * B - hs;
        e = sddc::launch_channel_stereo(h->tables, static_cast<const char *>(d_in) + done * is, in16, nch, n, in_stride, st.pos, st.word,
                                        st.d_modes, st.d_thr, st.window, st.attack, st.hang, st.d_state[st.cur], st.d_state[st.cur ^ 1],
                                        st.d_scratch, static_cast<char *>(d_left) + done * os, static_cast<char *>(d_right) + done * os,
                                        out16, out_stride, d_stereo, d_count, d_level, d_phase, done > 0, st.max_wgs, h->device, s);
        if (e != hipSuccess) break;
        st.cur ^= 1;
        st.pos += n;
        done += n;
    }
    const hipError_t er = st.readers.record(s);   // whatever was enqueued stays ordered
    HIP_TRY(e);
    HIP_TRY(er);
    return SDDC_OK;
}

int sddc_ddc_channel_stereo_device(sddc_ddc_t *h, const void *d_mpx, int nch, size_t nsamp, size_t in_stride, void *d_left,
                                   void *d_right, size_t out_stride, uint32_t *d_stereo, uint32_t *d_count, float *d_level,
                                   float *d_phase, void *hip_stream)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cpu) return fail(SDDC_ERR_STATE, "channel_stereo_device: a CPU handle has no device path");
    if (int rc = check_chst_args(h, d_mpx, nch, nsamp, in_stride, d_left, d_right, out_stride, d_stereo, d_count, d_level, d_phase))
        return rc;
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return chst_launch(h, d_mpx, nch, nsamp, in_stride, d_left, d_right, out_stride, d_stereo, d_count, d_level, d_phase,
                       (hipStream_t)hip_stream);
}

int sddc_ddc_channel_stereo_host(sddc_ddc_t *h, const void *mpx, int nch, size_t nsamp, size_t in_stride, void *left, void *right,
                                 size_t out_stride, uint32_t *stereo, uint32_t *count, float *level, float *phase)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_chst_args(h, mpx, nch, nsamp, in_stride, left, right, out_stride, stereo, count, level, phase)) return rc;
    ChannelStereo &st = h->chst;
    const bool in16 = st.in_fmt == SDDC_DDC_AUDIO_S16, out16 = st.out_fmt == SDDC_DDC_AUDIO_S16;
    if (h->cpu) {
        sddc::cpu::R2iq::channel_stereo(mpx, in16, nch, nsamp, nch > 1 ? in_stride : 0, st.word, st.modes.data(), st.thr.data(),
                                        st.window, st.attack, st.hang, st.pos, st.state_h.data(), left, right, out16,
                                        nch > 1 ? out_stride : 0, stereo, count, level, phase);
        st.pos += nsamp;
        return SDDC_OK;
    }
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    // the spans that hold every channel's samples and outputs; the right streams follow the left ones
    const size_t is = in16 ? 2 : 4, os = out16 ? 2 : 4;
    const size_t in_bytes = ((size_t)(nch - 1) * (nch > 1 ? in_stride : 0) + nsamp) * is;
    const size_t out_bytes = (((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os + 15) / 16 * 16;
    const size_t n = (size_t)nch;
    if (int rc = grow_device_buffer(&st.d_in, &st.in_cap, in_bytes, "channel_stereo_host", "input bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_out, &st.out_cap, 2 * out_bytes, "channel_stereo_host", "output bytes")) return rc;
    if (int rc = grow_device_buffer(&st.d_side, &st.side_cap, n * 6, "channel_stereo_host", "side outputs")) return rc;
    void *d_left = st.d_out, *d_right = static_cast<char *>(st.d_out) + out_bytes;
    uint32_t *d_stereo = stereo ? st.d_side : nullptr, *d_count = count ? st.d_side + n : nullptr;
    float *d_level = level ? reinterpret_cast<float *>(st.d_side + 2 * n) : nullptr;
    float *d_phase = phase ? reinterpret_cast<float *>(st.d_side + 4 * n) : nullptr;
    HIP_TRY(hipMemcpyAsync(st.d_in, mpx, in_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = chst_launch(h, st.d_in, nch, nsamp, in_stride, d_left, d_right, out_stride, d_stereo, d_count, d_level, d_phase,
                               h->stream);
    if (rc == SDDC_OK) {   // the streams alone: the caller's memory between them stays as it is
        const std::pair<void *, void *> outs[2] = {{left, d_left}, {right, d_right}};
        for (const auto &o : outs) {
            if (nch == 1 || out_stride == nsamp)
                HIP_TRY(hipMemcpyAsync(o.first, o.second, ((size_t)(nch - 1) * (nch > 1 ? out_stride : 0) + nsamp) * os,
                                       hipMemcpyDeviceToHost, h->stream));
            else
                HIP_TRY(hipMemcpy2DAsync(o.first, out_stride * os, o.second, out_stride * os, nsamp * os, n, hipMemcpyDeviceToHost,
                                         h->stream));
        }
        if (stereo) HIP_TRY(hipMemcpyAsync(stereo, d_stereo, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (count) HIP_TRY(hipMemcpyAsync(count, d_count, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (level) HIP_TRY(hipMemcpyAsync(level, d_level, n * 8, hipMemcpyDeviceToHost, h->stream));
        if (phase) HIP_TRY(hipMemcpyAsync(phase, d_phase, n * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // also after a failed launch: the caller's input is free again
    return rc;
}

// ---- host path: pipelined chunks ------------------------------------------------------
extern "C++" {

static hipError_t host_setup(sddc_ddc_t *h)
{
    if (h->host_ready) return hipSuccess;
    hipError_t e;
    const size_t in_bytes = (kHistory + (size_t)kHostChunk * kBlock) * sizeof(int16_t);
    const size_t out_bytes = (size_t)kHostChunk * kOutBlockMax;
    for (auto &sl : h->hs) {
        if ((e = hipMalloc(&sl.d_in, in_bytes)) != hipSuccess) return e;
        if ((e = hipMalloc(&sl.d_out, out_bytes)) != hipSuccess) return e;
        if ((e = hipHostMalloc(&sl.h_in, in_bytes, hipHostMallocDefault)) != hipSuccess) return e;
        if ((e = hipHostMalloc(&sl.h_out, out_bytes, hipHostMallocDefault)) != hipSuccess) return e;
        for (hipEvent_t *ev : {&sl.e_h2d, &sl.e_k, &sl.e_d2h})
            if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return e;
    }
    if ((e = hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking)) != hipSuccess) return e;
    if ((e = hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking)) != hipSuccess) return e;
    h->host_ready = true;
    return hipSuccess;
}

// true if [p, p + bytes) lies in memory registered through sddc_ddc_register_host
static bool host_registered(const sddc_ddc_t *h, const void *p, size_t bytes)
{
    const char *c = static_cast<const char *>(p);
    for (const auto &r : h->regions)
        if (c >= r.first && c + bytes <= r.first + r.second) return true;
    return false;
}

// nblk input blocks, block i at src(i) (host), output written contiguously to out.
// Chunk k of kHostChunk blocks goes through slot k % 2:
//   s_in   : wait e_k (kernel k-2 done with d_in) -> history D2D from the newest slot
//            -> H2D of the blocks (direct from registered memory, else via h_in) -> e_h2d
//   stream : wait e_h2d, e_d2h (D2H k-2 done with d_out) -> kernel -> e_k
//   s_out  : wait e_k -> D2H (direct into registered memory, else into h_out) -> e_d2h
// The host copies staged output of chunk k-1 while chunk k is in flight.
template <class Src>
static int host_pipeline(sddc_ddc_t *h, int nblk, Src src, void *out)
{
    HIP_TRY(host_setup(h));
    // one chunk: nothing to overlap, so skip the cross-stream event hops
    hipStream_t s_in = nblk <= kHostChunk ? h->stream : h->s_in;
    hipStream_t s_out = nblk <= kHostChunk ? h->stream : h->s_out;
    const size_t per_out = (size_t)(SDDC_DDC_OUT_BLOCK >> h->d) * (h->out_fmt == SDDC_DDC_FMT_CS16 ? 4 : 8);
    const size_t blk_bytes = (size_t)kBlock * sizeof(int16_t);
    char *outb = static_cast<char *>(out);
    const bool out_direct = host_registered(h, out, (size_t)nblk * per_out);
    int pend_slot = -1, pend_n = 0;        // staged output not yet copied to the caller
    size_t pend_off = 0;
    auto drain = [&]() -> int {
        if (pend_slot < 0) return SDDC_OK;
        HIP_TRY(hipEventSynchronize(h->hs[pend_slot].e_d2h));
        std::memcpy(outb + pend_off, h->hs[pend_slot].h_out, (size_t)pend_n * per_out);
        pend_slot = -1;
        return SDDC_OK;
    };
    int slot = h->last_slot < 0 ? 0 : 1 - h->last_slot;
    for (int done = 0; done < nblk; done += kHostChunk, slot ^= 1) {
        const int n = std::min(kHostChunk, nblk - done);
        auto &sl = h->hs[slot];
        // ---- input: history, then the blocks ----
        HIP_TRY(hipStreamWaitEvent(s_in, sl.e_k, 0));
        if (!h->hist_override.empty()) {   // sddc_ddc_set_history (pageable source: staged copy)
            HIP_TRY(hipMemcpyAsync(sl.d_in, h->hist_override.data(), kHistory * sizeof(int16_t),
                                   hipMemcpyHostToDevice, s_in));
            HIP_TRY(hipStreamSynchronize(s_in));   // the vector is cleared below
            h->hist_override.clear();
        } else if (h->last_slot < 0) {
            HIP_TRY(hipMemsetAsync(sl.d_in, 0, kHistory * sizeof(int16_t), s_in));
        } else {
            const auto &prev = h->hs[h->last_slot];
            HIP_TRY(hipMemcpyAsync(sl.d_in, prev.d_in + (size_t)h->last_n * kBlock, kHistory * sizeof(int16_t),
                                   hipMemcpyDeviceToDevice, s_in));
        }
        bool staged_in = false;
        for (int i = 0; i < n;) {
            const int16_t *p = src(done + i);
            int run = 1;   // merge blocks that are contiguous in host memory
            while (i + run < n && src(done + i + run) == p + (size_t)run * kBlock) run++;
            int16_t *dst = sl.d_in + kHistory + (size_t)i * kBlock;
            if (host_registered(h, p, run * blk_bytes)) {
                HIP_TRY(hipMemcpyAsync(dst, p, run * blk_bytes, hipMemcpyHostToDevice, s_in));
            } else {
                if (!staged_in) HIP_TRY(hipEventSynchronize(sl.e_h2d));   // h_in free again
                staged_in = true;
                std::memcpy(sl.h_in + (size_t)i * kBlock, p, run * blk_bytes);
                HIP_TRY(hipMemcpyAsync(dst, sl.h_in + (size_t)i * kBlock, run * blk_bytes, hipMemcpyHostToDevice,
                                       s_in));
            }
            i += run;
        }
        HIP_TRY(hipEventRecord(sl.e_h2d, s_in));
        h->last_slot = slot;
        h->last_n = n;
        // ---- kernel ----
        HIP_TRY(hipStreamWaitEvent(h->stream, sl.e_h2d, 0));
        HIP_TRY(hipStreamWaitEvent(h->stream, sl.e_d2h, 0));
        HIP_TRY(launch_single(h, sl.d_in, n, sl.d_out, h->stream));
        HIP_TRY(hipEventRecord(sl.e_k, h->stream));
        // ---- output ----
        if (int rc = drain()) return rc;   // chunk k-1's staged output (its slot is reused next)
        HIP_TRY(hipStreamWaitEvent(s_out, sl.e_k, 0));
        if (out_direct) {
            HIP_TRY(hipMemcpyAsync(outb + (size_t)done * per_out, sl.d_out, (size_t)n * per_out,
                                   hipMemcpyDeviceToHost, s_out));
        } else {
            HIP_TRY(hipMemcpyAsync(sl.h_out, sl.d_out, (size_t)n * per_out, hipMemcpyDeviceToHost, s_out));
            pend_slot = slot;
            pend_n = n;
            pend_off = (size_t)done * per_out;
        }
        HIP_TRY(hipEventRecord(sl.e_d2h, s_out));
        if (done == 0 && injected_late_failure(h))
            return fail(SDDC_ERR_HIP, "injected failure after the first chunk's D2H (SDDC_DDC_INJECT_FAIL_AFTER_D2H)");
    }
    if (int rc = drain()) return rc;
    HIP_TRY(hipStreamSynchronize(s_out));
    HIP_TRY(hipStreamSynchronize(s_in));   // callers may reuse their input buffers
    return SDDC_OK;
}
}  // extern "C++"

// CPU handle: the whole call on the calling thread (cpu/r2iq_cpu.h)
static int cpu_process(sddc_ddc_t *h, const int16_t *const *blocks, int nblk, void *out)
{
    sddc::cpu::Params p;
    p.d = h->d;
    p.tunebin = h->tunebin;
    p.lsb = h->lsb != 0;
    p.rand = h->rand != 0;
    p.cs16 = h->out_fmt == SDDC_DDC_FMT_CS16;
    p.scale = h->cs16_scale;
    std::vector<float2> starts;
    if (h->nco_fc != 0.f) {
        const long nb = (long)nblk * (SDDC_DDC_OUT_BLOCK >> h->d) / sddc::FineTune::kBlock;
        starts.resize((size_t)nb * sddc::FineTune::kLanes);
        h->nco.starts(nb, starts.data());
        p.nco_trig = reinterpret_cast<const float *>(h->nco.table());
        p.nco_starts = reinterpret_cast<const float *>(starts.data());
    }
    try {
        h->cpu->process(blocks, nblk, out, p);
    } catch (const std::exception &ex) {
        return fail(SDDC_ERR_NOMEM, "cpu backend: %s", ex.what());
    }
    return SDDC_OK;
}

int sddc_ddc_process_host(sddc_ddc_t *h, const int16_t *in, int nblk, void *out)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = check_process_args(h, in, nblk, out);
    if (rc) return rc;
    if (h->cpu) {
        std::vector<const int16_t *> blocks((size_t)nblk);
        for (int i = 0; i < nblk; i++) blocks[i] = in + (size_t)i * kBlock;
        return cpu_process(h, blocks.data(), nblk, out);
    }
    if (injected_failure(h)) return fail(SDDC_ERR_HIP, "injected failure (SDDC_DDC_INJECT_FAIL)");
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return host_pipeline(h, nblk, [in](int i) { return in + (size_t)i * kBlock; }, out);
}

int sddc_ddc_process_blocks(sddc_ddc_t *h, const int16_t *const *blocks, int nblk, void *out)
{
    if (!h) return fail(SDDC_ERR_ARG, "null handle");
    if (!blocks) return fail(SDDC_ERR_ARG, "null block list");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = check_process_args(h, nblk > 0 ? blocks[0] : nullptr, nblk, out);
    if (rc) return rc;
    for (int i = 0; i < nblk; i++)
        if (!blocks[i] || ((uintptr_t)blocks[i] & 3)) return fail(SDDC_ERR_ARG, "block %d null or unaligned", i);
    if (h->cpu) return cpu_process(h, blocks, nblk, out);
    if (injected_failure(h)) return fail(SDDC_ERR_HIP, "injected failure (SDDC_DDC_INJECT_FAIL)");
    DeviceGuard g(h->device);
    HIP_TRY(g.err);
    return host_pipeline(h, nblk, [blocks](int i) { return blocks[i]; }, out);
}

int sddc_ddc_register_host(sddc_ddc_t *h, void *ptr, size_t bytes)
{
    if (!h || !ptr || !bytes) return fail(SDDC_ERR_ARG, "register_host: null handle/pointer or zero size");
    std::lock_guard<std::mutex> lk(h->mu);
    for (const auto &r : h->regions)
        if (static_cast<char *>(ptr) < r.first + r.second && r.first < static_cast<char *>(ptr) + bytes)
            return fail(SDDC_ERR_ARG, "register_host: overlaps a registered region");
    if (!h->cpu) {   // a CPU handle reads host memory directly: bookkeeping only
        DeviceGuard g(h->device);
        HIP_TRY(g.err);
        HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    }
    h->regions.emplace_back(static_cast<const char *>(ptr), bytes);
    return SDDC_OK;
}

int sddc_ddc_unregister_host(sddc_ddc_t *h, void *ptr)
{
    if (!h || !ptr) return fail(SDDC_ERR_ARG, "unregister_host: null handle/pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    for (size_t i = 0; i < h->regions.size(); i++) {
        if (h->regions[i].first == ptr) {
            // in-flight host-path copies finished when process_* returned (synchronous)
            if (!h->cpu) {
                DeviceGuard g(h->device);
                HIP_TRY(g.err);
                HIP_TRY(hipHostUnregister(ptr));
            }
            h->regions.erase(h->regions.begin() + (long)i);
            return SDDC_OK;
        }
    }
    return fail(SDDC_ERR_ARG, "unregister_host: %p was not registered", ptr);
}

/* ---- batched FFTs (include/sddc_fft.h) ------------------------------------ */
int sddc_fft_supported(int kind, int n)
{
    const bool pow2 = n > 0 && (n & (n - 1)) == 0;
    if (!pow2) return 0;
    if (kind == 0) return n >= 64 && n <= 4096;
    if (kind == 1) return n >= 128 && n <= 8192;
    return 0;
}

int sddc_fft_c2c(const void *in, void *out, int n, int batch, int direction, void *hip_stream)
{
    if (!sddc_fft_supported(0, n)) return fail(SDDC_ERR_ARG, "c2c size %d unsupported (64..4096, power of 2)", n);
    if (batch <= 0 || !in || !out) return fail(SDDC_ERR_ARG, "c2c: batch %d / null buffer", batch);
    if (direction != SDDC_FFT_FORWARD && direction != SDDC_FFT_BACKWARD)
        return fail(SDDC_ERR_ARG, "c2c: direction must be -1 or +1");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(sddc::fft_prepare(s));
    HIP_TRY(sddc::fft_c2c(in, out, n, batch, direction, s));
    return SDDC_OK;
}

int sddc_fft_r2c(const float *in, void *out, int n, int batch, void *hip_stream)
{
    if (!sddc_fft_supported(1, n)) return fail(SDDC_ERR_ARG, "r2c size %d unsupported (128..8192, power of 2)", n);
    if (batch <= 0 || !in || !out) return fail(SDDC_ERR_ARG, "r2c: batch %d / null buffer", batch);
    if (in == out) return fail(SDDC_ERR_ARG, "r2c: in place is not supported");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(sddc::fft_prepare(s));
    HIP_TRY(sddc::fft_r2c(in, out, n, batch, s));
    return SDDC_OK;
}

}  // extern "C"
