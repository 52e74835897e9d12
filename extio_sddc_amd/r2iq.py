"""Host-side mirror of the reference's r2iq operator interface over the C ABI.

``R2iq`` exposes the method names and argument meanings of
``r2iqControlClass`` / ``fft_mt_r2iq`` (Core/r2iq.h:16-48,
Core/fft_mt_r2iq.h:21-31) so the parity tests read like the reference's own
tests; the work is done by the gfx950 kernels behind include/sddc_ddc.h.

Reference interface              -> here
  Init(gain, in, out)  .cpp:147  -> R2iq(gain, device)
  setDecimate(d)       r2iq.h:31 -> setDecimate(d)
  updateRand(v)        r2iq.h:25 -> updateRand(v) / getRand()
  setSideband(lsb)     r2iq.h:28 -> setSideband(lsb) / getSideband()
  getRatio()           r2iq.h:21 -> getRatio()
  setFreqOffset(off)   .cpp:101  -> setFreqOffset(off) -> fine-tune residual
  TurnOn()             .cpp:111  -> TurnOn()  (stream reset: zero history)
  worker body  impl.hpp:15-152   -> process(blocks) (host) / process_device(...) (HBM)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import DDCError, check

FMT_CF32 = 0   # SDDC_DDC_FMT_CF32
FMT_CS16 = 1   # SDDC_DDC_FMT_CS16

HALF_FFT = 4096        # fft_mt_r2iq.h:18
BLOCK = 65536          # config.h:80-81 transferSamples
FRAMES = 11            # fft_mt_r2iq.h:19 fftPerBuf
NDEC = 7               # r2iq.h:5 NDECIDX
OUT_BLOCK = 32768      # config.h:62 EXT_BLOCKLEN
NTAPS = 1025
BBRF103_GAINFACTOR = 7.8e-8   # config.h:57; DummyRadio's gain in the reference tests


def output_samples(d: int, nblk: int) -> int:
    return nblk * (OUT_BLOCK >> d)


def kaiser(ntaps: int, astop: float, fpass: float, fstop: float):
    """KaiserWindow (Core/fir.cpp:48-105); ntaps <= 0 returns the tap estimate."""
    L = _lib.load()
    if ntaps <= 0:
        return L.sddc_ddc_kaiser(ntaps, astop, fpass, fstop, None)
    out = np.zeros(ntaps, np.float32)
    n = L.sddc_ddc_kaiser(ntaps, astop, fpass, fstop, out.ctypes.data)
    return out[:n]


def filter_taps(d: int) -> np.ndarray:
    out = np.zeros(NTAPS, np.float32)
    check(_lib.load().sddc_ddc_filter_taps(d, out.ctypes.data))
    return out


def filter_response(gain: float, d: int) -> np.ndarray:
    out = np.zeros((HALF_FFT, 2), np.float32)
    check(_lib.load().sddc_ddc_filter_response(gain, d, out.ctypes.data))
    return out[:, 0] + 1j * out[:, 1]


def channel_tuning(offsets, d: int):
    """setFreqOffset's arithmetic per channel, without a handle (sddc_ddc_channel_tuning):
    offsets (fractions of Fs/2) -> (tunebins int32, fcs float32) for process_channels_device and
    R2iq.setChannelFineTune."""
    L = _lib.load()
    off = np.asarray(offsets, np.float32).reshape(-1)
    tbs, fcs = np.empty(off.size, np.int32), np.empty(off.size, np.float32)
    tb, fc = ctypes.c_int(0), ctypes.c_float(0.0)
    for i, o in enumerate(off):
        check(L.sddc_ddc_channel_tuning(float(o), d, ctypes.byref(tb), ctypes.byref(fc)))
        tbs[i], fcs[i] = tb.value, fc.value
    return tbs, fcs


FFTN = 8192                 # SDDC_DDC_FFTN: samples per frame, the spectrum window's length
SPECTRUM_BINS = 4096        # SDDC_DDC_SPECTRUM_BINS
WINDOW_RECT, WINDOW_HANN, WINDOW_BLACKMAN_HARRIS = 0, 1, 2
_WINDOWS = {"rect": WINDOW_RECT, "hann": WINDOW_HANN, "blackman_harris": WINDOW_BLACKMAN_HARRIS}


def spectrum_window(kind) -> np.ndarray:
    """The library's periodic 8192-point window (sddc_ddc_spectrum_window): kind is WINDOW_RECT /
    WINDOW_HANN / WINDOW_BLACKMAN_HARRIS or "rect" / "hann" / "blackman_harris"."""
    code = _WINDOWS[kind.lower()] if isinstance(kind, str) else int(kind)
    w = np.empty(FFTN, np.float32)
    check(_lib.load().sddc_ddc_spectrum_window(code, w.ctypes.data))
    return w


CHANNEL_SPECTRUM_SIZES = (256, 512, 1024, 2048, 4096)


def window(kind, n: int) -> np.ndarray:
    """The library's periodic n-point window (sddc_ddc_window; n = 2^k, 32..8192): kind as for
    spectrum_window.  window(kind, 8192) equals spectrum_window(kind) bit for bit."""
    code = _WINDOWS[kind.lower()] if isinstance(kind, str) else int(kind)
    w = np.empty(max(int(n), 0), np.float32)
    check(_lib.load().sddc_ddc_window(code, int(n), w.ctypes.data))
    return w


DECIM_MAX_TAPS = 1024       # SDDC_DDC_DECIM_MAX_TAPS
DECIM_MAX_FACTOR = 64       # SDDC_DDC_DECIM_MAX_FACTOR
CHANNEL_DECIMATE_TILE = 512  # ddc_kernels.h kChDecTile: the decimator kernel's outputs per tile


def channel_decimate_samples(factor: int, nsamp: int) -> int:
    """Outputs per channel of a channel_decimate call: nsamp / factor, 0 if the factor is outside
    2..64 or does not divide nsamp (sddc_ddc_channel_decimate_samples)."""
    if nsamp < 0:
        return 0
    return int(_lib.load().sddc_ddc_channel_decimate_samples(int(factor), int(nsamp)))


CHANNEL_RESAMPLE_MAX_UP = 32             # SDDC_DDC_RESAMPLE_MAX_UP
CHANNEL_RESAMPLE_MAX_DOWN = 256          # SDDC_DDC_RESAMPLE_MAX_DOWN
CHANNEL_RESAMPLE_MAX_TAPS = 4096         # SDDC_DDC_RESAMPLE_MAX_TAPS
CHANNEL_RESAMPLE_MAX_PHASE_TAPS = 1024   # SDDC_DDC_RESAMPLE_MAX_PHASE_TAPS: ceil(ntaps / up)


def resample_count(up: int, down: int, pos: int, nsamp: int) -> int:
    """Outputs per channel of a channel_resample call of nsamp samples at stream position pos:
    ceil((pos + nsamp) up / down) - ceil(pos up / down); 0 on factors outside 1..32 / 1..256, not
    coprime or both 1 (sddc_ddc_resample_count)."""
    if nsamp < 0 or pos < 0:
        return 0
    return int(_lib.load().sddc_ddc_resample_count(int(up), int(down), int(pos) & (2 ** 64 - 1), int(nsamp)))


DEMOD_AM, DEMOD_FM, DEMOD_BFO = 0, 1, 2   # SDDC_DDC_DEMOD_*
AUDIO_F32, AUDIO_S16 = 0, 1               # SDDC_DDC_AUDIO_*
CHANNEL_DEMOD_TILE = 2048                 # ddc_kernels.h kChDemTile: the demodulator kernel's samples per tile


def bfo_word(rel: float) -> int:
    """The BFO phase increment of a frequency of rel cycles per sample, rel in [-0.5, 0.5):
    round(rel * 2^32) mod 2^32 (sddc_ddc_bfo_word)."""
    return int(_lib.load().sddc_ddc_bfo_word(float(rel)))


AUDIO_BLOCK = 256                         # SDDC_DDC_AUDIO_BLOCK: the audio filter's block length B
AUDIO_MAX_SECTIONS = 4                    # SDDC_DDC_AUDIO_MAX_SECTIONS
(BIQUAD_IDENTITY, BIQUAD_DC_BLOCK, BIQUAD_ONE_POLE_LP, BIQUAD_LOWPASS, BIQUAD_HIGHPASS,
 BIQUAD_NOTCH) = range(6)                 # SDDC_DDC_BIQUAD_*


def biquad(kind: int, f: float = 0.25, q: float = 0.7071067811865476) -> np.ndarray:
    """One section (b0, b1, b2, a1, a2) as float32 (sddc_ddc_biquad): kind BIQUAD_*, f in cycles per
    sample in (0, 0.5), q read by LOWPASS, HIGHPASS and NOTCH.  DC_BLOCK: the corner; ONE_POLE_LP: a
    de-emphasis of time constant tau at sample rate fs is f = 1 / (2 pi tau fs)."""
    c = np.zeros(5, np.float32)
    check(_lib.load().sddc_ddc_biquad(int(kind), float(f), float(q), c.ctypes.data))
    return c


AGC_BLOCK = 256                           # SDDC_DDC_AGC_BLOCK: the AGC's block length B


def agc_decay(tau_samples: float) -> float:
    """The AGC release factor d of a time constant of tau_samples samples: float32(exp(-1 / tau)),
    1 - 2^-24 if that rounds to 1 (sddc_ddc_agc_decay)."""
    d = ctypes.c_float()
    check(_lib.load().sddc_ddc_agc_decay(float(tau_samples), ctypes.addressof(d)))
    return float(d.value)


BLANKER_BLOCK = 256                       # SDDC_DDC_BLANKER_BLOCK: the noise blanker's block length B
BLANKER_MEAN, BLANKER_MEDIAN = 0, 1       # SDDC_DDC_BLANKER_*: the reference of the last M block powers


def blanker_threshold(db: float) -> float:
    """The noise blanker's threshold k2 of db decibels above the reference power: float32(10^(db / 10)),
    0..120 dB (sddc_ddc_blanker_threshold)."""
    k2 = ctypes.c_float()
    check(_lib.load().sddc_ddc_blanker_threshold(float(db), ctypes.addressof(k2)))
    return float(k2.value)


SQUELCH_BLOCK = 256                       # SDDC_DDC_SQUELCH_BLOCK: the squelch's block length B
SQUELCH_OFF, SQUELCH_LEVEL, SQUELCH_NOISE, SQUELCH_MUTE = 0, 1, 2, 3   # SDDC_DDC_SQUELCH_*: a channel's mode
# SDDC_DDC_SQUELCH_SENSE_*: what the level is measured on
SQUELCH_SENSE_SELF, SQUELCH_SENSE_F32, SQUELCH_SENSE_S16, SQUELCH_SENSE_CF32, SQUELCH_SENSE_CS16 = 0, 1, 2, 3, 4


def squelch_blocks(seconds: float, fs: float) -> int:
    """An attack or a hang of `seconds` at the audio rate fs in blocks of 256 samples, rounded; 0..65535
    (sddc_ddc_squelch_blocks)."""
    b = ctypes.c_int()
    check(_lib.load().sddc_ddc_squelch_blocks(float(seconds), float(fs), ctypes.addressof(b)))
    return int(b.value)


TONE_BLOCK = 256                          # SDDC_DDC_TONE_BLOCK: the tone detector's block length B
# the 50 standard CTCSS frequencies in Hz
CTCSS_TONES = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8,
               118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8,
               177.3, 179.9, 183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6,
               241.8, 250.3, 254.1)


def tone_word(f: float, fs: float) -> int:
    """The phase word of a tone of f Hz at the sample rate fs: round(f / fs * 2^32) mod 2^32 (sddc_ddc_bfo_word)."""
    return bfo_word(float(f) / float(fs))


def tone_window(seconds: float, fs: float) -> int:
    """A window of `seconds` at the rate fs in blocks of 256 samples, rounded, 1..256 (sddc_ddc_tone_window)."""
    b = ctypes.c_int()
    check(_lib.load().sddc_ddc_tone_window(float(seconds), float(fs), ctypes.addressof(b)))
    return int(b.value)


DCS_BLOCK = 256                           # SDDC_DDC_DCS_BLOCK: the DCS decoder's block length B
DCS_ANY, DCS_OFF = -1, -2                 # SDDC_DDC_DCS_ANY (match the whole table), _OFF (bypass)
# the 104 standard DCS codes, as their three octal digits
DCS_CODES = tuple("""023 025 026 031 032 036 043 047 051 053 054 065 071 072 073 074 114 115 116 122 125 131 132 134 143 145 152
155 156 162 165 172 174 205 212 223 225 226 243 244 245 246 251 252 255 261 263 265 266 271 274 306 311 315 325 331 332 343 346
351 356 364 365 371 411 412 413 423 431 432 445 446 452 454 455 462 464 465 466 503 506 516 523 526 532 546 565 606 612 624 627
631 632 654 662 664 703 712 723 731 732 734 743 754""".split())


def dcs_codeword(code) -> int:
    """The 23-bit codeword (bit 0 first on the air) of a DCS code, given as its three octal digits ("023") or as
    the integer 0..511 they spell (sddc_ddc_dcs_codeword): 023 is 0x763813."""
    c = int(code, 8) if isinstance(code, str) else int(code)
    cw = ctypes.c_uint32()
    check(_lib.load().sddc_ddc_dcs_codeword(c, ctypes.addressof(cw)))
    return int(cw.value)


def dcs_window(fs: float, bitrate: float = 134.4):
    """(word, blocks): the bit phase word round(bitrate / fs * 2^32) and the shortest window ceil(24 * 2^32 / (256
    word)) in blocks of 256 samples (sddc_ddc_dcs_window); 8 kS/s gives 6 blocks, 48 kS/s 34."""
    w = ctypes.c_uint32()
    b = ctypes.c_int()
    check(_lib.load().sddc_ddc_dcs_window(float(fs), float(bitrate), ctypes.addressof(w), ctypes.addressof(b)))
    return int(w.value), int(b.value)


STEREO_BLOCK = 256                        # SDDC_DDC_STEREO_BLOCK: the stereo decoder's block length B
STEREO_MONO, STEREO_AUTO = 0, 1           # SDDC_DDC_STEREO_MONO (both outputs are the input), _AUTO


def stereo_pilot_word(fs: float) -> int:
    """The phase word of the 19 kHz stereo pilot at the MPX rate fs: round(19000 / fs * 2^32) (sddc_ddc_bfo_word)."""
    return bfo_word(19000.0 / fs)


def psd_to_dbfs(psd) -> np.ndarray:
    """R2iq.spectrum's output in dB relative to a full-scale real tone (amplitude 32768 reads
    32768^2 / 4 at its bin centre): 10 log10(4 psd / 32768^2); -inf where psd is 0."""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(4.0 * np.asarray(psd, np.float64) / 32768.0 ** 2)


def device_count() -> int:
    return _lib.load().sddc_ddc_device_count()


class R2iq:
    """The DDC for one stream on one GPU (one handle = one r2iq worker).
    ``device=DEVICE_CPU`` (-1) selects the library's AVX2 CPU backend instead (host path only)."""

    def __init__(self, gain: float = 1.0, device: int = 0):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        check(self._L.sddc_ddc_create(gain, device, ctypes.byref(h)))
        self._h = h
        self.gain = gain
        self.device = device
        self._d = 0
        self._rand = False
        self._lsb = False
        self._fmt = FMT_CF32
        self._decim = None   # (ntaps, factor, nch) of setChannelDecimator
        self._resamp = None  # (ntaps, up, down, nch) of setChannelResampler
        self._demod = None   # (nch, out_format) of setChannelDemodulator
        self._audio = None   # (nch, in_format, out_format) of setChannelAudioFilter
        self._aresamp = None  # (nch, in_format, out_format) of setChannelAudioResampler
        self._agc = None     # (nch, in_format, out_format) of setChannelAgc
        self._blanker = None  # (nch, format) of setChannelBlanker
        self._squelch = None  # (nch, sense, in_format, out_format) of setChannelSquelch
        self._tone = None     # (nch, ntones, sense_format, in_format, out_format) of setChannelToneDetector
        self._dcs = None      # (nch, sense_format, in_format, out_format) of setChannelDcsDecoder
        self._stereo = None   # (nch, in_format, out_format) of setChannelStereoDecoder

    # -- lifecycle --------------------------------------------------------
    @property
    def backend(self) -> str:
        """"hip" or "cpu": which backend this handle runs (sddc_ddc_backend)."""
        rc = self._L.sddc_ddc_backend(self._h)
        if rc < 0:
            check(rc)
        return "cpu" if rc == _lib.BACKEND_CPU else "hip"

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.sddc_ddc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- r2iqControlClass -------------------------------------------------
    def setDecimate(self, d: int) -> None:
        check(self._L.sddc_ddc_set_decimation(self._h, d))
        self._d = d

    def getDecimate(self) -> int:
        return self._d

    def getRatio(self) -> int:
        return 1 << self._d          # mratio[mdecimation], fft_mt_r2iq.cpp:32-36

    def updateRand(self, v: bool) -> None:
        check(self._L.sddc_ddc_set_rand(self._h, int(bool(v))))
        self._rand = bool(v)

    def getRand(self) -> bool:
        return self._rand

    def setSideband(self, lsb: bool) -> None:
        check(self._L.sddc_ddc_set_sideband(self._h, int(bool(lsb))))
        self._lsb = bool(lsb)

    def getSideband(self) -> bool:
        return self._lsb

    def setFreqOffset(self, offset: float) -> float:
        return float(self._L.sddc_ddc_set_freq_offset(self._h, offset))

    def setFineTune(self, fc: float) -> None:
        """Fused fine-tune NCO (the mixer RadioHandler applies after the r2iq, pf_mixer.cpp:
        750-856 via RadioHandler.cpp:33-37); fc = the residual from setFreqOffset, 0 = off.
        A new fc restarts the phase at 0, the same fc keeps it (RadioHandler.cpp:291-296)."""
        check(self._L.sddc_ddc_set_fine_tune(self._h, float(fc)))

    def setChannelFineTune(self, fcs) -> None:
        """Per-channel fine-tune NCO of process_channels_device: fcs[c] is channel c's fc (see
        channel_tuning), 0 leaves that channel unmixed; None or empty turns it off.  Per channel
        index an unchanged fc keeps the phase, a changed one restarts it at 0; another channel
        count restarts all (sddc_ddc_set_channel_fine_tune)."""
        if fcs is None or len(fcs) == 0:
            check(self._L.sddc_ddc_set_channel_fine_tune(self._h, None, 0))
            return
        fc = np.ascontiguousarray(np.asarray(fcs, np.float32).reshape(-1))
        check(self._L.sddc_ddc_set_channel_fine_tune(self._h, fc.ctypes.data, fc.size))

    def setTuneBin(self, tunebin: int) -> None:
        check(self._L.sddc_ddc_set_tunebin(self._h, tunebin))

    def getTuneBin(self) -> int:
        return self._L.sddc_ddc_get_tunebin(self._h)

    def TurnOn(self) -> None:
        check(self._L.sddc_ddc_reset(self._h))

    def setHistory(self, last4096: np.ndarray) -> None:
        """The next host-path call starts from these 4096 samples as its history."""
        h = np.ascontiguousarray(last4096, np.int16).reshape(-1)
        if h.size != HALF_FFT:
            raise DDCError(-1, f"history must hold {HALF_FFT} samples")
        check(self._L.sddc_ddc_set_history(self._h, h.ctypes.data))

    # -- the hot loop -----------------------------------------------------
    def setOutputFormat(self, fmt: str = "CF32", scale: float = 1.0) -> None:
        """"CF32" (default, the reference's format) or "CS16": int16 (I, Q) =
        saturate(rint(x * scale)) written by the kernels' output stage."""
        code = {"CF32": FMT_CF32, "CS16": FMT_CS16}[fmt.upper()]
        check(self._L.sddc_ddc_set_output_format(self._h, code, float(scale)))
        self._fmt = code

    def _out_dtype(self):
        return np.int16 if self._fmt == FMT_CS16 else np.float32

    def process(self, blocks: np.ndarray) -> np.ndarray:
        """Stateful host path: nblk blocks (int16) -> nblk*(32768>>d) complex64
        (CS16: an int16 array [n, 2])."""
        blocks = np.ascontiguousarray(blocks, np.int16).reshape(-1)
        if blocks.size % BLOCK:
            raise DDCError(-1, f"input length {blocks.size} is not a multiple of {BLOCK}")
        nblk = blocks.size // BLOCK
        out = np.empty((output_samples(self._d, nblk), 2), self._out_dtype())
        check(self._L.sddc_ddc_process_host(self._h, blocks.ctypes.data, nblk, out.ctypes.data))
        if self._fmt == FMT_CS16:
            return out
        return out.view(np.complex64).reshape(-1)

    def process_blocks(self, blocks) -> np.ndarray:
        """Host path over blocks scattered in memory (ring slots): a list of int16 arrays of
        65536 samples each; same output and history semantics as process()."""
        arrs = [np.ascontiguousarray(b, np.int16).reshape(-1) for b in blocks]
        if any(a.size != BLOCK for a in arrs):
            raise DDCError(-1, f"every block must hold {BLOCK} samples")
        ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        out = np.empty((output_samples(self._d, len(arrs)), 2), self._out_dtype())
        check(self._L.sddc_ddc_process_blocks(self._h, ptrs, len(arrs), out.ctypes.data))
        if self._fmt == FMT_CS16:
            return out
        return out.view(np.complex64).reshape(-1)

    def register_host(self, arr: np.ndarray) -> None:
        """Pin a host array for direct DMA on the host path (unregister before freeing it)."""
        check(self._L.sddc_ddc_register_host(self._h, arr.ctypes.data, arr.nbytes))

    def unregister_host(self, arr: np.ndarray) -> None:
        check(self._L.sddc_ddc_unregister_host(self._h, arr.ctypes.data))

    def process_device(self, d_in, nblk: int, d_out, stream=None) -> None:
        """Stateless HBM path.  d_in: int16 device tensor [4096 + nblk*65536];
        d_out: float32 (CS16: int16) device tensor [>= nblk*(32768>>d)*2].  Enqueued on
        `stream` (a torch.cuda.Stream or raw handle; default: torch's current stream)."""
        _check_device_buffers(d_in, nblk, d_out, output_samples(self._d, nblk) * 2, self._fmt)
        check(self._L.sddc_ddc_process_device(self._h, d_in.data_ptr(), nblk, d_out.data_ptr(),
                                              _stream_handle(stream)))

    def process_channels_device(self, d_in, nblk: int, tunebins, d_out, stream=None) -> None:
        """Many-channel path: d_out float32 (CS16: int16) [nch, nblk*(32768>>d)*2]."""
        tb = np.ascontiguousarray(np.asarray(tunebins, np.int32))
        nch = tb.size
        per = output_samples(self._d, nblk) * 2
        _check_device_buffers(d_in, nblk, d_out, per * nch, self._fmt)
        stride = d_out.stride(0) if d_out.dim() > 1 else per
        check(self._L.sddc_ddc_process_channels_device(self._h, d_in.data_ptr(), nblk, tb.ctypes.data, nch,
                                                       d_out.data_ptr(), stride, _stream_handle(stream)))

    # -- wideband spectrum ---------------------------------------------------
    def setSpectrumWindow(self, w) -> None:
        """The spectrum's 8192-point window (see spectrum_window); None = rectangular (default)."""
        if w is None:
            check(self._L.sddc_ddc_set_spectrum_window(self._h, None))
            return
        w = np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1))
        if w.size != FFTN:
            raise DDCError(-1, f"the spectrum window must hold {FFTN} values")
        check(self._L.sddc_ddc_set_spectrum_window(self._h, w.ctypes.data))

    def spectrum(self, buf: np.ndarray, blocks_per_row: int = 1) -> np.ndarray:
        """Averaged power spectrum of buf = [history 4096 | nblk blocks] (int16), host path:
        [nblk / blocks_per_row, 4096] float32, one row per blocks_per_row blocks (11 frames each).
        Stateless: process()'s history is neither read nor changed."""
        buf = np.ascontiguousarray(buf, np.int16).reshape(-1)
        if buf.size < HALF_FFT + BLOCK or (buf.size - HALF_FFT) % BLOCK:
            raise DDCError(-1, f"input length {buf.size} is not {HALF_FFT} + a multiple of {BLOCK}")
        nblk = (buf.size - HALF_FFT) // BLOCK
        if blocks_per_row < 1 or nblk % blocks_per_row:
            raise DDCError(-1, f"blocks_per_row {blocks_per_row} must be >= 1 and divide nblk {nblk}")
        psd = np.empty((nblk // blocks_per_row, SPECTRUM_BINS), np.float32)
        check(self._L.sddc_ddc_spectrum_host(self._h, buf.ctypes.data, nblk, blocks_per_row, psd.ctypes.data))
        return psd

    def spectrum_device(self, d_in, nblk: int, d_psd, blocks_per_row: int = 1, stream=None) -> None:
        """Stateless HBM path.  d_in: int16 device tensor [4096 + nblk*65536]; d_psd: float32 device
        tensor [>= (nblk / blocks_per_row) * 4096].  Enqueued on `stream` like process_device."""
        if blocks_per_row < 1 or nblk < 1 or nblk % blocks_per_row:
            raise DDCError(-1, f"blocks_per_row {blocks_per_row} must be >= 1 and divide nblk {nblk}")
        _check_device_buffers(d_in, nblk, d_psd, (nblk // blocks_per_row) * SPECTRUM_BINS)
        check(self._L.sddc_ddc_spectrum_device(self._h, d_in.data_ptr(), nblk, blocks_per_row, d_psd.data_ptr(),
                                               _stream_handle(stream)))


    # -- the channel stages' argument checks (spectrum, decimator, resampler) ------
    def _channel_host_array(self, iq):
        """(iq, nch, nsamp) of a channel stage's host input: contiguous, with the channel axis, in
        the handle's output format."""
        iq = np.asarray(iq)
        if self._fmt == FMT_CS16:
            if iq.dtype != np.int16 or iq.ndim not in (2, 3) or iq.shape[-1] != 2:
                raise DDCError(-1, "CS16 handle: iq must be int16 [nch, nsamp, 2]")
            iq = np.ascontiguousarray(iq.reshape((1,) + iq.shape if iq.ndim == 2 else iq.shape))
        else:
            if iq.dtype != np.complex64 or iq.ndim not in (1, 2):
                raise DDCError(-1, "CF32 handle: iq must be complex64 [nch, nsamp]")
            iq = np.ascontiguousarray(iq.reshape(1, -1) if iq.ndim == 1 else iq)
        return iq, iq.shape[0], iq.shape[1]

    def _check_channel_device(self, d_iq, d_out, nch, nsamp, in_stride, nout, out_stride):
        """The tensors of a stream stage's device call: on the device, of the handle's format,
        contiguous, and large enough for nch channels of nsamp samples in and nout out."""
        import torch
        if not (d_iq.is_cuda and d_out.is_cuda):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if self._fmt == FMT_CS16 else torch.float32
        if d_iq.dtype != want or d_out.dtype != torch.float32:
            raise DDCError(-1, f"d_iq must be {want} and d_out float32")
        if not (d_iq.is_contiguous() and d_out.is_contiguous()):
            raise DDCError(-1, "tensors must be contiguous")
        need = (nch - 1) * in_stride + 2 * nsamp
        if d_iq.numel() < need:
            raise DDCError(-1, f"d_iq has {d_iq.numel()} components, need {need}")
        need = (nch - 1) * out_stride + 2 * nout
        if d_out.numel() < need:
            raise DDCError(-1, f"d_out has {d_out.numel()} floats, need {need}")

    # -- channel spectrum ------------------------------------------------------
    def setChannelSpectrumWindow(self, w) -> None:
        """The channel spectrum's window (see window); its length, one of CHANNEL_SPECTRUM_SIZES, is
        the n of the calls that follow.  None = rectangular (default), for any n."""
        if w is None:
            check(self._L.sddc_ddc_set_channel_spectrum_window(self._h, None, 0))
            return
        w = np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1))
        check(self._L.sddc_ddc_set_channel_spectrum_window(self._h, w.ctypes.data, w.size))

    def channel_spectrum(self, iq: np.ndarray, n: int, hop: int = None, frames_per_row: int = 1,
                         nrows: int = None) -> np.ndarray:
        """Averaged power spectrum of the DDC's IQ output, host path: iq is complex64 [nch, nsamp]
        (CF32) or int16 [nch, nsamp, 2] (CS16), matching the handle's output format; a single
        stream may drop the channel axis.  Frame f of row r is the n samples at
        (r * frames_per_row + f) * hop (hop defaults to n / 2), nrows defaults to all whole rows.
        Returns float32 [nch, nrows, n], q = n / 2 the channel's centre, ascending in frequency."""
        iq, nch, nsamp = self._channel_host_array(iq)
        hop = n // 2 if hop is None else int(hop)
        if hop < 1 or frames_per_row < 1 or nsamp < n:
            raise DDCError(-1, f"hop {hop}, frames_per_row {frames_per_row} must be >= 1 and nsamp {nsamp} >= n {n}")
        if nrows is None:
            nrows = ((nsamp - n) // hop + 1) // frames_per_row
        if nrows < 1:
            raise DDCError(-1, f"{nsamp} samples do not hold one row of {frames_per_row} frames")
        psd = np.empty((nch, nrows, max(int(n), 0)), np.float32)
        check(self._L.sddc_ddc_channel_spectrum_host(self._h, iq.ctypes.data, nch, nsamp, 2 * nsamp, int(n), hop,
                                                     int(frames_per_row), int(nrows), psd.ctypes.data))
        return psd

    def channel_spectrum_device(self, d_iq, nch: int, nsamp: int, in_stride: int, n: int, hop: int,
                                frames_per_row: int, nrows: int, d_psd, stream=None) -> None:
        """Stateless HBM path on the buffer process_device / process_channels_device wrote: d_iq is a
        float32 (CS16: int16) device tensor, channel c at c * in_stride components, nsamp complex
        samples each; d_psd float32 [>= nch * nrows * n].  Enqueued on `stream` like process_device."""
        import torch
        if not (d_iq.is_cuda and d_psd.is_cuda):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if self._fmt == FMT_CS16 else torch.float32
        if d_iq.dtype != want or d_psd.dtype != torch.float32:
            raise DDCError(-1, f"d_iq must be {want} and d_psd float32")
        if not (d_iq.is_contiguous() and d_psd.is_contiguous()):
            raise DDCError(-1, "tensors must be contiguous")
        if nch < 1 or nsamp < 1 or nrows < 1 or n < 1:
            raise DDCError(-1, "nch, nsamp, nrows and n must be >= 1")
        need = (nch - 1) * in_stride + 2 * nsamp
        if d_iq.numel() < need:
            raise DDCError(-1, f"d_iq has {d_iq.numel()} components, need {need}")
        if d_psd.numel() < nch * nrows * n:
            raise DDCError(-1, f"d_psd has {d_psd.numel()} floats, need {nch * nrows * n}")
        check(self._L.sddc_ddc_channel_spectrum_device(self._h, d_iq.data_ptr(), nch, nsamp, in_stride, n, hop,
                                                       frames_per_row, nrows, d_psd.data_ptr(),
                                                       _stream_handle(stream)))

    # -- channel decimator ------------------------------------------------------
    def setChannelDecimator(self, taps, factor: int = 0, nch: int = 0) -> None:
        """The streaming decimating FIR of channel_decimate: real taps (1..1024, e.g. from kaiser),
        an integer factor 2..64 and the channel count of the calls that follow.  Every call zeroes
        the kept stream tails.  None or no taps turns the decimator off.  Output m of a channel is
        sum_j taps[j] x[m * factor - j]: the group delay of symmetric taps is (ntaps - 1) / 2 input
        samples."""
        if taps is None or len(taps) == 0:
            check(self._L.sddc_ddc_set_channel_decimator(self._h, None, 0, 0, 0))
            self._decim = None
            return
        t = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        check(self._L.sddc_ddc_set_channel_decimator(self._h, t.ctypes.data, t.size, int(factor), int(nch)))
        self._decim = (t.size, int(factor), int(nch))

    def resetChannelDecimator(self) -> None:
        """Zero every channel's tail: the next channel_decimate call starts a new stream."""
        check(self._L.sddc_ddc_channel_decimator_reset(self._h))

    def channel_decimate(self, iq: np.ndarray) -> np.ndarray:
        """The decimator on host arrays: iq is complex64 [nch, nsamp] (CF32) or int16 [nch, nsamp, 2]
        (CS16), matching the handle's output format, nsamp a multiple of the factor; a single stream
        may drop the channel axis.  Returns complex64 [nch, nsamp / factor] and keeps each
        channel's last ntaps - 1 samples for the next call."""
        if self._decim is None:
            raise DDCError(-4, "no channel decimator set")
        iq, nch, nsamp = self._channel_host_array(iq)
        nout = channel_decimate_samples(self._decim[1], nsamp)
        if nout == 0:
            raise DDCError(-1, f"nsamp {nsamp} must be a positive multiple of the factor {self._decim[1]}")
        out = np.empty((nch, nout), np.complex64)
        check(self._L.sddc_ddc_channel_decimate_host(self._h, iq.ctypes.data, nch, nsamp, 2 * nsamp, out.ctypes.data,
                                                     2 * nout))
        return out

    def channel_decimate_device(self, d_iq, nch: int, nsamp: int, in_stride: int, d_out, out_stride: int,
                                stream=None) -> None:
        """The decimator on the buffer process_device / process_channels_device wrote: d_iq is a
        float32 (CS16: int16) device tensor, channel c at c * in_stride components, nsamp complex
        samples each; d_out float32, channel c's nsamp / factor (I, Q) pairs at c * out_stride
        floats.  Enqueued on `stream` like process_device; the calls of one handle run in call order."""
        if self._decim is None:
            raise DDCError(-4, "no channel decimator set")
        nout = channel_decimate_samples(self._decim[1], nsamp)
        if nch < 1 or nout == 0:
            raise DDCError(-1, f"nch must be >= 1 and nsamp {nsamp} a positive multiple of the factor {self._decim[1]}")
        self._check_channel_device(d_iq, d_out, nch, nsamp, in_stride, nout, out_stride)
        check(self._L.sddc_ddc_channel_decimate_device(self._h, d_iq.data_ptr(), nch, nsamp, in_stride,
                                                       d_out.data_ptr(), out_stride, _stream_handle(stream)))

    # -- channel resampler ------------------------------------------------------
    def setChannelResampler(self, taps, up: int = 0, down: int = 0, nch: int = 0) -> None:
        """The streaming rational up / down polyphase FIR of channel_resample: real prototype taps
        (1..4096, at the input rate x up; ceil(ntaps / up) <= 1024), coprime factors 1..32 and
        1..256, and the channel count of the calls that follow.  There is no implied gain: for
        unity passband gain give taps with DC gain `up` (e.g. up * kaiser(...)).  Every call zeroes
        the kept stream tails and the position.  None or no taps turns the resampler off."""
        if taps is None or len(taps) == 0:
            check(self._L.sddc_ddc_set_channel_resampler(self._h, None, 0, 0, 0, 0))
            self._resamp = None
            return
        t = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        check(self._L.sddc_ddc_set_channel_resampler(self._h, t.ctypes.data, t.size, int(up), int(down), int(nch)))
        self._resamp = (t.size, int(up), int(down), int(nch))

    def resetChannelResampler(self) -> None:
        """Zero every channel's tail and the stream position: the next call starts a new stream."""
        check(self._L.sddc_ddc_channel_resampler_reset(self._h))

    def channel_resample_samples(self, nsamp: int) -> int:
        """Outputs per channel that the NEXT channel_resample call of nsamp samples produces (it
        depends on the stream position; 0 is a legal count)."""
        if self._resamp is None or nsamp < 0:
            return 0
        return int(self._L.sddc_ddc_channel_resample_samples(self._h, int(nsamp)))

    def channel_resample(self, iq: np.ndarray) -> np.ndarray:
        """The resampler on host arrays: iq is complex64 [nch, nsamp] (CF32) or int16 [nch, nsamp, 2]
        (CS16), matching the handle's output format, any nsamp >= 1; a single stream may drop the
        channel axis.  Returns complex64 [nch, nout] (nout may be 0) and keeps each channel's last
        ceil(ntaps / up) - 1 samples and the position for the next call."""
        if self._resamp is None:
            raise DDCError(-4, "no channel resampler set")
        iq, nch, nsamp = self._channel_host_array(iq)
        if nsamp < 1:
            raise DDCError(-1, "nsamp must be >= 1")
        nout = self.channel_resample_samples(nsamp)
        out = np.empty((nch, max(nout, 1)), np.complex64)
        got = ctypes.c_size_t(0)
        check(self._L.sddc_ddc_channel_resample_host(self._h, iq.ctypes.data, nch, nsamp, 2 * nsamp, out.ctypes.data,
                                                     2 * max(nout, 1), ctypes.addressof(got)))
        return out[:, :got.value]

    def channel_resample_device(self, d_iq, nch: int, nsamp: int, in_stride: int, d_out, out_stride: int,
                                stream=None) -> int:
        """The resampler on the buffer process_device / process_channels_device wrote: d_iq is a
        float32 (CS16: int16) device tensor, channel c at c * in_stride components, nsamp complex
        samples each; d_out float32, channel c's nout (I, Q) pairs at c * out_stride floats.  Returns
        nout = channel_resample_samples(nsamp) at the call (possibly 0).  Enqueued on `stream` like
        process_device; the calls of one handle run in call order."""
        if self._resamp is None:
            raise DDCError(-4, "no channel resampler set")
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        nout = self.channel_resample_samples(nsamp)
        self._check_channel_device(d_iq, d_out, nch, nsamp, in_stride, nout, out_stride)
        got = ctypes.c_size_t(0)
        check(self._L.sddc_ddc_channel_resample_device(self._h, d_iq.data_ptr(), nch, nsamp, in_stride,
                                                       d_out.data_ptr(), out_stride, ctypes.addressof(got),
                                                       _stream_handle(stream)))
        return int(got.value)

    # -- channel demodulator ------------------------------------------------------
    def setChannelDemodulator(self, modes, gains=None, bfo_words=None, out_format: int = AUDIO_F32) -> None:
        """The streaming demodulator of channel_demodulate: per channel a mode (DEMOD_AM: g |x|,
        DEMOD_FM: g angle(x[i] conj(x[i - 1])), DEMOD_BFO: g Re(x[i] e^{j 2 pi w (p + i) / 2^32})), a
        finite gain (default 1) and a BFO word (default 0, see bfo_word); out_format AUDIO_F32 or
        AUDIO_S16 (rounded to nearest even and clamped).  Every call zeroes the kept last samples and
        the stream position.  modes=None turns the demodulator off."""
        if modes is None or len(modes) == 0:
            check(self._L.sddc_ddc_set_channel_demodulator(self._h, None, None, None, 0, 0))
            self._demod = None
            return
        m = np.ascontiguousarray(np.asarray(modes, np.int32).reshape(-1))
        g = None if gains is None else np.ascontiguousarray(np.asarray(gains, np.float32).reshape(-1))
        w = None if bfo_words is None else np.ascontiguousarray(
            (np.asarray(bfo_words, np.int64).reshape(-1) & 0xffffffff).astype(np.uint32))
        if (g is not None and g.size != m.size) or (w is not None and w.size != m.size):
            raise DDCError(-1, "gains and bfo_words must have one value per mode")
        check(self._L.sddc_ddc_set_channel_demodulator(self._h, m.ctypes.data, None if g is None else g.ctypes.data,
                                                       None if w is None else w.ctypes.data, m.size, int(out_format)))
        self._demod = (m.size, int(out_format))

    def resetChannelDemodulator(self) -> None:
        """Zero every channel's last sample and the stream position: the next call starts a new stream."""
        check(self._L.sddc_ddc_channel_demodulator_reset(self._h))

    def channel_demodulate(self, iq: np.ndarray, power: bool = False):
        """The demodulator on host arrays: iq is complex64 [nch, nsamp] (CF32) or int16 [nch, nsamp, 2]
        (CS16), matching the handle's output format, any nsamp >= 1; a single stream may drop the
        channel axis.  Returns float32 (AUDIO_S16: int16) [nch, nsamp], with power=True also the
        float32 [nch] mean of |x|^2 over this call, and keeps each channel's last sample and the
        position for the next call."""
        if self._demod is None:
            raise DDCError(-4, "no channel demodulator set")
        iq, nch, nsamp = self._channel_host_array(iq)
        if nsamp < 1:
            raise DDCError(-1, "nsamp must be >= 1")
        out = np.empty((nch, nsamp), np.int16 if self._demod[1] == AUDIO_S16 else np.float32)
        pw = np.empty(nch, np.float32) if power else None
        check(self._L.sddc_ddc_channel_demodulate_host(self._h, iq.ctypes.data, nch, nsamp, 2 * nsamp, out.ctypes.data,
                                                       nsamp, None if pw is None else pw.ctypes.data))
        return (out, pw) if power else out

    def channel_demodulate_device(self, d_iq, nch: int, nsamp: int, in_stride: int, d_out, out_stride: int,
                                  d_power=None, stream=None) -> None:
        """The demodulator on the buffer process_channels_device, channel_decimate_device or
        channel_resample_device wrote: d_iq is a float32 (CS16: int16) device tensor, channel c at
        c * in_stride components, nsamp complex samples each; d_out float32 (AUDIO_S16: int16),
        channel c's nsamp outputs at c * out_stride samples; d_power None or a float32 device tensor
        of nch values.  Enqueued on `stream` like process_device; the calls of one handle run in call
        order."""
        import torch
        if self._demod is None:
            raise DDCError(-4, "no channel demodulator set")
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if not (d_iq.is_cuda and d_out.is_cuda and (d_power is None or d_power.is_cuda)):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if self._fmt == FMT_CS16 else torch.float32
        want_out = torch.int16 if self._demod[1] == AUDIO_S16 else torch.float32
        if d_iq.dtype != want or d_out.dtype != want_out:
            raise DDCError(-1, f"d_iq must be {want} and d_out {want_out}")
        if not (d_iq.is_contiguous() and d_out.is_contiguous()):
            raise DDCError(-1, "tensors must be contiguous")
        need = (nch - 1) * in_stride + 2 * nsamp
        if d_iq.numel() < need:
            raise DDCError(-1, f"d_iq has {d_iq.numel()} components, need {need}")
        need = (nch - 1) * out_stride + nsamp
        if d_out.numel() < need:
            raise DDCError(-1, f"d_out has {d_out.numel()} samples, need {need}")
        if d_power is not None and (d_power.dtype != torch.float32 or not d_power.is_contiguous()
                                    or d_power.numel() < nch):
            raise DDCError(-1, f"d_power must be a contiguous float32 tensor of at least {nch} values")
        check(self._L.sddc_ddc_channel_demodulate_device(self._h, d_iq.data_ptr(), nch, nsamp, in_stride,
                                                         d_out.data_ptr(), out_stride,
                                                         None if d_power is None else d_power.data_ptr(),
                                                         _stream_handle(stream)))


    # -- channel audio resampler ------------------------------------------------------
    def setChannelAudioResampler(self, taps, up: int = 0, down: int = 0, nch: int = 0, in_format: int = AUDIO_F32,
                                 out_format: int = AUDIO_F32) -> None:
        """The streaming rational up / down polyphase FIR of channel_audio_resample on REAL audio
        streams: taps, factors and nch as for setChannelResampler (no implied gain), in_format /
        out_format AUDIO_F32 or AUDIO_S16 (S16 is read as float(v) and written rounded to nearest
        even and clamped).  A GPU handle and a CPU handle produce the same bits.  Every call zeroes
        the kept stream tails and the position.  None or no taps turns the stage off."""
        if taps is None or len(taps) == 0:
            check(self._L.sddc_ddc_set_channel_audio_resampler(self._h, None, 0, 0, 0, 0, 0, 0))
            self._aresamp = None
            return
        t = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        check(self._L.sddc_ddc_set_channel_audio_resampler(self._h, t.ctypes.data, t.size, int(up), int(down), int(nch),
                                                           int(in_format), int(out_format)))
        self._aresamp = (int(nch), int(in_format), int(out_format))

    def setChannelAudioResamplerFormats(self, in_format: int, out_format: int) -> None:
        """The formats of the next calls, the stream left as it is (the tails hold sample values)."""
        if self._aresamp is None:
            raise DDCError(-4, "no channel audio resampler set")
        check(self._L.sddc_ddc_channel_audio_resampler_formats(self._h, int(in_format), int(out_format)))
        self._aresamp = (self._aresamp[0], int(in_format), int(out_format))

    def channel_audio_resampler_reset(self) -> None:
        """Zero every channel's tail and the stream position: the next call starts a new stream."""
        check(self._L.sddc_ddc_channel_audio_resampler_reset(self._h))

    def channel_audio_resample_samples(self, nsamp: int) -> int:
        """Outputs per channel that the NEXT channel_audio_resample call of nsamp samples produces
        (it depends on the stream position; 0 is a legal count)."""
        if self._aresamp is None or nsamp < 0:
            return 0
        return int(self._L.sddc_ddc_channel_audio_resample_samples(self._h, int(nsamp)))

    def channel_audio_resample_host(self, x: np.ndarray) -> np.ndarray:
        """The audio resampler on a host array: x is float32 (AUDIO_S16 in: int16) [nch, nsamp], any
        nsamp >= 1; a single stream may drop the channel axis.  Returns float32 (AUDIO_S16 out: int16)
        [nch, nout] (nout may be 0) and keeps each channel's last ceil(ntaps / up) - 1 sample values
        and the position for the next call."""
        if self._aresamp is None:
            raise DDCError(-4, "no channel audio resampler set")
        _, fin, fout = self._aresamp
        x = np.asarray(x, np.int16 if fin == AUDIO_S16 else np.float32)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[1] < 1:
            raise DDCError(-1, "x must be [nch, nsamp] with nsamp >= 1")
        nch, nsamp = x.shape
        nout = self.channel_audio_resample_samples(nsamp)
        out = np.empty((nch, max(nout, 1)), np.int16 if fout == AUDIO_S16 else np.float32)
        got = ctypes.c_size_t(0)
        check(self._L.sddc_ddc_channel_audio_resample_host(self._h, x.ctypes.data, nch, nsamp, nsamp, out.ctypes.data,
                                                           max(nout, 1), ctypes.addressof(got)))
        return out[:, :got.value]

    def channel_audio_resample_device(self, d_in, nch: int, nsamp: int, in_stride: int, d_out, out_stride: int,
                                      stream=None) -> int:
        """The audio resampler on the buffer channel_demodulate_device (or any audio stage) wrote: d_in
        is a float32 (AUDIO_S16 in: int16) device tensor, channel c's nsamp samples at c * in_stride;
        d_out float32 (AUDIO_S16 out: int16), channel c's nout outputs at c * out_stride.  Returns
        nout = channel_audio_resample_samples(nsamp) at the call (possibly 0).  Enqueued on `stream`
        like process_device; the calls of one handle run in call order."""
        import torch
        if self._aresamp is None:
            raise DDCError(-4, "no channel audio resampler set")
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if not (d_in.is_cuda and d_out.is_cuda):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if self._aresamp[1] == AUDIO_S16 else torch.float32
        want_out = torch.int16 if self._aresamp[2] == AUDIO_S16 else torch.float32
        if d_in.dtype != want or d_out.dtype != want_out:
            raise DDCError(-1, f"d_in must be {want} and d_out {want_out}")
        if not (d_in.is_contiguous() and d_out.is_contiguous()):
            raise DDCError(-1, "tensors must be contiguous")
        nout = self.channel_audio_resample_samples(nsamp)
        for name, t, stride, n in (("d_in", d_in, in_stride, nsamp), ("d_out", d_out, out_stride, nout)):
            need = (nch - 1) * stride + n
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} samples, need {need}")
        got = ctypes.c_size_t(0)
        check(self._L.sddc_ddc_channel_audio_resample_device(self._h, d_in.data_ptr(), nch, nsamp, in_stride,
                                                             d_out.data_ptr(), out_stride, ctypes.addressof(got),
                                                             _stream_handle(stream)))
        return int(got.value)

    # -- channel audio filter -------------------------------------------------------
    def setChannelAudioFilter(self, coeffs, in_format: int = AUDIO_F32, out_format: int = AUDIO_F32) -> None:
        """The streaming biquad cascade of channel_audio_filter: coeffs is float32 [nch, nsec, 5], per
        section (b0, b1, b2, a1, a2) as biquad() returns them, 1 <= nsec <= AUDIO_MAX_SECTIONS (pad a
        shorter channel with biquad(BIQUAD_IDENTITY)); every section must be stable.  in_format /
        out_format AUDIO_F32 or AUDIO_S16.  Every call zeroes the state and the stream position.
        coeffs=None turns the stage off."""
        if coeffs is None or np.size(coeffs) == 0:
            check(self._L.sddc_ddc_set_channel_audio_filter(self._h, None, 0, 0, 0, 0))
            self._audio = None
            return
        c = np.ascontiguousarray(np.asarray(coeffs, np.float32))
        if c.ndim != 3 or c.shape[2] != 5:
            raise DDCError(-1, "coeffs must be [nch, nsec, 5]")
        check(self._L.sddc_ddc_set_channel_audio_filter(self._h, c.ctypes.data, c.shape[1], c.shape[0], int(in_format),
                                                        int(out_format)))
        self._audio = (c.shape[0], int(in_format), int(out_format))

    def resetChannelAudioFilter(self) -> None:
        """Zero every channel's filter state and the stream position: the next call starts a new stream."""
        check(self._L.sddc_ddc_channel_audio_filter_reset(self._h))

    def channel_audio_filter(self, x: np.ndarray) -> np.ndarray:
        """The audio filter on a host array: x is float32 (AUDIO_S16 in: int16) [nch, nsamp], any nsamp
        >= 1; a single stream may drop the channel axis.  Returns float32 (AUDIO_S16 out: int16)
        [nch, nsamp] and keeps every channel's state for the next call."""
        if self._audio is None:
            raise DDCError(-4, "no channel audio filter set")
        nch, fin, fout = self._audio
        x = np.asarray(x, np.int16 if fin == AUDIO_S16 else np.float32)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[1] < 1:
            raise DDCError(-1, "x must be [nch, nsamp] with nsamp >= 1")
        nsamp = x.shape[1]
        out = np.empty((x.shape[0], nsamp), np.int16 if fout == AUDIO_S16 else np.float32)
        check(self._L.sddc_ddc_channel_audio_filter_host(self._h, x.ctypes.data, x.shape[0], nsamp, nsamp,
                                                         out.ctypes.data, nsamp))
        return out

    def channel_audio_filter_device(self, d_in, nch: int, nsamp: int, in_stride: int, d_out, out_stride: int,
                                    stream=None) -> None:
        """The audio filter on the buffer channel_demodulate_device wrote (the same buffer, stride and
        format): d_in is a float32 (AUDIO_S16 in: int16) device tensor, channel c's nsamp samples at
        c * in_stride; d_out float32 (AUDIO_S16 out: int16), channel c's outputs at c * out_stride;
        the two must not overlap.  Enqueued on `stream` like process_device; the calls of one handle
        run in call order."""
        import torch
        if self._audio is None:
            raise DDCError(-4, "no channel audio filter set")
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if not (d_in.is_cuda and d_out.is_cuda):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if self._audio[1] == AUDIO_S16 else torch.float32
        want_out = torch.int16 if self._audio[2] == AUDIO_S16 else torch.float32
        if d_in.dtype != want or d_out.dtype != want_out:
            raise DDCError(-1, f"d_in must be {want} and d_out {want_out}")
        if not (d_in.is_contiguous() and d_out.is_contiguous()):
            raise DDCError(-1, "tensors must be contiguous")
        for name, t, stride in (("d_in", d_in, in_stride), ("d_out", d_out, out_stride)):
            need = (nch - 1) * stride + nsamp
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} samples, need {need}")
        check(self._L.sddc_ddc_channel_audio_filter_device(self._h, d_in.data_ptr(), nch, nsamp, in_stride,
                                                           d_out.data_ptr(), out_stride, _stream_handle(stream)))

    # -- channel AGC ------------------------------------------------------------------
    def setChannelAgc(self, params, in_format: int = AUDIO_F32, out_format: int = AUDIO_F32) -> None:
        """The streaming peak AGC of channel_agc: params is float32 [nch, 3], per channel (T, d, F):
        the target peak level (0: the channel is bypassed), the release factor per sample
        (agc_decay) in [0, 1) and the envelope floor (the largest gain is T / F).  in_format /
        out_format AUDIO_F32 or AUDIO_S16.  Every call zeroes the envelopes and the stream position.
        params=None turns the stage off."""
        if params is None or np.size(params) == 0:
            check(self._L.sddc_ddc_set_channel_agc(self._h, None, 0, 0, 0))
            self._agc = None
            return
        p = np.ascontiguousarray(np.asarray(params, np.float32))
        if p.ndim != 2 or p.shape[1] != 3:
            raise DDCError(-1, "params must be [nch, 3]")
        check(self._L.sddc_ddc_set_channel_agc(self._h, p.ctypes.data, p.shape[0], int(in_format), int(out_format)))
        self._agc = (p.shape[0], int(in_format), int(out_format))

    def resetChannelAgc(self) -> None:
        """Zero every channel's envelopes and the stream position: the next call starts a new stream."""
        check(self._L.sddc_ddc_channel_agc_reset(self._h))

    def channel_agc(self, x: np.ndarray, envelope: bool = False):
        """The AGC on a host array: x is float32 (AUDIO_S16 in: int16) [nch, nsamp], any nsamp >= 1; a
        single stream may drop the channel axis.  Returns float32 (AUDIO_S16 out: int16) [nch, nsamp],
        with envelope=True also the float32 [nch] running envelopes after the last sample, and keeps
        every channel's state for the next call."""
        if self._agc is None:
            raise DDCError(-4, "no channel AGC set")
        nch, fin, fout = self._agc
        x = np.asarray(x, np.int16 if fin == AUDIO_S16 else np.float32)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[1] < 1:
            raise DDCError(-1, "x must be [nch, nsamp] with nsamp >= 1")
        nsamp = x.shape[1]
        out = np.empty((x.shape[0], nsamp), np.int16 if fout == AUDIO_S16 else np.float32)
        env = np.empty(x.shape[0], np.float32) if envelope else None
        check(self._L.sddc_ddc_channel_agc_host(self._h, x.ctypes.data, x.shape[0], nsamp, nsamp, out.ctypes.data, nsamp,
                                                None if env is None else env.ctypes.data))
        return (out, env) if envelope else out

    def channel_agc_device(self, d_in, nch: int, nsamp: int, in_stride: int, d_out, out_stride: int, d_env=None,
                           stream=None) -> None:
        """The AGC on the buffer channel_demodulate_device or channel_audio_filter_device wrote (the same
        buffer, stride and format): d_in is a float32 (AUDIO_S16 in: int16) device tensor, channel c's
        nsamp samples at c * in_stride; d_out float32 (AUDIO_S16 out: int16), channel c's outputs at
        c * out_stride; the two must not overlap; d_env None or a float32 device tensor of nch values
        that receives the running envelopes after the last sample.  Enqueued on `stream` like
        process_device; the calls of one handle run in call order."""
        import torch
        if self._agc is None:
            raise DDCError(-4, "no channel AGC set")
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if not (d_in.is_cuda and d_out.is_cuda and (d_env is None or d_env.is_cuda)):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if self._agc[1] == AUDIO_S16 else torch.float32
        want_out = torch.int16 if self._agc[2] == AUDIO_S16 else torch.float32
        if d_in.dtype != want or d_out.dtype != want_out:
            raise DDCError(-1, f"d_in must be {want} and d_out {want_out}")
        if not (d_in.is_contiguous() and d_out.is_contiguous()):
            raise DDCError(-1, "tensors must be contiguous")
        for name, t, stride in (("d_in", d_in, in_stride), ("d_out", d_out, out_stride)):
            need = (nch - 1) * stride + nsamp
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} samples, need {need}")
        if d_env is not None and (d_env.dtype != torch.float32 or not d_env.is_contiguous() or d_env.numel() < nch):
            raise DDCError(-1, f"d_env must be a contiguous float32 tensor of at least {nch} values")
        check(self._L.sddc_ddc_channel_agc_device(self._h, d_in.data_ptr(), nch, nsamp, in_stride, d_out.data_ptr(),
                                                  out_stride, None if d_env is None else d_env.data_ptr(),
                                                  _stream_handle(stream)))

    # -- channel noise blanker --------------------------------------------------------
    def setChannelBlanker(self, params, guard: int, ref_blocks: int, ref_mode: int = BLANKER_MEAN,
                          fmt: int = FMT_CF32) -> None:
        """The streaming impulse blanker of channel_blank: params is float32 [nch, 2], per channel (k2,
        qmin): the threshold as a power ratio over the reference (blanker_threshold; 0: the channel is
        bypassed, a pure delay) and an absolute floor on |x|^2 below which nothing is blanked.  guard:
        samples blanked on each side of a hit, 0..64, and the delay of every channel; ref_blocks: the
        reference is the BLANKER_MEAN or BLANKER_MEDIAN power of the last 1..16 blocks of 256 samples;
        fmt: FMT_CF32 or FMT_CS16, the format of this stage's buffers.  Every call zeroes the state and
        the stream position.  params=None turns the stage off."""
        if params is None or np.size(params) == 0:
            check(self._L.sddc_ddc_set_channel_blanker(self._h, None, 0, 0, 0, 0, 0))
            self._blanker = None
            return
        p = np.ascontiguousarray(np.asarray(params, np.float32))
        if p.ndim != 2 or p.shape[1] != 2:
            raise DDCError(-1, "params must be [nch, 2]")
        check(self._L.sddc_ddc_set_channel_blanker(self._h, p.ctypes.data, p.shape[0], int(guard), int(ref_blocks),
                                                   int(ref_mode), int(fmt)))
        self._blanker = (p.shape[0], int(fmt))

    def resetChannelBlanker(self) -> None:
        """Zero every channel's state and the stream position: the next call starts a new stream."""
        check(self._L.sddc_ddc_channel_blanker_reset(self._h))

    def channel_blank(self, x: np.ndarray, count: bool = False):
        """The blanker on a host array: x is complex64 [nch, nsamp] (FMT_CS16: int16 [nch, nsamp, 2]), any
        nsamp >= 1; a single stream may drop the channel axis.  Returns the same shape and type, delayed
        by the guard, with count=True also the uint32 [nch] blanked outputs of this call, and keeps every
        channel's state for the next call."""
        if self._blanker is None:
            raise DDCError(-4, "no channel blanker set")
        nch, fmt = self._blanker
        if fmt == FMT_CS16:
            x = np.asarray(x, np.int16)
            if x.ndim == 2:
                x = x[None]
            if x.ndim != 3 or x.shape[2] != 2 or x.shape[1] < 1:
                raise DDCError(-1, "x must be int16 [nch, nsamp, 2] with nsamp >= 1")
        else:
            x = np.asarray(x, np.complex64)
            if x.ndim == 1:
                x = x[None]
            if x.ndim != 2 or x.shape[1] < 1:
                raise DDCError(-1, "x must be complex64 [nch, nsamp] with nsamp >= 1")
        x = np.ascontiguousarray(x)
        nsamp = x.shape[1]
        out = np.empty_like(x)
        cnt = np.empty(x.shape[0], np.uint32) if count else None
        check(self._L.sddc_ddc_channel_blank_host(self._h, x.ctypes.data, x.shape[0], nsamp, 2 * nsamp, out.ctypes.data,
                                                  2 * nsamp, None if cnt is None else cnt.ctypes.data))
        return (out, cnt) if count else out

    def channel_blank_device(self, d_iq, nch: int, nsamp: int, in_stride: int, d_out, out_stride: int, d_count=None,
                             stream=None) -> None:
        """The blanker on a device buffer laid out as process_channels_device writes it: d_iq is a float32
        (FMT_CS16: int16) device tensor of components, channel c's nsamp IQ samples at c * in_stride
        components; d_out the same type, channel c's nsamp outputs at c * out_stride; strides even and
        >= 2 * nsamp; the two must not overlap; d_count None or an int32 device tensor of nch values that
        receives the blanked outputs of this call.  Enqueued on `stream` like process_device; the calls
        of one handle run in call order."""
        import torch
        if self._blanker is None:
            raise DDCError(-4, "no channel blanker set")
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if not (d_iq.is_cuda and d_out.is_cuda and (d_count is None or d_count.is_cuda)):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if self._blanker[1] == FMT_CS16 else torch.float32
        if d_iq.dtype != want or d_out.dtype != want:
            raise DDCError(-1, f"d_iq and d_out must be {want}")
        if not (d_iq.is_contiguous() and d_out.is_contiguous()):
            raise DDCError(-1, "tensors must be contiguous")
        for name, t, stride in (("d_iq", d_iq, in_stride), ("d_out", d_out, out_stride)):
            need = (nch - 1) * stride + 2 * nsamp
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} components, need {need}")
        if d_count is not None and (d_count.dtype != torch.int32 or not d_count.is_contiguous() or d_count.numel() < nch):
            raise DDCError(-1, f"d_count must be a contiguous int32 tensor of at least {nch} values")
        check(self._L.sddc_ddc_channel_blank_device(self._h, d_iq.data_ptr(), nch, nsamp, in_stride, d_out.data_ptr(),
                                                    out_stride, None if d_count is None else d_count.data_ptr(),
                                                    _stream_handle(stream)))

    # -- channel squelch --------------------------------------------------------
    def setChannelSquelch(self, modes, thresholds, attack: int = 1, hang: int = 0, fade: int = 0,
                          sense: int = SQUELCH_SENSE_SELF, fmt_in: int = AUDIO_F32, fmt_out: int = AUDIO_F32) -> None:
        """The streaming gate of channel_squelch: modes is int [nch] (SQUELCH_OFF: always open, _LEVEL: opens on
        a high level, _NOISE: opens on a low level, _MUTE: always closed); thresholds float32 [nch, 2] = (T_open,
        T_close) as mean squares per sample of the sense stream (LEVEL: T_close <= T_open, NOISE: T_close >=
        T_open).  attack: 1..255 blocks of 256 samples above T_open before a channel opens; hang: 0..65535
        blocks it stays open below T_close (squelch_blocks); fade: 1 ramps the opening and the closing block;
        sense: SQUELCH_SENSE_*, what the level is measured on; fmt_in / fmt_out: AUDIO_F32 or AUDIO_S16.
        Every call zeroes the state and the stream position.  modes=None turns the stage off."""
        if modes is None or np.size(modes) == 0:
            check(self._L.sddc_ddc_set_channel_squelch(self._h, None, None, 0, 0, 0, 0, 0, 0, 0))
            self._squelch = None
            return
        m = np.ascontiguousarray(np.asarray(modes, np.int32).reshape(-1))
        t = np.ascontiguousarray(np.asarray(thresholds, np.float32))
        if t.ndim != 2 or t.shape != (m.shape[0], 2):
            raise DDCError(-1, "thresholds must be [nch, 2] with one row per mode")
        check(self._L.sddc_ddc_set_channel_squelch(self._h, m.ctypes.data, t.ctypes.data, m.shape[0], int(attack), int(hang),
                                                   int(fade), int(sense), int(fmt_in), int(fmt_out)))
        self._squelch = (m.shape[0], int(sense), int(fmt_in), int(fmt_out))

    def resetChannelSquelch(self) -> None:
        """Zero every channel's state and the stream position: the next call starts a closed stream."""
        check(self._L.sddc_ddc_channel_squelch_reset(self._h))

    def channel_squelch(self, x: np.ndarray, sense=None, open: bool = True, count: bool = False, level: bool = False):  # noqa: A002
        """The squelch on a host array: x is float32 (AUDIO_S16 in: int16) [nch, nsamp], any nsamp >= 1; a
        single stream may drop the channel axis.  sense: the sense stream of the set kind with the same
        nsamp: float32 or int16 [nch, nsamp], complex64 [nch, nsamp] (SENSE_CF32) or int16 [nch, nsamp, 2]
        (SENSE_CS16); ignored with SENSE_SELF.  Returns float32 (AUDIO_S16 out: int16) [nch, nsamp], followed
        by each side output that is asked for: open (uint32 [nch], `open` after the last completed block),
        count (uint32 [nch], this call's samples in open blocks), level (float32 [nch], the last block level);
        with none of them the outputs alone.  Keeps every channel's state for the next call."""
        if self._squelch is None:
            raise DDCError(-4, "no channel squelch set")
        nch, kind, fin, fout = self._squelch
        x = np.asarray(x, np.int16 if fin == AUDIO_S16 else np.float32)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[1] < 1:
            raise DDCError(-1, "x must be [nch, nsamp] with nsamp >= 1")
        nsamp = x.shape[1]
        sp, sstride = None, 0
        if kind != SQUELCH_SENSE_SELF:
            if sense is None:
                raise DDCError(-1, "this sense kind needs a sense stream")
            cplx = kind in (SQUELCH_SENSE_CF32, SQUELCH_SENSE_CS16)
            s = np.asarray(sense, {SQUELCH_SENSE_F32: np.float32, SQUELCH_SENSE_S16: np.int16,
                                   SQUELCH_SENSE_CF32: np.complex64, SQUELCH_SENSE_CS16: np.int16}[kind])
            if s.ndim == (2 if kind == SQUELCH_SENSE_CS16 else 1):
                s = s[None]
            s = np.ascontiguousarray(s)
            if s.shape[:2] != x.shape or s.shape[2:] != ((2,) if kind == SQUELCH_SENSE_CS16 else ()):
                raise DDCError(-1, "the sense stream must have the audio's [nch, nsamp]")
            sp, sstride = s.ctypes.data, (2 if cplx else 1) * nsamp
        out = np.empty((x.shape[0], nsamp), np.int16 if fout == AUDIO_S16 else np.float32)
        o = np.empty(x.shape[0], np.uint32) if open else None
        c = np.empty(x.shape[0], np.uint32) if count else None
        lv = np.empty(x.shape[0], np.float32) if level else None
        check(self._L.sddc_ddc_channel_squelch_host(self._h, x.ctypes.data, sp, x.shape[0], nsamp, nsamp, sstride,
                                                    out.ctypes.data, nsamp, *(None if a is None else a.ctypes.data
                                                                              for a in (o, c, lv))))
        side = tuple(a for a in (o, c, lv) if a is not None)
        return (out,) + side if side else out

    def channel_squelch_device(self, d_audio, d_sense, nch: int, nsamp: int, in_stride: int, sense_stride: int, d_out,
                               out_stride: int, d_open=None, d_count=None, d_level=None, stream=None) -> None:
        """The squelch on the buffer channel_demodulate_device, channel_audio_filter_device or
        channel_agc_device wrote: d_audio is a float32 (AUDIO_S16 in: int16) device tensor, channel c's nsamp
        samples at c * in_stride; d_sense the sense stream of the set kind (float32 or int16 components,
        channel c's at c * sense_stride components; None with SENSE_SELF); d_out float32 (AUDIO_S16 out:
        int16), channel c's outputs at c * out_stride; d_out must overlap neither input.  d_open, d_count:
        None or int32 device tensors of nch values; d_level: None or a float32 one.  Enqueued on `stream`
        like process_device; the calls of one handle run in call order."""
        import torch
        if self._squelch is None:
            raise DDCError(-4, "no channel squelch set")
        _, kind, fin, fout = self._squelch
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if kind == SQUELCH_SENSE_SELF:
            d_sense = None
        elif d_sense is None:
            raise DDCError(-1, "this sense kind needs d_sense")
        sides = (("d_open", d_open, torch.int32), ("d_count", d_count, torch.int32), ("d_level", d_level, torch.float32))
        if not all(t is None or t.is_cuda for t in (d_audio, d_out, d_sense, d_open, d_count, d_level)):
            raise DDCError(-1, "device path needs device tensors")
        want = torch.int16 if fin == AUDIO_S16 else torch.float32
        want_out = torch.int16 if fout == AUDIO_S16 else torch.float32
        if d_audio.dtype != want or d_out.dtype != want_out:
            raise DDCError(-1, f"d_audio must be {want} and d_out {want_out}")
        bufs = [("d_audio", d_audio, in_stride, 1), ("d_out", d_out, out_stride, 1)]
        if d_sense is not None:
            want_s = torch.int16 if kind in (SQUELCH_SENSE_S16, SQUELCH_SENSE_CS16) else torch.float32
            if d_sense.dtype != want_s:
                raise DDCError(-1, f"d_sense must be {want_s}")
            bufs.append(("d_sense", d_sense, sense_stride, 2 if kind in (SQUELCH_SENSE_CF32, SQUELCH_SENSE_CS16) else 1))
        for name, t, stride, per in bufs:
            if not t.is_contiguous():
                raise DDCError(-1, "tensors must be contiguous")
            need = (nch - 1) * stride + per * nsamp
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} components, need {need}")
        for name, t, dt in sides:
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.numel() < nch):
                raise DDCError(-1, f"{name} must be a contiguous {dt} tensor of at least {nch} values")
        check(self._L.sddc_ddc_channel_squelch_device(self._h, d_audio.data_ptr(), None if d_sense is None else d_sense.data_ptr(),
                                                      nch, nsamp, in_stride, sense_stride, d_out.data_ptr(), out_stride,
                                                      *(None if t is None else t.data_ptr() for _, t, _ in sides),
                                                      _stream_handle(stream)))

    # -- channel tone detector ----------------------------------------------------
    def setChannelToneDetector(self, words, masks, thresholds, window: int = 16, attack: int = 1, hang: int = 0,
                               fmt_sense: int = AUDIO_F32, fmt_in: int = AUDIO_F32, fmt_out: int = AUDIO_F32) -> None:
        """The streaming tone squelch of channel_tone: words is uint32 [ntones], 1..64 phase words (tone_word);
        masks uint64 [nch], the tones each channel listens for (0: bypass, always open); thresholds float32
        [nch, 3] = (rho_open, rho_close, e_min): the share of a window's energy in its best tone that opens and
        that keeps open (0 < rho_close <= rho_open <= 1) and the mean square per sample below which a window is
        silence.  window: 1..256 blocks of 256 samples (tone_window); attack: 1..255 windows before a channel
        opens; hang: 0..65535 windows it stays open without the tone; fmt_*: AUDIO_F32 or AUDIO_S16 of the
        sense stream, the audio and the output.  Every call zeroes the state and the stream position.
        words=None turns the stage off."""
        if words is None or np.size(words) == 0:
            check(self._L.sddc_ddc_set_channel_tone_detector(self._h, None, 0, None, None, 0, 0, 0, 0, 0, 0, 0))
            self._tone = None
            return
        w = np.ascontiguousarray(np.asarray(words, np.uint32).reshape(-1))
        m = np.ascontiguousarray(np.asarray(masks, np.uint64).reshape(-1))
        t = np.ascontiguousarray(np.asarray(thresholds, np.float32))
        if t.ndim != 2 or t.shape != (m.shape[0], 3):
            raise DDCError(-1, "thresholds must be [nch, 3] with one row per mask")
        check(self._L.sddc_ddc_set_channel_tone_detector(self._h, w.ctypes.data, w.shape[0], m.ctypes.data, t.ctypes.data,
                                                         m.shape[0], int(window), int(attack), int(hang), int(fmt_sense),
                                                         int(fmt_in), int(fmt_out)))
        self._tone = (m.shape[0], w.shape[0], int(fmt_sense), int(fmt_in), int(fmt_out))

    def resetChannelToneDetector(self) -> None:
        """Zero every channel's state and the stream position: the next call starts a closed stream."""
        check(self._L.sddc_ddc_channel_tone_reset(self._h))

    def channel_tone(self, sense: np.ndarray, audio=None):
        """The tone detector on host arrays: sense is float32 (AUDIO_S16 sense: int16) [nch, nsamp], any nsamp
        >= 1; audio None (detect only) or float32 / int16 [nch, nsamp]; a single stream may drop the channel
        axis.  Returns a dict: out (float32 / int16 [nch, nsamp], None without audio), tone (int32 [nch], the
        best tone of the last completed window where it held the closing threshold, else -1), open (uint32
        [nch]), count (uint32 [nch], this call's samples in open windows), level (float32 [nch, 2] = P_best, E
        of the last completed window), powers (float32 [nch, ntones]).  Keeps every channel's state for the
        next call."""
        if self._tone is None:
            raise DDCError(-4, "no channel tone detector set")
        nch, ntones, fs, fin, fout = self._tone
        s = np.asarray(sense, np.int16 if fs == AUDIO_S16 else np.float32)
        if s.ndim == 1:
            s = s[None, :]
        s = np.ascontiguousarray(s)
        if s.ndim != 2 or s.shape[1] < 1:
            raise DDCError(-1, "sense must be [nch, nsamp] with nsamp >= 1")
        n, nsamp = s.shape
        a = out = None
        if audio is not None:
            a = np.asarray(audio, np.int16 if fin == AUDIO_S16 else np.float32)
            if a.ndim == 1:
                a = a[None, :]
            a = np.ascontiguousarray(a)
            if a.shape != s.shape:
                raise DDCError(-1, "the audio must have the sense stream's [nch, nsamp]")
            out = np.empty((n, nsamp), np.int16 if fout == AUDIO_S16 else np.float32)
        tone = np.empty(n, np.int32)
        o = np.empty(n, np.uint32)
        c = np.empty(n, np.uint32)
        lv = np.empty((n, 2), np.float32)
        pw = np.empty((n, ntones), np.float32)
        check(self._L.sddc_ddc_channel_tone_host(self._h, s.ctypes.data, nsamp, None if a is None else a.ctypes.data, n, nsamp,
                                                 nsamp, None if out is None else out.ctypes.data, nsamp, tone.ctypes.data,
                                                 o.ctypes.data, c.ctypes.data, lv.ctypes.data, pw.ctypes.data))
        return {"out": out, "tone": tone, "open": o, "count": c, "level": lv, "powers": pw}

    def channel_tone_device(self, d_sense, sense_stride: int, d_audio, nch: int, nsamp: int, in_stride: int, d_out,
                            out_stride: int, d_tone=None, d_open=None, d_count=None, d_level=None, d_powers=None,
                            stream=None) -> None:
        """The tone detector on device buffers: d_sense is a float32 (AUDIO_S16 sense: int16) device tensor,
        channel c's nsamp samples at c * sense_stride; d_audio None (detect only, d_out None too) or the audio
        buffer of the demodulator, the audio filter or the AGC, channel c's samples at c * in_stride, with d_out
        its gated copy at c * out_stride; d_out must overlap neither input.  d_tone, d_open, d_count: None or
        int32 device tensors of nch values; d_level: None or float32 [nch, 2]; d_powers: None or float32 [nch,
        ntones].  Enqueued on `stream` like process_device; the calls of one handle run in call order."""
        import torch
        if self._tone is None:
            raise DDCError(-4, "no channel tone detector set")
        _, ntones, fs, fin, fout = self._tone
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if (d_audio is None) != (d_out is None):
            raise DDCError(-1, "d_audio and d_out go together")
        sides = (("d_tone", d_tone, torch.int32, nch), ("d_open", d_open, torch.int32, nch), ("d_count", d_count, torch.int32, nch),
                 ("d_level", d_level, torch.float32, 2 * nch), ("d_powers", d_powers, torch.float32, nch * ntones))
        if not all(t is None or t.is_cuda for t in (d_sense, d_audio, d_out, d_tone, d_open, d_count, d_level, d_powers)):
            raise DDCError(-1, "device path needs device tensors")
        bufs = [("d_sense", d_sense, sense_stride, torch.int16 if fs == AUDIO_S16 else torch.float32)]
        if d_audio is not None:
            bufs += [("d_audio", d_audio, in_stride, torch.int16 if fin == AUDIO_S16 else torch.float32),
                     ("d_out", d_out, out_stride, torch.int16 if fout == AUDIO_S16 else torch.float32)]
        for name, t, stride, dt in bufs:
            if t is None or t.dtype != dt or not t.is_contiguous():
                raise DDCError(-1, f"{name} must be a contiguous {dt} tensor")
            need = (nch - 1) * stride + nsamp
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} samples, need {need}")
        for name, t, dt, cnt in sides:
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.numel() < cnt):
                raise DDCError(-1, f"{name} must be a contiguous {dt} tensor of at least {cnt} values")
        check(self._L.sddc_ddc_channel_tone_device(self._h, d_sense.data_ptr(), sense_stride,
                                                   None if d_audio is None else d_audio.data_ptr(), nch, nsamp, in_stride,
                                                   None if d_out is None else d_out.data_ptr(), out_stride,
                                                   *(None if t is None else t.data_ptr() for _, t, _, _ in sides),
                                                   _stream_handle(stream)))

    # -- channel DCS decoder -------------------------------------------------------
    def setChannelDcsDecoder(self, codewords, params, word: int, window: int, e_open: int = 1, e_close: int = 2,
                             attack: int = 1, hang: int = 0, fmt_sense: int = AUDIO_F32, fmt_in: int = AUDIO_F32,
                             fmt_out: int = AUDIO_F32) -> None:
        """The streaming digital code squelch of channel_dcs_host / channel_dcs_device: codewords is uint32
        [ncodes], 1..128 23-bit codewords (dcs_codeword); params int32 [nch, 3] = (code, invert, eye): an index
        into the table, DCS_ANY (match the whole table) or DCS_OFF (bypass, always open), whether the received
        word is complemented before matching, and the eye 0..256 that 256 Q / N must reach.  word, window: the bit
        phase word and the window in blocks of 256 samples (dcs_window); e_open <= e_close: 0..3 bit errors that
        open and that keep open; attack: 1..255 windows before a channel opens; hang: 0..65535 windows it stays
        open without the code; fmt_*: AUDIO_F32 or AUDIO_S16 of the sense stream, the audio and the output.
        Every call zeroes the state and the stream position.  codewords=None turns the stage off."""
        if codewords is None or np.size(codewords) == 0:
            check(self._L.sddc_ddc_set_channel_dcs_decoder(self._h, None, 0, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
            self._dcs = None
            return
        cw = np.ascontiguousarray(np.asarray(codewords, np.uint32).reshape(-1))
        p = np.ascontiguousarray(np.asarray(params, np.int32))
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise DDCError(-1, "params must be [nch, 3] = (code, invert, eye)")
        if not 0 <= int(word) < 2 ** 32:
            raise DDCError(-1, "word must be a uint32")
        check(self._L.sddc_ddc_set_channel_dcs_decoder(self._h, cw.ctypes.data, cw.shape[0], p.ctypes.data, p.shape[0], int(word),
                                                       int(window), int(e_open), int(e_close), int(attack), int(hang),
                                                       int(fmt_sense), int(fmt_in), int(fmt_out)))
        self._dcs = (p.shape[0], int(fmt_sense), int(fmt_in), int(fmt_out))

    def resetChannelDcsDecoder(self) -> None:
        """Zero every channel's state and the stream position: the next call starts a closed stream."""
        check(self._L.sddc_ddc_channel_dcs_reset(self._h))

    def channel_dcs_host(self, sense: np.ndarray, audio=None):
        """The DCS decoder on host arrays: sense is float32 (AUDIO_S16 sense: int16) [nch, nsamp], any nsamp >= 1;
        audio None (detect only) or float32 / int16 [nch, nsamp]; a single stream may drop the channel axis.
        Returns a dict: out (float32 / int16 [nch, nsamp], None without audio), code (int32 [nch], the best table
        index of the last completed window where it held the closing limits, else -1), open (uint32 [nch]), count
        (uint32 [nch], this call's samples in open windows), info (uint32 [nch, 4] = Q, N, d, t of the last
        completed window).  Keeps every channel's state for the next call."""
        if self._dcs is None:
            raise DDCError(-4, "no channel DCS decoder set")
        nch, fs, fin, fout = self._dcs
        s = np.asarray(sense, np.int16 if fs == AUDIO_S16 else np.float32)
        if s.ndim == 1:
            s = s[None, :]
        s = np.ascontiguousarray(s)
        if s.ndim != 2 or s.shape[1] < 1:
            raise DDCError(-1, "sense must be [nch, nsamp] with nsamp >= 1")
        n, nsamp = s.shape
        a = out = None
        if audio is not None:
            a = np.asarray(audio, np.int16 if fin == AUDIO_S16 else np.float32)
            if a.ndim == 1:
                a = a[None, :]
            a = np.ascontiguousarray(a)
            if a.shape != s.shape:
                raise DDCError(-1, "the audio must have the sense stream's [nch, nsamp]")
            out = np.empty((n, nsamp), np.int16 if fout == AUDIO_S16 else np.float32)
        code = np.empty(n, np.int32)
        o = np.empty(n, np.uint32)
        c = np.empty(n, np.uint32)
        info = np.empty((n, 4), np.uint32)
        check(self._L.sddc_ddc_channel_dcs_host(self._h, s.ctypes.data, nsamp, None if a is None else a.ctypes.data, n, nsamp,
                                                nsamp, None if out is None else out.ctypes.data, nsamp, code.ctypes.data,
                                                o.ctypes.data, c.ctypes.data, info.ctypes.data))
        return {"out": out, "code": code, "open": o, "count": c, "info": info}

    channel_dcs = channel_dcs_host

    def channel_dcs_device(self, d_sense, sense_stride: int, d_audio, nch: int, nsamp: int, in_stride: int, d_out,
                           out_stride: int, d_code=None, d_open=None, d_count=None, d_info=None, stream=None) -> None:
        """The DCS decoder on device buffers: d_sense is a float32 (AUDIO_S16 sense: int16) device tensor, channel
        c's nsamp samples at c * sense_stride; d_audio None (detect only, d_out None too) or the audio buffer of
        the demodulator, the audio filter or the AGC, channel c's samples at c * in_stride, with d_out its gated
        copy at c * out_stride; d_out must overlap neither input.  d_code, d_open, d_count: None or int32 device
        tensors of nch values; d_info: None or int32 [nch, 4].  Enqueued on `stream` like process_device; the calls
        of one handle run in call order."""
        import torch
        if self._dcs is None:
            raise DDCError(-4, "no channel DCS decoder set")
        _, fs, fin, fout = self._dcs
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        if (d_audio is None) != (d_out is None):
            raise DDCError(-1, "d_audio and d_out go together")
        sides = (("d_code", d_code, torch.int32, nch), ("d_open", d_open, torch.int32, nch), ("d_count", d_count, torch.int32, nch),
                 ("d_info", d_info, torch.int32, 4 * nch))
        if not all(t is None or t.is_cuda for t in (d_sense, d_audio, d_out, d_code, d_open, d_count, d_info)):
            raise DDCError(-1, "device path needs device tensors")
        bufs = [("d_sense", d_sense, sense_stride, torch.int16 if fs == AUDIO_S16 else torch.float32)]
        if d_audio is not None:
            bufs += [("d_audio", d_audio, in_stride, torch.int16 if fin == AUDIO_S16 else torch.float32),
                     ("d_out", d_out, out_stride, torch.int16 if fout == AUDIO_S16 else torch.float32)]
        for name, t, stride, dt in bufs:
            if t is None or t.dtype != dt or not t.is_contiguous():
                raise DDCError(-1, f"{name} must be a contiguous {dt} tensor")
            need = (nch - 1) * stride + nsamp
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} samples, need {need}")
        for name, t, dt, cnt in sides:
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.numel() < cnt):
                raise DDCError(-1, f"{name} must be a contiguous {dt} tensor of at least {cnt} values")
        check(self._L.sddc_ddc_channel_dcs_device(self._h, d_sense.data_ptr(), sense_stride,
                                                  None if d_audio is None else d_audio.data_ptr(), nch, nsamp, in_stride,
                                                  None if d_out is None else d_out.data_ptr(), out_stride,
                                                  *(None if t is None else t.data_ptr() for _, t, _, _ in sides),
                                                  _stream_handle(stream)))

    # -- channel stereo decoder ------------------------------------------------------
    def setChannelStereoDecoder(self, pilot_word: int, modes, params, window: int = 8, attack: int = 1, hang: int = 0,
                                fmt_in: int = AUDIO_F32, fmt_out: int = AUDIO_F32) -> None:
        """The streaming WFM stereo decoder of channel_stereo / channel_stereo_device: pilot_word is the 19 kHz
        pilot's phase word (stereo_pilot_word); modes uint8 [nch], STEREO_MONO (both outputs are the input) or
        STEREO_AUTO; params float32 [nch, 4] = (rho_open, rho_close, e_min, g): the share of a window's energy in
        the pilot that opens and that keeps open (0 < rho_close <= rho_open <= 1; 0.004 and 0.002 are the starting
        point), the mean square per sample below which a window is silence, and the separation gain (1).  window:
        1..256 blocks of 256 samples (8 at 250 kS/s); attack: 1..255 windows before a channel turns stereo; hang:
        0..65535 windows it stays stereo without the pilot; fmt_*: AUDIO_F32 or AUDIO_S16 of the MPX and of the two
        outputs.  Every call starts a new stream.  modes=None turns the stage off."""
        if modes is None or np.size(modes) == 0:
            check(self._L.sddc_ddc_set_channel_stereo_decoder(self._h, 0, None, None, 0, 0, 0, 0, 0, 0))
            self._stereo = None
            return
        m = np.ascontiguousarray(np.asarray(modes, np.uint8).reshape(-1))
        p = np.ascontiguousarray(np.asarray(params, np.float32))
        if p.ndim != 2 or p.shape != (m.shape[0], 4):
            raise DDCError(-1, "params must be [nch, 4] with one row per mode")
        check(self._L.sddc_ddc_set_channel_stereo_decoder(self._h, int(pilot_word) & 0xffffffff, m.ctypes.data, p.ctypes.data,
                                                          m.shape[0], int(window), int(attack), int(hang), int(fmt_in),
                                                          int(fmt_out)))
        self._stereo = (m.shape[0], int(fmt_in), int(fmt_out))

    def resetChannelStereoDecoder(self) -> None:
        """A new stream: every channel mono, q = (1, 0), the position 0."""
        check(self._L.sddc_ddc_channel_stereo_reset(self._h))

    def channel_stereo(self, mpx: np.ndarray):
        """The stereo decoder on host arrays: mpx is float32 (AUDIO_S16 input: int16) [nch, nsamp], any nsamp >= 1; a
        single stream may drop the channel axis.  Returns a dict: left, right (float32 / int16 [nch, nsamp]),
        stereo (uint32 [nch], the gate for the next window), count (uint32 [nch], this call's samples written in
        stereo), level (float32 [nch, 2] = P, E of the last completed window), phase (float32 [nch, 2] = (qr, qi) in
        force).  Keeps every channel's state for the next call."""
        if self._stereo is None:
            raise DDCError(-4, "no channel stereo decoder set")
        nch, fin, fout = self._stereo
        x = np.asarray(mpx, np.int16 if fin == AUDIO_S16 else np.float32)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[1] < 1:
            raise DDCError(-1, "mpx must be [nch, nsamp] with nsamp >= 1")
        n, nsamp = x.shape
        left, right = (np.empty((n, nsamp), np.int16 if fout == AUDIO_S16 else np.float32) for _ in range(2))
        st = np.empty(n, np.uint32)
        c = np.empty(n, np.uint32)
        lv = np.empty((n, 2), np.float32)
        ph = np.empty((n, 2), np.float32)
        check(self._L.sddc_ddc_channel_stereo_host(self._h, x.ctypes.data, n, nsamp, nsamp, left.ctypes.data, right.ctypes.data,
                                                   nsamp, st.ctypes.data, c.ctypes.data, lv.ctypes.data, ph.ctypes.data))
        return {"left": left, "right": right, "stereo": st, "count": c, "level": lv, "phase": ph}

    def channel_stereo_device(self, d_mpx, nch: int, nsamp: int, in_stride: int, d_left, d_right, out_stride: int,
                              d_stereo=None, d_count=None, d_level=None, d_phase=None, stream=None) -> None:
        """The stereo decoder on device buffers: d_mpx is a float32 (AUDIO_S16 input: int16) device tensor, the
        FM demodulator's audio buffer, channel c's nsamp samples at c * in_stride; d_left and d_right take channel
        c's outputs at c * out_stride and overlap neither the input nor each other (two views of one tensor, the
        right one nch * out_stride after the left one, make 2 nch streams for one audio resampler call).  d_stereo,
        d_count: None or int32 device tensors of nch values; d_level, d_phase: None or float32 [nch, 2].  Enqueued on
        `stream` like process_device; the calls of one handle run in call order."""
        import torch
        if self._stereo is None:
            raise DDCError(-4, "no channel stereo decoder set")
        _, fin, fout = self._stereo
        if nch < 1 or nsamp < 1:
            raise DDCError(-1, "nch and nsamp must be >= 1")
        sides = (("d_stereo", d_stereo, torch.int32, nch), ("d_count", d_count, torch.int32, nch),
                 ("d_level", d_level, torch.float32, 2 * nch), ("d_phase", d_phase, torch.float32, 2 * nch))
        if not all(t is not None and t.is_cuda for t in (d_mpx, d_left, d_right)) or \
                not all(t is None or t.is_cuda for _, t, _, _ in sides):
            raise DDCError(-1, "device path needs device tensors")
        odt = torch.int16 if fout == AUDIO_S16 else torch.float32
        bufs = (("d_mpx", d_mpx, in_stride, torch.int16 if fin == AUDIO_S16 else torch.float32),
                ("d_left", d_left, out_stride, odt), ("d_right", d_right, out_stride, odt))
        for name, t, stride, dt in bufs:
            if t.dtype != dt or not t.is_contiguous():
                raise DDCError(-1, f"{name} must be a contiguous {dt} tensor")
            need = (nch - 1) * stride + nsamp
            if t.numel() < need:
                raise DDCError(-1, f"{name} has {t.numel()} samples, need {need}")
        for name, t, dt, cnt in sides:
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.numel() < cnt):
                raise DDCError(-1, f"{name} must be a contiguous {dt} tensor of at least {cnt} values")
        check(self._L.sddc_ddc_channel_stereo_device(self._h, d_mpx.data_ptr(), nch, nsamp, in_stride, d_left.data_ptr(),
                                                     d_right.data_ptr(), out_stride,
                                                     *(None if t is None else t.data_ptr() for _, t, _, _ in sides),
                                                     _stream_handle(stream)))


def _check_device_buffers(d_in, nblk, d_out, out_floats, fmt=0):
    import torch
    if not (d_in.is_cuda and d_out.is_cuda):
        raise DDCError(-1, "device path needs device tensors")
    want = torch.int16 if fmt == FMT_CS16 else torch.float32
    if d_in.dtype != torch.int16 or d_out.dtype != want:
        raise DDCError(-1, f"d_in must be int16 and d_out {want}")
    if not (d_in.is_contiguous() and d_out.is_contiguous()):
        raise DDCError(-1, "tensors must be contiguous")
    if d_in.numel() < HALF_FFT + nblk * BLOCK:
        raise DDCError(-1, f"d_in has {d_in.numel()} samples, need {HALF_FFT + nblk * BLOCK}")
    if d_out.numel() < out_floats:
        raise DDCError(-1, f"d_out has {d_out.numel()} floats, need {out_floats}")


def _stream_handle(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream
