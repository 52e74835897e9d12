"""extio_sddc_amd — MI355X-native real-to-IQ DDC (drop-in for ExtIO_sddc's fft_mt_r2iq).

The product is the gfx950 library behind include/sddc_ddc.h and the drop-in C++
class in include/fft_mt_r2iq.h; this package is its Python host mirror (ctypes).
"""
from ._lib import BACKEND_CPU, BACKEND_HIP, DEVICE_CPU, DDCError, build, load  # noqa: F401
from .r2iq import (BBRF103_GAINFACTOR, BLOCK, FRAMES, HALF_FFT, NDEC, OUT_BLOCK,  # noqa: F401
                   R2iq, channel_tuning, device_count, filter_response, filter_taps, kaiser, output_samples)
from .r2iq import (FFTN, SPECTRUM_BINS, WINDOW_BLACKMAN_HARRIS, WINDOW_HANN, WINDOW_RECT,  # noqa: F401
                   psd_to_dbfs, spectrum_window)
from .r2iq import CHANNEL_SPECTRUM_SIZES, window  # noqa: F401
from .r2iq import (CHANNEL_DECIMATE_TILE, DECIM_MAX_FACTOR, DECIM_MAX_TAPS,  # noqa: F401
                   channel_decimate_samples)
from .r2iq import (CHANNEL_RESAMPLE_MAX_DOWN, CHANNEL_RESAMPLE_MAX_PHASE_TAPS,  # noqa: F401
                   CHANNEL_RESAMPLE_MAX_TAPS, CHANNEL_RESAMPLE_MAX_UP, resample_count)
from .r2iq import (AUDIO_F32, AUDIO_S16, CHANNEL_DEMOD_TILE, DEMOD_AM, DEMOD_BFO, DEMOD_FM,  # noqa: F401
                   bfo_word)
from .r2iq import (AUDIO_BLOCK, AUDIO_MAX_SECTIONS, BIQUAD_DC_BLOCK, BIQUAD_HIGHPASS, BIQUAD_IDENTITY,  # noqa: F401
                   BIQUAD_LOWPASS, BIQUAD_NOTCH, BIQUAD_ONE_POLE_LP, biquad)
from .r2iq import AGC_BLOCK, agc_decay  # noqa: F401
from .r2iq import BLANKER_BLOCK, BLANKER_MEAN, BLANKER_MEDIAN, blanker_threshold  # noqa: F401
from .r2iq import (SQUELCH_BLOCK, SQUELCH_LEVEL, SQUELCH_MUTE, SQUELCH_NOISE, SQUELCH_OFF, SQUELCH_SENSE_CF32,  # noqa: F401
                   SQUELCH_SENSE_CS16, SQUELCH_SENSE_F32, SQUELCH_SENSE_S16, SQUELCH_SENSE_SELF, squelch_blocks)
from .r2iq import CTCSS_TONES, TONE_BLOCK, tone_window, tone_word  # noqa: F401
from .r2iq import DCS_ANY, DCS_BLOCK, DCS_CODES, DCS_OFF, dcs_codeword, dcs_window  # noqa: F401
from .r2iq import STEREO_AUTO, STEREO_BLOCK, STEREO_MONO, stereo_pilot_word  # noqa: F401

__all__ = ["R2iq", "DDCError", "DEVICE_CPU", "BACKEND_CPU", "BACKEND_HIP", "build", "load", "kaiser", "filter_taps", "filter_response",
           "channel_tuning", "device_count", "output_samples", "HALF_FFT", "BLOCK", "FRAMES", "NDEC", "OUT_BLOCK",
           "BBRF103_GAINFACTOR", "spectrum_window", "psd_to_dbfs", "FFTN", "SPECTRUM_BINS", "WINDOW_RECT", "WINDOW_HANN",
           "WINDOW_BLACKMAN_HARRIS", "window", "CHANNEL_SPECTRUM_SIZES", "channel_decimate_samples", "CHANNEL_DECIMATE_TILE",
           "DECIM_MAX_TAPS", "DECIM_MAX_FACTOR", "resample_count", "CHANNEL_RESAMPLE_MAX_UP", "CHANNEL_RESAMPLE_MAX_DOWN",
           "CHANNEL_RESAMPLE_MAX_TAPS", "CHANNEL_RESAMPLE_MAX_PHASE_TAPS", "DEMOD_AM", "DEMOD_FM", "DEMOD_BFO", "AUDIO_F32",
           "AUDIO_S16", "CHANNEL_DEMOD_TILE", "bfo_word", "AUDIO_BLOCK", "AUDIO_MAX_SECTIONS", "BIQUAD_IDENTITY",
           "BIQUAD_DC_BLOCK", "BIQUAD_ONE_POLE_LP", "BIQUAD_LOWPASS", "BIQUAD_HIGHPASS", "BIQUAD_NOTCH", "biquad",
           "AGC_BLOCK", "agc_decay", "BLANKER_BLOCK", "BLANKER_MEAN", "BLANKER_MEDIAN", "blanker_threshold",
           "SQUELCH_BLOCK", "SQUELCH_OFF", "SQUELCH_LEVEL", "SQUELCH_NOISE", "SQUELCH_MUTE", "SQUELCH_SENSE_SELF",
           "SQUELCH_SENSE_F32", "SQUELCH_SENSE_S16", "SQUELCH_SENSE_CF32", "SQUELCH_SENSE_CS16", "squelch_blocks",
           "TONE_BLOCK", "CTCSS_TONES", "tone_word", "tone_window", "DCS_BLOCK", "DCS_ANY", "DCS_OFF", "DCS_CODES",
           "dcs_codeword", "dcs_window", "STEREO_BLOCK", "STEREO_MONO", "STEREO_AUTO", "stereo_pilot_word"]
