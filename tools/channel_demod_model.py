"""The channel demodulator (include/sddc_ddc.h, sddc_ddc_channel_demodulate_*) in float64 numpy: the
statement of the definition that every backend is checked against, its error bounds, and the seeded
inputs of tests/test_channel_demod_cpu.py and tests/test_gpu_channel_demod.py.

For channel c with mode m, gain g, BFO word w, stream index i, sample values x[i] = (I, Q) (float32
values as given, CS16: (float32)v * (float32)(1 / cs16_scale)), x[-1] = 0 and stream position p:
  AM   y = g |x[i]|
  FM   y = g angle(x[i] conj(x[i - 1])),   angle(0) = 0
  BFO  y = g Re(x[i] e^{j phi_i}),          phi_i = 2 pi ((w (p + i)) mod 2^32) / 2^32
formed in float64.  The bounds, u = 2^-24 (sddc_ddc.h):
  AM   |y - y64| <= 4 u |y64|
  FM   |y - g theta64| <= |g| (4 u + 8 u |theta64|)      where |x[i]| |x[i - 1]| > 0
  BFO  |y - y64| <= |g| (|I| + |Q|) 6 u
  S16  the model's F32 value converted by the stated rule differs by at most 1 code
  P    |P - P64| <= gamma_n P64,  n = nsamp + 3,  gamma_n = n u / (1 - n u)
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location(
    "channel_decimate_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "channel_decimate_model.py"))
_D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_D)

U = 2.0 ** -24
AM, FM, BFO = 0, 1, 2
F32, S16 = 0, 1
values, cs16_values, as_cf32, as_cs16 = _D.values, _D.cs16_values, _D.as_cf32, _D.as_cs16

# gains that keep every mode's output of the inputs below inside +-30000, so that S16 neither
# clamps nor meets the tests' poison code
GAINS = {AM: 0.5, FM: 9000.0, BFO: 0.4}
S16_POISON = 31000


def make_input(kind: str, nch: int, nsamp: int, pos: int = 0) -> np.ndarray:
    """complex128 [nch, nsamp] with integer parts within int16 (channel_decimate_model.make_input:
    noise, edges, impulse), or kind = "tone": amplitude 12000 at 0.05 + 0.01 c cycles per sample."""
    if kind == "tone":
        t = np.arange(nsamp, dtype=np.float64)
        out = np.zeros((nch, nsamp), np.complex128)
        for c in range(nch):
            v = 12000.0 * np.exp(2j * np.pi * ((0.05 + 0.01 * c) * t + 0.1 * c))
            out[c] = np.rint(v.real) + 1j * np.rint(v.imag)
        return out
    return _D.make_input(kind, nch, nsamp, 8, pos)


def channel_params(nch: int, modes=None):
    """(modes int32, gains float32, words uint32) of nch channels: the modes cycle AM, FM, BFO unless
    given, the gains are GAINS' with a per-channel factor, the words differ per channel."""
    m = np.array([c % 3 for c in range(nch)] if modes is None else modes, np.int32)
    assert m.size == nch
    g = np.array([GAINS[int(k)] * (1.0 - 0.01 * (c % 7)) * (-1.0 if c % 5 == 4 else 1.0) for c, k in enumerate(m)],
                 np.float32)
    w = ((np.arange(nch, dtype=np.uint64) * 2654435761 + 0x12345678) & 0xffffffff).astype(np.uint32)
    return m, g, w


def phase(words, pos: int, nsamp: int) -> np.ndarray:
    """float64 [nch, nsamp]: 2 pi ((w (pos + i)) mod 2^32) / 2^32, exactly reduced."""
    w = np.asarray(words, np.uint64).reshape(-1, 1)
    i = (np.uint64(pos % 2 ** 32) + np.arange(nsamp, dtype=np.uint64)) & np.uint64(0xffffffff)
    return 2.0 * np.pi * ((w * i[None, :]) & np.uint64(0xffffffff)).astype(np.float64) / 2.0 ** 32


def demodulate(x, modes, gains, words, pos: int = 0, prev=None):
    """(y64 float64 [nch, nsamp], theta64 the discriminator's angle (0 elsewhere), mask: False where
    the FM bound does not apply, i.e. |x[i]| |x[i - 1]| == 0) on sample values x (complex128);
    prev: complex [nch] last sample values before x (None: zeros, a new stream)."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    nch, n = x.shape
    g = np.asarray(gains, np.float32).astype(np.float64).reshape(-1, 1)
    m = np.asarray(modes).reshape(-1)
    xp = np.concatenate([np.zeros((nch, 1), np.complex128) if prev is None
                         else np.asarray(prev, np.complex128).reshape(nch, 1), x[:, :-1]], axis=1)
    z = x * np.conj(xp)
    theta = np.arctan2(z.imag, z.real)
    ph = phase(words, pos, n)
    y = np.where((m == AM)[:, None], np.abs(x),
                 np.where((m == FM)[:, None], theta, x.real * np.cos(ph) - x.imag * np.sin(ph))) * g
    theta = np.where((m == FM)[:, None], theta, 0.0)
    mask = ~((m == FM)[:, None] & (np.abs(x) * np.abs(xp) == 0))
    return y, theta, mask


def bound(x, modes, gains, words, pos: int = 0, prev=None) -> np.ndarray:
    """float64 [nch, nsamp]: the bound of |y - y64| per sample (inf where the FM bound does not apply)."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    y, theta, mask = demodulate(x, modes, gains, words, pos, prev)
    g = np.abs(np.asarray(gains, np.float32).astype(np.float64)).reshape(-1, 1)
    m = np.asarray(modes).reshape(-1)
    b = np.where((m == AM)[:, None], 4 * U * np.abs(y),
                 np.where((m == FM)[:, None], g * (4 * U + 8 * U * np.abs(theta)),
                          g * (np.abs(x.real) + np.abs(x.imag)) * 6 * U))
    return np.where(mask, b, np.inf)


def excess(y, x, modes, gains, words, pos: int = 0, prev=None) -> float:
    """max over samples of |y - y64| - bound: <= 0 when y holds the bounds."""
    ref = demodulate(x, modes, gains, words, pos, prev)[0]
    b = bound(x, modes, gains, words, pos, prev)
    d = np.abs(np.asarray(y, np.float64).reshape(ref.shape) - ref)
    return float(np.where(np.isfinite(b), d - b, -1.0).max())


def to_s16(y) -> np.ndarray:
    """SDDC_DDC_AUDIO_S16 of float values: round to nearest even, clamp, NaN -> 0."""
    y = np.asarray(y, np.float64)
    return np.clip(np.rint(np.where(np.isnan(y), 0.0, y)), -32768, 32767).astype(np.int16)


def power(x) -> np.ndarray:
    """float64 [nch]: the mean of |x|^2 over the call."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    return (x.real ** 2 + x.imag ** 2).sum(axis=1) / x.shape[1]


def power_bound(x, factor: float = 1.0) -> np.ndarray:
    """float64 [nch]: factor * gamma_n P64 with n = nsamp + 3."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    n = x.shape[1] + 3
    return factor * (n * U / (1.0 - n * U)) * power(x)
