"""The channel decimator (include/sddc_ddc.h, sddc_ddc_channel_decimate_*) in float64 numpy: the
statement of the definition that every backend is checked against, its error bound, and the seeded
inputs of tests/test_channel_decimate_cpu.py and tests/test_gpu_channel_decimate.py.

  v_c[i] = sum_{j < ntaps} h[j] x_c[i - j]      x_c[i] = 0 for i < 0 (zero history)
  y_c[m] = v_c[m R]                              m = 0 .. nsamp / R - 1

x are the float32 sample values as given (CS16: (float32)v * (float32)(1 / cs16_scale)) and h the
float32 taps as given; the sums are formed in float64.

The bound: each component of a backend's y is a float32 dot product of ntaps terms, so for any
summation order, with or without FMA,
  |y - y64| <= gamma sum_j |h[j]| |x[mR - j]|,   gamma = n u / (1 - n u),  u = 2^-24,  n = ntaps + 1,
per output and component, from the model's own sum of |h| |x|.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def values(x) -> np.ndarray:
    """complex128 [nch, nsamp] of float32 sample values given as a complex array."""
    x = np.asarray(x)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    return x.astype(np.complex64).astype(np.complex128)


def cs16_values(codes, cs16_scale: float) -> np.ndarray:
    """The sample values a backend reads from int16 [nch, nsamp, 2] (or [nch, 2 nsamp]) codes:
    (float32)v * (float32)(1 / cs16_scale), as complex128."""
    v = np.asarray(codes, np.int16)
    v = v.reshape(v.shape[0], -1, 2).astype(np.float32) * np.float32(1.0 / float(cs16_scale))
    return v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)


def _frames(x: np.ndarray, ntaps: int, R: int) -> np.ndarray:
    """[nch, nout, ntaps]: x[mR - j] for j = 0 .. ntaps - 1, zero history."""
    nch, nsamp = x.shape
    assert nsamp % R == 0
    xp = np.concatenate([np.zeros((nch, ntaps - 1), x.dtype), x], axis=1)
    idx = (np.arange(nsamp // R) * R + ntaps - 1)[:, None] - np.arange(ntaps)[None, :]
    return xp[:, idx]


def decimate(x, taps, R: int) -> np.ndarray:
    """complex128 [nch, nsamp / R]: the definition on sample values x (see values / cs16_values)."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    h = np.asarray(taps, np.float32).astype(np.float64).reshape(-1)
    return _frames(x, h.size, R) @ h


def bound(x, taps, R: int):
    """(bound of the real parts, bound of the imaginary parts), float64 [nch, nsamp / R] each:
    gamma sum_j |h[j]| |x[mR - j]| with n = ntaps + 1."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    h = np.abs(np.asarray(taps, np.float32).astype(np.float64).reshape(-1))
    n = h.size + 1
    gamma = n * U / (1.0 - n * U)
    return gamma * (_frames(np.abs(x.real), h.size, R) @ h), gamma * (_frames(np.abs(x.imag), h.size, R) @ h)


def excess(y, x, taps, R: int, factor: float = 1.0) -> float:
    """max over outputs and components of |y - y64| - factor * bound: <= 0 when y holds the bound."""
    ref = decimate(x, taps, R)
    br, bi = bound(x, taps, R)
    y = np.asarray(y).astype(np.complex128).reshape(ref.shape)
    return float(max((np.abs(y.real - ref.real) - factor * br).max(), (np.abs(y.imag - ref.imag) - factor * bi).max()))


def make_taps(ntaps: int, seed: int = 7) -> np.ndarray:
    """Seeded float32 taps without symmetry (a swapped orientation shows), all non-zero."""
    rng = np.random.default_rng(seed + ntaps)
    h = rng.uniform(0.25, 1.0, ntaps) * rng.choice([-1.0, 1.0], ntaps) / np.sqrt(ntaps)
    return h.astype(np.float32)


# the two-tone input: a strong tone in the decimated band, a weaker one outside it
TWOTONE_AMPL = (20000.0, 9000.0)


def make_input(kind: str, nch: int, nsamp: int, R: int = 8, pos: int = 0) -> np.ndarray:
    """The seeded test inputs: complex128 [nch, nsamp] with integer parts within int16, so the same
    input serves CF32 (as_cf32) and CS16 (as_cs16).  The channels differ.
    noise: Gaussian, sigma 1000; twotone: tones at 0.11 / R and 0.37 cycles per sample; impulse:
    1.0 at sample `pos` of every channel; edges: full-scale +-32767 / -32768 codes in a seeded order."""
    t = np.arange(nsamp, dtype=np.float64)
    out = np.zeros((nch, nsamp), np.complex128)
    for c in range(nch):
        if kind == "noise":
            rng = np.random.default_rng(300 + c)
            v = rng.normal(0.0, 1000.0, nsamp) + 1j * rng.normal(0.0, 1000.0, nsamp)
        elif kind == "twotone":
            v = (TWOTONE_AMPL[0] * np.exp(2j * np.pi * (0.11 / R * t + 0.1 * (c + 1)))
                 + TWOTONE_AMPL[1] * np.exp(2j * np.pi * (0.37 * t + 0.07 * c)))
        elif kind == "impulse":
            v = np.zeros(nsamp, np.complex128)
            if 0 <= pos < nsamp:
                v[pos] = 1.0
        elif kind == "edges":
            rng = np.random.default_rng(400 + c)
            full = np.array([32767.0, -32768.0])
            v = rng.choice(full, nsamp) + 1j * rng.choice(full, nsamp)
        else:
            raise ValueError(kind)
        out[c] = np.rint(v.real) + 1j * np.rint(v.imag)
    assert np.abs(out.real).max() <= 32768 and np.abs(out.imag).max() <= 32768
    return out


def as_cf32(x, extra: int = 0, fill: float = 0.0) -> np.ndarray:
    """float32 [nch, 2 nsamp + extra] components (extra: unused components between the streams,
    holding `fill`)."""
    x = np.asarray(x)
    buf = np.full((x.shape[0], 2 * x.shape[1] + extra), fill, np.float32)
    buf[:, 0:2 * x.shape[1]:2] = x.real
    buf[:, 1:2 * x.shape[1]:2] = x.imag
    return buf


def as_cs16(x, extra: int = 0, fill: int = 0) -> np.ndarray:
    """int16 [nch, 2 nsamp + extra] codes; the sample value is this * (float32)(1 / cs16_scale)."""
    x = np.asarray(x)
    buf = np.full((x.shape[0], 2 * x.shape[1] + extra), fill, np.int16)
    buf[:, 0:2 * x.shape[1]:2] = np.clip(x.real, -32768, 32767).astype(np.int16)
    buf[:, 1:2 * x.shape[1]:2] = np.clip(x.imag, -32768, 32767).astype(np.int16)
    return buf
