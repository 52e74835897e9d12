"""The channel resampler (include/sddc_ddc.h, sddc_ddc_channel_resample_*) in float64 numpy: the
statement of the definition that every backend is checked against, its error bound, and the seeded
inputs of tests/test_channel_resample_cpu.py and tests/test_gpu_channel_resample.py.

  u_c[iL] = x_c[i], 0 elsewhere;   v_c[n] = sum_k h[k] u_c[n - k];   y_c[m] = v_c[mM]
in its polyphase form, with mM = sL + p (0 <= p < L), K = ceil(ntaps / L), h[k] = 0 for k >= ntaps:
  y_c[m] = sum_{j < K} h[p + jL] x_c[s - j]      x_c[i] = 0 for i < 0 (zero history)
for the stream's outputs m = ceil(pos L / M) .. ceil((pos + nsamp) L / M) - 1 of a call of nsamp
samples at position pos (count()).

x are the float32 sample values as given (CS16: (float32)v * (float32)(1 / cs16_scale)) and h the
float32 taps as given; the sums are formed in float64.

The bound: each component of a backend's y is a float32 dot product of at most K terms, so for any
summation order, with or without FMA,
  |y - y64| <= gamma sum_j |h[p + jL]| |x[s - j]|,   gamma = n u / (1 - n u),  u = 2^-24,  n = K + 1,
per output and component, from the model's own sum of |g| |x|.
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


def count(L: int, M: int, pos: int, nsamp: int) -> int:
    """ceil((pos + nsamp) L / M) - ceil(pos L / M) in exact integers."""
    return -((-(pos + nsamp) * L) // M) - -((-pos * L) // M)


def _frames(x: np.ndarray, ntaps: int, L: int, M: int):
    """(frames [nch, nout, K] = x[s - j], phases [nout]) of the whole stream x from position 0."""
    nch, nsamp = x.shape
    K = -(-ntaps // L)
    m = np.arange(count(L, M, 0, nsamp), dtype=np.int64)
    s, p = (m * M) // L, (m * M) % L
    xp = np.concatenate([np.zeros((nch, K - 1), x.dtype), x], axis=1)
    idx = (s + K - 1)[:, None] - np.arange(K)[None, :]
    return xp[:, idx], p


def _phase_taps(h: np.ndarray, L: int) -> np.ndarray:
    """g[p, j] = h[p + jL], zero beyond ntaps: float64 [L, K]."""
    K = -(-h.size // L)
    g = np.zeros(L * K, np.float64)
    g[:h.size] = h
    return np.ascontiguousarray(g.reshape(K, L).T)


def resample(x, taps, L: int, M: int) -> np.ndarray:
    """complex128 [nch, ceil(nsamp L / M)]: the definition on the whole stream of sample values x."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    h = np.asarray(taps, np.float32).astype(np.float64).reshape(-1)
    f, p = _frames(x, h.size, L, M)
    return np.einsum("cmk,mk->cm", f, _phase_taps(h, L)[p])


def bound(x, taps, L: int, M: int):
    """(bound of the real parts, bound of the imaginary parts), float64 [nch, nout] each:
    gamma sum_j |h[p + jL]| |x[s - j]| with n = K + 1."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    h = np.abs(np.asarray(taps, np.float32).astype(np.float64).reshape(-1))
    n = -(-h.size // L) + 1
    gamma = n * U / (1.0 - n * U)
    g = _phase_taps(h, L)
    fr, p = _frames(np.abs(x.real), h.size, L, M)
    fi, _ = _frames(np.abs(x.imag), h.size, L, M)
    return gamma * np.einsum("cmk,mk->cm", fr, g[p]), gamma * np.einsum("cmk,mk->cm", fi, g[p])


def excess(y, x, taps, L: int, M: int, factor: float = 1.0) -> float:
    """max over outputs and components of |y - y64| - factor * bound: <= 0 when y holds the bound
    (-inf for a stream without an output)."""
    ref = resample(x, taps, L, M)
    br, bi = bound(x, taps, L, M)
    y = np.asarray(y).astype(np.complex128).reshape(ref.shape)
    if ref.size == 0:
        return -np.inf
    return float(max((np.abs(y.real - ref.real) - factor * br).max(), (np.abs(y.imag - ref.imag) - factor * bi).max()))


def make_taps(ntaps: int, seed: int = 11) -> np.ndarray:
    """Seeded float32 taps without symmetry (a swapped orientation or phase shows), all non-zero."""
    rng = np.random.default_rng(seed + ntaps)
    h = rng.uniform(0.25, 1.0, ntaps) * rng.choice([-1.0, 1.0], ntaps) / np.sqrt(ntaps)
    return h.astype(np.float32)


def make_input(kind: str, nch: int, nsamp: int, pos: int = 0) -> np.ndarray:
    """The seeded test inputs: complex128 [nch, nsamp] with integer parts within int16, so the same
    input serves CF32 (as_cf32) and CS16 (as_cs16).  The channels differ.
    noise: Gaussian, sigma 1000; impulse: 1.0 at sample `pos` of every channel; edges: full-scale
    +-32767 / -32768 codes in a seeded order."""
    out = np.zeros((nch, nsamp), np.complex128)
    for c in range(nch):
        if kind == "noise":
            rng = np.random.default_rng(500 + c)
            v = rng.normal(0.0, 1000.0, nsamp) + 1j * rng.normal(0.0, 1000.0, nsamp)
        elif kind == "impulse":
            v = np.zeros(nsamp, np.complex128)
            if 0 <= pos < nsamp:
                v[pos] = 1.0
        elif kind == "edges":
            rng = np.random.default_rng(600 + c)
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


def nsamp_for(L: int, M: int, nout: int) -> int:
    """The fewest samples from position 0 that give nout outputs: floor((nout - 1) M / L) + 1."""
    return ((nout - 1) * M) // L + 1 if nout > 0 else 0
