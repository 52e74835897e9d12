"""The channel audio resampler (include/sddc_ddc.h, sddc_ddc_channel_audio_resample_*) in numpy: the
definition in float32, operation by operation, that both backends must match bit for bit; the exact
sum in float64 with its error bound; and the seeded inputs of tests/test_channel_audio_resample_cpu.py
and tests/test_gpu_channel_audio_resample.py.

For real sample values x (F32 as stored, S16 as float32(v)) and real taps h, output m of the stream has
m M = s L + p (0 <= p < L), K = ceil(ntaps / L), h[k] = 0 for k >= ntaps, x[i] = 0 for i < 0:
  a[j mod 4] = fmaf(h[p + jL], x[s - j], a[j mod 4])   for j = 0 .. K - 1;   y = (a0 + a1) + (a2 + a3)
resample32 runs exactly this, vectorised across the outputs and never across j.  Its float32 fma is
the product and sum in float64 (the product of two float32 is exact there), the sum corrected to
round-to-odd from its error term, then rounded to float32: the correctly rounded fmaf, as
tools/channel_tone_model.py forms it.

The bound: a float32 dot product of at most K terms, so for any summation order
  |y - y64| <= gamma sum_j |h[p + jL]| |x[s - j]|,   gamma = n u / (1 - n u),  u = 2^-24,  n = K + 1.
S16 output adds 1/2 and the clamp.
"""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
AUDIO_F32, AUDIO_S16 = 0, 1


def fmaf32(a, b, c):
    """float32 fma(a, b, c), correctly rounded."""
    a, b, c = (np.asarray(v, f32).astype(f64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def values(x) -> np.ndarray:
    """float32 [nch, nsamp] sample values of a float32 or int16 array, as a backend reads them."""
    x = np.asarray(x)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    return x.astype(f32)


def count(L: int, M: int, pos: int, nsamp: int) -> int:
    """ceil((pos + nsamp) L / M) - ceil(pos L / M) in exact integers."""
    return -((-(pos + nsamp) * L) // M) - -((-pos * L) // M)


def nsamp_for(L: int, M: int, nout: int) -> int:
    """The fewest samples from position 0 that give nout outputs: floor((nout - 1) M / L) + 1."""
    return ((nout - 1) * M) // L + 1 if nout > 0 else 0


def phase_taps(h, L: int) -> np.ndarray:
    """g[p, j] = h[p + jL], zero beyond ntaps: [L, K] in h's dtype."""
    h = np.asarray(h).reshape(-1)
    K = -(-h.size // L)
    g = np.zeros(L * K, h.dtype)
    g[:h.size] = h
    return np.ascontiguousarray(g.reshape(K, L).T)


def _frames(x: np.ndarray, K: int, L: int, M: int):
    """(frames [nch, nout, K] = x[s - j], phases [nout]) of the whole stream x from position 0."""
    nch, nsamp = x.shape
    m = np.arange(count(L, M, 0, nsamp), dtype=np.int64)
    s, p = (m * M) // L, (m * M) % L
    xp = np.concatenate([np.zeros((nch, K - 1), x.dtype), x], axis=1)
    idx = (s + K - 1)[:, None] - np.arange(K)[None, :]
    return xp[:, idx], p


def resample32(x, taps, L: int, M: int) -> np.ndarray:
    """float32 [nch, ceil(nsamp L / M)]: the definition on the whole stream of sample values x, in the
    definition's order."""
    x = values(x)
    h = np.asarray(taps, f32).reshape(-1)
    K = -(-h.size // L)
    f, p = _frames(x, K, L, M)
    g = phase_taps(h, L)[p]                       # [nout, K]
    a = [np.zeros(f.shape[:2], f32) for _ in range(4)]
    for j in range(K):
        a[j & 3] = fmaf32(g[None, :, j], f[:, :, j], a[j & 3])
    with np.errstate(all="ignore"):
        return ((a[0] + a[1]) + (a[2] + a[3])).astype(f32)


def to_s16(y) -> np.ndarray:
    """demod_math.h's audio rounding: nearest even, clamp to [-32768, 32767], NaN -> 0."""
    y = np.asarray(y, f32)
    with np.errstate(all="ignore"):
        r = np.rint(np.clip(np.where(np.isnan(y), f32(0), y), f32(-32768), f32(32767)))
    return r.astype(np.int16)


def resample_fmt(x, taps, L: int, M: int, out_format: int) -> np.ndarray:
    """resample32 in the output format: float32, or int16 through to_s16."""
    y = resample32(x, taps, L, M)
    return to_s16(y) if out_format == AUDIO_S16 else y


def resample64(x, taps, L: int, M: int) -> np.ndarray:
    """float64 [nch, nout]: the exact sum (to float64 rounding) of the same float32 values and taps."""
    x = values(x).astype(f64)
    h = np.asarray(taps, f32).astype(f64).reshape(-1)
    f, p = _frames(x, -(-h.size // L), L, M)
    return np.einsum("cmk,mk->cm", f, phase_taps(h, L)[p])


def bound(x, taps, L: int, M: int) -> np.ndarray:
    """float64 [nch, nout]: gamma sum_j |h[p + jL]| |x[s - j]| with n = K + 1."""
    x = np.abs(values(x).astype(f64))
    h = np.abs(np.asarray(taps, f32).astype(f64).reshape(-1))
    n = -(-h.size // L) + 1
    gamma = n * U / (1.0 - n * U)
    f, p = _frames(x, n - 1, L, M)
    return gamma * np.einsum("cmk,mk->cm", f, phase_taps(h, L)[p])


def excess(y, x, taps, L: int, M: int, out_format: int = AUDIO_F32) -> float:
    """max over outputs of |y - y64| - bound (S16: against the clamped exact sum, plus 1/2): <= 0 when y
    holds the bound (-inf for a stream without an output)."""
    ref, b = resample64(x, taps, L, M), bound(x, taps, L, M)
    if ref.size == 0:
        return -np.inf
    y = np.asarray(y).astype(f64).reshape(ref.shape)
    if out_format == AUDIO_S16:
        ref, b = np.clip(ref, -32768.0, 32767.0), b + 0.5
    return float((np.abs(y - ref) - b).max())


def make_taps(ntaps: int, seed: int = 23) -> np.ndarray:
    """Seeded float32 taps without symmetry (a swapped orientation or phase shows), all non-zero."""
    rng = np.random.default_rng(seed + ntaps)
    h = rng.uniform(0.25, 1.0, ntaps) * rng.choice([-1.0, 1.0], ntaps) / np.sqrt(ntaps)
    return h.astype(f32)


def make_input(kind: str, nch: int, nsamp: int, fmt: int = AUDIO_F32) -> np.ndarray:
    """The seeded test inputs, [nch, nsamp] in the format's dtype; the channels differ.
    noise: Gaussian, sigma 3000 (F32: with a fraction, S16: rounded codes); edges: full-scale +-32767 /
    -32768 in a seeded order."""
    out = np.zeros((nch, nsamp), f64)
    for c in range(nch):
        rng = np.random.default_rng(700 + c)
        if kind == "noise":
            out[c] = rng.normal(0.0, 3000.0, nsamp)
        elif kind == "edges":
            out[c] = rng.choice(np.array([32767.0, -32768.0]), nsamp)
        else:
            raise ValueError(kind)
    if fmt == AUDIO_S16:
        return np.clip(np.rint(out), -32768, 32767).astype(np.int16)
    return out.astype(f32)
