"""The wideband averaged power spectrum (include/sddc_ddc.h, sddc_ddc_spectrum_*) in float64 numpy:
the statement of the definition that every backend is checked against, and the seeded inputs of
tests/test_spectrum_cpu.py and tests/test_gpu_spectrum.py.

  buf       = [history 4096 | nblk blocks of 65536] int16
  frame k of block b = the 8192 samples at 65536 b + 6144 k, k = 0..10
  X_f[k]    = sum_j w[j] x_f[j] e^{-2 pi i jk/8192},  k = 0..4095
  psd[r][k] = 1/(11 bpr) sum_{frames f of row r} |X_f[k]|^2 / (sum_j w[j])^2
"""
from __future__ import annotations

import numpy as np

HALF, FFTN, HOP, BLOCK, FRAMES = 4096, 8192, 6144, 65536, 11

# periodic cosine-sum windows: w[j] = sum_m (-1)^m a_m cos(2 pi m j / 8192)
COEFFS = {
    "rect": (1.0,),
    "hann": (0.5, 0.5),
    "blackman_harris": (0.35875, 0.48829, 0.14128, 0.01168),
}
# a 7-term flat-top (HFT144D): negative lobes, positive sum
FLATTOP7 = (1.0, 1.96760033, 1.57983607, 0.81123644, 0.22583558, 0.02773848, 0.00090360)


def cosine_window(coeffs) -> np.ndarray:
    """float64 periodic window over 8192 points."""
    j = np.arange(FFTN, dtype=np.float64)
    w = np.zeros(FFTN)
    for m, a in enumerate(coeffs):
        w += (-1.0) ** m * a * np.cos(2.0 * np.pi * m * j / FFTN)
    return w


def window(kind: str) -> np.ndarray:
    return cosine_window(COEFFS[kind])


def derandomise(x: np.ndarray) -> np.ndarray:
    """convert_float<rand>: an odd sample v is v ^ 0xFFFE = -v."""
    x = np.asarray(x).astype(np.int64)
    return np.where(x & 1, -x, x)


def randomise(x: np.ndarray) -> np.ndarray:
    """The ADC's randomiser on int16 samples: odd samples XORed with -2 (its own inverse)."""
    x = np.asarray(x, np.int16)
    return np.where(x & 1, x ^ np.int16(-2), x).astype(np.int16)


def psd(buf, nblk: int, bpr: int = 1, w=None, rand: bool = False) -> np.ndarray:
    """float64 [nblk / bpr, 4096]; w: the 8192-point window as the backend holds it (None = rectangular)."""
    buf = np.asarray(buf).reshape(-1)
    assert buf.size == HALF + nblk * BLOCK and bpr >= 1 and nblk % bpr == 0
    x = (derandomise(buf) if rand else buf).astype(np.float64)
    w = np.ones(FFTN) if w is None else np.asarray(w, np.float64)
    out = np.zeros((nblk // bpr, HALF))
    for b in range(nblk):
        idx = BLOCK * b + HOP * np.arange(FRAMES)[:, None] + np.arange(FFTN)[None, :]
        X = np.fft.rfft(x[idx] * w[None, :], axis=1)[:, :HALF]
        out[b // bpr] += (X.real ** 2 + X.imag ** 2).sum(axis=0)
    return out / (FRAMES * bpr * w.sum() ** 2)


def dbfs(p) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(4.0 * np.asarray(p, np.float64) / 32768.0 ** 2)


def make_input(kind: str, nblk: int) -> np.ndarray:
    """The seeded test inputs, int16 [4096 + nblk * 65536]."""
    L = HALF + nblk * BLOCK
    t = np.arange(L, dtype=np.float64)
    if kind == "noise":
        v = np.random.default_rng(7).normal(0.0, 3000.0, L)
    elif kind == "twotone":   # a near-full-scale off-bin tone + a -80 dBFS on-bin tone (bin 3000)
        v = (30000.0 * np.cos(2.0 * np.pi * 1234.37 / FFTN * t + 0.3) + 3.2768 * np.cos(2.0 * np.pi * 3000.0 / FFTN * t)
             + np.random.default_rng(11).uniform(-0.5, 0.5, L))
    elif kind == "fs4":       # the bin next to the split's pivot
        v = 32767.0 * np.cos(2.0 * np.pi * 2047.0 / FFTN * t)
    else:
        raise ValueError(kind)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)
