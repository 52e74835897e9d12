"""The channel spectrum (include/sddc_ddc.h, sddc_ddc_channel_spectrum_*) in float64 numpy: the
statement of the definition that every backend is checked against, and the seeded inputs of
tests/test_channel_spectrum_cpu.py and tests/test_gpu_channel_spectrum.py.

  x[c]         = channel c's complex samples (CS16: the int16 pair / cs16_scale)
  frame f of row r starts at sample (r fpr + f) hop
  X_f[k]       = sum_j w[j] x[start_f + j] e^{-2 pi i jk/n},   k = 0..n-1
  psd[c][r][q] = 1/fpr sum_{f < fpr} |X_f[(q + n/2) mod n]|^2 / (sum_j w[j])^2

q ascends in frequency: q = n/2 is DC, q = 0 is -fs/2 (np.fft.fftshift).
"""
from __future__ import annotations

import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)

# periodic cosine-sum windows: w[j] = sum_m (-1)^m a_m cos(2 pi m j / n)
COEFFS = {
    "rect": (1.0,),
    "hann": (0.5, 0.5),
    "blackman_harris": (0.35875, 0.48829, 0.14128, 0.01168),
}


def window(kind: str, n: int) -> np.ndarray:
    """float64 periodic window over n points."""
    j = np.arange(n, dtype=np.float64)
    w = np.zeros(n)
    for m, a in enumerate(COEFFS[kind]):
        w += (-1.0) ** m * a * np.cos(2.0 * np.pi * m * j / n)
    return w


def nsamp_for(n: int, hop: int, fpr: int, nrows: int) -> int:
    """The shortest stream that holds nrows rows: (nrows fpr - 1) hop + n."""
    return (nrows * fpr - 1) * hop + n


def psd(x, n: int, hop: int, fpr: int, nrows: int, w=None) -> np.ndarray:
    """float64 [nch, nrows, n] of x = complex [nch, nsamp]; w: the n-point window as the backend
    holds it (None = rectangular)."""
    x = np.asarray(x, np.complex128)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    assert nsamp_for(n, hop, fpr, nrows) <= x.shape[1]
    w = np.ones(n) if w is None else np.asarray(w, np.float64)
    assert w.shape == (n,)
    starts = (np.arange(nrows * fpr) * hop)[:, None] + np.arange(n)[None, :]
    X = np.fft.fftshift(np.fft.fft(x[:, starts] * w, axis=-1), axes=-1)     # [nch, nrows fpr, n]
    p = (X.real ** 2 + X.imag ** 2).reshape(x.shape[0], nrows, fpr, n).sum(axis=2)
    return p / (fpr * w.sum() ** 2)


# the two-tone input: a strong tone between bins, 80 dB below it a tone on a bin centre
TWOTONE_AMPL = 30000.0
TWOTONE_WEAK = TWOTONE_AMPL * 1e-4


def twotone_bins(n: int):
    """(the strong tone's frequency in bins, the weak tone's bin, the quiet bins away from both),
    as signed bins: q = bin + n/2."""
    return -(n // 5) + 0.37, 3 * n // 16, np.arange(n // 4, 3 * n // 8)


# the edges input: (signed bin, amplitude); q = 0, n/2 and 3n/4
def edges_tones(n: int):
    return ((-n // 2, 8000.0), (0, 5000.0), (n // 4, 3000.0))


def make_input(kind: str, n: int, nch: int, nsamp: int) -> np.ndarray:
    """The seeded test inputs: complex128 [nch, nsamp] with integer parts within int16, so the same
    input serves CF32 (as_cf32) and CS16 (as_cs16).  The channels differ."""
    t = np.arange(nsamp, dtype=np.float64)
    out = np.empty((nch, nsamp), np.complex128)
    for c in range(nch):
        if kind == "noise":
            rng = np.random.default_rng(100 + c)
            v = rng.normal(0.0, 1000.0, nsamp) + 1j * rng.normal(0.0, 1000.0, nsamp)
        elif kind == "twotone":
            b1, b2, _ = twotone_bins(n)
            rng = np.random.default_rng(200 + c)
            v = (TWOTONE_AMPL * np.exp(2j * np.pi * (b1 * t / n + 0.1 * (c + 1)))
                 + TWOTONE_WEAK * np.exp(2j * np.pi * (b2 * t / n + 0.07 * c))
                 + rng.uniform(-0.5, 0.5, nsamp) + 1j * rng.uniform(-0.5, 0.5, nsamp))
        elif kind == "edges":
            v = np.zeros(nsamp, np.complex128)
            for i, (b, a) in enumerate(edges_tones(n)):
                v += a / (c + 1) * np.exp(2j * np.pi * (b * t / n + 0.11 * i + 0.05 * c))
        else:
            raise ValueError(kind)
        out[c] = np.rint(v.real) + 1j * np.rint(v.imag)
    assert np.abs(out.real).max() <= 32767 and np.abs(out.imag).max() <= 32767
    return out


def as_cf32(x, extra: int = 0) -> np.ndarray:
    """float32 [nch, 2 nsamp + extra] components (extra: unused components between the streams)."""
    x = np.asarray(x)
    buf = np.zeros((x.shape[0], 2 * x.shape[1] + extra), np.float32)
    buf[:, 0:2 * x.shape[1]:2] = x.real
    buf[:, 1:2 * x.shape[1]:2] = x.imag
    return buf


def as_cs16(x, extra: int = 0) -> np.ndarray:
    """int16 [nch, 2 nsamp + extra] components; the sample value is this / cs16_scale."""
    return as_cf32(x, extra).astype(np.int16)
