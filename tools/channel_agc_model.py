"""The channel AGC's model (include/sddc_ddc.h, sddc_ddc_channel_agc_*; csrc/agc_math.h; numpy only).

  make_input      seeded float32 streams: loud, then 40 dB down from sample 100 on, with a burst of
                  +46 dB on samples 300..339 of every third channel, so that the envelope carried
                  across the block boundaries decides the gain of the quiet part
  make_params     [nch, 3] = (T, d, F): d cycles through DECAYS, T through TARGETS, F through FLOORS
  block_decay     dB = float32(d^B) exactly as the library builds it (eight squarings in float64)
  definition32    the definition (E, R, Zr, the boundary step) in float32: numpy's *, / and comparisons
                  on float32 are the same correctly rounded operations as the library's; `sabotage`
                  breaks the block form on purpose for the discrimination test
  recurrence64    the float64 plain recurrence e[n] = max(|x[n]|, d e[n-1]), y = T x / max(e, F) on the
                  same float32 parameters and samples: the reference y64
  bounds          bound[n] >= |y[n] - y64[n]| for the definition's float32 arithmetic

The bound (the header states it).  Every candidate |x[t]| d^(n-t) of the maximum reaches R through at
most B - 1 rounded multiplies in the zero-start pass of its own block, one multiply by dB per later
boundary (one rounding, plus dB's own rounding) and at most B multiplies in n's block.  max is
monotone, so R is within (2 B + 2 K(n)) u of e64 relatively, K(n) = ceil((n + 1) / B) the blocks the
stream has touched; the quotient and the product round once each:
    |y[n] - y64[n]| <= 1.01 (2 B + 2 K(n) + 2) u |y64[n]|
and the 1.01 covers the second order.  A stream that starts inside a block crosses no more boundaries
than one that starts at a block's first sample, so the same K(n) holds for it.  A bypassed channel's
output is its input: bound 0.
"""
from __future__ import annotations

import numpy as np

B = 256                    # SDDC_DDC_AGC_BLOCK
U = 2.0 ** -24
FLT_MAX = np.float32(np.finfo(np.float32).max)
DECAYS = [0.5, 0.9, 0.99, 0.999, 0.9999, 1 - 2.0 ** -16, 1 - 2.0 ** -20, 1 - 2.0 ** -24]
TARGETS = [0.5, 16384.0]
FLOORS = [1e-4, 2.0 ** -60]


def make_input(nch, n, seed=1):
    """[nch, n] float32: N(0, 0.3^2), scaled by 0.01 from sample 100 on, and by a further 200 on
    samples 300..339 of every third channel."""
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal((nch, n))
    x[:, 100:] *= 0.01
    x[0::3, 300:340] *= 200.0
    return x.astype(np.float32)


def make_params(nch):
    """[nch, 3] float32 (T, d, F): 48 channels hold every combination of DECAYS, TARGETS and FLOORS."""
    c = np.arange(nch)
    p = np.zeros((nch, 3), np.float32)
    p[:, 0] = np.asarray(TARGETS, np.float32)[(c // 8) % 2]
    p[:, 1] = np.asarray(DECAYS, np.float32)[c % 8]
    p[:, 2] = np.asarray(FLOORS, np.float32)[(c // 16) % 2]
    return p


def block_decay(d, steps=B):
    """float32(d^steps) of float32 d; steps = B: eight squarings in float64, as the library."""
    p = np.asarray(d, np.float32).astype(np.float64)
    if steps == B:
        for _ in range(8):
            p = p * p
    else:
        p = p ** steps
    with np.errstate(under="ignore"):
        return p.astype(np.float32)


def magnitude(x):
    """a = |x|; a NaN gives 0, an infinity FLT_MAX (x float32 or float64, the result likewise)."""
    a = np.abs(x)
    a = np.where(np.isnan(a), a.dtype.type(0), a)
    return np.where(a > a.dtype.type(FLT_MAX), a.dtype.type(FLT_MAX), a)


def s16(y):
    """SDDC_DDC_AUDIO_S16: round to nearest even, clamp to [-32768, 32767], NaN becomes 0."""
    y = np.where(np.isnan(y), np.float32(0), y)
    return np.rint(np.clip(y, np.float32(-32768), np.float32(32767))).astype(np.int16)


def definition32(x, params, pos=0, out16=False, sabotage=None, trace=False):
    """The definition on x [nch, n] (float32, or int16 read as float32) with params [nch, 3], from
    zero state at stream position pos.  Returns (y [nch, n] float32 or int16, env [nch] float32: R
    after the last sample), with trace=True also R after every sample's step [nch, n].  sabotage:
    "no_carry" drops E at the block boundaries (E = Zr), "dB255" builds dB from B - 1 steps."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float32)
    p = np.asarray(params, np.float32).reshape(-1, 3)
    nch, n = x.shape
    T, d, F = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    dB = block_decay(d, B - 1 if sabotage == "dB255" else B)
    bypass = T == 0
    E, R, Zr = (np.zeros(nch, np.float32) for _ in range(3))
    y = np.zeros((nch, n), np.float32)
    Rt = np.zeros((nch, n), np.float32) if trace else None
    pos = int(pos)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for i in range(n):
            xi = x[:, i]
            a = magnitude(xi)
            t = d * R
            R = np.where(a > t, a, t)
            t = d * Zr
            Zr = np.where(a > t, a, t)
            den = np.where(R > F, R, F)
            g = T / den
            y[:, i] = np.where(bypass, xi, g * xi)
            if trace:
                Rt[:, i] = R
            pos += 1
            if pos % B == 0:
                t = np.zeros(nch, np.float32) if sabotage == "no_carry" else dB * E
                E = np.where(Zr > t, Zr, t)
                R = E.copy()
                Zr = np.zeros(nch, np.float32)
    assert y.dtype == np.float32 and R.dtype == np.float32
    out = s16(y) if out16 else y
    return (out, R, Rt) if trace else (out, R)


def recurrence64(x, params):
    """(y64 [nch, n], e64 [nch, n]) of the float64 plain recurrence on the float32 values."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float32).astype(np.float64)
    p = np.asarray(params, np.float32).reshape(-1, 3).astype(np.float64)
    nch, n = x.shape
    T, d, F = p[:, 0], p[:, 1], p[:, 2]
    e = np.zeros(nch)
    y, et = np.zeros((nch, n)), np.zeros((nch, n))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            e = np.maximum(magnitude(x[:, i]), d * e)
            et[:, i] = e
            y[:, i] = np.where(T == 0, x[:, i], T * x[:, i] / np.maximum(e, F))
    return y, et


def bounds(x, params):
    """bound [nch, n] on |y - y64| (F32 output; S16 output adds 1/2 and the clamp)."""
    y64, _ = recurrence64(x, params)
    p = np.asarray(params, np.float32).reshape(-1, 3)
    n = y64.shape[1]
    K = np.ceil((np.arange(n) + 1) / B)
    bnd = 1.01 * (2 * B + 2 * K + 2)[None, :] * U * np.abs(y64)
    bnd[p[:, 0] == 0] = 0.0
    return bnd


if __name__ == "__main__":
    # the bound on the seeded input, the sabotaged forms against it, per release factor
    nch, n = 48, 5 * B + 17
    x, p = make_input(nch, n), make_params(nch)
    y64, _ = recurrence64(x, p)
    bnd = bounds(x, p)
    forms = {"definition": None, "no carry": "no_carry", "255-step dB": "dB255"}
    ratio = {k: np.abs(definition32(x, p, sabotage=s)[0].astype(np.float64) - y64) / bnd for k, s in forms.items()}
    print(f"{nch} x {n}, worst err / bound per d:")
    for k, dk in enumerate(DECAYS):
        print(f"  d = 1 - {1 - dk:.3g}: " + ", ".join(f"{name} {r[k::8].max():.3g}" for name, r in ratio.items()))
