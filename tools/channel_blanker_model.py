"""The channel noise blanker's model (include/sddc_ddc.h, sddc_ddc_channel_blank_*; csrc/blanker_math.h;
numpy only).

  make_params     [nch, 2] = (k2, qmin); channel 1 of several is bypassed (k2 = 0)
  make_input      seeded complex64 streams, complex N(0, 0.3^2) plus a 0.1 tone, with single-sample and
                  three-sample impulses of 100 x the rms at the positions where the block form, the guard
                  and a cut into calls or runs can go wrong; returns the streams and the positions
  make_periodic   the same noise with a three-sample impulse every `period` samples: (clean, dirty, mask)
  to_cs16         a complex64 stream as int16 [nch, n, 2] codes (x * scale, rounded, clipped)
  definition      the definition, in float32 (numpy's *, + and comparisons on float32 are the library's
                  correctly rounded operations; the tree is repeated a[..., 0::2] + a[..., 1::2]) or, with
                  dtype=np.float64, evaluated in float64 on the same float32 samples and parameters
  count           the blanked outputs of a call that covers outputs [a, b) of the stream

definition returns a dict: y (the outputs, the input's type and shape), out_blank [nch, n] (output n is
blanked: blank[n - g], false for n < g), hit [nch, n], q [nch, n] and t [nch, n] (the threshold of the
sample's block; +inf in block 0).
"""
from __future__ import annotations

import numpy as np

B = 256                    # SDDC_DDC_BLANKER_BLOCK
MEAN, MEDIAN = 0, 1
U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)


def make_params(nch, k2=10.0, qmin=1e-6):
    p = np.zeros((nch, 2), np.float32)
    p[:, 0] = k2
    p[:, 1] = qmin
    if nch > 1:
        p[1, 0] = 0.0      # bypassed: a pure delay
    return p


def _noise(nch, nsamp, seed):
    rng = np.random.default_rng(seed)
    x = (0.3 / np.sqrt(2.0)) * (rng.standard_normal((nch, nsamp)) + 1j * rng.standard_normal((nch, nsamp)))
    f = 0.01 + 0.003 * np.arange(nch)[:, None]
    return x + 0.1 * np.exp(2j * np.pi * f * np.arange(nsamp)[None, :]), rng


def impulse_positions(nsamp, guard):
    """The stream indices of make_input's impulses (first samples), sorted, inside the stream."""
    g = guard
    pos = [0, g - 1, g, B - 1, B, B + 1, nsamp - 1, nsamp - 1 - g]
    for k in (2, 3, 6, 64, 258):   # block boundaries, also run boundaries of runs of 1, 2 and 3 blocks
        pos += [k * B - g - 1, k * B - g, k * B + g]
    a = 4 * B + 40                 # two hits 2 g + 1 apart (the masks abut) and two 2 g + 2 apart (one survives)
    pos += [a, a + 2 * g + 1, a + B // 2, a + B // 2 + 2 * g + 2]
    return sorted({p for p in pos if 0 <= p < nsamp})


def make_input(nch, nsamp, guard, seed=1, amp=30.0):
    x, rng = _noise(nch, nsamp, seed)
    pos = impulse_positions(nsamp, guard)
    for j, p in enumerate(pos):
        ln = 1 if j % 2 == 0 else 3
        ph = np.exp(2j * np.pi * rng.random(nch))
        x[:, p:p + ln] = amp * ph[:, None]
    return x.astype(np.complex64), pos


def make_periodic(nch, nsamp, period=997, seed=2, amp=30.0):
    clean, rng = _noise(nch, nsamp, seed)
    dirty = clean.copy()
    mask = np.zeros(nsamp, bool)
    for p in range(period // 2, nsamp - 3, period):
        dirty[:, p:p + 3] = amp * np.exp(2j * np.pi * rng.random(nch))[:, None]
        mask[p:p + 3] = True
    return clean.astype(np.complex64), dirty.astype(np.complex64), mask


def to_cs16(x, scale=1000.0):
    x = np.asarray(x, np.complex64)
    v = np.stack([x.real, x.imag], axis=-1).astype(np.float64) * scale
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def _tree(a):
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def definition(x, params, guard, ref_blocks, ref_mode=MEAN, dtype=np.float32):
    x = np.asarray(x)
    cs16 = x.dtype == np.int16
    if cs16:
        I, Q = x[..., 0].astype(dtype), x[..., 1].astype(dtype)
    else:
        x = x.astype(np.complex64, copy=False)
        I, Q = x.real.astype(dtype), x.imag.astype(dtype)
    nch, n = I.shape
    g, M = int(guard), int(ref_blocks)
    params = np.asarray(params, np.float32)
    k2, qmin = params[:, 0], params[:, 1].astype(dtype)
    thr = (k2.astype(np.float64) / 256.0).astype(dtype)
    with np.errstate(all="ignore"):
        q = (I * I) + (Q * Q)
        fin = q <= dtype(FLT_MAX)
        qz = np.where(fin, q, dtype(0))
        nfull, nblocks = n // B, (n + B - 1) // B
        p = _tree(qz[:, :nfull * B].reshape(nch, nfull, B)) if nfull else np.zeros((nch, 0), dtype)
        tk = np.full((nch, nblocks), np.inf, dtype)
        for k in range(1, nblocks):
            nn = min(k, M)
            w = p[:, k - nn:k]
            if ref_mode == MEAN:
                S = w[:, 0]
                for b in range(1, nn):
                    S = S + w[:, b]
                P = S * dtype(1.0 / nn)
            else:
                P = np.sort(w, axis=1)[:, (nn - 1) // 2]
            t = thr * P
            tk[:, k] = np.where(t > qmin, t, qmin)
        t = np.repeat(tk, B, axis=1)[:, :n]
        hit = (~fin | (q > t)) & (k2 > 0)[:, None]
    idx = np.arange(n)[None, :]
    last = np.maximum.accumulate(np.where(hit, idx, -(1 << 40)), axis=1)
    out_blank = (last >= idx - 2 * g) & (idx >= g)
    y = np.zeros_like(x)
    if g < n:
        y[:, g:] = x[:, :n - g]
    y[out_blank] = 0
    return {"y": y, "out_blank": out_blank, "hit": hit, "q": q, "t": t}


def count(model, a, b):
    """uint32 [nch]: the blanked outputs among outputs a <= n < b of the stream."""
    return model["out_blank"][:, a:b].sum(axis=1).astype(np.uint32)
