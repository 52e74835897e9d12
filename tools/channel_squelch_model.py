"""The channel squelch's model (include/sddc_ddc.h, sddc_ddc_channel_squelch_*; csrc/squelch_math.h; numpy
only).

  make_case       seeded audio and sense streams with the modes and thresholds that go with them: low noise
                  and keyed bursts 40 dB apart with the thresholds between them (>= 18 dB from either; in
                  NOISE channels the two levels are swapped), burst lengths of A + 1, A - 1, A and A + H + 3
                  blocks, gaps of H + 2, H and H + 1 blocks, every burst starting off the block grid, and one
                  NaN and one Inf sense sample in bursts of the last gated channel (float sense kinds)
  sense_q         q of every sense sample
  definition      the definition, in float32 (numpy's *, + and comparisons on float32 are the library's
                  correctly rounded operations; the tree is repeated a[..., 0::2] + a[..., 1::2]) or, with
                  dtype=np.float64, the levels evaluated in float64 on the same samples and thresholds
  undecided       the complete blocks whose float64 level lies within 1.01 * 11 * 2^-24 * T of a threshold T
                  of their channel: where float32 and float64 may decide differently
  open_at, count, level_at   the side outputs of a call that ends at / covers given stream indices

definition returns a dict: y (the outputs), G [nch, nblocks] (the gate of every block that holds a sample,
OFF: 1, MUTE: 0), kind [nch, nblocks] (0 zero, 1 pass, 2 fade up, 3 fade down), p [nch, nfull] (the levels),
bad, u, v [nch, nfull] and open_after [nch, nfull] (`open` after each complete block, as d_open reports it).
"""
from __future__ import annotations

import numpy as np

B = 256                                  # SDDC_DDC_SQUELCH_BLOCK
OFF, LEVEL, NOISE, MUTE = 0, 1, 2, 3     # SDDC_DDC_SQUELCH_*
SELF, F32, S16, CF32, CS16 = 0, 1, 2, 3, 4   # SDDC_DDC_SQUELCH_SENSE_*
AUDIO_F32, AUDIO_S16 = 0, 1
U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
KINDS = (SELF, F32, S16, CF32, CS16)
LO, HI = 0.01, 1.0                        # rms of the noise and of a burst (float kinds)
S16_SCALE = 3000.0                        # the same in int16 codes: 30 and 3000
NAN_PAYLOAD = 0x7FC12345


def sense_dtype_is_int(kind, in16):
    return kind in (S16, CS16) or (kind == SELF and in16)


def thresholds_for(modes, scale=1.0):
    """[nch, 2] = (T_open, T_close) as mean squares: 1.5e-2 and 6.7e-3 times scale^2 (LEVEL; swapped for
    NOISE), between the noise's 1e-4 and a burst's 1."""
    mid = LO * HI * scale * scale
    t = np.zeros((len(modes), 2), np.float32)
    for c, m in enumerate(modes):
        t[c] = (mid / 1.5, mid * 1.5) if m == NOISE else (mid * 1.5, mid / 1.5)
    return t


def modes_for(nch, single=LEVEL):
    return np.array([single] if nch == 1 else [(LEVEL, NOISE, OFF, MUTE)[c % 4] for c in range(nch)], np.int32)


def burst_spans(nsamp, A, H, c=0):
    """[(start, stop)] of channel c's bursts inside the stream; no start is a multiple of B."""
    lens = [A + 1, A - 1, A, A + H + 3]
    gaps = [H + 2, H, H + 1]
    at = B + 37 + 11 * (c % 19)
    spans, j = [], 0
    while at < nsamp:
        ln = lens[j % 4] * B + 3 * (j % 5)
        if ln > 0:
            spans.append((at, min(nsamp, at + ln)))
        at += ln + max(gaps[j % 3] * B, 1) + 5
        if at % B == 0:
            at += 1
        j += 1
    return spans


def make_case(nch, nsamp, A, H, kind=SELF, in16=False, single=LEVEL, seed=1):
    """(audio [nch, nsamp], sense or None, modes [nch], thresholds [nch, 2]).  audio: float32, or int16 when
    in16; sense: None (SELF), float32 / int16 [nch, nsamp], complex64 [nch, nsamp] or int16 [nch, nsamp, 2]."""
    rng = np.random.default_rng(seed + 1000 * kind + (500 if in16 else 0))
    modes = modes_for(nch, single)
    cplx = kind in (CF32, CS16)
    env = np.empty((nch, nsamp))
    for c in range(nch):
        lo, hi = (HI, LO) if modes[c] == NOISE else (LO, HI)
        env[c] = lo
        for a, b in burst_spans(nsamp, A, H, c):
            env[c, a:b] = hi
    if cplx:
        s = env * (rng.standard_normal((nch, nsamp)) + 1j * rng.standard_normal((nch, nsamp))) / np.sqrt(2.0)
    else:
        s = env * rng.standard_normal((nch, nsamp))
    integer = sense_dtype_is_int(kind, in16)
    scale = S16_SCALE if integer else 1.0
    if integer:
        if cplx:
            sense = np.clip(np.rint(np.stack([s.real, s.imag], -1) * scale), -32768, 32767).astype(np.int16)
        else:
            sense = np.clip(np.rint(s * scale), -32768, 32767).astype(np.int16)
    else:
        sense = s.astype(np.complex64 if cplx else np.float32)
        gated = [c for c in range(nch) if modes[c] in (LEVEL, NOISE)]
        if gated:   # one NaN and one Inf in bursts of the last gated channel
            c = gated[-1]
            spans = burst_spans(nsamp, A, H, c)
            if spans:
                a, b = spans[3] if len(spans) > 3 else spans[0]
                sense[c, (a + b) // 2] = np.nan
                a, b = spans[2] if len(spans) > 2 else spans[0]
                sense[c, min(a + 5, nsamp - 1)] = np.inf
    if kind == SELF:
        audio, sense = sense, None
    else:
        t = np.arange(nsamp)[None, :]
        a = 0.5 * np.sin(2 * np.pi * (0.01 + 0.003 * np.arange(nch)[:, None]) * t) + 0.05 * rng.standard_normal((nch, nsamp))
        audio = np.clip(np.rint(a * 16000.0), -32768, 32767).astype(np.int16) if in16 else a.astype(np.float32)
    return audio, sense, modes, thresholds_for(modes, scale)


def sense_q(audio, sense, kind, dtype=np.float32):
    s = np.asarray(audio if kind == SELF else sense)
    with np.errstate(all="ignore"):
        if kind in (CF32, CS16):
            if kind == CF32:
                s = s.astype(np.complex64, copy=False)
                i, q = s.real.astype(dtype), s.imag.astype(dtype)
            else:
                i, q = s[..., 0].astype(dtype), s[..., 1].astype(dtype)
            return (i * i) + (q * q)
        x = s.astype(dtype)
        return x * x


def _tree(a):
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def _levels(audio, sense, kind, dtype):
    q = sense_q(audio, sense, kind, dtype)
    nch, n = q.shape
    nfull = n // B
    with np.errstate(all="ignore"):
        fin = q <= dtype(FLT_MAX)
        qz = np.where(fin, q, dtype(0))
        if nfull:
            p = _tree(qz[:, :nfull * B].reshape(nch, nfull, B))
            bad = (~fin)[:, :nfull * B].reshape(nch, nfull, B).any(axis=-1)
        else:
            p, bad = np.zeros((nch, 0), dtype), np.zeros((nch, 0), bool)
    return p, bad


def s16_out(y):
    """demod_s16: round to nearest even, clamp, NaN -> 0"""
    y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        v = np.rint(np.clip(np.where(np.isnan(y), np.float32(0), y), -32768.0, 32767.0))
    return v.astype(np.int16)


def definition(audio, sense, kind, modes, thresholds, A, H, fade, fmt_out=AUDIO_F32, dtype=np.float32):
    audio = np.asarray(audio)
    nch, n = audio.shape
    modes = np.asarray(modes, np.int32)
    T = np.asarray(thresholds, np.float32) * np.float32(256.0)   # exact
    p, bad = _levels(audio, sense, kind, dtype)
    nfull, nblocks = p.shape[1], (n + B - 1) // B
    To, Tc = T[:, 0:1].astype(dtype), T[:, 1:2].astype(dtype)
    noise = (modes == NOISE)[:, None]
    with np.errstate(all="ignore"):
        u = np.where(noise, p < To, p > To) & ~bad
        v = np.where(noise, p < Tc, p > Tc) & ~bad
    gated = (modes == LEVEL) | (modes == NOISE)
    r = np.zeros(nch, np.int64)
    nn = np.zeros(nch, np.int64)
    op = np.zeros(nch, bool)
    G = np.zeros((nch, nblocks + 1), bool)          # G[:, k]: open after block k - 1
    for k in range(nfull):
        r = np.where(u[:, k], np.minimum(r + 1, A), 0)
        nn = np.where(v[:, k], 0, np.minimum(nn + 1, H + 1))
        op = np.where(op, nn <= H, r >= A) & gated
        G[:, k + 1] = op
    open_after = G[:, 1:nfull + 1] | (modes == OFF)[:, None]
    G = G[:, :nblocks]
    Gp = np.concatenate([np.zeros((nch, 1), bool), G[:, :-1]], axis=1)
    kind_k = np.where(G, 1, 0)
    if fade:
        kind_k = np.where(G & ~Gp, 2, np.where(~G & Gp, 3, kind_k))
    kind_k = np.where((modes == OFF)[:, None], 1, np.where((modes == MUTE)[:, None], 0, kind_k))
    G = (G & gated[:, None]) | (modes == OFF)[:, None]
    ks = np.repeat(kind_k, B, axis=1)[:, :n]
    i = (np.arange(n) % B)[None, :]
    w = np.where(ks == 2, i + 1, 255 - i).astype(np.float32) * np.float32(1.0 / 256.0)
    x = audio.astype(np.float32)
    with np.errstate(all="ignore"):
        y = np.where(ks == 1, x, np.where(ks == 0, np.float32(0), x * w)).astype(np.float32)
    if fmt_out == AUDIO_S16:
        y = s16_out(y)
    elif audio.dtype == np.float32:   # kPass passes the stored word (np.where may quiet a NaN)
        yb, xb = y.view(np.uint32), np.ascontiguousarray(audio).view(np.uint32)
        yb[ks == 1] = xb[ks == 1]
    return {"y": y, "G": G, "kind": kind_k, "p": p.astype(np.float32) if dtype == np.float32 else p, "bad": bad, "u": u,
            "v": v, "open_after": open_after, "modes": modes, "n": n}


def undecided(audio, sense, kind, modes, thresholds):
    """The number of complete blocks of gated channels with |p64 - T| <= 1.01 * 11 * 2^-24 * T for T = 256
    T_open or 256 T_close."""
    p, bad = _levels(audio, sense, kind, np.float64)
    T = np.asarray(thresholds, np.float32).astype(np.float64) * 256.0
    modes = np.asarray(modes)
    gated = ((modes == LEVEL) | (modes == NOISE))[:, None]
    cnt = 0
    for j in range(2):
        t = T[:, j:j + 1]
        cnt += int((gated & ~bad & (np.abs(p - t) <= 1.01 * 11 * U * t)).sum())
    return cnt


def open_at(model, end):
    """uint32 [nch]: d_open of a call that ends at stream index `end` (exclusive)."""
    k = end // B
    if k == 0:
        return (model["modes"] == OFF).astype(np.uint32)
    return model["open_after"][:, k - 1].astype(np.uint32)


def level_at(model, end):
    k = end // B
    nch = model["G"].shape[0]
    return model["p"][:, k - 1].astype(np.float32) if k else np.zeros(nch, np.float32)


def count(model, a, b):
    """uint32 [nch]: the samples a <= i < b of the stream whose block has G = 1."""
    g = np.repeat(model["G"], B, axis=1)[:, :model["n"]]
    return g[:, a:b].sum(axis=1).astype(np.uint32)


def transitions(model):
    """(openings, closings) among the gates of the gated channels."""
    g = model["G"].astype(np.int8)
    gated = ((model["modes"] == LEVEL) | (model["modes"] == NOISE))[:, None]
    d = np.diff(g, axis=1) * gated
    return int((d > 0).sum()), int((d < 0).sum())
