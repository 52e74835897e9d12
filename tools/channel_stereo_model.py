"""The channel stereo decoder's model (include/sddc_ddc.h, sddc_ddc_channel_stereo_*; csrc/stereo_math.h; numpy
only).  fmaf32, sincos_word, sincos64, the tree, the scaling and the S16 conversion are channel_tone_model.py's.

  definition      the definition in float32, bit for bit (numpy's *, +, -, / and sqrt on float32 are the library's
                  correctly rounded operations), or, with dtype=np.float64, evaluated in float64 on the same
                  samples, words and scaled parameters with cos and sin of the exact phases; q_force gives the q
                  of every window from outside (the float32 model's, for the second part of the bound)
  bound_q, bound_lr, undecided   stereo_math.h's derived bounds and the windows tone_math.h's leave undecided
  stereo_at, level_at, phase_at, count   the side outputs of a call that ends at / covers stream indices
  mpx             the multiplex of a left and a right signal with a pilot sin(psi + alpha)
  make_case       seeded MPX streams: AUTO channels whose pilot comes and goes off the window grid, with a NaN in
                  a closed window and a sample whose square overflows in an open one (float input), a MONO
                  channel, an AUTO channel without a pilot (NaN and Inf samples pass with their bits)

definition returns a dict: left, right [nch, n], G [nch, nwin] (whether a window that holds a sample is written
in stereo), and per complete window P, E, bad, u, v, gate_after [nch, nfull], Q_after [nch, nfull, 2], X.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("channel_tone_model",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "channel_tone_model.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

B = 256                                  # SDDC_DDC_STEREO_BLOCK
MONO, AUTO = 0, 1
AUDIO_F32, AUDIO_S16 = 0, 1
U = 2.0 ** -24
FLT_MAX = T.FLT_MAX
NAN_PAYLOAD = 0x7FC12345
FS = 250000.0
PILOT = 19000.0
S16_SCALE = 8000.0
RHO_OPEN, RHO_CLOSE, E_MIN = 0.004, 0.002, 1e-6
f32, f64 = np.float32, np.float64
fmaf32, sincos_word, sincos64, s16_out = T.fmaf32, T.sincos_word, T.sincos64, T.s16_out


def word(fs=FS):
    """round(19000 / fs * 2^32) (sddc_ddc_bfo_word)"""
    return T.word(PILOT, fs)


def scale(params, W):
    """[nch, 4] float32 (To, Tc, Emin, g2): tone_scale of the first three, 2 g"""
    p = np.asarray(params, f32)
    out = np.empty(p.shape, f32)
    out[:, :3] = T.scale(p[:, :3], W)
    out[:, 3] = f32(2) * p[:, 3]
    return out


def definition(mpx, w, modes, params, W, A, H, fmt_out=AUDIO_F32, pos0=0, dtype=f32, q_force=None):
    """pos0: the stream position of sample 0, a multiple of 256 W.  q_force: [nch, nwin, 2] or None."""
    mpx = np.asarray(mpx)
    nch, n = mpx.shape
    w = int(w) & 0xffffffff
    w2 = (2 * w) & 0xffffffff
    WB = W * B
    assert pos0 % WB == 0
    modes = np.asarray(modes)
    auto = modes == AUTO
    Tp = scale(params, W).astype(dtype)
    nfull, nwin, nb = n // WB, (n + WB - 1) // WB, n // WB * W
    exact = dtype == f32
    sc = sincos_word if exact else sincos64
    i = np.arange(B, dtype=np.uint32)
    with np.errstate(all="ignore"):
        xs = mpx.astype(f32)
        fin = (xs * xs) <= f32(FLT_MAX)
        x = np.where(fin, xs, f32(0)).astype(dtype)
        xb = x[:, :nb * B].reshape(nch, nb, B)
        bad = (~fin)[:, :nfull * WB].reshape(nch, nfull, WB).any(axis=-1)
        pk = T._tree(xb * xb)
        p256 = ((pos0 + B * np.arange(nb, dtype=np.uint64)) & np.uint64(0xffffffff)).astype(np.uint32)
        c_i, s_i = sc(np.uint32(w) * i)
        cr, sr = sc(np.uint32(w) * p256)
        Ck, Sk = T._tree(xb * c_i), T._tree(xb * s_i)
        if exact:
            re, im = fmaf32(Ck, cr, -(Sk * sr)), fmaf32(Ck, sr, Sk * cr)
        else:
            re, im = Ck * cr - Sk * sr, Ck * sr + Sk * cr
        re, im, pk = (a.reshape(nch, nfull, W) for a in (re, im, pk))
        Zr, Zi, E = (np.zeros((nch, nfull), dtype) for _ in range(3))
        for b in range(W):
            Zr, Zi, E = Zr + re[:, :, b], Zi + im[:, :, b], E + pk[:, :, b]
        P = (Zr * Zr) + (Zi * Zi)
        live = ~bad & (E > Tp[:, 2:3])
        u = live & (P > Tp[:, 0:1] * E)
        v = live & (P > Tp[:, 1:2] * E)
        # the phase of every window, used where v holds
        nn = np.sqrt(P)
        vr, vi = Zi / nn, Zr / nn
        if exact:
            qr, qi = fmaf32(vr, vr, -(vi * vi)), (f32(2) * vr) * vi
        else:
            qr, qi = vr * vr - vi * vi, (2.0 * vr) * vi
    r = np.zeros(nch, np.int64)
    nnn = np.zeros(nch, np.int64)
    op = np.zeros(nch, bool)
    q = np.zeros((nch, 2), dtype)
    q[:, 0] = 1
    gate = np.zeros((nch, nfull + 1), bool)          # gate[:, j]: open after window j - 1
    Q = np.zeros((nch, nfull + 1, 2), dtype)
    Q[:, 0] = q
    for j in range(nfull):
        q = np.where(v[:, j:j + 1], np.stack([qr[:, j], qi[:, j]], axis=1), q)
        r = np.where(u[:, j], np.minimum(r + 1, A), 0)
        nnn = np.where(v[:, j], 0, np.minimum(nnn + 1, H + 1))
        op = np.where(op, nnn <= H, r >= A)
        gate[:, j + 1] = op
        Q[:, j + 1] = q
    G = gate[:, :nwin] & auto[:, None]
    Qw = Q[:, :nwin] if q_force is None else np.asarray(q_force).astype(dtype)
    # the outputs, block by block (the last one padded)
    nblk = (n + B - 1) // B
    xo = np.zeros((nch, nblk * B), f32)
    xo[:, :n] = xs
    xo = xo.reshape(nch, nblk, B).astype(dtype)
    jb = np.arange(nblk) // W
    p256o = ((pos0 + B * np.arange(nblk, dtype=np.uint64)) & np.uint64(0xffffffff)).astype(np.uint32)
    with np.errstate(all="ignore"):
        tc, ts = sc(np.uint32(w2) * i)
        rc, rs = sc(np.uint32(w2) * p256o)
        qrb, qib = Qw[:, jb, 0], Qw[:, jb, 1]
        if exact:
            rr, ri = fmaf32(qrb, rc, -(qib * rs)), fmaf32(qrb, rs, qib * rc)
            sub = fmaf32(tc, ri[:, :, None], ts * rr[:, :, None])
        else:
            rr, ri = qrb * rc - qib * rs, qrb * rs + qib * rc
            sub = tc * ri[:, :, None] + ts * rr[:, :, None]
        d = (Tp[:, 3][:, None, None] * xo) * sub
        L, R = (xo + d).reshape(nch, -1)[:, :n], (xo - d).reshape(nch, -1)[:, :n]
    g = np.repeat(G, WB, axis=1)[:, :n]
    out = []
    for y in (L, R):
        if not exact:
            out.append(np.where(g, y, xs.astype(f64)))
            continue
        with np.errstate(all="ignore"):
            y = np.where(g, y, xs).astype(f32)
        if fmt_out == AUDIO_S16:
            y = s16_out(y)
        elif mpx.dtype == np.float32:   # a passed sample is the stored word (np.where may quiet a NaN)
            yb, ab = y.view(np.uint32), np.ascontiguousarray(mpx).view(np.uint32)
            yb[~g] = ab[~g]
        out.append(y)
    X = np.abs(x.astype(f64))[:, :nfull * WB].reshape(nch, nfull, WB).sum(axis=-1)
    return {"left": out[0], "right": out[1], "G": G, "P": P, "E": E, "bad": bad, "u": u, "v": v, "gate_after": gate[:, 1:],
            "Q_after": Q[:, 1:], "Qw": Q[:, :nwin], "auto": auto, "n": n, "W": W, "T": Tp, "X": X, "Pbest": P,
            "bypass": np.zeros(nch, bool)}


def bound_q(P64, X, W):
    """stereo_math.h: |qr - qr64|, |qi - qi64| <= dv (2 + dv) + 2.02 u, dv = r / (1 - r / 2) + 3.02 u, r = sqrt(2) (38 +
    W) u X / sqrt(P64); 4 (no bound) where r >= 1"""
    with np.errstate(all="ignore"):
        r = np.sqrt(2.0) * (38 + W) * U * X / np.sqrt(P64)
        dv = r / (1.0 - r / 2.0) + 3.02 * U
        return np.where(r < 1.0, dv * (2.0 + dv) + 2.02 * U, 4.0)


def bound_lr(x, g2):
    """stereo_math.h: |L - L64|, |R - R64| <= 1.01 u (|x| + 22 |g2 x|) given the same q"""
    x = np.abs(np.asarray(x, f64))
    return 1.01 * U * (x + 22.0 * np.abs(f64(g2)) * x)


def undecided(m64):
    """bool [nch, nfull]: the windows of the float64 evaluation in which u or v may differ in float32 (tone_math.h)"""
    return T.undecided(m64)


def _last(m, end):
    return end // (m["W"] * B) - 1


def stereo_at(m, end):
    j = _last(m, end)
    nch = m["G"].shape[0]
    return (m["gate_after"][:, j] & m["auto"]).astype(np.uint32) if j >= 0 else np.zeros(nch, np.uint32)


def level_at(m, end):
    j = _last(m, end)
    nch = m["G"].shape[0]
    return np.stack([m["P"][:, j], m["E"][:, j]], axis=1).astype(f32) if j >= 0 else np.zeros((nch, 2), f32)


def phase_at(m, end):
    j = _last(m, end)
    nch = m["G"].shape[0]
    return m["Q_after"][:, j].astype(f32) if j >= 0 else np.tile(f32([1, 0]), (nch, 1))


def count(m, a, b):
    """uint32 [nch]: the samples a <= i < b of the stream written in stereo."""
    g = np.repeat(m["G"], m["W"] * B, axis=1)[:, :m["n"]]
    return g[:, a:b].sum(axis=1).astype(np.uint32)


def mpx(left, right, fs=FS, pilot=0.1, alpha=0.0, t0=0, df=0.0):
    """0.45 (L + R) + 0.45 (L - R) sin(2 psi) + pilot sin(psi), psi = 2 pi (19000 + df) (t0 + i) / fs + alpha (float64)"""
    left, right = np.asarray(left, f64), np.asarray(right, f64)
    t = t0 + np.arange(left.shape[-1], dtype=f64)
    psi = 2 * np.pi * (PILOT + df) / fs * t + alpha
    return 0.45 * (left + right) + 0.45 * (left - right) * np.sin(2 * psi) + pilot * np.sin(psi)


def make_case(nch, nsamp, W, in16=False, seed=1):
    """(mpx [nch, nsamp], word, modes [nch], params [nch, 4]).  Channel c: c % 4 == 1 is MONO with a pilot, c % 4 ==
    2 AUTO without one, the others AUTO with a pilot that drops out for stretches off the window grid."""
    rng = np.random.default_rng(seed + 17 * W + (500 if in16 else 0))
    WB = W * B
    t = np.arange(nsamp, dtype=f64)
    s = np.zeros((nch, nsamp))
    modes = np.full(nch, AUTO, np.uint8)
    for c in range(nch):
        fl, fr = 400.0 + 37.0 * (c % 29), 1000.0 + 91.0 * (c % 31)
        left, right = 0.6 * np.sin(2 * np.pi * fl / FS * t + 0.1 * c), 0.5 * np.sin(2 * np.pi * fr / FS * t + 0.7)
        kind = c % 4
        pil = np.full(nsamp, 0.1)
        if kind == 1:
            modes[c] = MONO
        elif kind == 2:
            pil[:] = 0.0
        else:   # on for 5 to 7 windows, off for 3, off the grid
            at, k = 0, 0
            while at < nsamp:
                on = WB * (5 + (k + c) % 3) + 37 + 11 * (c % 19)
                off = 3 * WB + 5
                pil[at + on:at + on + off] = 0.0
                at += on + off
                k += 1
        psi = 2 * np.pi * PILOT / FS * t + 0.3 + 0.4 * c
        s[c] = 0.45 * (left + right) + 0.45 * (left - right) * np.sin(2 * psi) + pil * np.sin(psi)
        s[c] += 0.003 * rng.standard_normal(nsamp)
    if in16:
        x = np.clip(np.rint(s * S16_SCALE), -32768, 32767).astype(np.int16)
    else:
        x = s.astype(f32)
        for c in range(nch):
            kind = c % 4
            if kind in (1, 2) and nsamp > 9:        # passed with their bits
                x.view(np.uint32)[c, nsamp // 2] = NAN_PAYLOAD
                x[c, nsamp // 3] = (np.inf, -np.inf)[c % 2]
            elif kind == 0:
                if nsamp > WB:
                    x[c, WB // 2] = np.nan          # window 0 is closed on a new stream: it turns bad
                if nsamp > 4 * WB + 40:
                    x[c, 4 * WB + 40] = 1e30        # an open window (A <= 3): its square overflows, the value does not
    sc = S16_SCALE ** 2 if in16 else 1.0
    params = np.tile(np.array([RHO_OPEN, RHO_CLOSE, E_MIN * sc, 1.0], f32), (nch, 1))
    params[:, 3] = f32(1.0) + f32(0.125) * (np.arange(nch) % 3).astype(f32)
    return x, word(), modes, params
