"""The channel tone detector's model (include/sddc_ddc.h, sddc_ddc_channel_tone_*; csrc/tone_math.h; numpy
only).

  fmaf32          the correctly rounded float32 fused multiply-add: the product is exact in float64, the sum is
                  rounded to odd there (TwoSum's residual says which way), and 53 >= 24 + 2 bits make the last
                  rounding to float32 the fused one's
  sincos_word     demod_sincos_word on uint32 arrays, bit for bit
  definition      the definition in float32 (numpy's *, + and comparisons on float32 are the library's
                  correctly rounded operations; the tree is repeated a[..., 0::2] + a[..., 1::2]; the folds run
                  in block order from +0) or, with dtype=np.float64, evaluated in float64 on the same samples,
                  words and scaled thresholds with cos and sin of the exact phase
  bound_p, bound_te, undecided   tone_math.h's derived bounds and the windows they leave undecided
  tone_at, open_at, level_at, powers_at, count   the side outputs of a call that ends at / covers stream indices
  make_case       seeded sense streams in segments of one to three windows off the window grid: silence, noise,
                  a tone of the table in noise (strong, or with its share of the energy next to a threshold),
                  and NaN / Inf samples (float sense), with masks, thresholds and an audio stream

definition returns a dict: y (None without audio), G [nch, nwin] (the gate of every window that holds a
sample), and per complete window P [nch, nfull, ntones], Pbest, E, best, bad, u, v, open_after [nch, nfull].
"""
from __future__ import annotations

import numpy as np

B = 256                                  # SDDC_DDC_TONE_BLOCK
AUDIO_F32, AUDIO_S16 = 0, 1
U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
NAN_PAYLOAD = 0x7FC12345
FS = 12000.0
S16_SCALE = 8000.0
CTCSS = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8,
         123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9,
         183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
f32, f64 = np.float32, np.float64


def word(f, fs=FS):
    """round(f / fs * 2^32) mod 2^32 (sddc_ddc_bfo_word)"""
    return int(np.rint(f / fs * 2.0 ** 32)) % 2 ** 32


def table(ntones):
    """uint32 [ntones] and the frequencies: the CTCSS tones, then 1750 Hz and twelve more up to 3 kHz."""
    fr = (list(CTCSS) + [1750.0] + [300.0 + 210.0 * k for k in range(13)])[:ntones]
    return np.array([word(f) for f in fr], np.uint32), fr


def fmaf32(a, b, c):
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


def sincos_word(w):
    """(c, s) float32 of uint32 words: demod_math.h's demod_sincos_word"""
    w = np.asarray(w, np.uint32)
    k = (w + np.uint32(0x20000000)) >> np.uint32(30)
    r = (w - (k << np.uint32(30))).astype(np.uint32).view(np.int32)
    z = r.astype(f32) * f32(2.0 ** -29)
    q = z * z
    sp = np.full(w.shape, f32(float.fromhex("0x1.507834p-22")), f32)
    for co in ("-0x1.32d2ccp-15", "0x1.466bc6p-9", "-0x1.4abbcep-4", "0x1.921fb6p-1"):
        sp = fmaf32(sp, q, f32(float.fromhex(co)))
    cp = np.full(w.shape, f32(float.fromhex("-0x1.a6d1f2p-26")), f32)
    for co in ("0x1.e1f506p-19", "-0x1.55d3c8p-12", "0x1.03c1f0p-6", "-0x1.3bd3ccp-2", "0x1.0p0"):
        cp = fmaf32(cp, q, f32(float.fromhex(co)))
    sp = sp * z
    zero = f32(0)
    kk = k & np.uint32(3)
    c = np.where(kk == 0, cp, np.where(kk == 1, zero - sp, np.where(kk == 2, zero - cp, sp)))
    s = np.where(kk == 0, sp, np.where(kk == 1, cp, np.where(kk == 2, zero - sp, zero - cp)))
    return c.astype(f32), s.astype(f32)


def sincos64(w):
    ph = 2.0 * np.pi * np.asarray(w, np.uint32).astype(f64) / 2.0 ** 32
    return np.cos(ph), np.sin(ph)


def _tree(a):
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def scale(thresholds, W):
    """[nch, 3] float32 (To, Tc, Emin) = (float)((double)x * 256 W)"""
    return (np.asarray(thresholds, f32).astype(f64) * 256.0 * W).astype(f32)


def s16_out(y):
    """demod_s16: round to nearest even, clamp, NaN -> 0"""
    y = np.asarray(y, f32)
    with np.errstate(all="ignore"):
        v = np.rint(np.clip(np.where(np.isnan(y), f32(0), y), -32768.0, 32767.0))
    return v.astype(np.int16)


def definition(sense, audio, words, masks, thresholds, W, A, H, fmt_out=AUDIO_F32, pos0=0, dtype=f32):
    """pos0: the stream position of sample 0, a multiple of 256 W."""
    sense = np.asarray(sense)
    nch, n = sense.shape
    words = np.asarray(words, np.uint32)
    nt = words.shape[0]
    WB = W * B
    assert pos0 % WB == 0
    T = scale(thresholds, W).astype(dtype)
    nfull, nwin, nb = n // WB, (n + WB - 1) // WB, n // WB * W
    exact = dtype == f32
    with np.errstate(all="ignore"):
        xs = sense.astype(f32)
        fin = (xs * xs) <= f32(FLT_MAX)
        x = np.where(fin, xs, f32(0)).astype(dtype)
        xb = x[:, :nb * B].reshape(nch, nb, B)
        bad = (~fin)[:, :nfull * WB].reshape(nch, nfull, WB).any(axis=-1)
        pk = _tree(xb * xb)
        E = np.zeros((nch, nfull), dtype)
        for b in range(W):
            E = E + pk.reshape(nch, nfull, W)[:, :, b]
        P = np.zeros((nch, nfull, nt), dtype)
        i = np.arange(B, dtype=np.uint32)
        p256 = ((pos0 + B * np.arange(nb, dtype=np.uint64)) & np.uint64(0xffffffff)).astype(np.uint32)
        for t in range(nt):
            chans = [c for c in range(nch) if (int(masks[c]) >> t) & 1]
            if not chans or nfull == 0:
                continue
            c_i, s_i = (sincos_word if exact else sincos64)(words[t] * i)
            cr, sr = (sincos_word if exact else sincos64)(words[t] * p256)
            xa = xb[chans]
            Ck, Sk = _tree(xa * c_i), _tree(xa * s_i)
            if exact:
                re = fmaf32(Ck, cr, -(Sk * sr))
                im = fmaf32(Ck, sr, Sk * cr)
            else:
                re, im = Ck * cr - Sk * sr, Ck * sr + Sk * cr
            re, im = re.reshape(len(chans), nfull, W), im.reshape(len(chans), nfull, W)
            zr = np.zeros((len(chans), nfull), dtype)
            zi = np.zeros((len(chans), nfull), dtype)
            for b in range(W):
                zr = zr + re[:, :, b]
                zi = zi + im[:, :, b]
            P[chans, :, t] = (zr * zr) + (zi * zi)
        best = np.full((nch, nfull), -1, np.int32)
        Pbest = np.zeros((nch, nfull), dtype)
        for t in range(nt):
            inm = np.array([(int(masks[c]) >> t) & 1 for c in range(nch)], bool)[:, None]
            take = inm & ((best < 0) | (P[:, :, t] > Pbest))
            best = np.where(take, t, best)
            Pbest = np.where(take, P[:, :, t], Pbest)
        live = ~bad & (E > T[:, 2:3])
        u = live & (Pbest > T[:, 0:1] * E)
        v = live & (Pbest > T[:, 1:2] * E)
    bypass = np.array([int(m) == 0 for m in masks], bool)
    r = np.zeros(nch, np.int64)
    nn = np.zeros(nch, np.int64)
    op = np.zeros(nch, bool)
    G = np.zeros((nch, nfull + 1), bool)          # G[:, j]: open after window j - 1
    for j in range(nfull):
        r = np.where(u[:, j], np.minimum(r + 1, A), 0)
        nn = np.where(v[:, j], 0, np.minimum(nn + 1, H + 1))
        op = np.where(op, nn <= H, r >= A)
        G[:, j + 1] = op
    open_after = G[:, 1:] | bypass[:, None]
    G = G[:, :nwin] | bypass[:, None]
    y = None
    if audio is not None:
        audio = np.asarray(audio)
        g = np.repeat(G, WB, axis=1)[:, :n]
        with np.errstate(all="ignore"):
            y = np.where(g, audio.astype(f32), f32(0)).astype(f32)
        if fmt_out == AUDIO_S16:
            y = s16_out(y)
        elif audio.dtype == np.float32:   # an open sample is the stored word (np.where may quiet a NaN)
            yb, ab = y.view(np.uint32), np.ascontiguousarray(audio).view(np.uint32)
            yb[g] = ab[g]
    X = np.abs(x.astype(f64))[:, :nfull * WB].reshape(nch, nfull, WB).sum(axis=-1)
    return {"y": y, "G": G, "P": P, "Pbest": Pbest, "E": E, "best": best, "bad": bad, "u": u, "v": v, "open_after": open_after,
            "bypass": bypass, "n": n, "W": W, "T": T, "X": X, "nt": nt}


def bound_p(P64, X, W):
    """tone_math.h: |P_t - P_t64| <= 1.01 (2 sqrt(2) eps X sqrt(P64) + 2 eps^2 X^2 + 3 u P64), eps = (38 + W) u"""
    eps = (38 + W) * U
    return 1.01 * (2.0 * np.sqrt(2.0) * eps * X * np.sqrt(P64) + 2.0 * eps * eps * X * X + 3.0 * U * P64)


def bound_te(T, E64, W):
    """tone_math.h: |T E - (T E)64| <= 1.01 (W + 9) u T E64"""
    return 1.01 * (W + 9) * U * T * E64


def undecided(m64):
    """bool [nch, nfull]: the windows of the float64 evaluation in which u or v may differ in float32."""
    W, T, E, Pb, X = m64["W"], m64["T"].astype(f64), m64["E"], m64["Pbest"], m64["X"]
    near = np.abs(E - T[:, 2:3]) <= 1.01 * (W + 8) * U * E
    for j in (0, 1):
        t = T[:, j:j + 1]
        near |= np.abs(Pb - t * E) <= bound_p(Pb, X, W) + bound_te(t, E, W)
    return near & ~m64["bad"] & ~m64["bypass"][:, None]


def _last(m, end):
    return end // (m["W"] * B) - 1


def tone_at(m, end):
    j = _last(m, end)
    nch = m["G"].shape[0]
    return np.where(m["v"][:, j], m["best"][:, j], -1).astype(np.int32) if j >= 0 else np.full(nch, -1, np.int32)


def open_at(m, end):
    j = _last(m, end)
    return (m["open_after"][:, j] if j >= 0 else m["bypass"]).astype(np.uint32)


def level_at(m, end):
    j = _last(m, end)
    nch = m["G"].shape[0]
    return np.stack([m["Pbest"][:, j], m["E"][:, j]], axis=1).astype(f32) if j >= 0 else np.zeros((nch, 2), f32)


def powers_at(m, end):
    j = _last(m, end)
    return m["P"][:, j, :].astype(f32) if j >= 0 else np.zeros((m["G"].shape[0], m["nt"]), f32)


def count(m, a, b):
    """uint32 [nch]: the samples a <= i < b of the stream whose window is open."""
    g = np.repeat(m["G"], m["W"] * B, axis=1)[:, :m["n"]]
    return g[:, a:b].sum(axis=1).astype(np.uint32)


def masks_for(nch, ntones, mask_tones):
    """uint64 [nch]: mask_tones tones spread over the table; with three or more channels the first three are
    0 (bypass), one tone and every tone."""
    sel = sorted({(7 * k + 3) % ntones for k in range(ntones)})[:mask_tones] if mask_tones < ntones else range(ntones)
    one = sum(1 << t for t in sel)
    allm = (1 << ntones) - 1
    out = []
    for c in range(nch):
        out.append(one if nch < 3 else (0, 1 << (5 % ntones), allm, one)[c % 4])
    return np.array(out, np.uint64)


RHO_OPEN, RHO_CLOSE, E_MIN = 0.2, 0.1, 1e-6


def make_case(nch, nsamp, W, ntones=64, mask_tones=1, sense16=False, in16=False, seed=1):
    """(sense [nch, nsamp], audio [nch, nsamp], words [ntones], masks [nch], thresholds [nch, 3])."""
    rng = np.random.default_rng(seed + 17 * W + 1000 * mask_tones + (500 if sense16 else 0))
    words, freqs = table(ntones)
    masks = masks_for(nch, ntones, mask_tones)
    WB = W * B
    s = np.zeros((nch, nsamp))
    special = []
    for c in range(nch):
        tones = [t for t in range(ntones) if (int(masks[c]) >> t) & 1] or [0]
        at, j = 0, 0
        while at < nsamp:
            ln = min(nsamp - at, WB * (1 + j % 3) + 37 + 11 * (c % 19))
            kind = (j + c) % 6
            t = np.arange(at, at + ln)
            noise = 0.05 * rng.standard_normal(ln)
            if kind == 0:
                seg = 1e-5 * rng.standard_normal(ln)                    # silence: below e_min
            elif kind == 1:
                seg = noise
            else:
                f = freqs[tones[(j // 2) % len(tones)]]
                # strong; or P / (256 W E) next to rho_open / rho_close.  A real tone of amplitude a gives |Z|^2 =
                # (a N / 2)^2, half its share of the energy: a^2 / 2 = rho (a^2 / 2 + 0.0025) reads rho / 2
                rho = {2: 0.9, 3: 2 * RHO_OPEN, 4: 2 * RHO_CLOSE, 5: 0.6}[kind]
                a = np.sqrt(2.0 * rho * 0.0025 / (1.0 - rho))
                seg = a * np.cos(2 * np.pi * f / FS * t + 0.3 * c) + noise
            s[c, at:at + ln] = seg
            if kind == 5 and ln > 9:
                special.append((c, at + ln // 2))
            at += ln
            j += 1
    if sense16:
        sense = np.clip(np.rint(s * S16_SCALE), -32768, 32767).astype(np.int16)
    else:
        sense = s.astype(f32)
        for q, (c, at) in enumerate(special):
            sense[c, at] = (np.nan, np.inf, -np.inf)[q % 3]
    t = np.arange(nsamp)[None, :]
    a = 0.5 * np.sin(2 * np.pi * (0.01 + 0.003 * np.arange(nch)[:, None]) * t) + 0.05 * rng.standard_normal((nch, nsamp))
    if in16:
        audio = np.clip(np.rint(a * 16000.0), -32768, 32767).astype(np.int16)
    else:
        audio = a.astype(f32)
        audio.view(np.uint32)[:, nsamp // 2] = NAN_PAYLOAD
    sc = S16_SCALE ** 2 if sense16 else 1.0
    thr = np.tile(np.array([RHO_OPEN, RHO_CLOSE, E_MIN * sc], f32), (nch, 1))
    return sense, audio, words, masks, thr
