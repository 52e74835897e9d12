"""The channel DCS decoder's model (include/sddc_ddc.h, sddc_ddc_channel_dcs_*; csrc/dcs_math.h; numpy only) and a
DCS signal generator.

  codeword        the (23, 12) encoder: d = 0x800 | code, parity = (d x^11) mod 0xC75 over GF(2), parity << 12 | d
  rotations, distance   the 23 rotations of a codeword in 23 bits; the minimum popcount distance over them
  window          (word, blocks) of a sample rate and a bit rate; counts: N[t]
  subbin_sums     S [nch, nwin, 192] of whole windows: the signs sorted by m(n) = (w n) >> 29
  bit_sums        c [.., 8, 23] from S (the sliding sums); bit_sums_direct: the same from the floor form,
                  floor((w n - t 2^29) / 2^32) = b, sample by sample (the identity the CPU test pins)
  definition      the whole definition; returns a dict: y (None without audio), G [nch, nwin] (the gate of every
                  window that holds a sample) and per complete window Q, N, d, t, best, word, u, v, open_after
  code_at, open_at, info_at, count   the side outputs of a call that ends at / covers stream indices
  nrz             the NRZ +-1 stream of a codeword at a phase word and a fractional bit offset
  fm              a real FM carrier modulated by a message (the pipeline test's ADC stream)
  table, make_case   seeded cases: segments off the window grid of silence, noise, codes of the table in noise
                  (either polarity), NaN / Inf / zero samples, with per-channel settings and an audio stream
"""
from __future__ import annotations

import numpy as np

B = 256                                  # SDDC_DDC_DCS_BLOCK
AUDIO_F32, AUDIO_S16 = 0, 1
ANY, OFF = -1, -2                        # SDDC_DDC_DCS_ANY, _OFF
BITS, PHASES, SUBBINS, SPAN = 23, 8, 192, 184
MASK = (1 << BITS) - 1
NO_MATCH = 24
NAN_PAYLOAD = 0x7FC12345
S16_SCALE = 8000.0
f32 = np.float32
DCS_CODES = tuple("""023 025 026 031 032 036 043 047 051 053 054 065 071 072 073 074 114 115 116 122 125 131 132 134 143 145 152
155 156 162 165 172 174 205 212 223 225 226 243 244 245 246 251 252 255 261 263 265 266 271 274 306 311 315 325 331 332 343 346
351 356 364 365 371 411 412 413 423 431 432 445 446 452 454 455 462 464 465 466 503 506 516 523 526 532 546 565 606 612 624 627
631 632 654 662 664 703 712 723 731 732 734 743 754""".split())


def codeword(code):
    """The 23-bit codeword of a code given as its octal digits ("023") or as the integer they spell."""
    c = int(code, 8) if isinstance(code, str) else int(code)
    assert 0 <= c < 512
    d = 0x800 | c
    rem = d << 11
    for bit in range(22, 10, -1):
        if (rem >> bit) & 1:
            rem ^= 0xC75 << (bit - 11)
    return (rem << 12) | d


def rot(cw, r):
    return ((cw << r) | (cw >> (BITS - r))) & MASK


def rotations(cw):
    return [rot(int(cw), r) for r in range(BITS)]


def popcount(v):
    """popcount of uint32 arrays (or ints)"""
    v = np.asarray(v, np.uint32)
    v = v - ((v >> np.uint32(1)) & np.uint32(0x55555555))
    v = (v & np.uint32(0x33333333)) + ((v >> np.uint32(2)) & np.uint32(0x33333333))
    v = (v + (v >> np.uint32(4))) & np.uint32(0x0F0F0F0F)
    return ((v * np.uint32(0x01010101)) >> np.uint32(24)).astype(np.int64)


def distance(word, cw):
    """min over the 23 rotations of cw of popcount(word xor rotation); word may be an array"""
    rr = np.array(rotations(cw), np.uint32)
    return popcount(np.asarray(word, np.uint32)[..., None] ^ rr).min(axis=-1)


def window(fs, bitrate=134.4):
    """(word, blocks) = (round(bitrate / fs * 2^32), ceil(24 * 2^32 / (256 word)))"""
    w = int(np.rint(bitrate / fs * 2.0 ** 32))
    assert 1 <= w <= 2 ** 29
    return w, -((-24 * 2 ** 32) // (B * w))


def smallest_word(W):
    """the smallest phase word that a window of W blocks admits: 256 W w >= 24 * 2^32"""
    return -((-24 * 2 ** 32) // (B * W))


def subbin_index(w, W):
    """m(n) for n < 256 W"""
    return ((np.uint64(w) * np.arange(W * B, dtype=np.uint64)) >> np.uint64(29)).astype(np.int64)


def counts(w, W):
    """N[t], t = 0..7: the number of n < 256 W with t <= m(n) < t + 184"""
    m = subbin_index(w, W)
    return np.array([int(((m >= t) & (m < t + SPAN)).sum()) for t in range(PHASES)], np.int64)


def sign(x):
    """+1, -1 or 0 per sample; a NaN is 0"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return (x > 0).astype(np.int64) - (x < 0).astype(np.int64)


def subbin_sums(s, w, W):
    """s [nch, nwin * 256 W] signs -> S [nch, nwin, 192]"""
    nch, n = s.shape
    WB = W * B
    assert n % WB == 0
    m = subbin_index(w, W)
    sel = np.zeros((WB, SUBBINS), f32)
    ok = m < SUBBINS
    sel[np.arange(WB)[ok], m[ok]] = 1
    # a sum of at most 65536 values of -1, 0, +1 is exact in float32
    return (s.reshape(nch * (n // WB), WB).astype(f32) @ sel).astype(np.int64).reshape(nch, n // WB, SUBBINS)


def bit_sums(S):
    """S [..., 192] -> c [..., 8, 23]: c[t][b] = S[8 b + t] + .. + S[8 b + t + 7]"""
    cs = np.concatenate([np.zeros(S.shape[:-1] + (1,), np.int64), np.cumsum(S, axis=-1)], axis=-1)
    t = np.arange(PHASES)[:, None]
    b = np.arange(BITS)[None, :]
    return cs[..., 8 * b + t + 8] - cs[..., 8 * b + t]


def bit_sums_direct(s, w, W):
    """s [256 W] signs of one window -> c [8, 23] by the floor form: the sum of s over floor((w n - t 2^29) / 2^32) = b"""
    n = np.arange(W * B, dtype=object)
    c = np.zeros((PHASES, BITS), np.int64)
    for t in range(PHASES):
        bb = np.array([(int(w) * int(i) - t * 2 ** 29) // 2 ** 32 for i in n], np.int64)   # Python's floor division
        for b in range(BITS):
            c[t, b] = int(s[bb == b].sum())
    return c


def s16_out(y):
    """demod_s16: round to nearest even, clamp, NaN -> 0"""
    y = np.asarray(y, f32)
    with np.errstate(all="ignore"):
        v = np.rint(np.clip(np.where(np.isnan(y), f32(0), y), -32768.0, 32767.0))
    return v.astype(np.int16)


def definition(sense, audio, codewords, params, w, W, e_open, e_close, A, H, fmt_out=AUDIO_F32):
    sense = np.asarray(sense)
    nch, n = sense.shape
    cws = [int(c) for c in np.asarray(codewords).reshape(-1)]
    params = np.asarray(params, np.int64).reshape(nch, 3)
    code, invert, eye = params[:, 0], params[:, 1], params[:, 2]
    WB = W * B
    nfull, nwin = n // WB, (n + WB - 1) // WB
    N_t = counts(w, W)
    S = subbin_sums(sign(sense[:, :nfull * WB]), w, W)
    c = bit_sums(S)                                           # [nch, nfull, 8, 23]
    Qt = np.abs(c).sum(axis=-1)                               # [nch, nfull, 8]
    t = np.argmax(Qt, axis=-1)                                # the first largest
    Q = np.take_along_axis(Qt, t[..., None], axis=-1)[..., 0]
    ct = np.take_along_axis(c, t[..., None, None], axis=-2)[..., 0, :]
    word = ((ct > 0).astype(np.int64) << np.arange(BITS)).sum(axis=-1)
    word = np.where(invert[:, None] == 1, word ^ MASK, word)
    N = N_t[t]
    d = np.full((nch, nfull), NO_MATCH, np.int64)
    best = np.full((nch, nfull), -1, np.int64)
    if nfull:
        dall = np.stack([distance(word, cw) for cw in cws], axis=-1)   # [nch, nfull, ncodes]
        for ch in range(nch):
            cand = range(len(cws)) if code[ch] == ANY else ([int(code[ch])] if code[ch] >= 0 else [])
            for i in cand:                                    # ascending: the lowest d, then the lowest i
                take = dall[ch, :, i] < d[ch]
                d[ch] = np.where(take, dall[ch, :, i], d[ch])
                best[ch] = np.where(take, i, best[ch])
    good = 256 * Q >= eye[:, None] * N
    u = good & (d <= e_open)
    v = good & (d <= e_close)
    bypass = code == OFF
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
    return {"y": y, "G": G, "S": S, "c": c, "Q": Q, "N": N, "d": d, "t": t, "best": best, "word": word, "u": u, "v": v,
            "open_after": open_after, "bypass": bypass, "n": n, "W": W}


def _last(m, end):
    return end // (m["W"] * B) - 1


def code_at(m, end):
    j = _last(m, end)
    nch = m["G"].shape[0]
    return np.where(m["v"][:, j], m["best"][:, j], -1).astype(np.int32) if j >= 0 else np.full(nch, -1, np.int32)


def open_at(m, end):
    j = _last(m, end)
    return (m["open_after"][:, j] if j >= 0 else m["bypass"]).astype(np.uint32)


def info_at(m, end):
    j = _last(m, end)
    nch = m["G"].shape[0]
    if j < 0:
        return np.zeros((nch, 4), np.uint32)
    return np.stack([m["Q"][:, j], m["N"][:, j], m["d"][:, j], m["t"][:, j]], axis=1).astype(np.uint32)


def count(m, a, b):
    """uint32 [nch]: the samples a <= i < b of the stream whose window is open."""
    g = np.repeat(m["G"], m["W"] * B, axis=1)[:, :m["n"]]
    return g[:, a:b].sum(axis=1).astype(np.uint32)


def nrz(cw, w, n, offset=0.0, start=0):
    """float64 [n]: +1 / -1 for the bits of cw, bit 0 first, repeated; bit k covers the samples start + i with
    floor((w (start + i) + offset 2^32) / 2^32) = k (offset in bits, any fraction)."""
    ph = np.uint64(w) * (np.uint64(start) + np.arange(n, dtype=np.uint64)) + np.uint64(int(offset * 2.0 ** 32) % (BITS << 32))
    k = ((ph >> np.uint64(32)) % np.uint64(BITS)).astype(np.int64)
    return np.where((int(cw) >> k) & 1, 1.0, -1.0)


def fm(message, fc, dev, amp, phase=0.0):
    """A real carrier of fc cycles per sample, frequency-modulated by dev * message cycles per sample."""
    t = np.arange(message.shape[0], dtype=np.float64)
    return amp * np.cos(2.0 * np.pi * (fc * t + dev * np.cumsum(message)) + phase)


def table(ncodes):
    """uint32 [ncodes]: the standard codes' codewords, then those of the lowest other codes."""
    std = [int(c, 8) for c in DCS_CODES]
    rest = [c for c in range(512) if c not in std]
    return np.array([codeword(c) for c in (std + rest)[:ncodes]], np.uint32)


def params_for(nch, ncodes, eye=96):
    """int32 [nch, 3] = (code, invert, eye): with three or more channels the first three are OFF, one code and
    ANY; then single codes and ANY of either polarity."""
    out = []
    for c in range(nch):
        if nch < 3:
            out.append(((5 * c + 2) % ncodes if c % 2 == 0 else ANY, 0, eye))
        else:
            kind = c % 5
            out.append(((OFF, 0, eye), ((7 * c + 3) % ncodes, 0, eye), (ANY, 0, eye), ((3 * c + 1) % ncodes, 1, eye),
                        (ANY, 1, 0))[kind])
    return np.array(out, np.int32)


def make_case(nch, nsamp, W, w, ncodes=104, sense16=False, in16=False, seed=1):
    """(sense [nch, nsamp], audio [nch, nsamp], codewords [ncodes], params [nch, 3])."""
    rng = np.random.default_rng(seed + 17 * W + 1000 * ncodes + (500 if sense16 else 0))
    cws = table(ncodes)
    params = params_for(nch, ncodes)
    WB = W * B
    s = np.zeros((nch, nsamp))
    special = []
    for c in range(nch):
        own = int(params[c, 0]) if params[c, 0] >= 0 else (11 * c + 5) % ncodes
        at, j = 0, 0
        while at < nsamp:
            ln = min(nsamp - at, WB * (1 + j % 3) + 37 + 11 * (c % 19))
            kind = (j + c + 2) % 6
            if kind == 0:
                seg = np.zeros(ln)                                       # silence: every sign is 0
            elif kind == 1:
                seg = rng.standard_normal(ln)                            # noise alone
            else:
                i = own if kind != 4 else (own + 1 + j) % ncodes         # the channel's code, or another one
                cw = int(cws[i]) ^ (MASK if params[c, 1] else 0)
                if kind == 5:
                    cw ^= 1 << ((j + c) % BITS) | 1 << ((3 * j + c + 7) % BITS)   # bit errors: one or two
                seg = nrz(cw, w, ln, offset=rng.uniform(0, BITS)) + (0.5 if kind != 3 else 1.5) * rng.standard_normal(ln)
            s[c, at:at + ln] = seg
            if kind == 2 and ln > 9:
                special.append((c, at + ln // 2))
            at += ln
            j += 1
    if sense16:
        sense = np.clip(np.rint(s * S16_SCALE), -32768, 32767).astype(np.int16)
        for q, (c, at) in enumerate(special):
            sense[c, at] = (-32768, 0, 32767)[q % 3]
    else:
        sense = s.astype(f32)
        for q, (c, at) in enumerate(special):
            sense[c, at] = (np.nan, np.inf, -np.inf, 0.0, -0.0)[q % 5]
    t = np.arange(nsamp)[None, :]
    a = 0.5 * np.sin(2 * np.pi * (0.01 + 0.003 * np.arange(nch)[:, None]) * t) + 0.05 * rng.standard_normal((nch, nsamp))
    if in16:
        audio = np.clip(np.rint(a * 16000.0), -32768, 32767).astype(np.int16)
    else:
        audio = a.astype(f32)
        audio.view(np.uint32)[:, nsamp // 2] = NAN_PAYLOAD
    return sense, audio, cws, params
