"""The channel audio filter's model (include/sddc_ddc.h, sddc_ddc_channel_audio_filter_*; numpy only).

  design64        the section designers' closed forms in float64
  recurrence64    the float64 plain recurrence on the float32 coefficients: the reference y64
  block_matrix    M = float32(A^B) exactly as the library builds it (B zero-input steps in double on
                  each unit vector, every product and sum one rounded double operation)
  block_form      the definition (E, R, Zr, adv) in float32 with a pluggable fmaf: fmaf_fast (through
                  float64, correct except for rare double roundings) or fmaf_exact (a Fraction, then
                  one correct rounding to float32); `sabotage` breaks it on purpose for the
                  discrimination test
  bound           bound[n] >= |y[n] - y64[n]| for the definition's float32 arithmetic

The bound, to first order in u = 2^-24 (the header states it).  A step of section k rounds five
values: y_k; the new s1_k and the inner fmaf(b1, x, s2), which both enter s1_k; the new s2_k and b2 x,
which both enter s2_k.  That is three error sources per section with magnitudes u |y_k|,
u (|s1_k| + |inner_k|) and u (|s2_k| + |b2 x|).  A unit error in y_k is a unit error of the input of
the sections after k and -a1, -a2 in section k's new states: the linearised step gives its direct
effect d_q on this sample's output and the perturbation v_q of the state after the step; errors in
s1_k, s2_k are unit state perturbations.  G[m] = c A^m is the output of zero-input step m from each
unit state (A and c read off one zero-input step per unit state), so the response of a source m + 1
samples later is
|G[m] v_q|: the absolute value of the powers' response, not a power of |A| (which diverges for
resonant sections).  R restarts from E at every block boundary, so the running recurrence's
roundings count inside the output's own block only; earlier blocks contribute the zero-state
recurrence's roundings (their magnitudes are those of the zero-state signals) and, per boundary and
row i, adv's 2S fmaf roundings and the rounding of M's entries: (2S + 1) u (|Z_i| + sum_j |M_ij| |E_j|).
The factor 1.01 covers the second order and the 2^-53 roundings of the model itself.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

B = 256                    # SDDC_DDC_AUDIO_BLOCK
U = 2.0 ** -24
IDENTITY, DC_BLOCK, ONE_POLE_LP, LOWPASS, HIGHPASS, NOTCH = range(6)


def design64(kind, f=0.25, q=np.sqrt(0.5)):
    """(b0, b1, b2, a1, a2) in float64 by the closed forms of sddc_ddc_biquad."""
    if kind == IDENTITY:
        return np.array([1.0, 0, 0, 0, 0])
    w = 2.0 * np.pi * f
    if kind == DC_BLOCK:
        r = np.exp(-w)
        return np.array([(1 + r) / 2, -(1 + r) / 2, 0, -r, 0])
    if kind == ONE_POLE_LP:
        al = np.exp(-w)
        return np.array([1 - al, 0, 0, -al, 0])
    cw, alpha = np.cos(w), np.sin(w) / (2 * q)
    a0 = 1 + alpha
    a1, a2 = -2 * cw / a0, (1 - alpha) / a0
    if kind == LOWPASS:
        b0 = (1 - cw) / (2 * a0)
        return np.array([b0, 2 * b0, b0, a1, a2])
    if kind == HIGHPASS:
        b0 = (1 + cw) / (2 * a0)
        return np.array([b0, -2 * b0, b0, a1, a2])
    if kind == NOTCH:
        return np.array([1 / a0, a1, 1 / a0, a1, a2])
    raise ValueError(kind)


def response(coef, f):
    """H(e^{j 2 pi f}) of the cascade coef [S, 5] in float64."""
    z1 = np.exp(-2j * np.pi * f)
    h = 1.0 + 0j
    for b0, b1, b2, a1, a2 in np.asarray(coef, np.float64):
        h *= (b0 + b1 * z1 + b2 * z1 * z1) / (1 + a1 * z1 + a2 * z1 * z1)
    return h


def stable(c):
    return abs(float(c[4])) < 1 and abs(float(c[3])) < 1 + float(c[4])


def _step64(cf, s, x, inject=-1):
    """One step in float64 with plain * and +; inject = k adds 1 to y_k (the linearised step).
    Returns y and, per section, (y_k, inner_k, b2 x_k)."""
    sig = []
    for k in range(len(cf)):
        b0, b1, b2, a1, a2 = cf[k]
        y = b0 * x + s[2 * k]
        if k == inject:
            y += 1.0
        inner = b1 * x + s[2 * k + 1]
        s[2 * k] = (-a1) * y + inner
        last = b2 * x
        s[2 * k + 1] = (-a2) * y + last
        sig.append((y, inner, last))
        x = y
    return x, sig


def _cf64(coef):
    return [tuple(float(v) for v in sec) for sec in np.asarray(coef, np.float32)]


def trace64(x, coef, reset_every=0):
    """The float64 recurrence of one channel: y [n], the source magnitudes mags [n, 3S] (|y_k|,
    |s1_k| + |inner_k|, |s2_k| + |b2 x_k| after the step) and the state before every step and after
    the last, states [n + 1, 2S] (with reset_every: before the reset).  reset_every = B zeroes the
    state at every block start: the zero-state recurrence."""
    cf = _cf64(coef)
    S = len(cf)
    n = len(x)
    y = np.zeros(n)
    mags = np.zeros((n, 3 * S))
    states = np.zeros((n + 1, 2 * S))
    s = [0.0] * (2 * S)
    for i in range(n):
        if reset_every and i % reset_every == 0:
            s = [0.0] * (2 * S)
        if not reset_every:
            states[i] = s
        y[i], sig = _step64(cf, s, float(x[i]))
        if reset_every:
            states[i + 1] = s
        for k, (yk, inner, last) in enumerate(sig):
            mags[i, 3 * k] = abs(yk)
            mags[i, 3 * k + 1] = abs(s[2 * k]) + abs(inner)
            mags[i, 3 * k + 2] = abs(s[2 * k + 1]) + abs(last)
    if not reset_every:
        states[n] = s
    return y, mags, states


def recurrence64(x, coef):
    """y64 [nch, n] of x [nch, n] through coef [nch, S, 5]."""
    x = np.atleast_2d(x)
    return np.stack([trace64(x[c], coef[c])[0] for c in range(x.shape[0])])


def block_matrix(coef, steps=B):
    """M [2S, 2S] float32 of one channel's coef [S, 5] (steps != B: the sabotaged matrix)."""
    cf = _cf64(coef)
    n = 2 * len(cf)
    M = np.zeros((n, n), np.float32)
    for col in range(n):
        s = [0.0] * n
        s[col] = 1.0
        for _ in range(steps):
            _step64(cf, s, 0.0)
        M[:, col] = np.asarray(s, np.float64).astype(np.float32)
    return M


def fmaf_fast(a, b, c):
    return float(np.float32(float(a) * float(b) + float(c)))


def round_f32(v: Fraction) -> float:
    """v rounded to the nearest float32, ties to even, subnormals included (no overflow)."""
    if v == 0:
        return 0.0
    sign = -1.0 if v < 0 else 1.0
    m = abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1                      # 2^e <= m < 2^(e+1)
    e = max(e, -126)
    q = m / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * float(n) * 2.0 ** (e - 23)


def fmaf_exact(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def block_form(x, coef, M=None, fmaf=fmaf_fast, sabotage=None, pos=0):
    """The definition on one channel in float32: x [n], coef [S, 5] -> y [n] float32.  sabotage:
    "drop_z" leaves Z out of adv, ("skip_adv", b) skips the adv at boundary b (a wrong M is passed as
    M).  pos: the stream position of x[0]."""
    cf = _cf64(coef)
    S = len(cf)
    N = 2 * S
    M = block_matrix(coef) if M is None else M
    Mf = [[float(M[i, j]) for j in range(N)] for i in range(N)]
    E, R, Z = [0.0] * N, [0.0] * N, [0.0] * N

    def step(s, v):
        for k in range(S):
            b0, b1, b2, a1, a2 = cf[k]
            yk = fmaf(b0, v, s[2 * k])
            s[2 * k] = fmaf(-a1, yk, fmaf(b1, v, s[2 * k + 1]))
            s[2 * k + 1] = fmaf(-a2, yk, fmaf(b2, v, 0.0))   # b2 * x: one rounding
            v = yk
        return v

    y = np.zeros(len(x), np.float32)
    n = pos
    for i in range(len(x)):
        v = float(np.float32(x[i]))
        y[i] = step(R, v)
        step(Z, v)
        n += 1
        if n % B == 0:
            if sabotage == ("skip_adv", n // B):
                nE = list(E)
            else:
                nE = []
                for r in range(N):
                    acc = 0.0 if sabotage == "drop_z" else Z[r]
                    for j in range(N):
                        acc = fmaf(Mf[r][j], E[j], acc)
                    nE.append(acc)
            E, R, Z = nE, list(nE), [0.0] * N
    return y


def _conv(a, r):
    """sum_{t' <= t} a[t'] r[t - t'] for t < len(a); long inputs through the FFT (its rounding, some
    1e-16 of the largest term, is far inside the bound's 1.01)."""
    n = len(a)
    if n <= 4096:
        return np.convolve(a, r[:n])[:n]
    m = 1 << int(np.ceil(np.log2(2 * n)))
    return np.fft.irfft(np.fft.rfft(a, m) * np.fft.rfft(r[:n], m), m)[:n]


def bound(x, coef):
    """bound [n] of one channel (x [n], coef [S, 5]) for a stream that starts at position 0."""
    cf = _cf64(coef)
    S = len(cf)
    N = 2 * S
    n = len(x)
    _, full, fstates = trace64(x, coef)
    _, zs, zstates = trace64(x, coef, reset_every=B)
    M = np.abs(block_matrix(coef).astype(np.float64))
    # one zero-input step from unit state i: the output c[i] and the new state A[:, i]; G[m] = c A^m
    A, c = np.zeros((N, N)), np.zeros(N)
    for i in range(N):
        s = [0.0] * N
        s[i] = 1.0
        c[i] = _step64(cf, s, 0.0)[0]
        A[:, i] = s
    G = np.zeros((n + 1, N))
    g = c
    for m in range(n + 1):
        G[m] = g
        g = g @ A
    # the sources: direct effect d_q and response r_q[m] = |G[m] v_q|
    d = np.zeros(3 * S)
    r = np.zeros((3 * S, n + 1))
    for k in range(S):
        s = [0.0] * N
        out, _ = _step64(cf, s, 0.0, inject=k)
        d[3 * k] = abs(out)
        r[3 * k] = np.abs(G @ np.asarray(s))
        r[3 * k + 1] = np.abs(G[:, 2 * k])
        r[3 * k + 2] = np.abs(G[:, 2 * k + 1])
    # errors made before sample i: the zero-state recurrence's over the whole stream, and inside
    # i's own block the running recurrence's in their place
    acc = full @ d
    for q in range(3 * S):
        lag = np.concatenate([[0.0], _conv(zs[:, q], r[q])[:-1]])
        for lo in range(0, n, B):
            hi = min(n, lo + B)
            own = np.convolve(full[lo:hi, q] - zs[lo:hi, q], r[q, :B])[:hi - lo]
            lag[lo + 1:hi] += own[:-1]
        acc = acc + lag
    out = U * acc
    for b in range(1, (n - 1) // B + 1):
        E, Z = np.abs(fstates[(b - 1) * B]), np.abs(zstates[b * B])
        a = (2 * S + 1) * U * (Z + M @ E)
        out[b * B:] += np.abs(G[:n - b * B]) @ a
    return 1.01 * out


def bounds(x, coef):
    x = np.atleast_2d(x)
    return np.stack([bound(x[c], coef[c]) for c in range(x.shape[0])])


def make_input(nch, n, seed=1):
    """Audio-like float32 streams in (-1, 1) with a DC part: [nch, n]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.4 * rng.standard_normal((nch, n))
    for c in range(nch):
        x[c] += 0.3 + 0.25 * np.sin(2 * np.pi * (0.003 + 0.011 * (c % 7)) * t + c)
    return np.clip(x, -0.999, 0.999).astype(np.float32)
