"""The channel stereo decoder without a GPU (pytest -m "not gpu"): the CPU backend against the numpy model of the
definition (tools/channel_stereo_model.py) bit for bit, the stream properties (cuts, reset, the position next
to the phase wrap), the pilot measurement against the tone detector's, the derived bounds of stereo_math.h
against the float64 evaluation, the function on a synthesised multiplex (separation, mono fall-back, gate
timing) and the argument checks of the C ABI.  B = the block length (STEREO_BLOCK).
"""
from __future__ import annotations

import functools
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load("channel_stereo_model")

from extio_sddc_amd import STEREO_BLOCK as B  # noqa: E402
from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, DEVICE_CPU, STEREO_AUTO, STEREO_MONO, DDCError, R2iq,  # noqa: E402
                            stereo_pilot_word)

ERR_ARG, ERR_STATE = -1, -4
F, S = AUDIO_F32, AUDIO_S16
COMBOS = [(F, F), (F, S), (S, F), (S, S)]   # (input, outputs)
# (nch, nsamp, W): the GPU test's shapes, and a stream of 40 windows at each W
SHAPES = [(1, 1, 3), (1, B, 3), (1, 3 * B + 17, 3), (3, 2 * 8 * B + 3, 8), (1024, 2, 8), (1, 66 * B + 5, 1), (2, 258 * B + 1, 3),
          (4, 40 * B + 3, 1), (4, 40 * 3 * B + 3, 3), (4, 40 * 8 * B + 3, 8)]
A_H = (2, 1)
SIDES = ("stereo", "count", "level", "phase")


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def case(nch, n, W, in16):
    x, w, modes, params = M.make_case(nch, n, W, in16)
    for a in (x, modes, params):
        a.setflags(write=False)
    return x, w, modes, params


@functools.lru_cache(maxsize=None)
def model(nch, n, W, combo, pos0=0):
    x, w, modes, params = case(nch, n, W, combo[0] == S)
    return M.definition(x, w, modes, params, W, *A_H, combo[1], pos0)


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run(r, x, cuts):
    """The stream in calls of `cuts` samples: (left, right) and the side outputs of every call."""
    ls, rs, sides, at = [], [], [], 0
    for ln in cuts:
        o = r.channel_stereo(x[:, at:at + ln])
        ls.append(o.pop("left"))
        rs.append(o.pop("right"))
        sides.append(o)
        at += ln
    return (np.concatenate(ls, axis=1), np.concatenate(rs, axis=1)), sides


def check_against_model(y, sides, m, cuts, what=None):
    for a, name in zip(y, ("left", "right")):
        assert a.dtype == m[name].dtype
        np.testing.assert_array_equal(bits(a), bits(m[name]), err_msg=f"{name} {what}")
    at = 0
    for s, ln in zip(sides, cuts):
        end = at + ln
        np.testing.assert_array_equal(s["stereo"], M.stereo_at(m, end), err_msg=f"stereo {what}")
        np.testing.assert_array_equal(s["count"], M.count(m, at, end), err_msg=f"count {what}")
        np.testing.assert_array_equal(bits(s["level"]), bits(M.level_at(m, end)), err_msg=f"level {what}")
        np.testing.assert_array_equal(bits(s["phase"]), bits(M.phase_at(m, end)), err_msg=f"phase {what}")
        at = end


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-W{s[2]}")
def test_cpu_equals_the_model(cpu, shape):
    nch, n, W = shape
    for combo in COMBOS:
        x, w, modes, params = case(nch, n, W, combo[0] == S)
        cpu.setChannelStereoDecoder(w, modes, params, W, *A_H, *combo)
        y, sides = run(cpu, x, [n])
        check_against_model(y, sides, model(nch, n, W, combo), [n], (shape, combo))


def test_the_rich_case_is_rich():
    """Open and closed windows, a bad window, a MONO channel and an AUTO channel without a pilot; the non-finite
    samples of the closed streams pass with their bits."""
    nch, n, W = SHAPES[-1]
    x, w, modes, params = case(nch, n, W, False)
    m = model(nch, n, W, (F, F))
    assert list(modes) == [STEREO_AUTO, STEREO_MONO, STEREO_AUTO, STEREO_AUTO]
    for c in (0, 3):
        assert m["G"][c].any() and not m["G"][c].all() and m["v"][c].any() and not m["v"][c].all()
    assert m["bad"][0].sum() >= 2 and m["G"][0][np.flatnonzero(m["bad"][0])[-1]]   # one bad window while in stereo
    assert not m["G"][1].any() and m["gate_after"][1].any()      # MONO: the pilot is seen, nothing is decoded
    assert not m["G"][2].any() and not m["u"][2].any()           # no pilot
    for c in (1, 2):
        for name in ("left", "right"):
            np.testing.assert_array_equal(bits(m[name][c]), bits(x[c]))
    assert (bits(m["left"][0]) != bits(m["right"][0])).any()


CUTS = {"one": lambda n, W: [1, n - 1], "edges": lambda n, W: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n, W: [100, B, n - B - 100],
        "window": lambda n, W: [W * B - 2, 1, 1, 1, 1, n - W * B - 2], "inside": lambda n, W: [W * B + W * B // 2 + 7, n - W * B - W * B // 2 - 7]}


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_any_cut_into_calls_gives_the_same_bits(cpu, cut):
    for k, (nch, n, W) in enumerate((SHAPES[3], SHAPES[6], SHAPES[8])):
        combo = COMBOS[k % len(COMBOS)]
        cuts = CUTS[cut](n, W)
        x, w, modes, params = case(nch, n, W, combo[0] == S)
        cpu.setChannelStereoDecoder(w, modes, params, W, *A_H, *combo)
        y, sides = run(cpu, x, cuts)
        check_against_model(y, sides, model(nch, n, W, combo), cuts, (cut, nch, n, W))


def test_reset_restores_a_new_stream(cpu):
    nch, n, W = SHAPES[8]
    x, w, modes, params = case(nch, n, W, False)
    m = model(nch, n, W, (F, F))
    cpu.setChannelStereoDecoder(w, modes, params, W, *A_H)
    run(cpu, x[:, :n // 2 + 11], [n // 2 + 11])
    cpu.resetChannelStereoDecoder()
    check_against_model(*run(cpu, x, [n]), m, [n])
    o = None
    cpu.resetChannelStereoDecoder()
    o = cpu.channel_stereo(x[:, :1])
    assert not o["stereo"].any() and not o["count"].any() and not o["level"].any()
    np.testing.assert_array_equal(o["phase"], np.tile(np.float32([1, 0]), (nch, 1)))


@pytest.mark.parametrize("in16", [False, True])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_level_equals_the_tone_detectors(cpu, W, in16):
    """(P, E) is the tone detector's d_level for the tone table {w} and the same W on the same stream."""
    nch, n = 4, 40 * W * B + 3
    x, w, modes, params = case(nch, n, W, in16)
    fmt = S if in16 else F
    cpu.setChannelStereoDecoder(w, modes, params, W, *A_H, fmt, F)
    cpu.setChannelToneDetector([w], np.ones(nch, np.uint64), params[:, :3], W, *A_H, fmt)
    cuts = [W * B - 1, 1, 5 * W * B + 77, n - 6 * W * B - 77]
    _, sides = run(cpu, x, cuts)
    at, seen = 0, set()
    for s, ln in zip(sides, cuts):
        t = cpu.channel_tone(x[:, at:at + ln])
        np.testing.assert_array_equal(bits(s["level"]), bits(t["level"]))
        seen.add(bits(s["level"]).tobytes())
        at += ln
    assert len(seen) == len(cuts)


@pytest.mark.parametrize("scale", [2.0 ** -20, 1.0, 2.0 ** 12])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_float64_checks(W, scale):
    """The decisions match the float64 evaluation outside tone_math.h's bounds; q is within stereo_bound_q of the
    float64 q wherever a window sets it; L and R are within stereo_bound_lr of the float64 evaluation given the same
    float32 q."""
    nch, n = 4, 40 * W * B + 3
    x0, w, modes, params0 = case(nch, n, W, False)
    x = (x0 * np.float32(scale)).astype(np.float32)
    params = params0.copy()
    params[:, 2] = (params0[:, 2].astype(np.float64) * scale * scale).astype(np.float32)
    m32 = M.definition(x, w, modes, params, W, *A_H)
    m64 = M.definition(x, w, modes, params, W, *A_H, dtype=np.float64)
    und = M.undecided(m64)
    for name in ("u", "v"):
        assert (m32[name] == m64[name])[~und].all()
    assert und.mean() < 0.2
    sets = m32["v"] & m64["v"]
    assert sets.sum() >= 20
    err = np.abs(m32["Q_after"].astype(np.float64) - m64["Q_after"]).max(axis=-1)
    bound = M.bound_q(m64["P"], m64["X"], W)
    print(f"W {W} scale {scale}: max |q - q64| {err[sets].max():.3e}, the bound there {bound[sets][np.argmax(err[sets])]:.3e}")
    assert (err[sets] <= bound[sets]).all() and bound[sets].max() < 0.05
    # the outputs, given the float32 q, where both evaluations decode
    m64q = M.definition(x, w, modes, params, W, *A_H, dtype=np.float64, q_force=m32["Qw"])
    g = np.repeat(m32["G"] & m64q["G"], W * B, axis=1)[:, :n] & np.isfinite(x)
    assert g.sum() > 10 * W * B
    g2 = M.scale(params, W)[:, 3:4]
    lim = M.bound_lr(x, g2)
    for name in ("left", "right"):
        with np.errstate(invalid="ignore"):   # the streams' non-finite samples, which g leaves out
            e = np.abs(m32[name].astype(np.float64) - m64q[name])
        worst = np.argmax(np.where(g, e / np.maximum(lim, 1e-300), 0))
        print(f"  {name}: max error / bound {e.ravel()[worst] / lim.ravel()[worst]:.3f}")
        assert (e[g] <= lim[g]).all()
    assert (M.undecided(m64q) == und).all()


@pytest.mark.parametrize("W", [3, 8])
def test_the_position_next_to_the_phase_wrap(cpu, W):
    WB = W * B
    pos0 = (2 ** 32 // WB - 2) * WB
    nch, n, combo = 3, 4 * WB + 17, (F, F)
    x, w, modes, params = case(nch, n, W, False)
    m = model(nch, n, W, combo, pos0)
    assert not np.array_equal(bits(M.phase_at(m, n)), bits(M.phase_at(model(nch, n, W, combo), n)))
    cpu.setChannelStereoDecoder(w, modes, params, W, *A_H)
    f = cpu._L.sddc_ddc_internal_chst_set_position
    assert f(cpu._h, pos0 + B) == ERR_ARG and f(cpu._h, pos0) == 0
    cuts = [WB + 5, WB, n - 2 * WB - 5]
    check_against_model(*run(cpu, x, cuts), m, cuts)


FS, WF, AF = 250000.0, 8, 2


def _projection(y, f):
    """The amplitude of the tone f in y, a whole number of its cycles, under a Hann window: it keeps the decoder's
    images around 19, 38, 57 and 76 kHz, which are no whole number of cycles and are the low-pass's to remove, out of
    the audio tones' bins."""
    n = y.shape[-1]
    t = np.arange(n)
    win = 1.0 - np.cos(2 * np.pi * t / n)
    return np.abs((y.astype(np.float64) * win * np.exp(-2j * np.pi * f / FS * t)).sum()) * 2 / n


def _separation(left, right, fl, fr, start):
    """dB: the left tone against the right tone in the left output, and the converse in the right output"""
    l, r = left[start:], right[start:]
    return (20 * np.log10(_projection(l, fl) / _projection(l, fr)), 20 * np.log10(_projection(r, fr) / _projection(r, fl)))


@functools.lru_cache(maxsize=None)
def function_case():
    """fs = 250 kS/s, W = 8, g = 1, pilot 0.1 at alpha = 0.7, a left tone of 8 and a right tone of 25 cycles per
    window, 12 windows.  The pilot is no whole number of cycles per window (155.648), so the tones leak into its bin
    by about 0.9 / (pi (155.6 - k)) of their amplitude and turn the measured phase; amplitudes of 0.3 and 0.25 keep
    that error below 0.01 rad, which is what the condition on the input (80 dB in float64) asks for."""
    WB = WF * B
    n = 12 * WB
    fl, fr = 8 * FS / WB, 25 * FS / WB
    t = np.arange(n)
    left, right = 0.3 * np.sin(2 * np.pi * fl / FS * t + 0.2), 0.25 * np.sin(2 * np.pi * fr / FS * t + 1.1)
    x = M.mpx(left, right, FS, 0.1, 0.7).astype(np.float32)[None, :]
    x.setflags(write=False)
    return x, fl, fr, n


def test_function_separation(cpu):
    """The float64 model alone separates the synthesised multiplex by >= 80 dB; the float32 stage is within 1 dB of
    the float64 figure or reaches 80 dB itself."""
    x, fl, fr, n = function_case()
    w = stereo_pilot_word(FS)
    assert w == M.word(FS)
    params = np.float32([[M.RHO_OPEN, M.RHO_CLOSE, M.E_MIN, 1.0]])
    start = (AF + 1) * WF * B
    m64 = M.definition(x, w, [STEREO_AUTO], params, WF, AF, 0, dtype=np.float64)
    assert m64["G"][0, AF:].all() and not m64["G"][0, :AF].any()
    s64 = _separation(m64["left"][0], m64["right"][0], fl, fr, start)
    cpu.setChannelStereoDecoder(w, [STEREO_AUTO], params, WF, AF, 0)
    o = cpu.channel_stereo(x)
    s32 = _separation(o["left"][0], o["right"][0], fl, fr, start)
    share = o["level"][0, 0] / (WF * B * o["level"][0, 1])
    print(f"separation float64 {s64[0]:.1f} / {s64[1]:.1f} dB, float32 {s32[0]:.1f} / {s32[1]:.1f} dB, pilot share {share:.4f}")
    assert min(s64) >= 80.0
    for a, b in zip(s32, s64):
        assert a >= 80.0 or a >= b - 1.0
    assert o["stereo"][0] == 1 and o["count"][0] == n - AF * WF * B and 0.004 < share < 0.2
    # the decoded tones: 0.45 (L + R) + 0.45 (L - R) = 0.9 L
    assert abs(_projection(o["left"][0, start:], fl) - 0.9 * 0.3) < 1e-4 and abs(_projection(o["right"][0, start:], fr) - 0.9 * 0.25) < 1e-4


def test_function_mono_fallbacks(cpu):
    x, fl, fr, n = function_case()
    w = stereo_pilot_word(FS)
    params = np.float32([[M.RHO_OPEN, M.RHO_CLOSE, M.E_MIN, 1.0]])
    # without the pilot: L = R = x bit for bit, never stereo
    t = np.arange(n)
    nopilot = (x[0].astype(np.float64) - 0.1 * np.sin(2 * np.pi * 19000.0 / FS * t + 0.7)).astype(np.float32)[None, :]
    cpu.setChannelStereoDecoder(w, [STEREO_AUTO], params, WF, AF, 0)
    o = cpu.channel_stereo(nopilot)
    assert o["stereo"][0] == 0 and o["count"][0] == 0
    np.testing.assert_array_equal(bits(o["left"]), bits(nopilot))
    np.testing.assert_array_equal(bits(o["right"]), bits(nopilot))
    # g = 0: stereo is detected, L = R = x in value
    params0 = params.copy()
    params0[0, 3] = 0.0
    cpu.setChannelStereoDecoder(w, [STEREO_AUTO], params0, WF, AF, 0)
    o = cpu.channel_stereo(x)
    assert o["stereo"][0] == 1 and o["count"][0] == n - AF * WF * B
    assert (o["left"] == x).all() and (o["right"] == x).all()
    # MONO: the bypass
    cpu.setChannelStereoDecoder(w, [STEREO_MONO], params, WF, AF, 0)
    o = cpu.channel_stereo(x)
    assert o["stereo"][0] == 0 and o["count"][0] == 0
    np.testing.assert_array_equal(bits(o["left"]), bits(x))
    np.testing.assert_array_equal(bits(o["right"]), bits(x))


@pytest.mark.parametrize("A,H", [(1, 0), (2, 1), (3, 2)])
def test_gate_timing(cpu, A, H):
    """A pilot that starts (late) in window j opens window j + 1 + A and holds H windows after it stops (early in
    window k): the windows k + 1 .. k + H are still decoded, with the q of window k - 1."""
    W, j, k = 2, 3, 12
    WB = W * B
    n = (k + H + 4) * WB
    t = np.arange(n)
    rng = np.random.default_rng(5)
    prog = 0.3 * np.sin(2 * np.pi * 1000.0 / FS * t) + 0.01 * rng.standard_normal(n)
    on = (t >= j * WB + 9 * WB // 10) & (t < k * WB + WB // 10)
    x = (prog + 0.1 * on * np.sin(2 * np.pi * 19000.0 / FS * t + 0.5)).astype(np.float32)[None, :]
    params = np.float32([[M.RHO_OPEN, M.RHO_CLOSE, M.E_MIN, 1.0]])
    cpu.setChannelStereoDecoder(stereo_pilot_word(FS), [STEREO_AUTO], params, W, A, H)
    decoded, phases = [], []
    for i in range(n // WB):
        o = cpu.channel_stereo(x[:, i * WB:(i + 1) * WB])
        decoded.append(int(o["count"][0]))
        phases.append(o["phase"][0].copy())
        assert (o["count"][0] == 0) == np.array_equal(bits(o["left"]), bits(x[:, i * WB:(i + 1) * WB]))
    assert decoded == [WB if j + 1 + A <= i <= k + H else 0 for i in range(n // WB)]
    # q follows the pilot while it is there and is held from window k - 1 on
    assert abs(np.arctan2(phases[k - 1][1], phases[k - 1][0]) - 1.0) < 0.02
    for i in range(k, n // WB):
        np.testing.assert_array_equal(bits(phases[i]), bits(phases[k - 1]))
    assert not np.array_equal(bits(phases[k - 2]), bits(phases[k - 1]))


def test_set_and_call_validity(cpu):
    L = cpu._L
    nch, n = 2, 600
    w = stereo_pilot_word(FS)
    good = np.float32([[0.004, 0.002, 1e-6, 1.0]] * nch)
    modes = np.uint8([STEREO_AUTO, STEREO_MONO])

    def set_(word=w, m=modes, p=good, c=nch, window=8, attack=1, hang=0, fin=F, fout=F):
        p = np.ascontiguousarray(p, np.float32)
        m = np.ascontiguousarray(m, np.uint8)
        return L.sddc_ddc_set_channel_stereo_decoder(cpu._h, word, m.ctypes.data, p.ctypes.data, c, window, attack, hang, fin, fout)

    x = np.zeros((nch, n), np.float32)
    left, right = np.zeros((nch, n), np.float32), np.zeros((nch, n), np.float32)

    def call(x_=None, c=nch, m=n, xs=n, l_=None, r_=None, ost=n):
        x_ = x.ctypes.data if x_ is None else x_
        l_ = left.ctypes.data if l_ is None else l_
        r_ = right.ctypes.data if r_ is None else r_
        return L.sddc_ddc_channel_stereo_host(cpu._h, x_, c, m, xs, l_, r_, ost, None, None, None, None)

    assert call() == ERR_STATE and L.sddc_ddc_channel_stereo_reset(cpu._h) == ERR_STATE      # before a set
    with pytest.raises(DDCError):
        cpu.channel_stereo(x)

    def bad_params(col, value):
        p = good.copy()
        p[1, col] = value
        return p

    for kw in ({"word": 0}, {"m": [STEREO_AUTO, 2]}, {"c": -1}, {"c": 1 << 20}, {"window": 0}, {"window": 257}, {"attack": 0},
               {"attack": 256}, {"hang": -1}, {"hang": 65536}, {"fin": 2}, {"fout": -1}, {"p": bad_params(0, 0.0)},
               {"p": bad_params(0, 1.5)}, {"p": bad_params(1, 0.0)}, {"p": bad_params(1, 0.005)}, {"p": bad_params(0, np.nan)},
               {"p": bad_params(2, -1.0)}, {"p": bad_params(2, np.inf)}, {"p": bad_params(3, -0.5)}, {"p": bad_params(3, np.nan)},
               {"p": bad_params(3, 3e38)}):
        assert set_(**kw) == ERR_ARG, kw
        assert call() == ERR_STATE, kw          # a refused set sets nothing
    assert set_() == 0
    assert call() == 0
    assert call(c=1) == ERR_STATE and call(m=0) == ERR_ARG and call(m=(1 << 40) + 1, xs=1 << 41, ost=1 << 41) == ERR_ARG
    assert call(xs=n - 1) == ERR_ARG and call(ost=n - 1) == ERR_ARG
    assert call(x_=0) == ERR_ARG and call(l_=0) == ERR_ARG and call(r_=0) == ERR_ARG
    assert call(x_=x.ctypes.data + 2, m=n - 1) == ERR_ARG and call(l_=left.ctypes.data + 2, m=n - 1) == ERR_ARG
    assert call(l_=x.ctypes.data) == ERR_ARG and call(r_=x.ctypes.data + 4 * n) == ERR_ARG     # an output on the input
    assert call(r_=left.ctypes.data) == ERR_ARG and call(r_=left.ctypes.data + 4 * n) == ERR_ARG   # on each other
    # a failed call leaves the stream where it was: the position is still n
    xr = M.make_case(nch, 3 * n, 1)[0]
    cpu.setChannelStereoDecoder(w, modes, good, 1)
    a = cpu.channel_stereo(xr[:, :n])
    assert call(m=0) == ERR_ARG
    b = cpu.channel_stereo(xr[:, n:])
    cpu.setChannelStereoDecoder(w, modes, good, 1)
    whole = cpu.channel_stereo(xr)
    np.testing.assert_array_equal(bits(np.concatenate([a["left"], b["left"]], axis=1)), bits(whole["left"]))
    np.testing.assert_array_equal(bits(b["phase"]), bits(whole["phase"]))
    # two output views of one buffer, the right streams after the left ones, are legal
    lr = np.zeros((2 * nch, n), np.float32)
    assert call(l_=lr.ctypes.data, r_=lr.ctypes.data + 4 * nch * n) == 0
    assert L.sddc_ddc_set_channel_stereo_decoder(cpu._h, 0, None, None, 0, 0, 0, 0, 0, 0) == 0   # off
    assert call() == ERR_STATE


def test_the_abi_constants_and_params():
    with open(os.path.join(ROOT, "include", "sddc_ddc.h")) as f:
        pub = f.read()
    with open(os.path.join(ROOT, "extio_sddc_amd", "csrc", "sddc_ddc_internal.h")) as f:
        internal = f.read()
    for name, value in (("BLOCK", B), ("MAX_WINDOW", 256), ("MONO", STEREO_MONO), ("AUTO", STEREO_AUTO)):
        assert re.search(rf"#define\s+SDDC_DDC_STEREO_{name}\s+{value}\b", pub)
    assert re.search(r"#define\s+SDDC_DDC_PARAM_CHST_MAX_WGS\s+31\b", internal)
    assert re.search(r"#define\s+SDDC_DDC_PARAM_CHST_RUN_BLOCKS\s+32\b", internal)
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        f = r._L.sddc_ddc_internal_set_param
        assert f(r._h, 31, 3) == 0 and f(r._h, 32, 8) == 0 and f(r._h, 31, -1) == ERR_ARG and f(r._h, 32, (1 << 20) + 1) == ERR_ARG
