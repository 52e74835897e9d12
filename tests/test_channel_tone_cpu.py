"""The channel tone detector without a GPU: the CPU backend (sddc_ddc_channel_tone_host of a CPU handle)
against the numpy float32 transcription of the definition bit for bit, outputs and all five side outputs,
for any cut (tools/channel_tone_model.py); its decisions and powers against the float64 evaluation within
the bounds that csrc/tone_math.h derives; a stream next to the 2^32 wrap of the sample phase; the 50 CTCSS
tones in noise; the gate's timing; and the error returns.

The bounds are the header's derived ones (bound_p, bound_te in the model): nothing here is fitted to the code
under test.
"""
from __future__ import annotations

import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load("channel_tone_model")

from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, CTCSS_TONES, DEVICE_CPU, TONE_BLOCK, DDCError, R2iq,  # noqa: E402
                            tone_window, tone_word)
from extio_sddc_amd._lib import load  # noqa: E402

B = TONE_BLOCK
ERR_ARG, ERR_STATE = -1, -4
WINDOWS = [1, 3, 16]
MASKS = [1, 9, 64]
# (sense S16, audio: None or (in, out))
COMBOS = [(False, None), (True, None), (False, (AUDIO_F32, AUDIO_F32)), (True, (AUDIO_F32, AUDIO_S16)),
          (False, (AUDIO_S16, AUDIO_F32)), (True, (AUDIO_S16, AUDIO_S16))]


def shapes(W):
    return [(1, 1), (1, B), (1, W * B), (1, 3 * W * B + 17), (3, 2 * W * B + 3)]


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def case(nch, n, W, mask_tones, sense16, in16, ntones=64):
    arrs = M.make_case(nch, n, W, ntones, mask_tones, sense16, in16)
    for a in arrs:
        a.setflags(write=False)
    return arrs


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_cut(r, sense, audio, cut):
    """The stream through channel_tone in calls of the cut's lengths: outputs and per-call side outputs."""
    ys, sides, a = [], [], 0
    for ln in cut:
        o = r.channel_tone(sense[:, a:a + ln], None if audio is None else audio[:, a:a + ln])
        ys.append(o["out"])
        sides.append(o)
        a += ln
    assert a == sense.shape[1]
    return (None if audio is None else np.concatenate(ys, axis=1)), sides


def check_sides(ref, cut, sides, what, pos=0):
    a = pos
    for ln, o in zip(cut, sides):
        assert np.array_equal(o["tone"], M.tone_at(ref, a + ln)), (what, a)
        assert np.array_equal(o["open"], M.open_at(ref, a + ln)), (what, a)
        assert np.array_equal(o["count"], M.count(ref, a, a + ln)), (what, a)
        assert np.array_equal(bits(o["level"]), bits(M.level_at(ref, a + ln))), (what, a)
        assert np.array_equal(bits(o["powers"]), bits(M.powers_at(ref, a + ln))), (what, a)
        a += ln


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("shape", range(5))
def test_cpu_equals_model(cpu, W, shape):
    nch, n = shapes(W)[shape]
    A, H = (1, 0) if W == 16 else (2, 1)
    for mt in MASKS:
        for sense16, fmts in COMBOS:
            fin, fout = fmts or (AUDIO_F32, AUDIO_F32)
            sense, audio, words, masks, thr = case(nch, n, W, mt, sense16, fin == AUDIO_S16)
            audio = audio if fmts else None
            ref = M.definition(sense, audio, words, masks, thr, W, A, H, fout)
            cpu.setChannelToneDetector(words, masks, thr, W, A, H, AUDIO_S16 if sense16 else AUDIO_F32, fin, fout)
            y, sides = run_cut(cpu, sense, audio, [n])
            what = (W, nch, n, mt, sense16, fmts)
            if fmts:
                assert y.dtype == ref["y"].dtype
                assert np.array_equal(bits(y), bits(ref["y"])), what
            else:
                assert y is None
            check_sides(ref, [n], sides, what)


def test_case_is_rich():
    """The generator's streams open and close gates, hold bad windows, and a NaN passes with its payload."""
    W, nch = 3, 3
    n = 12 * W * B + 3
    sense, audio, words, masks, thr = case(nch, n, W, 9, False, False)
    ref = M.definition(sense, audio, words, masks, thr, W, 1, 0)
    assert ref["bad"].any() and ref["u"].any() and (~ref["v"][1:]).any()
    g = ref["G"][1:].astype(np.int8)
    assert (np.diff(g, axis=1) > 0).any() and (np.diff(g, axis=1) < 0).any()
    assert (bits(ref["y"])[0] == M.NAN_PAYLOAD).sum() == 1      # the bypass channel passes the NaN's word
    assert ref["best"][0].max() == -1 and (ref["best"][2] >= 0).all()


@pytest.mark.parametrize("W,mt", [(1, 9), (3, 64), (16, 1)])
def test_any_cut_gives_the_same_bits(cpu, W, mt):
    nch, n = 3, 5 * W * B + 17
    sense, audio, words, masks, thr = case(nch, n, W, mt, False, False)
    ref = M.definition(sense, audio, words, masks, thr, W, 2, 1)
    rng = np.random.default_rng(5)
    cuts = [[1, B - 1, 1, B, 100], [W * B - 5, 10], [W * B, W * B], [B + 7] * 3]
    cuts.append(list(rng.integers(1, max(2, n // 6), 5)))
    for cut in cuts:
        cut = [int(v) for v in cut]
        cut.append(n - sum(cut))
        assert cut[-1] > 0
        cpu.setChannelToneDetector(words, masks, thr, W, 2, 1)
        y, sides = run_cut(cpu, sense, audio, cut)
        assert np.array_equal(bits(y), bits(ref["y"])), cut
        check_sides(ref, cut, sides, cut)
    # reset starts the same stream again
    cpu.resetChannelToneDetector()
    y, sides = run_cut(cpu, sense, audio, [n])
    assert np.array_equal(bits(y), bits(ref["y"]))
    check_sides(ref, [n], sides, "reset")
    # a channel alone equals the channel among others
    for c in range(nch):
        cpu.setChannelToneDetector(words, masks[c:c + 1], thr[c:c + 1], W, 2, 1)
        o = cpu.channel_tone(sense[c], audio[c])
        assert np.array_equal(bits(o["out"]), bits(ref["y"][c:c + 1])), c
        assert o["tone"][0] == sides[0]["tone"][c] and o["open"][0] == sides[0]["open"][c] and o["count"][0] == sides[0]["count"][c]
        assert np.array_equal(bits(o["level"][0]), bits(sides[0]["level"][c]))
        assert np.array_equal(bits(o["powers"][0]), bits(sides[0]["powers"][c]))


@pytest.mark.parametrize("W", WINDOWS)
def test_decisions_against_float64(W):
    """u or v may differ from the float64 evaluation only inside the header's derived band."""
    nch, n = 3, 24 * W * B
    tot = und = 0
    for mt, sense16 in ((1, False), (9, True), (64, False)):
        sense, _, words, masks, thr = case(nch, n, W, mt, sense16, False)
        m32 = M.definition(sense, None, words, masks, thr, W, 1, 0)
        m64 = M.definition(sense, None, words, masks, thr, W, 1, 0, dtype=np.float64)
        near = M.undecided(m64)
        assert ((m32["u"] == m64["u"]) | near).all() and ((m32["v"] == m64["v"]) | near).all()
        assert (m32["bad"] == m64["bad"]).all()
        tot += near.size
        und += int(near.sum())
        assert m64["u"].any() and (~m64["v"][1:] & ~m64["bad"][1:]).any()
    print(f"W={W}: {und} of {tot} windows inside the undecided band")
    assert und < tot // 10     # the band is narrow: the check above says something


@pytest.mark.parametrize("W", [1, 16])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -30, 2.0 ** 30])
def test_accuracy_against_float64(cpu, W, scale):
    """Every P_t, E and To * E of the CPU backend against float64, within tone_math.h's derived bounds."""
    nch, n = 3, 6 * W * B
    sense, _, words, masks, thr = case(nch, n, W, 64, False, False)
    sense = (sense * np.float32(scale)).astype(np.float32)     # exact: a power of two
    sense = np.where(np.isfinite(sense), sense, np.float32(0))
    thr = thr.copy()
    thr[:, 2] = 0
    m64 = M.definition(sense, None, words, masks, thr, W, 1, 0, dtype=np.float64)
    cpu.setChannelToneDetector(words, masks, thr, W, 1, 0)
    worst_p = worst_e = 0.0
    for j in range(n // (W * B)):
        o = cpu.channel_tone(sense[:, j * W * B:(j + 1) * W * B])
        P, P64 = o["powers"].astype(np.float64), m64["P"][:, j, :]
        X, E64 = m64["X"][:, j], m64["E"][:, j]
        bp = M.bound_p(P64, X[:, None], W)
        assert (np.abs(P - P64) <= bp).all(), j
        E = o["level"][:, 1].astype(np.float64)
        assert (np.abs(E - E64) <= 1.01 * (W + 8) * M.U * E64).all(), j
        To = m64["T"][:, 0].astype(np.float64)
        te = (m64["T"][:, 0] * o["level"][:, 1]).astype(np.float64)       # the float32 product the decision uses
        assert (np.abs(te - To * E64) <= M.bound_te(To, E64, W)).all(), j
        nz = bp > 0
        worst_p = max(worst_p, float((np.abs(P - P64)[nz] / bp[nz]).max()))
        worst_e = max(worst_e, float((np.abs(te - To * E64) / np.maximum(M.bound_te(To, E64, W), 1e-300)).max()))
    print(f"W={W} scale={scale:g}: worst |P - P64| / bound {worst_p:.3f}, worst |To E - (To E)64| / bound {worst_e:.3f}")


@pytest.mark.parametrize("W", [3, 16])
def test_stream_next_to_the_phase_wrap(cpu, W):
    """A stream whose block rotation w_t * (uint32)(256 k) crosses 2^32: set_position, then the model's bits."""
    WB = W * B
    pos0 = (2 ** 32 // WB - 2) * WB
    nch, n = 3, 4 * WB + 17
    sense, audio, words, masks, thr = case(nch, n, W, 64, False, False)
    ref = M.definition(sense, audio, words, masks, thr, W, 1, 0, pos0=pos0)
    ref0 = M.definition(sense, audio, words, masks, thr, W, 1, 0)
    assert not np.array_equal(bits(ref["P"]), bits(ref0["P"]))          # the position is in the bits
    f = load().sddc_ddc_internal_chtone_set_position
    assert f(cpu._h, pos0) == ERR_STATE
    cpu.setChannelToneDetector(words, masks, thr, W, 1, 0)
    assert f(cpu._h, pos0 + B) == (ERR_ARG if W > 1 else 0)
    assert f(cpu._h, pos0) == 0
    for cut in ([n], [WB + 5, WB, n - 2 * WB - 5]):
        assert f(cpu._h, pos0) == 0
        y, sides = run_cut(cpu, sense, audio, cut)
        assert np.array_equal(bits(y), bits(ref["y"])), cut
        a = 0
        for ln, o in zip(cut, sides):
            a += ln
            assert np.array_equal(bits(o["powers"]), bits(M.powers_at(ref, a)))
            assert np.array_equal(bits(o["level"]), bits(M.level_at(ref, a)))
            assert np.array_equal(o["tone"], M.tone_at(ref, a))
        cpu.resetChannelToneDetector()


def test_ctcss_function(cpu):
    """Each of the 50 CTCSS tones in turn at amplitude 0.1 in white noise at 6 dB SNR, three windows each and
    a window of noise alone after it, fs = 12000, W = 16, rho_open = 0.2, rho_close = 0.1: d_tone names the
    right tone in every window and -1 on noise.  No miss is allowed."""
    fs, W, amp = 12000.0, 16, 0.1
    WB = W * B
    sigma = np.sqrt(amp * amp / 2.0 / 10.0 ** 0.6)
    rng = np.random.default_rng(2026)
    nt = len(CTCSS_TONES)
    assert nt == 50 and CTCSS_TONES[0] == 67.0 and CTCSS_TONES[-1] == 254.1 and CTCSS_TONES[12] == 100.0
    assert tone_window(0.34, fs) == 16 and tone_word(3000.0, fs) == 2 ** 30
    words = np.array([tone_word(f, fs) for f in CTCSS_TONES], np.uint32)
    x = sigma * rng.standard_normal(nt * 4 * WB)
    t = np.arange(3 * WB)
    for k, f in enumerate(CTCSS_TONES):
        x[k * 4 * WB:k * 4 * WB + 3 * WB] += amp * np.cos(2 * np.pi * f / fs * (t + k * 4 * WB) + 0.7 * k)
    x = x.astype(np.float32)[None, :]
    masks = np.array([(1 << nt) - 1], np.uint64)
    thr = np.array([[0.2, 0.1, 0.0]], np.float32)
    cpu.setChannelToneDetector(words, masks, thr, W, 1, 0)
    wrong, ratio, rho_min, rho_noise = 0, np.inf, np.inf, 0.0
    for j in range(nt * 4):
        o = cpu.channel_tone(x[:, j * WB:(j + 1) * WB])
        want = j // 4 if j % 4 < 3 else -1
        wrong += int(o["tone"][0] != want)
        P = np.sort(o["powers"][0].astype(np.float64))
        rho = float(o["level"][0, 0]) / (WB * float(o["level"][0, 1]))
        if want >= 0:
            ratio, rho_min = min(ratio, P[-1] / P[-2]), min(rho_min, rho)
            assert int(np.argmax(o["powers"][0])) == want
        else:
            rho_noise = max(rho_noise, rho)
    print(f"wrong {wrong} of {nt * 4}; best / runner-up >= {ratio:.1f}; P / (256 W E) >= {rho_min:.3f} on tones, "
          f"<= {rho_noise:.4f} on noise")
    assert wrong == 0


def test_gate_timing(cpu):
    """The gate opens A windows after the tone starts and closes more than H windows after it ends; the gate after
    window j applies to window j + 1."""
    fs, W, A, H = 12000.0, 3, 2, 1
    WB = W * B
    rng = np.random.default_rng(3)
    nw, t0, t1 = 14, 2, 7                       # the tone fills windows t0 .. t1 - 1
    x = 0.03 * rng.standard_normal(nw * WB)
    t = np.arange(t0 * WB, t1 * WB)
    x[t0 * WB:t1 * WB] += 0.1 * np.cos(2 * np.pi * 100.0 / fs * t)
    audio = np.ones((1, nw * WB), np.float32)
    cpu.setChannelToneDetector([tone_word(100.0, fs)], np.array([1], np.uint64), np.array([[0.2, 0.1, 0.0]], np.float32), W, A, H)
    o = cpu.channel_tone(x.astype(np.float32), audio)
    open_windows = o["out"].reshape(nw, WB)
    assert all((w == w[0]).all() for w in open_windows)                   # a window is open or closed as a whole
    got = [int(w[0]) for w in open_windows]
    want = [1 if t0 + A <= j < t1 + H + 1 else 0 for j in range(nw)]
    assert got == want, (got, want)
    assert o["count"][0] == sum(want) * WB and o["open"][0] == 0 and o["tone"][0] == -1


def test_tone_window_validity():
    assert tone_window(0.0, 12000.0) == 1 and tone_window(256 * 256 / 12000.0, 12000.0) == 256
    for sec, fs in ((-1.0, 8000.0), (257 * 256 / 8000.0, 8000.0), (float("nan"), 8000.0), (1.0, 0.0), (1.0, float("inf"))):
        with pytest.raises(DDCError) as e:
            tone_window(sec, fs)
        assert e.value.code == ERR_ARG
    assert load().sddc_ddc_tone_window(1.0, 8000.0, None) == ERR_ARG


def test_set_call_validity(cpu):
    f = cpu._L.sddc_ddc_set_channel_tone_detector
    assert cpu._L.sddc_ddc_channel_tone_reset(cpu._h) == ERR_STATE          # nothing set
    with pytest.raises(DDCError) as ex:
        cpu.channel_tone(np.zeros((1, 4), np.float32))
    assert ex.value.code == ERR_STATE
    nch, nt = 3, 9
    words = M.table(nt)[0]
    masks = np.array([0, 1 << 8, (1 << nt) - 1], np.uint64)
    thr = np.tile(np.float32([0.2, 0.1, 1e-6]), (nch, 1))
    ok = (16, 1, 0, 0, 0, 0)                                                   # W, A, H, formats

    def call(w=words, n=nt, m=masks, t=thr, c=nch, rest=ok):
        return f(cpu._h, w.ctypes.data, n, m.ctypes.data, t.ctypes.data, c, *rest)

    assert call() == 0
    bad_m = masks.copy()
    bad_m[1] = 1 << nt                                                         # a bit at ntones
    assert call(m=bad_m) == ERR_ARG
    bad_m[1] = 1 << 63
    assert call(m=bad_m) == ERR_ARG
    for col, vals in ((0, (0.0, -0.1, 1.5, np.nan, 0.05)), (1, (0.0, -0.1, 0.3, np.nan)), (2, (-1e-6, np.nan, np.inf, 3e38))):
        for v in vals:                                                         # 0.05 / 0.3: rho_close > rho_open
            t = thr.copy()
            t[2, col] = v
            assert call(t=t) == ERR_ARG, (col, v)
    for rest in ((0, 1, 0, 0, 0, 0), (257, 1, 0, 0, 0, 0), (16, 0, 0, 0, 0, 0), (16, 256, 0, 0, 0, 0), (16, 1, -1, 0, 0, 0),
                 (16, 1, 65536, 0, 0, 0), (16, 1, 0, 2, 0, 0), (16, 1, 0, 0, -1, 0), (16, 1, 0, 0, 0, 2)):
        assert call(rest=rest) == ERR_ARG, rest
    for rest in ((1, 1, 0, 0, 0, 0), (256, 255, 65535, 1, 1, 1)):
        assert call(rest=rest) == 0, rest
    assert call(n=0) == ERR_ARG and call(n=65) == ERR_ARG and call(c=-1) == ERR_ARG
    big_m, big_t = np.ones(1025, np.uint64), np.tile(np.float32([0.2, 0.1, 0.0]), (1025, 1))
    assert call(m=big_m, t=big_t, c=1025) == ERR_ARG
    with pytest.raises(DDCError):
        cpu.setChannelToneDetector(words, masks, np.zeros((3, 2), np.float32))
    # a failed set call sets nothing; a set call with no words turns the stage off
    cpu.setChannelToneDetector(words, masks, thr, 16)
    assert call(rest=(0, 1, 0, 0, 0, 0)) == ERR_ARG
    assert cpu.channel_tone(np.zeros((nch, 4), np.float32))["open"].tolist() == [1, 0, 0]
    cpu.setChannelToneDetector(None, None, None)
    assert cpu._L.sddc_ddc_channel_tone_reset(cpu._h) == ERR_STATE
    full = np.array([(1 << 64) - 1], np.uint64)                               # 64 tones: every bit is a tone
    assert f(cpu._h, M.table(64)[0].ctypes.data, 64, full.ctypes.data, thr.ctypes.data, 1, *ok) == 0


def test_call_validity(cpu):
    f = cpu._L.sddc_ddc_channel_tone_host
    nch, n = 3, 2 * B
    s = np.zeros((nch, n), np.float32)
    a = np.zeros((nch, 2 * n), np.float32)
    out = np.zeros((nch, n), np.float32)
    side = np.zeros(nch * (5 + 9), np.uint32)          # tone, open, count, level [nch][2], powers [nch][9]
    sp, ap, op = s.ctypes.data, a.ctypes.data, out.ctypes.data
    assert f(cpu._h, sp, n, ap, nch, n, 2 * n, op, n, None, None, None, None, None) == ERR_STATE     # nothing set
    words = M.table(9)[0]
    cpu.setChannelToneDetector(words, np.array([0, 1, 511], np.uint64), np.tile(np.float32([0.2, 0.1, 0.0]), (nch, 1)), 2)
    d = side.ctypes.data
    assert f(cpu._h, sp, n, ap, nch, n, 2 * n, op, n, d, d + 4 * nch, d + 8 * nch, d + 12 * nch, d + 20 * nch) == 0
    assert f(cpu._h, sp, n, None, nch, n, 0, None, 0, None, None, None, None, None) == 0            # detect only
    assert f(cpu._h, sp, n, ap, 2, n, 2 * n, op, n, None, None, None, None, None) == ERR_STATE      # another nch
    assert f(cpu._h, sp, n, None, nch, n, 0, op, n, None, None, None, None, None) == ERR_ARG        # d_out without d_audio
    assert f(cpu._h, sp, n, ap, nch, n, 2 * n, None, n, None, None, None, None, None) == ERR_ARG    # audio without d_out
    assert f(cpu._h, None, n, ap, nch, n, 2 * n, op, n, None, None, None, None, None) == ERR_ARG
    assert f(cpu._h, sp, n, ap, nch, 0, 2 * n, op, n, None, None, None, None, None) == ERR_ARG
    assert f(cpu._h, sp, 1 << 42, ap, nch, (1 << 40) + 1, 1 << 42, op, 1 << 42, None, None, None, None, None) == ERR_ARG
    for strides in ((n - 1, 2 * n, n), (n, n - 1, n), (n, 2 * n, n - 1)):                            # strides below the streams
        assert f(cpu._h, sp, strides[0], ap, nch, n, strides[1], op, strides[2], None, None, None, None, None) == ERR_ARG
    assert f(cpu._h, sp + 2, n, ap, nch, n - 1, 2 * n, op, n, None, None, None, None, None) == ERR_ARG   # misaligned
    assert f(cpu._h, sp, n, ap, nch, n, 2 * n, op, n, d + 2, None, None, None, None) == ERR_ARG
    # overlapping buffers: the output on the audio, and the output on the sense stream
    assert f(cpu._h, sp, n, ap, nch, n, 2 * n, ap + 4 * n, 2 * n, None, None, None, None, None) == ERR_ARG
    assert f(cpu._h, sp, n, ap, nch, n, 2 * n, sp + 4 * (n - 1), n, None, None, None, None, None) == ERR_ARG
    # a failed call changes no state: the stream is still at 2 n samples of zeros
    o = cpu.channel_tone(s)
    assert o["count"].tolist() == [n, 0, 0]
