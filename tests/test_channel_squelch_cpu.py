"""The channel squelch without a GPU: the CPU backend (sddc_ddc_channel_squelch_host of a CPU handle) against
the numpy float32 transcription of the definition bit for bit, outputs, open, count and level, for any cut
(tools/channel_squelch_model.py); its gates against the float64 evaluation; what passes and what is closed;
and the error returns.

The generator keeps noise and bursts 40 dB apart and the thresholds at least 18 dB from either, so the
float64 evaluation must put no block inside the header's undecided band |p - T| <= 1.01 * 11 * 2^-24 * T (3
roundings in q, 8 tree levels): the count is asserted to be 0 for every case used here and in
tests/test_gpu_channel_squelch.py, because one undecided block changes every gate after it.  Nothing here is
fitted to the code under test.
"""
from __future__ import annotations

import functools
import importlib.util
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load("channel_squelch_model")

from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, DEVICE_CPU, SQUELCH_BLOCK, SQUELCH_LEVEL, SQUELCH_MUTE,  # noqa: E402
                            SQUELCH_NOISE, SQUELCH_OFF, SQUELCH_SENSE_CF32, SQUELCH_SENSE_CS16, SQUELCH_SENSE_F32,
                            SQUELCH_SENSE_S16, SQUELCH_SENSE_SELF, DDCError, R2iq, squelch_blocks)
from extio_sddc_amd._lib import load  # noqa: E402

B = SQUELCH_BLOCK
ERR_ARG, ERR_STATE = -1, -4
SHAPES = [(1, 1), (1, B), (1, 3 * B + 17), (3, 2 * B + 3), (1024, 2), (1, 66 * B + 5), (2, 258 * B + 1)]
CONFIGS = [(1, 0, 0), (3, 2, 1), (16, 70, 1), (1, 65535, 0)]   # (A, H, fade)
KINDS = [SQUELCH_SENSE_SELF, SQUELCH_SENSE_F32, SQUELCH_SENSE_S16, SQUELCH_SENSE_CF32, SQUELCH_SENSE_CS16]
FORMATS = [AUDIO_F32, AUDIO_S16]
NAN_PAYLOAD = M.NAN_PAYLOAD


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def case(nch, n, A, H, kind, in16, single=SQUELCH_LEVEL):
    audio, sense, modes, thr = M.make_case(nch, n, A, H, kind, in16, single)
    for a in (audio, sense, modes, thr):
        if a is not None:
            a.setflags(write=False)
    return audio, sense, modes, thr


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def cuts_of(n):
    """The issue's cuts [1, B - 1, 1, B, rest] and [100, B, rest], shortened to the stream."""
    res = []
    for c in ([1, B - 1, 1, B], [100, B]):
        acc, cut = 0, []
        for v in c:
            if acc + v >= n:
                break
            cut.append(v)
            acc += v
        cut.append(n - acc)
        res.append(cut)
    return res


def run_cut(r, audio, sense, cut):
    """The stream through channel_squelch in calls of the cut's lengths: outputs and per-call side outputs."""
    ys, sides, a = [], [], 0
    for ln in cut:
        s = None if sense is None else sense[:, a:a + ln]
        y, o, c, lv = r.channel_squelch(audio[:, a:a + ln], s, open=True, count=True, level=True)
        ys.append(y)
        sides.append((o, c, lv))
        a += ln
    return np.concatenate(ys, axis=1), sides


def check_against_model(r, audio, sense, modes, thr, A, H, fade, kind, fin, fout, cuts):
    ref = M.definition(audio, sense, kind, modes, thr, A, H, fade, fout)
    for cut in cuts:
        r.setChannelSquelch(modes, thr, A, H, fade, kind, fin, fout)
        y, sides = run_cut(r, audio, sense, cut)
        what = (A, H, fade, kind, fin, fout, cut[:4])
        assert y.dtype == ref["y"].dtype
        assert np.array_equal(bits(y), bits(ref["y"])), what
        a = 0
        for ln, (o, c, lv) in zip(cut, sides):
            assert np.array_equal(o, M.open_at(ref, a + ln)), (what, a)
            assert np.array_equal(c, M.count(ref, a, a + ln)), (what, a)
            assert np.array_equal(bits(lv), bits(M.level_at(ref, a + ln))), (what, a)
            a += ln
        assert a == audio.shape[1]
    return ref


@pytest.mark.parametrize("in16", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_generator_leaves_no_block_undecided_and_moves_the_gates(kind, in16):
    """For every case of this file and of the GPU file: no block in the undecided band of the float64
    evaluation, and at least one opening and one closing where the stream is long enough."""
    for (nch, n), (A, H, fade) in itertools.product(SHAPES, CONFIGS):
        for single in (SQUELCH_LEVEL, SQUELCH_NOISE) if nch == 1 else (SQUELCH_LEVEL,):
            audio, sense, modes, thr = case(nch, n, A, H, kind, in16, single)
            assert M.undecided(audio, sense, kind, modes, thr) == 0, (nch, n, A, H, single)
            if n >= (A + H + 6) * B:
                ref = M.definition(audio, sense, kind, modes, thr, A, H, fade)
                up, down = M.transitions(ref)
                assert up >= 1 and down >= 1, (nch, n, A, H, single, up, down)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cpu_backend_equals_model_bit_for_bit(cpu, shape, kind):
    """Every sense kind x F32 / S16 in x F32 / S16 out, the four modes mixed in one call (nch > 1), fade 0
    and 1, and the cuts."""
    nch, n = shape
    for (A, H, fade), fin, fout in itertools.product(CONFIGS, FORMATS, FORMATS):
        audio, sense, modes, thr = case(nch, n, A, H, kind, fin == AUDIO_S16)
        cuts = [[n]] + (cuts_of(n) if n <= 66 * B + 5 else [])
        ref = check_against_model(cpu, audio, sense, modes, thr, A, H, fade, kind, fin, fout, cuts)
        if nch > 1:
            assert ref["G"][modes == SQUELCH_OFF].all() and not ref["G"][modes == SQUELCH_MUTE].any()


@pytest.mark.parametrize("single", [SQUELCH_LEVEL, SQUELCH_NOISE])
def test_a_single_noise_or_level_channel_and_the_other_fade(cpu, single):
    n = 66 * B + 5
    for (A, H, fade), kind in itertools.product(CONFIGS, (SQUELCH_SENSE_SELF, SQUELCH_SENSE_CF32)):
        audio, sense, modes, thr = case(1, n, A, H, kind, False, single)
        check_against_model(cpu, audio, sense, modes, thr, A, H, 1 - fade, kind, AUDIO_F32, AUDIO_F32, [[n], [100, B, n - B - 100]])


@pytest.mark.parametrize("kind", KINDS)
def test_gates_equal_the_float64_evaluation(kind):
    for (nch, n), (A, H, fade) in itertools.product(SHAPES[2:], CONFIGS):
        audio, sense, modes, thr = case(nch, n, A, H, kind, False)
        r32 = M.definition(audio, sense, kind, modes, thr, A, H, fade)
        r64 = M.definition(audio, sense, kind, modes, thr, A, H, fade, dtype=np.float64)
        for key in ("G", "kind", "u", "v", "bad", "open_after"):
            assert np.array_equal(r32[key], r64[key]), (key, nch, n, A, H)
        assert np.array_equal(bits(r32["y"]), bits(r64["y"]))


def test_single_samples_across_a_transition(cpu):
    """A call per sample from the block before an opening to the block after it, and the same for a closing,
    gives the bits of one call."""
    nch, n, (A, H, fade) = 3, 30 * B + 3, (3, 2, 1)
    kind = SQUELCH_SENSE_F32
    audio, sense, modes, thr = case(nch, n, A, H, kind, False)
    ref = M.definition(audio, sense, kind, modes, thr, A, H, fade)
    d = np.diff(ref["G"][0].astype(int))
    k_up, k_down = int(np.flatnonzero(d > 0)[0]) + 1, int(np.flatnonzero(d < 0)[0]) + 1
    for k in (k_up, k_down):
        a, b = (k - 1) * B - 3, (k + 1) * B + 3
        cut = [a] + [1] * (b - a) + [n - b]
        check_against_model(cpu, audio, sense, modes, thr, A, H, fade, kind, AUDIO_F32, AUDIO_F32, [cut])


def test_open_samples_pass_bit_for_bit_and_closed_ones_are_plus_zero(cpu):
    n, (A, H) = 40 * B, (2, 1)
    kind = SQUELCH_SENSE_F32
    _, sense, modes, thr = case(1, n, A, H, kind, False)
    rng = np.random.default_rng(5)
    audio = -np.abs(rng.standard_normal((1, n))).astype(np.float32) - np.float32(0.5)   # every sample negative
    ref = M.definition(audio, sense, kind, modes, thr, A, H, 0)
    g = np.repeat(ref["G"], B, axis=1)[:, :n]
    assert g.any() and not g.all()
    w = audio.view(np.uint32).copy()
    i_open = int(np.flatnonzero(g[0])[7])
    w[0, i_open] = NAN_PAYLOAD | 0x80000000          # a signalling-free NaN with a payload and a sign
    audio = w.view(np.float32)
    for fade in (0, 1):
        cpu.setChannelSquelch(modes, thr, A, H, fade, kind, AUDIO_F32, AUDIO_F32)
        y = cpu.channel_squelch(audio, sense, open=False)
        kinds = np.repeat(ref["kind"] if fade == 0 else M.definition(audio, sense, kind, modes, thr, A, H, 1)["kind"], B, axis=1)[:, :n]
        assert np.array_equal(bits(y)[kinds == 1], w[kinds == 1])
        assert bits(y)[0, i_open] == NAN_PAYLOAD | 0x80000000
        assert (bits(y)[kinds == 0] == 0).all()      # +0: no sign bit although every input is negative
        assert (kinds == 0).any()
        cpu.setChannelSquelch(modes, thr, A, H, fade, kind, AUDIO_F32, AUDIO_S16)
        y16 = cpu.channel_squelch(audio, sense, open=False)
        assert (y16[kinds == 0] == 0).all() and y16[0, i_open] == 0
    # every int16 code through an open gate (OFF, and a LEVEL channel held open by its hang), S16 and F32 out
    codes = np.arange(-32768, 32768, dtype=np.int16)[None, :]
    hold = np.concatenate([np.full((1, 2 * B), 20000, np.int16), codes], axis=1)
    for fout in FORMATS:
        cpu.setChannelSquelch([SQUELCH_OFF], np.zeros((1, 2), np.float32), 1, 0, 1, SQUELCH_SENSE_SELF, AUDIO_S16, fout)
        y = cpu.channel_squelch(codes, open=False)
        assert np.array_equal(y, codes.astype(y.dtype))
        cpu.setChannelSquelch([SQUELCH_LEVEL], np.float32([[1e6, 1e6]]), 1, 65535, 0, SQUELCH_SENSE_SELF, AUDIO_S16, fout)
        y, o, c = cpu.channel_squelch(hold, open=True, count=True)
        assert np.array_equal(y[:, 2 * B:], codes.astype(y.dtype)) and o[0] == 1 and c[0] == 65536 + B


def test_nan_and_inf_sense_samples_mark_their_block_bad(cpu):
    n, A, H = 12 * B, 1, 0
    x = np.full((1, n), 0.5, np.float32)
    thr = np.float32([[0.01, 0.01]])
    x[0, 5 * B + 9] = np.nan
    x[0, 8 * B + 200] = np.inf
    cpu.setChannelSquelch([SQUELCH_LEVEL], thr, A, H, 0, SQUELCH_SENSE_SELF)
    y, o, c, lv = cpu.channel_squelch(x, open=True, count=True, level=True)
    ref = M.definition(x, None, M.SELF, [SQUELCH_LEVEL], thr, A, H, 0)
    assert np.array_equal(bits(y), bits(ref["y"]))
    expect = np.ones(12, bool)
    expect[[0, 6, 9]] = False            # the stream's first block, and the block after each bad one
    assert np.array_equal(ref["G"][0], expect)
    assert c[0] == 9 * B and o[0] == 1 and lv[0] == np.float32(64.0)
    assert np.isnan(y[0, 5 * B + 9]) and np.isinf(y[0, 8 * B + 200])   # open samples pass as they are


def test_level_runs_in_off_and_mute_and_calibrates_thresholds(cpu):
    rng = np.random.default_rng(3)
    n = 4 * B + 10
    x = (0.25 * rng.standard_normal((2, n))).astype(np.float32)
    cpu.setChannelSquelch([SQUELCH_OFF, SQUELCH_MUTE], np.zeros((2, 2), np.float32), 1, 0, 0, SQUELCH_SENSE_SELF)
    y, o, c, lv = cpu.channel_squelch(x, open=True, count=True, level=True)
    assert np.array_equal(bits(y[0]), bits(x[0])) and (bits(y[1]) == 0).all()
    assert list(o) == [1, 0] and list(c) == [n, 0]
    ms = (x[:, 3 * B:4 * B].astype(np.float64) ** 2).mean(axis=1)
    assert np.allclose(lv / 256.0, ms, rtol=1e-5)


def test_squelch_blocks():
    assert squelch_blocks(0.0, 12000.0) == 0
    assert squelch_blocks(0.5, 12000.0) == 23                  # 23.4
    assert squelch_blocks(1.0, 48000.0) == 188                 # 187.5 rounds to even
    assert squelch_blocks(65535 * 256 / 8000.0, 8000.0) == 65535
    for sec, fs in ((-1.0, 8000.0), (65536 * 256 / 8000.0, 8000.0), (float("nan"), 8000.0), (1.0, 0.0), (1.0, float("inf"))):
        with pytest.raises(DDCError) as e:
            squelch_blocks(sec, fs)
        assert e.value.code == ERR_ARG
    assert load().sddc_ddc_squelch_blocks(1.0, 8000.0, None) == ERR_ARG


def test_set_call_validity(cpu):
    f = cpu._L.sddc_ddc_set_channel_squelch
    assert cpu._L.sddc_ddc_channel_squelch_reset(cpu._h) == ERR_STATE       # nothing set
    nch = 4
    modes = np.array([SQUELCH_LEVEL, SQUELCH_NOISE, SQUELCH_OFF, SQUELCH_MUTE], np.int32)
    thr = M.thresholds_for(modes)
    ok = (3, 2, 1, SQUELCH_SENSE_SELF, AUDIO_F32, AUDIO_F32)
    assert f(cpu._h, modes.ctypes.data, thr.ctypes.data, nch, *ok) == 0
    for ch, col, vals in ((0, 0, (np.nan, np.inf, -1e-30, 2.0 ** 81)), (1, 1, (np.nan, np.inf, -1.0, 2.0 ** 81)),
                          (2, 0, (np.nan, -1.0)), (3, 1, (np.inf,))):
        for v in vals:
            t = thr.copy()
            t[ch, col] = v
            assert f(cpu._h, modes.ctypes.data, t.ctypes.data, nch, *ok) == ERR_ARG, (ch, col, v)
    t = thr.copy()
    t[0] = t[0, ::-1]                    # LEVEL with T_close > T_open
    assert f(cpu._h, modes.ctypes.data, t.ctypes.data, nch, *ok) == ERR_ARG
    t = thr.copy()
    t[1] = t[1, ::-1]                    # NOISE with T_close < T_open
    assert f(cpu._h, modes.ctypes.data, t.ctypes.data, nch, *ok) == ERR_ARG
    t = thr.copy()
    t[0] = t[1] = (2.0 ** 80, 2.0 ** 80)     # equal thresholds and the upper edge are legal; OFF / MUTE: any order
    t[2] = t[2, ::-1]
    assert f(cpu._h, modes.ctypes.data, t.ctypes.data, nch, *ok) == 0
    for m in (-1, 4):
        md = modes.copy()
        md[3] = m
        assert f(cpu._h, md.ctypes.data, thr.ctypes.data, nch, *ok) == ERR_ARG
    for bad in ((0, 2, 1, 0, 0, 0), (256, 2, 1, 0, 0, 0), (3, -1, 1, 0, 0, 0), (3, 65536, 1, 0, 0, 0), (3, 2, 2, 0, 0, 0),
                (3, 2, -1, 0, 0, 0), (3, 2, 1, -1, 0, 0), (3, 2, 1, 5, 0, 0), (3, 2, 1, 0, 2, 0), (3, 2, 1, 0, 0, -1)):
        assert f(cpu._h, modes.ctypes.data, thr.ctypes.data, nch, *bad) == ERR_ARG, bad
    for edge in ((1, 0, 0, 0, 0, 0), (255, 65535, 1, 4, 1, 1)):
        assert f(cpu._h, modes.ctypes.data, thr.ctypes.data, nch, *edge) == 0
    assert f(cpu._h, modes.ctypes.data, thr.ctypes.data, -1, *ok) == ERR_ARG
    big_m, big_t = np.full(1025, SQUELCH_LEVEL, np.int32), np.tile(np.float32([1.0, 0.5]), (1025, 1))
    assert f(cpu._h, big_m.ctypes.data, big_t.ctypes.data, 1025, *ok) == ERR_ARG
    assert f(cpu._h, big_m.ctypes.data, big_t.ctypes.data, 1024, *ok) == 0
    with pytest.raises(DDCError):
        cpu.setChannelSquelch(modes, np.zeros((3, 2), np.float32))
    # a failed set call sets nothing: the 1024 channels stay
    assert f(cpu._h, modes.ctypes.data, thr.ctypes.data, nch, 0, 2, 1, 0, 0, 0) == ERR_ARG
    x = np.zeros((1024, 4), np.float32)
    out = np.empty_like(x)
    assert cpu._L.sddc_ddc_channel_squelch_host(cpu._h, x.ctypes.data, None, 1024, 4, 4, 0, out.ctypes.data, 4, None, None, None) == 0


def test_call_errors_failed_calls_reset_and_the_off_switch(cpu):
    f = cpu._L.sddc_ddc_channel_squelch_host
    nch, n = 3, 40
    x = np.zeros((nch, n), np.float32)
    sn = np.zeros((nch, n), np.complex64)
    out = np.empty_like(x)
    side = np.empty(nch, np.uint32)
    xp, sp, op = x.ctypes.data, sn.ctypes.data, out.ctypes.data
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n, op, n, None, None, None) == ERR_STATE        # nothing set
    with pytest.raises(DDCError) as ex:
        cpu.channel_squelch(x)
    assert ex.value.code == ERR_STATE
    modes = M.modes_for(nch)
    thr = M.thresholds_for(modes)
    cpu.setChannelSquelch(modes, thr, 2, 1, 1, SQUELCH_SENSE_CF32)
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n, op, n, side.ctypes.data, None, None) == 0
    assert f(cpu._h, xp, sp, 2, n, n, 2 * n, op, n, None, None, None) == ERR_STATE          # another nch
    assert f(cpu._h, xp, sp, nch, 0, n, 2 * n, op, n, None, None, None) == ERR_ARG
    assert f(cpu._h, xp, sp, nch, (1 << 40) + 1, 1 << 42, 1 << 43, op, 1 << 42, None, None, None) == ERR_ARG
    assert f(cpu._h, xp, sp, nch, n, n - 1, 2 * n, op, n, None, None, None) == ERR_ARG      # strides below the streams
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n - 2, op, n, None, None, None) == ERR_ARG
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n, op, n - 1, None, None, None) == ERR_ARG
    assert f(cpu._h, xp, sp, nch, n - 1, n, 2 * n - 1, op, n, None, None, None) == ERR_ARG  # odd complex stride
    assert f(cpu._h, None, sp, nch, n, n, 2 * n, op, n, None, None, None) == ERR_ARG
    assert f(cpu._h, xp, None, nch, n, n, 2 * n, op, n, None, None, None) == ERR_ARG        # no sense with CF32
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n, None, n, None, None, None) == ERR_ARG
    assert f(cpu._h, xp + 2, sp, nch, n - 1, n, 2 * n, op, n, None, None, None) == ERR_ARG  # half a sample
    assert f(cpu._h, xp, sp + 4, nch, n - 1, n, 2 * n, op, n, None, None, None) == ERR_ARG  # half a complex sample
    assert f(cpu._h, xp, sp, nch, n - 1, n, 2 * n, op + 2, n, None, None, None) == ERR_ARG
    for k in range(3):
        s = [None, None, None]
        s[k] = side.ctypes.data + 2
        assert f(cpu._h, xp, sp, nch, n, n, 2 * n, op, n, *s) == ERR_ARG
    # overlap: in place, the output on the sense stream, the output starting inside the input's last stream
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n, xp, n, None, None, None) == ERR_ARG
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n, sp, n, None, None, None) == ERR_ARG
    both = np.zeros(2 * nch * n, np.float32)
    last = both.ctypes.data + 4 * (nch * n - 1)
    assert f(cpu._h, both.ctypes.data, sp, nch, n, n, 2 * n, last, n, None, None, None) == ERR_ARG
    assert f(cpu._h, both.ctypes.data, sp, nch, n, n, 2 * n, last + 4, n, None, None, None) == 0   # adjacent is legal
    assert cpu._L.sddc_ddc_channel_squelch_device(cpu._h, xp, sp, nch, n, n, 2 * n, op, n, None, None, None, None) == ERR_STATE
    # SELF ignores the sense pointer
    cpu.setChannelSquelch(modes, thr, 2, 1, 1, SQUELCH_SENSE_SELF)
    assert f(cpu._h, xp, None, nch, n, n, 0, op, n, None, None, None) == 0
    # a failed call changes no state: the stream goes on as if it had not happened
    A, H, fade, kind = 2, 1, 1, SQUELCH_SENSE_CF32
    nl = 20 * B + 7
    audio, sense, modes, thr = case(nch, nl, A, H, kind, False)
    ref = M.definition(audio, sense, kind, modes, thr, A, H, fade)
    assert M.transitions(ref)[0] >= 1
    cpu.setChannelSquelch(modes, thr, A, H, fade, kind)
    y1 = cpu.channel_squelch(audio[:, :1300], sense[:, :1300], open=False)
    assert f(cpu._h, xp, sp, nch, 0, n, 2 * n, op, n, None, None, None) == ERR_ARG
    assert f(cpu._h, xp, None, nch, n, n, 2 * n, op, n, None, None, None) == ERR_ARG
    y2, o, c = cpu.channel_squelch(audio[:, 1300:], sense[:, 1300:], open=True, count=True)
    assert np.array_equal(bits(np.concatenate([y1, y2], axis=1)), bits(ref["y"]))
    assert np.array_equal(o, M.open_at(ref, nl)) and np.array_equal(c, M.count(ref, 1300, nl))
    # reset starts a closed stream: the same bits again, although the stream ended with open channels
    cpu.resetChannelSquelch()
    y, o = cpu.channel_squelch(audio, sense)
    assert np.array_equal(bits(y), bits(ref["y"]))
    assert (bits(y[0, :B]) == 0).all()
    # the off switch
    cpu.setChannelSquelch(None, None)
    assert f(cpu._h, xp, sp, nch, n, n, 2 * n, op, n, None, None, None) == ERR_STATE
    assert cpu._L.sddc_ddc_channel_squelch_reset(cpu._h) == ERR_STATE
    assert cpu._L.sddc_ddc_set_channel_squelch(cpu._h, modes.ctypes.data, thr.ctypes.data, 0, 0, 0, 0, 0, 0, 0) == 0
