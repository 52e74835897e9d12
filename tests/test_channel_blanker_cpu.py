"""The channel noise blanker without a GPU: the CPU backend (sddc_ddc_channel_blank_host of a CPU handle)
against the numpy float32 transcription of the definition bit for bit, outputs and counts, for any cut
(tools/channel_blanker_model.py); against the float64 evaluation outside a borderline set; that it does
its job on a stream with impulses; non-finite samples and zeros; and the error returns.

The borderline set is the header's: |q64 - t64| <= 1.01 (8 + M + 5) u t64 (three roundings of q, eight
tree levels, M - 1 additions and a multiply for the mean, thr's rounding and its multiply).  The power
bounds of the job test are the expected values 1 - 11 / 997 - 9 e^-10 = 0.989 (three samples and a guard
of 4 on each side every 997, and the noise's own exceedances with their guards) within [0.97, 1.0], and
3 * 900 / 997 / 0.1 + 1 = 28 against the required 20.  Nothing here is fitted to the code under test.
"""
from __future__ import annotations

import ctypes
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


M = _load("channel_blanker_model")

from extio_sddc_amd import BLANKER_BLOCK, BLANKER_MEAN, BLANKER_MEDIAN, DEVICE_CPU, DDCError, R2iq, blanker_threshold  # noqa: E402
from extio_sddc_amd.r2iq import FMT_CF32, FMT_CS16  # noqa: E402
from extio_sddc_amd._lib import load  # noqa: E402

B = BLANKER_BLOCK
U = 2.0 ** -24
ERR_ARG, ERR_STATE = -1, -4
SHAPES = [(1, 1), (1, B), (1, 3 * B + 17), (3, 2 * B + 3), (1024, 2), (1, 66 * B + 5), (2, 258 * B + 1)]
REFS = [1, 3, 8, 16]
GUARDS = [0, 1, 5, 64]
MODES = [BLANKER_MEAN, BLANKER_MEDIAN]
FORMATS = [FMT_CF32, FMT_CS16]
NAN_PAYLOAD = 0x7FC12345


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def signal(nch, n, g, fmt):
    """make_input's stream; in CF32 the bypassed channel 1 carries NaNs with a payload."""
    x, pos = M.make_input(nch, n, g)
    if fmt == FMT_CS16:
        x = M.to_cs16(x)
    elif nch > 1 and n > 1:
        w = x.view(np.uint32).reshape(nch, n, 2)
        w[1, n // 3, 0] = NAN_PAYLOAD
        w[1, n - 1, 1] = NAN_PAYLOAD | 0x80000000
    x.setflags(write=False)
    return x, tuple(pos)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cuts_of(n, g, pos):
    """The issue's cuts, and one with a hit within g on either side of it."""
    out = [[1, B - 1, 1, B], [100, B]]
    late = [p for p in pos if p > B + g]
    if late:
        p = late[len(late) // 2]
        out.append([max(1, p - g // 2), g // 2 + 1 + g // 2])
    res = []
    for c in out:
        c = [v for v in c if v > 0]
        acc, cut = 0, []
        for v in c:
            if acc + v >= n:
                break
            cut.append(v)
            acc += v
        cut.append(n - acc)
        res.append(cut)
    return res


def run_cut(r, x, cut):
    """The stream through channel_blank in calls of the cut's lengths: outputs and per-call counts."""
    ys, cs, a = [], [], 0
    for ln in cut:
        y, c = r.channel_blank(x[:, a:a + ln], count=True)
        ys.append(y)
        cs.append(c)
        a += ln
    return np.concatenate(ys, axis=1), cs


def check_against_model(r, x, pos, p, g, m, mode, fmt, cuts):
    ref = M.definition(x, p, g, m, mode)
    n = x.shape[1]
    for cut in cuts:
        r.setChannelBlanker(p, g, m, mode, fmt)
        y, cs = run_cut(r, x, cut)
        assert np.array_equal(bits(y), bits(ref["y"])), (g, m, mode, fmt, cut)
        a = 0
        for ln, c in zip(cut, cs):
            assert np.array_equal(c, M.count(ref, a, a + ln)), (g, m, mode, fmt, cut, a)
            a += ln
        assert a == n
    return ref


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cpu_backend_equals_model_bit_for_bit(cpu, shape, mode, fmt):
    nch, n = shape
    p = M.make_params(nch, qmin=1e-6 if fmt == FMT_CF32 else 1.0)
    hits = 0
    for g in GUARDS:
        x, pos = signal(nch, n, g, fmt)
        for m in REFS:
            cuts = [[n]] + (cuts_of(n, g, pos) if (m, g) in ((1, 0), (3, 5), (16, 64), (8, 1)) or n <= 3 * B + 17 else [])
            ref = check_against_model(cpu, x, pos, p, g, m, mode, fmt, cuts)
            hits += int(ref["hit"].sum())
            if nch > 1:   # the bypassed channel: the input delayed by g, bit for bit
                assert not ref["out_blank"][1].any()
    if n > B + 1:
        assert hits > 0   # the impulses past block 0 are found


def test_bypassed_channel_keeps_nan_payloads(cpu):
    nch, n, g = 3, 2 * B + 3, 5
    x, _ = signal(nch, n, g, FMT_CF32)
    cpu.setChannelBlanker(M.make_params(nch), g, 3)
    y = cpu.channel_blank(x)
    assert np.array_equal(bits(y[1, g:]), bits(x[1, :n - g]))
    assert (bits(y[1, :g]) == 0).all()
    assert NAN_PAYLOAD in bits(y[1])


@pytest.mark.parametrize("mode", MODES)
def test_hits_agree_with_float64_outside_the_borderline_set(cpu, mode):
    nch, n, g = 16, 40 * B + 17, 4
    x, pos = M.make_input(nch, n, g, seed=7)
    p = M.make_params(nch, k2=10.0, qmin=0.0)
    p[1, 0] = 10.0
    for m in REFS:
        r32 = check_against_model(cpu, x, pos, p, g, m, mode, FMT_CF32, [[n]])
        r64 = M.definition(x, p, g, m, mode, dtype=np.float64)
        fin = np.isfinite(r64["t"])
        border = np.zeros(r64["q"].shape, bool)
        border[fin] = np.abs(r64["q"][fin] - r64["t"][fin]) <= 1.01 * (8 + m + 5) * U * r64["t"][fin]
        assert border.mean() <= 1e-3
        assert np.array_equal(r32["hit"][~border], r64["hit"][~border]), m


@pytest.mark.parametrize("mode", MODES)
def test_blanks_periodic_impulses_and_keeps_the_rest(cpu, mode):
    nch, n, g = 4, 64 * B, 4
    clean, dirty, mask = M.make_periodic(nch, n)
    p = np.tile(np.float32([blanker_threshold(10.0), 0.0]), (nch, 1))
    for m in REFS:
        cpu.setChannelBlanker(p, g, m, mode)
        y = cpu.channel_blank(dirty)
        late = np.arange(n) >= B                       # past block 0
        imp = mask & late
        assert (y[:, g:][:, imp[:n - g]] == 0).all()   # every impulse sample is blanked
        pw = lambda a: float(np.mean(np.abs(a.astype(np.complex128)) ** 2))  # noqa: E731
        p_clean = pw(clean[:, B:n - g])
        assert pw(dirty[:, B:n - g]) >= 20.0 * p_clean
        ratio = pw(y[:, B + g:]) / p_clean
        assert 0.97 <= ratio <= 1.0, (m, ratio)


def test_non_finite_samples_are_blanked_and_do_not_poison_the_reference(cpu):
    n, g, m = 6 * B, 5, 3
    x, _ = M.make_input(1, n, g, seed=3)
    x = x.copy()
    x[0, :] = M._noise(1, n, 3)[0].astype(np.complex64)   # no impulses
    clean = x.copy()
    i_nan, i_inf = 2 * B + 40, 2 * B + 140
    x[0, i_nan] = complex(np.nan, 0.1)
    x[0, i_inf] = complex(0.1, -np.inf)
    p = np.float32([[100.0, 0.0]])
    for mode in MODES:
        cpu.setChannelBlanker(p, g, m, mode)
        y = cpu.channel_blank(x)
        cpu.setChannelBlanker(p, g, m, mode)
        yc = cpu.channel_blank(clean)
        assert np.isfinite(y.view(np.float32)).all()
        for i in (i_nan, i_inf):
            assert (y[0, i:i + 2 * g + 1] == 0).all()          # outputs i + g - g .. i + g + g
        diff = np.flatnonzero(bits(y).reshape(-1, 2).any(axis=1) != bits(yc).reshape(-1, 2).any(axis=1))
        assert set(diff) <= set(range(i_nan, i_nan + 2 * g + 1)) | set(range(i_inf, i_inf + 2 * g + 1))
        assert np.array_equal(bits(y[0, 3 * B + g:]), bits(yc[0, 3 * B + g:]))   # the next M blocks and on
        ref = M.definition(x, p, g, m, mode)
        assert np.array_equal(bits(y), bits(ref["y"]))


def test_zeros_then_signal_needs_qmin(cpu):
    n, g = 3 * B, 2
    x = M._noise(1, n, 5)[0].astype(np.complex64)
    x[0, :2 * B] = 0
    for mode in MODES:
        cpu.setChannelBlanker(np.float32([[10.0, 0.0]]), g, 2, mode)
        y = cpu.channel_blank(x)
        assert (y[0, 2 * B + g:] == 0).all()                   # the reference is 0: everything is a hit
        cpu.setChannelBlanker(np.float32([[10.0, 4.0]]), g, 2, mode)   # |x|^2 is some 0.1
        y = cpu.channel_blank(x)
        assert np.array_equal(bits(y[0, g:]), bits(x[0, :n - g]))


def test_threshold_values():
    assert blanker_threshold(0.0) == 1.0
    assert blanker_threshold(10.0) == 10.0
    assert blanker_threshold(20.0) == 100.0
    assert blanker_threshold(120.0) == float(np.float32(1e12))
    assert blanker_threshold(3.0) == float(np.float32(10.0 ** 0.3))
    for bad in (-0.001, 120.001, float("nan"), float("inf")):
        with pytest.raises(DDCError) as e:
            blanker_threshold(bad)
        assert e.value.code == ERR_ARG
    assert load().sddc_ddc_blanker_threshold(10.0, None) == ERR_ARG


def test_set_call_validity(cpu):
    f = cpu._L.sddc_ddc_set_channel_blanker
    assert cpu._L.sddc_ddc_channel_blanker_reset(cpu._h) == ERR_STATE       # nothing set
    nch = 3
    good = M.make_params(nch)
    ok = (8, 8, BLANKER_MEAN, FMT_CF32)
    assert f(cpu._h, good.ctypes.data, nch, *ok) == 0
    for col, vals in ((0, (np.nan, np.inf, -1.0, 0.5, 2.0 ** 41)), (1, (np.nan, np.inf, -1e-30, 2.0 ** 81))):
        for v in vals:
            q = good.copy()
            q[2, col] = v
            assert f(cpu._h, q.ctypes.data, nch, *ok) == ERR_ARG, (col, v)
    for k2, qmin in ((1.0, 0.0), (2.0 ** 40, 2.0 ** 80), (0.0, 0.0)):
        q = good.copy()
        q[2] = (k2, qmin)
        assert f(cpu._h, q.ctypes.data, nch, *ok) == 0
    for bad in ((-1, 8, 0, 0), (65, 8, 0, 0), (8, 0, 0, 0), (8, 17, 0, 0), (8, 8, 2, 0), (8, 8, -1, 0), (8, 8, 0, 2), (8, 8, 0, -1)):
        assert f(cpu._h, good.ctypes.data, nch, *bad) == ERR_ARG, bad
    for edge in ((0, 1, 0, 0), (64, 16, 1, 1)):
        assert f(cpu._h, good.ctypes.data, nch, *edge) == 0
    assert f(cpu._h, good.ctypes.data, -1, *ok) == ERR_ARG
    big = np.tile(np.float32([10.0, 0.0]), (1025, 1))
    assert f(cpu._h, big.ctypes.data, 1025, *ok) == ERR_ARG
    assert f(cpu._h, big.ctypes.data, 1024, *ok) == 0
    with pytest.raises(DDCError):
        cpu.setChannelBlanker(np.zeros((2, 3), np.float32), 8, 8)
    # a failed set call sets nothing: the 1024 channels stay
    assert f(cpu._h, good.ctypes.data, nch, 65, 8, 0, 0) == ERR_ARG
    x = np.zeros((1024, 4), np.complex64)
    out = np.empty_like(x)
    assert cpu._L.sddc_ddc_channel_blank_host(cpu._h, x.ctypes.data, 1024, 4, 8, out.ctypes.data, 8, None) == 0


def test_call_errors_and_the_off_switch(cpu):
    f = cpu._L.sddc_ddc_channel_blank_host
    nch, n = 3, 40
    x = np.zeros((nch, n), np.complex64)
    out = np.empty_like(x)
    cnt = np.empty(nch, np.uint32)
    s = 2 * n
    args = (x.ctypes.data, nch, n, s, out.ctypes.data, s, cnt.ctypes.data)
    assert f(cpu._h, *args) == ERR_STATE                                    # nothing set
    with pytest.raises(DDCError) as ex:
        cpu.channel_blank(x)
    assert ex.value.code == ERR_STATE
    cpu.setChannelBlanker(M.make_params(nch), 4, 2)
    assert f(cpu._h, *args) == 0
    assert f(cpu._h, x.ctypes.data, 2, n, s, out.ctypes.data, s, cnt.ctypes.data) == ERR_STATE   # another nch
    assert f(cpu._h, x.ctypes.data, nch, 0, s, out.ctypes.data, s, None) == ERR_ARG
    assert f(cpu._h, x.ctypes.data, nch, (1 << 40) + 1, 1 << 42, out.ctypes.data, 1 << 42, None) == ERR_ARG
    assert f(cpu._h, x.ctypes.data, nch, n, s - 2, out.ctypes.data, s, None) == ERR_ARG          # stride < 2 nsamp
    assert f(cpu._h, x.ctypes.data, nch, n, s, out.ctypes.data, s - 2, None) == ERR_ARG
    assert f(cpu._h, x.ctypes.data, nch, n - 1, s - 1, out.ctypes.data, s, None) == ERR_ARG      # odd stride
    assert f(cpu._h, x.ctypes.data, nch, n - 1, s, out.ctypes.data, s - 1, None) == ERR_ARG
    assert f(cpu._h, None, nch, n, s, out.ctypes.data, s, None) == ERR_ARG
    assert f(cpu._h, x.ctypes.data, nch, n, s, None, s, None) == ERR_ARG
    assert f(cpu._h, x.ctypes.data + 4, nch, n - 1, s, out.ctypes.data, s, None) == ERR_ARG      # half a sample in
    assert f(cpu._h, x.ctypes.data, nch, n - 1, s, out.ctypes.data + 4, s, None) == ERR_ARG
    assert f(cpu._h, x.ctypes.data, nch, n - 1, s, out.ctypes.data, s, cnt.ctypes.data + 2) == ERR_ARG
    # overlap: in place, and the output starting inside the input's last stream
    assert f(cpu._h, x.ctypes.data, nch, n, s, x.ctypes.data, s, None) == ERR_ARG
    both = np.zeros(2 * nch * n, np.complex64)
    last = both.ctypes.data + 8 * (nch * n - 1)
    assert f(cpu._h, both.ctypes.data, nch, n, s, last, s, None) == ERR_ARG
    assert f(cpu._h, both.ctypes.data, nch, n, s, last + 8, s, None) == 0                         # adjacent is legal
    assert cpu._L.sddc_ddc_channel_blank_device(cpu._h, x.ctypes.data, nch, n, s, out.ctypes.data, s, None, None) == ERR_STATE
    # a failed call changes no state: the stream goes on as if it had not happened
    g, m = 4, 2
    xs, pos = M.make_input(nch, 3 * B, g)
    ref = M.definition(xs, M.make_params(nch), g, m)
    cpu.setChannelBlanker(M.make_params(nch), g, m)
    y1 = cpu.channel_blank(xs[:, :300])
    assert f(cpu._h, x.ctypes.data, nch, 0, s, out.ctypes.data, s, None) == ERR_ARG
    y2 = cpu.channel_blank(xs[:, 300:])
    assert np.array_equal(bits(np.concatenate([y1, y2], axis=1)), bits(ref["y"]))
    # reset starts a new stream
    cpu.resetChannelBlanker()
    assert np.array_equal(bits(cpu.channel_blank(xs)), bits(ref["y"]))
    # the off switch
    cpu.setChannelBlanker(None, 0, 0)
    assert f(cpu._h, *args) == ERR_STATE
    assert cpu._L.sddc_ddc_channel_blanker_reset(cpu._h) == ERR_STATE
    assert cpu._L.sddc_ddc_set_channel_blanker(cpu._h, M.make_params(nch).ctypes.data, 0, 0, 0, 0, 0) == 0
