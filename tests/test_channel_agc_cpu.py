"""The channel AGC without a GPU: the CPU backend (sddc_ddc_channel_agc_host of a CPU handle) against
the numpy float32 transcription of the definition bit for bit, within the float64 recurrence's bound
(tools/channel_agc_model.py), the bound's power to tell a broken block form from a right one, the cut
invariance, the properties of the definition, subnormal and non-finite values, and the error returns.

The bound is the header's: 1.01 (2 B + 2 K(n) + 2) u |y64[n]|, K(n) = ceil((n + 1) / B): every candidate
of the maximum passes at most B - 1 + B rounded multiplies and two roundings per block boundary, and
the output rounds twice more.  Nothing here is fitted to the code under test.
"""
from __future__ import annotations

import ctypes
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load("channel_agc_model")

from extio_sddc_amd import AGC_BLOCK, AUDIO_F32, AUDIO_S16, DEVICE_CPU, DDCError, R2iq, agc_decay  # noqa: E402

B = AGC_BLOCK
U = 2.0 ** -24
ERR_ARG, ERR_STATE = -1, -4
S16_SCALE = 2000.0          # float streams as int16: the loud part some 600 rms, the quiet part some 6
SHAPES = [(1, 1), (1, B), (1, 3 * B + 17), (3, 2 * B + 3), (48, 5 * B + 17)]
FORMATS = [(AUDIO_F32, AUDIO_F32), (AUDIO_S16, AUDIO_S16), (AUDIO_F32, AUDIO_S16), (AUDIO_S16, AUDIO_F32)]
FEW = [27, 3, 44]           # rows of make_params(48) for shapes of up to three channels: (T, d, F) all differ


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def params(nch):
    """[nch, 3]; channel 1 (of several) is bypassed."""
    p = M.make_params(48)
    p = p if nch == 48 else p[FEW[:nch]].copy()
    if nch > 1:
        p[1, 0] = 0.0
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def signal(nch, n, fin=AUDIO_F32):
    x = M.make_input(nch, n)
    if fin == AUDIO_S16:
        x = np.round(x * S16_SCALE).astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def definition(nch, n, fin, fout):
    """(y, env) of definition32, shared by the tests."""
    y, env = M.definition32(signal(nch, n, fin), params(nch), out16=fout == AUDIO_S16)
    y.setflags(write=False)
    env.setflags(write=False)
    return y, env


@functools.lru_cache(maxsize=None)
def reference(nch, n, fin):
    """(y64, bound) of the float64 recurrence."""
    x, p = signal(nch, n, fin), params(nch)
    out = M.recurrence64(x, p)[0], M.bounds(x, p)
    for a in out:
        a.setflags(write=False)
    return out


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chagc_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint64], ctypes.c_int
    return f(r._h, pos)


# -- 1. the definition bit for bit, and within the bound ------------------------------------------
@pytest.mark.parametrize("fin,fout", FORMATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_backend_is_the_definition_and_within_the_bound(cpu, shape, fin, fout):
    nch, n = shape
    x, p = signal(nch, n, fin), params(nch)
    cpu.setChannelAgc(p, fin, fout)
    y, env = cpu.channel_agc(x, envelope=True)
    want, wenv = definition(nch, n, fin, fout)
    assert y.dtype == want.dtype and y.shape == (nch, n) and env.dtype == np.float32 and env.shape == (nch,)
    assert np.array_equal(bits(y), bits(want)), f"{np.count_nonzero(bits(y) != bits(want))} samples differ"
    assert np.array_equal(bits(env), bits(wenv))
    if nch > 1:   # the bypassed channel: the sample as it is, and its envelope still moves
        if fin == AUDIO_F32 and fout == AUDIO_F32:
            assert np.array_equal(bits(y[1]), bits(x[1]))
        elif fin == AUDIO_S16:
            assert np.array_equal(y[1], x[1].astype(y.dtype))
        assert env[1] > 0
    y64, bnd = reference(nch, n, fin)
    slack = 0.5 if fout == AUDIO_S16 else 0.0
    err = np.abs(y.astype(np.float64) - (np.clip(y64, -32768, 32767) if fout == AUDIO_S16 else y64))
    assert np.all(err <= bnd + slack)
    if nch == 48 and fout == AUDIO_F32:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bnd > 0, err / bnd, 0.0)
        for k, d in enumerate(M.DECAYS):
            print(f"{fin}->{fout} d = 1 - {1 - d:.3g}: worst err / bound {ratio[k::8].max():.3f}")


# -- 2. the bound can see a broken block form ------------------------------------------------------
def test_bound_tells_a_broken_block_form():
    nch, n = SHAPES[-1]
    x, p = signal(nch, n), M.make_params(nch)
    y64, bnd = M.recurrence64(x, p)[0], M.bounds(x, p)
    good = np.abs(M.definition32(x, p)[0].astype(np.float64) - y64) / bnd
    assert good.max() <= 1
    for sabotage in ("no_carry", "dB255"):
        ratio = np.abs(M.definition32(x, p, sabotage=sabotage)[0].astype(np.float64) - y64) / bnd
        for k in (2, 3):   # d = 0.99 and 0.999
            print(f"{sabotage} d = {M.DECAYS[k]}: {ratio[k::8].max():.3g} x the bound (the definition: {good[k::8].max():.3f})")
            assert ratio[k::8].max() >= 10
        if sabotage == "dB255":   # invisible where one step is 2^-20 of the envelope, 30 times inside the bound
            assert ratio[6::8].max() <= 1 and ratio[7::8].max() <= 1


# -- 3. stream properties ---------------------------------------------------------------------------
CUTS = {"one": lambda n: [n], "edges": lambda n: [1, B - 1, 1, B, n - 2 * B - 1], "per-sample": lambda n: [1] * n,
        "10+20": lambda n: [10, 20]}


@pytest.mark.parametrize("fin,fout", FORMATS[:2])
@pytest.mark.parametrize("cut", list(CUTS))
def test_cuts_are_bit_identical(cpu, cut, fin, fout):
    nch = 3
    n = {"per-sample": B + 2, "10+20": 30}.get(cut, 3 * B + 40)
    x, p = signal(nch, n, fin), params(nch)
    want, wenv = definition(nch, n, fin, fout)
    cpu.setChannelAgc(p, fin, fout)
    at, parts, env = 0, [], None
    for m in CUTS[cut](n):
        y, env = cpu.channel_agc(np.ascontiguousarray(x[:, at:at + m]), envelope=True)
        parts.append(y)
        at += m
    assert at == n
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(want))
    assert np.array_equal(bits(env), bits(wenv))
    # a reset starts the same stream again
    cpu.resetChannelAgc()
    assert np.array_equal(bits(cpu.channel_agc(x)), bits(want))


def test_a_stream_that_starts_inside_a_block(cpu):
    nch, n, pos = 3, 2 * B + 3, 5 * B + 200
    x, p = signal(nch, n), params(nch)
    want, wenv = M.definition32(x, p, pos=pos)
    cpu.setChannelAgc(p)
    assert set_position(cpu, pos) == 0
    y, env = cpu.channel_agc(x, envelope=True)
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(env), bits(wenv))
    assert not np.array_equal(bits(y), bits(definition(nch, n, AUDIO_F32, AUDIO_F32)[0]))   # the position matters


# -- 4. properties of the definition ------------------------------------------------------------------
def test_output_never_exceeds_the_target_and_a_new_peak_sits_on_it(cpu):
    nch, n = SHAPES[-1]
    x, p = signal(nch, n), M.make_params(nch)
    cpu.setChannelAgc(p)
    y = cpu.channel_agc(x).astype(np.float64)
    T, F = p[:, :1].astype(np.float64), p[:, 2:].astype(np.float64)
    assert np.all(np.abs(y) <= T * (1 + 2 * U))
    _, _, R = M.definition32(x, p, trace=True)
    a = np.abs(x)
    peak = (R == a) & (a.astype(np.float64) > F)          # the step took the sample: den = |x|
    assert peak[:, :100].any() and peak[:, 100:].any()
    assert np.all(np.abs(np.abs(y[peak]) - np.broadcast_to(T, y.shape)[peak]) <= 2 * U * np.broadcast_to(T, y.shape)[peak])


# -- 5. subnormals and non-finite input -----------------------------------------------------------------
def test_decay_into_subnormals_is_the_definition(cpu):
    p = np.array([[0.5, 0.5, 2.0 ** -60]], np.float32)
    assert M.block_decay(p[:, 1])[0] == 0                 # dB underflows to 0 and is accepted
    x = np.zeros((1, 200), np.float32)
    x[0, 0] = 1.0
    cpu.setChannelAgc(p)
    tiny = float(np.finfo(np.float32).tiny)
    at = 0
    for end in (130, 140, 200):
        y, env = cpu.channel_agc(x[:, at:end], envelope=True)
        wy, wenv = M.definition32(x[:, :end], p)
        assert np.array_equal(bits(y), bits(wy[:, at:])) and np.array_equal(bits(env), bits(wenv))
        if end < 200:
            assert 0 < env[0] < tiny and env[0] == 2.0 ** -(end - 1)
        else:
            assert env[0] == 0
        at = end


def test_nan_and_infinity(cpu):
    nch, n, at = 3, B + 40, 50
    p = params(nch)
    x = signal(nch, n).copy()
    x[:, at] = 0.0
    xn = x.copy()
    xn[:, at] = np.nan
    for fout in (AUDIO_F32, AUDIO_S16):
        cpu.setChannelAgc(p, AUDIO_F32, fout)
        y0, env0 = cpu.channel_agc(x, envelope=True)
        cpu.resetChannelAgc()
        y, env = cpu.channel_agc(xn, envelope=True)
        wy, wenv = M.definition32(xn, p, out16=fout == AUDIO_S16)
        other = np.arange(n) != at
        assert np.array_equal(bits(y[:, other]), bits(y0[:, other])) and np.array_equal(bits(env), bits(env0))
        assert np.array_equal(bits(env), bits(wenv))
        if fout == AUDIO_F32:
            assert np.isnan(y[:, at]).all() and not np.isnan(y[:, other]).any()
            assert np.array_equal(np.isnan(y), np.isnan(wy)) and np.array_equal(bits(y[:, other]), bits(wy[:, other]))
        else:
            assert (y[:, at] == 0).all() and np.array_equal(y, wy)
    xi = x[:, :at + 1].copy()
    xi[0, at], xi[2, at] = np.inf, -np.inf
    cpu.setChannelAgc(p)
    y, env = cpu.channel_agc(xi, envelope=True)
    assert env[0] == np.finfo(np.float32).max and env[2] == np.finfo(np.float32).max and np.isfinite(env[1])
    assert np.array_equal(bits(env), bits(M.definition32(xi, p)[1]))


# -- 6. arguments ------------------------------------------------------------------------------------------
def test_agc_decay():
    for tau in (0.5, 1.0, 48.0, 1000.0, 2.5e5):
        assert agc_decay(tau) == float(np.float32(math.exp(-1.0 / tau)))
    assert agc_decay(1e12) == 1.0 - 2.0 ** -24            # exp rounds to 1.0f
    assert agc_decay(2.0 ** 25) == 1.0 - 2.0 ** -24 and agc_decay(1e-9) == 0.0
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(DDCError) as e:
            agc_decay(bad)
        assert e.value.code == ERR_ARG
    from extio_sddc_amd import load
    assert load().sddc_ddc_agc_decay(100.0, None) == ERR_ARG


def test_set_rejects_bad_parameters_and_sets_nothing(cpu):
    nch, n, cut = 3, 2 * B + 3, 100
    x, p = signal(nch, n), params(nch)
    want, wenv = definition(nch, n, AUDIO_F32, AUDIO_F32)
    f = cpu._L.sddc_ddc_set_channel_agc
    assert cpu._L.sddc_ddc_channel_agc_reset(cpu._h) == ERR_STATE           # nothing set
    assert set_position(cpu, 5) == ERR_STATE
    cpu.setChannelAgc(p)
    first = cpu.channel_agc(np.ascontiguousarray(x[:, :cut]))
    nan, inf = float("nan"), float("inf")
    bad_values = {0: [-0.5, nan, inf, 2.0 ** -61, 2.0 ** 61, -2.0 ** -70],
                  1: [-0.1, 1.0, 1.5, nan, inf, -inf],
                  2: [0.0, -1e-4, nan, inf, 2.0 ** -61, 2.0 ** 61]}
    for col, values in bad_values.items():
        for v in values:
            q = np.ascontiguousarray(p.copy())
            q[2, col] = v
            assert f(cpu._h, q.ctypes.data, nch, AUDIO_F32, AUDIO_F32) == ERR_ARG, (col, v)
    q = np.ascontiguousarray(p)
    assert f(cpu._h, q.ctypes.data, nch, 2, AUDIO_F32) == ERR_ARG
    assert f(cpu._h, q.ctypes.data, nch, AUDIO_F32, -1) == ERR_ARG
    assert f(cpu._h, q.ctypes.data, -1, AUDIO_F32, AUDIO_F32) == ERR_ARG
    big = np.ascontiguousarray(np.tile(p[:1], (1025, 1)))
    assert f(cpu._h, big.ctypes.data, 1025, AUDIO_F32, AUDIO_F32) == ERR_ARG
    with pytest.raises(DDCError):
        cpu.setChannelAgc(np.zeros((3, 2), np.float32))
    # the limits themselves are valid (on another handle), and the stream here goes on bit-exactly
    with R2iq(gain=1.0, device=DEVICE_CPU) as other:
        other.setChannelAgc(np.array([[2.0 ** -60, 0.0, 2.0 ** 60], [2.0 ** 60, 1 - 2.0 ** -24, 2.0 ** -60], [-0.0, 0.5, 1.0]],
                                     np.float32))
    rest, env = cpu.channel_agc(np.ascontiguousarray(x[:, cut:]), envelope=True)
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(want)) and np.array_equal(bits(env), bits(wenv))


@pytest.mark.parametrize("fin,fout", FORMATS[:2])
def test_process_errors_leave_the_outputs_and_the_state_untouched(cpu, fin, fout):
    nch, n, cut = 3, 2 * B + 3, 100
    x, p = signal(nch, n, fin), params(nch)
    want, wenv = definition(nch, n, fin, fout)
    poison = 0x7fff if fout == AUDIO_S16 else np.nan
    out = np.full((nch, n), poison, want.dtype)
    env = np.full(nch, np.nan, np.float32)
    xin = np.ascontiguousarray(x)
    f = cpu._L.sddc_ddc_channel_agc_host
    args = (xin.ctypes.data, nch, n, n, out.ctypes.data, n, env.ctypes.data)
    assert f(cpu._h, *args) == ERR_STATE                                     # nothing set
    cpu.setChannelAgc(p, fin, fout)
    first = cpu.channel_agc(np.ascontiguousarray(x[:, :cut]))
    half_in, half_out = (1 if fin == AUDIO_S16 else 2), (1 if fout == AUDIO_S16 else 2)
    assert f(cpu._h, xin.ctypes.data, 2, n, n, out.ctypes.data, n, env.ctypes.data) == ERR_STATE
    assert f(cpu._h, xin.ctypes.data, nch, 0, n, out.ctypes.data, n, env.ctypes.data) == ERR_ARG
    assert f(cpu._h, xin.ctypes.data, nch, (1 << 40) + 1, 1 << 41, out.ctypes.data, 1 << 41, env.ctypes.data) == ERR_ARG
    assert f(cpu._h, xin.ctypes.data, nch, n, n - 1, out.ctypes.data, n, env.ctypes.data) == ERR_ARG
    assert f(cpu._h, xin.ctypes.data, nch, n, n, out.ctypes.data, n - 1, env.ctypes.data) == ERR_ARG
    assert f(cpu._h, None, nch, n, n, out.ctypes.data, n, env.ctypes.data) == ERR_ARG
    assert f(cpu._h, xin.ctypes.data, nch, n, n, None, n, env.ctypes.data) == ERR_ARG
    assert f(cpu._h, xin.ctypes.data + half_in, nch, n - 1, n, out.ctypes.data, n, env.ctypes.data) == ERR_ARG
    assert f(cpu._h, xin.ctypes.data, nch, n - 1, n, out.ctypes.data + half_out, n, env.ctypes.data) == ERR_ARG
    assert cpu._L.sddc_ddc_channel_agc_device(cpu._h, xin.ctypes.data, nch, n, n, out.ctypes.data, n, None, None) == ERR_STATE
    assert (out == poison).all() if fout == AUDIO_S16 else np.isnan(out).all()
    assert np.isnan(env).all()
    rest, e = cpu.channel_agc(np.ascontiguousarray(x[:, cut:]), envelope=True)
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(want)) and np.array_equal(bits(e), bits(wenv))
    # the host call writes the streams alone, and env may be null
    cpu.resetChannelAgc()
    wide = np.full((nch, n + 3), poison, want.dtype)
    assert f(cpu._h, xin.ctypes.data, nch, n, n, wide.ctypes.data, n + 3, None) == 0
    assert np.array_equal(bits(wide[:, :n]), bits(want))
    assert (wide[:, n:] == poison).all() if fout == AUDIO_S16 else np.isnan(wide[:, n:]).all()
    cpu.setChannelAgc(None)
    assert f(cpu._h, *args) == ERR_STATE
    with pytest.raises(DDCError) as ex:
        cpu.channel_agc(x)
    assert ex.value.code == ERR_STATE
