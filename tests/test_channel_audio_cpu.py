"""The channel audio filter without a GPU: the CPU backend (sddc_ddc_channel_audio_filter_host of a CPU
handle) against the definition evaluated with an exact-rational fmaf, within the float64 model's
bound (tools/channel_audio_model.py), the bound's power to tell a broken block form from a right one,
the cut invariance, the section designers and the error returns.

The bound is the header's: per sample five roundings per section, per block boundary (2S + 1) u
(|Z_i| + sum_j |M_ij| |E_j|) per row, each carried to the output through the absolute value of the
recurrence's own response, times 1.01.  Nothing here is fitted to the code under test.
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


M = _load("channel_audio_model")

from extio_sddc_amd import (AUDIO_BLOCK, AUDIO_F32, AUDIO_S16, BIQUAD_DC_BLOCK, BIQUAD_HIGHPASS,  # noqa: E402
                            BIQUAD_IDENTITY, BIQUAD_LOWPASS, BIQUAD_NOTCH, BIQUAD_ONE_POLE_LP, DEVICE_CPU, DDCError, R2iq,
                            biquad)

B = AUDIO_BLOCK
ERR_ARG, ERR_STATE = -1, -4


def chain_set():
    return np.stack([biquad(BIQUAD_DC_BLOCK, 1e-3), biquad(BIQUAD_HIGHPASS, 0.01, 2.0), biquad(BIQUAD_LOWPASS, 0.2, 5.0),
                     biquad(BIQUAD_ONE_POLE_LP, 0.05)])


def resonant_set():
    return np.stack([biquad(BIQUAD_LOWPASS, 0.01, 30.0)])


def ringing_set():
    """Memory beyond B (the pole radius is 1 - 0.003) with the poles well away from z = 1."""
    return np.stack([biquad(BIQUAD_LOWPASS, 0.1, 100.0)])


def dc_ringing_set():
    return np.stack([biquad(BIQUAD_DC_BLOCK, 1e-3), biquad(BIQUAD_LOWPASS, 0.1, 100.0)])


SETS = {"chain": chain_set, "resonant": resonant_set, "ringing": ringing_set, "dc+ringing": dc_ringing_set}
# A matrix of B - 1 steps is wrong by A^(B-1) (I - A) E, which is small in itself where every slow pole
# lies next to z = 1 (the DC blocker, the 0.01 low-pass): there the sabotage moves the output by 8 and
# 57 bounds only (printed below), so it is asserted on the sets whose long memory rings at 0.1 fs.
SABOTAGES = {"short_matrix": ["ringing", "dc+ringing"], "drop_z": list(SETS), "skip_adv": list(SETS)}


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def signal(nch, n):
    x = M.make_input(nch, n)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """(coef [1, S, 5], x [1, n], y64 [1, n], bound [1, n]) of a filter set, shared by the tests."""
    coef = SETS[name]()[None]
    x = signal(1, n)
    out = coef, x, M.recurrence64(x, coef), M.bounds(x, coef)
    for a in out:
        a.setflags(write=False)
    return out


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chaud_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint64], ctypes.c_int
    return f(r._h, pos)


# -- 1. the definition, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("nsec", [1, 3])
def test_cpu_backend_is_the_definition(cpu, nsec):
    secs = [biquad(BIQUAD_HIGHPASS, 0.02, 1.5), biquad(BIQUAD_DC_BLOCK, 2e-3), biquad(BIQUAD_LOWPASS, 0.11, 4.0)][:nsec]
    coef = np.stack(secs)
    n = 2 * B + 5
    x = signal(1, n)
    Mm = M.block_matrix(coef)
    want = M.block_form(x[0], coef, Mm, fmaf=M.fmaf_exact)
    cpu.setChannelAudioFilter(coef[None])
    got = cpu.channel_audio_filter(x)
    assert got.dtype == np.float32 and got.shape == (1, n)
    assert np.array_equal(got[0], want), f"first difference at {np.flatnonzero(got[0] != want)[:4]}"
    # the rational fmaf is not idle: the float64 short cut agrees with it here too
    assert np.array_equal(M.block_form(x[0], coef, Mm), want)


def test_round_f32_is_correct_rounding():
    from fractions import Fraction
    one = Fraction(1)
    ulp = Fraction(1, 2 ** 23)
    assert M.round_f32(one + ulp / 2) == 1.0                          # a tie goes to even
    assert M.round_f32(one + 3 * ulp / 2) == float(1 + 2 * ulp)
    assert M.round_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == float(1 + ulp)
    assert M.round_f32(Fraction(3, 2 ** 150)) == 2.0 ** -148          # subnormal: 1.5 quanta, a tie, to even
    assert M.round_f32(Fraction(-5, 2 ** 151)) == -(2.0 ** -149)      # 1.25 quanta


# -- 2. within the float64 model's bound ------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_cpu_backend_within_bound(cpu, name):
    n = 4 * B + 37
    coef, x, y64, bnd = reference(name, n)
    cpu.setChannelAudioFilter(coef)
    y = cpu.channel_audio_filter(x).astype(np.float64)
    err = np.abs(y - y64)
    scale = np.abs(y64).max()
    print(f"{name}: max err {err.max() / (M.U * scale):.2f} u max|y|, max bound {bnd.max() / (M.U * scale):.2f} u max|y|, "
          f"worst err / bound {np.max(err / bnd):.3f}")
    assert np.all(err <= bnd)


def test_s16_formats(cpu):
    n = 2 * B + 9
    coef, x, y64, bnd = reference("chain", n)
    xs = np.round(x * 20000).astype(np.int16)
    y64 = M.recurrence64(xs.astype(np.float32), coef)
    bnd = M.bounds(xs.astype(np.float32), coef)
    cpu.setChannelAudioFilter(coef, AUDIO_S16, AUDIO_S16)
    ys = cpu.channel_audio_filter(xs)
    assert ys.dtype == np.int16
    assert np.all(np.abs(ys - np.clip(y64, -32768, 32767)) <= bnd + 0.5)
    cpu.setChannelAudioFilter(coef, AUDIO_S16, AUDIO_F32)
    yf = cpu.channel_audio_filter(xs)
    assert np.array_equal(np.clip(np.rint(yf), -32768, 32767).astype(np.int16), ys)


# -- 3. the bound tells a broken block form from a right one ----------------------------------
@pytest.mark.parametrize("sabotage", list(SABOTAGES))
def test_bound_discriminates(sabotage):
    n = 4 * B + 37
    for name in SETS:
        coef, x, y64, bnd = reference(name, n)
        right = M.block_form(x[0], coef[0])
        assert np.all(np.abs(right - y64[0]) <= bnd[0]), name
        if sabotage == "short_matrix":
            y = M.block_form(x[0], coef[0], M.block_matrix(coef[0], steps=B - 1))
        elif sabotage == "drop_z":
            y = M.block_form(x[0], coef[0], sabotage="drop_z")
        else:
            y = M.block_form(x[0], coef[0], sabotage=("skip_adv", 2))
        ratio = np.max(np.abs(y - y64[0]) / bnd[0])
        print(f"{name} {sabotage}: worst err / bound {ratio:.3g}")
        if name in SABOTAGES[sabotage]:
            assert ratio >= 100, name


# -- 4. cuts ------------------------------------------------------------------------------------
def run_cuts(r, x, cuts):
    out, i = [], 0
    for n in cuts:
        out.append(r.channel_audio_filter(x[:, i:i + n]))
        i += n
    assert i == x.shape[1]
    return np.concatenate(out, axis=1)


def mixed_coef():
    ident = biquad(BIQUAD_IDENTITY)
    return np.stack([np.stack([biquad(BIQUAD_DC_BLOCK, 1e-3), biquad(BIQUAD_LOWPASS, 0.01, 30.0)]),
                     np.stack([ident, ident]),
                     np.stack([biquad(BIQUAD_NOTCH, 0.07, 8.0), biquad(BIQUAD_ONE_POLE_LP, 0.03)])])


@pytest.mark.parametrize("cuts", [[1, B - 1, 1, B, B + 40], [100, B, 2 * B - 59], [1] * (B + 2), [10, 20]],
                         ids=["edges", "100", "per-sample", "10+20"])
def test_cuts_are_bit_identical(cpu, cuts):
    coef = mixed_coef()
    x = signal(3, sum(cuts))
    cpu.setChannelAudioFilter(coef)
    whole = cpu.channel_audio_filter(x)
    assert np.array_equal(whole[1], x[1])              # the identity channel passes its samples through
    cpu.resetChannelAudioFilter()
    assert np.array_equal(run_cuts(cpu, x, cuts), whole)


def test_set_position_moves_the_block_edges(cpu):
    coef = mixed_coef()[:1]
    x = signal(1, B + 30)
    cpu.setChannelAudioFilter(coef)
    assert set_position(cpu, B - 7) == 0
    got = cpu.channel_audio_filter(x)
    want = M.block_form(x[0], coef[0], pos=B - 7)
    assert np.array_equal(got[0], want)


# -- 5. the designers ---------------------------------------------------------------------------
DESIGNS = [(BIQUAD_IDENTITY, 0.25, 1.0), (BIQUAD_DC_BLOCK, 1e-3, 1.0), (BIQUAD_DC_BLOCK, 0.02, 1.0),
           (BIQUAD_ONE_POLE_LP, 0.0442, 1.0), (BIQUAD_ONE_POLE_LP, 0.3, 1.0), (BIQUAD_LOWPASS, 0.01, 30.0),
           (BIQUAD_LOWPASS, 0.2, 5.0), (BIQUAD_LOWPASS, 0.45, 0.5), (BIQUAD_HIGHPASS, 0.00625, 0.7071),
           (BIQUAD_HIGHPASS, 0.01, 2.0), (BIQUAD_NOTCH, 0.07, 8.0), (BIQUAD_NOTCH, 0.25, 1.0)]


@pytest.mark.parametrize("kind,f,q", DESIGNS)
def test_designers(kind, f, q):
    c = biquad(kind, f, q)
    want = M.design64(kind, f, q)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert c.dtype == np.float32 and np.all(np.abs(c.astype(np.float64) - want) <= ulp)
    assert M.stable(c)
    if kind == BIQUAD_DC_BLOCK:
        assert c[1] == -c[0] and c[2] == 0
    if kind == BIQUAD_HIGHPASS:
        assert c[1] == np.float32(-2) * c[0] and c[2] == c[0]
    if kind in (BIQUAD_DC_BLOCK, BIQUAD_HIGHPASS):
        assert float(c[0]) + float(c[1]) + float(c[2]) == 0.0     # DC is rejected exactly
    if kind == BIQUAD_LOWPASS:
        # the float rounding of the coefficients: b1 = 2 b0 and b2 = b0 exactly, so the numerator moves
        # by u relative; the denominator D = 1 + a1 z^-1 + a2 z^-2 by at most u (|a1| + |a2|)
        z1 = np.exp(-2j * np.pi * f)
        D = abs(1 + float(c[3]) * z1 + float(c[4]) * z1 * z1)
        rel = 1.1 * M.U * (1 + (abs(float(c[3])) + abs(float(c[4]))) / D)
        assert abs(abs(M.response(c[None], f)) - q) <= rel * q


@pytest.mark.parametrize("kind,f,q", [(-1, 0.1, 1), (6, 0.1, 1), (BIQUAD_LOWPASS, 0.0, 1), (BIQUAD_LOWPASS, 0.5, 1),
                                      (BIQUAD_DC_BLOCK, -0.1, 1), (BIQUAD_LOWPASS, float("nan"), 1),
                                      (BIQUAD_HIGHPASS, 0.1, 0.0), (BIQUAD_NOTCH, 0.1, float("inf")),
                                      (BIQUAD_NOTCH, 0.1, float("nan"))])
def test_designer_errors(kind, f, q):
    with pytest.raises(DDCError) as e:
        biquad(kind, f, q)
    assert e.value.code == ERR_ARG


# -- 6. error returns ---------------------------------------------------------------------------
def raw_set(r, coef, nsec, nch, fin=AUDIO_F32, fout=AUDIO_F32):
    c = np.ascontiguousarray(coef, np.float32)
    return r._L.sddc_ddc_set_channel_audio_filter(r._h, c.ctypes.data, nsec, nch, fin, fout)


def test_error_returns(cpu):
    x = signal(1, 40)
    with pytest.raises(DDCError) as e:
        cpu.channel_audio_filter(x)
    assert e.value.code == ERR_STATE
    assert cpu._L.sddc_ddc_channel_audio_filter_reset(cpu._h) == ERR_STATE
    good = mixed_coef()[:1]
    cpu.setChannelAudioFilter(good)
    first = cpu.channel_audio_filter(x[:, :10])
    # a failed set sets nothing: the filter and its state go on
    bad = good.copy()
    bad[0, 1, 4] = 1.0                                   # a2 = 1: on the triangle's edge
    assert raw_set(cpu, bad, 2, 1) == ERR_ARG
    bad = good.copy()
    bad[0, 0, 3] = np.float32(1.0) + bad[0, 0, 4]        # |a1| = 1 + a2
    assert raw_set(cpu, bad, 2, 1) == ERR_ARG
    bad = good.copy()
    bad[0, 0, 0] = np.nan
    assert raw_set(cpu, bad, 2, 1) == ERR_ARG
    assert raw_set(cpu, good, 0, 1) == ERR_ARG
    assert raw_set(cpu, good, 5, 1) == ERR_ARG
    assert raw_set(cpu, good, 2, -1) == ERR_ARG
    assert raw_set(cpu, good, 2, 1025) == ERR_ARG
    assert raw_set(cpu, good, 2, 1, 2, 0) == ERR_ARG
    assert raw_set(cpu, good, 2, 1, 0, 7) == ERR_ARG
    f = cpu._L.sddc_ddc_channel_audio_filter_host
    out = np.full(40, np.nan, np.float32)
    assert f(cpu._h, x.ctypes.data, 2, 10, 10, out.ctypes.data, 10) == ERR_STATE      # another nch
    assert f(cpu._h, x.ctypes.data, 1, 0, 0, out.ctypes.data, 0) == ERR_ARG
    assert f(cpu._h, None, 1, 10, 10, out.ctypes.data, 10) == ERR_ARG
    assert f(cpu._h, x.ctypes.data + 2, 1, 10, 10, out.ctypes.data, 10) == ERR_ARG     # alignment
    assert f(cpu._h, x.ctypes.data, 1, (1 << 40) + 1, 0, out.ctypes.data, 0) == ERR_ARG
    assert np.all(np.isnan(out))
    rest = cpu.channel_audio_filter(x[:, 10:])
    cpu.setChannelAudioFilter(good)
    assert np.array_equal(np.concatenate([first, rest], axis=1), cpu.channel_audio_filter(x))
    # strides of several channels
    cpu.setChannelAudioFilter(mixed_coef())
    x3 = signal(3, 40)
    assert f(cpu._h, x3.ctypes.data, 3, 40, 39, out.ctypes.data, 40) == ERR_ARG
    # off: the stage is gone
    cpu.setChannelAudioFilter(None)
    with pytest.raises(DDCError):
        cpu.channel_audio_filter(x)
    # a device call on a CPU handle
    cpu.setChannelAudioFilter(good)
    g = cpu._L.sddc_ddc_channel_audio_filter_device
    assert g(cpu._h, x.ctypes.data, 1, 10, 10, out.ctypes.data, 10, None) == ERR_STATE
