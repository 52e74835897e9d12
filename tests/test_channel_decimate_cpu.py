"""The channel decimator on the CPU backend (no GPU): sddc_ddc_channel_decimate_host of a CPU handle
against the float64 model and its derived bound (tools/channel_decimate_model.py), the impulse
response bit for bit, the stream cut into calls, reset, and the error returns of the C ABI.

The bar: every output component within gamma sum_j |h[j]| |x[mR - j]|, gamma = n u / (1 - n u),
n = ntaps + 1, u = 2^-24, computed per output from the model's own sum.
Shapes (nch, R, ntaps, nsamp / R): those of tests/test_gpu_channel_decimate.py, T the GPU kernel's tile.
"""
from __future__ import annotations

import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("channel_decimate_model",
                                               os.path.join(ROOT, "tools", "channel_decimate_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

from extio_sddc_amd import CHANNEL_DECIMATE_TILE as T  # noqa: E402
from extio_sddc_amd import DEVICE_CPU, DDCError, R2iq, channel_decimate_samples  # noqa: E402

CS16_SCALE = 4.0
ERR_ARG, ERR_STATE = -1, -4
FORMATS = ["CF32", "CS16"]
SHAPES = [(1, 2, 1, 1), (1, 8, 3, T + 1), (1, 3, 3, T - 1), (3, 5, 21, 2 * T + 1), (2, 64, 1024, 3), (1024, 8, 65, 2)]


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


def set_format(r, fmt):
    r.setOutputFormat(fmt, CS16_SCALE if fmt == "CS16" else 1.0)


@functools.lru_cache(maxsize=None)
def signal(kind, nch, nsamp, R):
    x = M.make_input(kind, nch, nsamp, R)
    x.setflags(write=False)
    return x


def host_iq(x, fmt):
    if fmt == "CS16":
        return M.as_cs16(x).reshape(x.shape[0], x.shape[1], 2)
    return M.as_cf32(x).view(np.complex64)


def sample_values(x, fmt):
    """What the backend reads: the float32 values of the model's input in this format."""
    return M.cs16_values(M.as_cs16(x), CS16_SCALE) if fmt == "CS16" else M.values(x)


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def test_tile_constant_matches_the_kernel_header():
    import re
    src = open(os.path.join(ROOT, "extio_sddc_amd", "csrc", "ddc_kernels.h")).read()
    assert int(re.search(r"constexpr int kChDecTile = (\d+);", src).group(1)) == T


def test_lds_layout_model():
    """tools/channel_decimate_banks.py against the launch's own layout: the same tile and pitch, the
    tile inside the LDS, conflict-free reads for every pitch picked, no store conflicts on the
    benchmark's rows at R = 8 and 16 and at most 2-way ones at R = 32; the direct layout would read
    8-way at R = 8."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import channel_decimate_banks as B
    finally:
        sys.path.pop(0)
    f = R2iq.__init__.__globals__["_lib"].load().sddc_ddc_internal_chdec_layout
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3
    assert B.TILE == T and B.read_conflicts(8, 0, transposed=False) == 14
    tile, pitch, cost = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cases = [(s[1], s[2]) for s in SHAPES] + [(8, 65), (16, 129), (32, 257), (2, 1024), (64, 1), (63, 1000), (7, 1024)]
    for R, ntaps in cases:
        for cs16 in (0, 1):
            assert f(R, ntaps, cs16, ctypes.byref(tile), ctypes.byref(pitch), ctypes.byref(cost)) == 0
            assert (tile.value, pitch.value, cost.value) == B.layout(R, ntaps, cs16), (R, ntaps, cs16)
            assert 1 <= tile.value <= T and pitch.value * R <= B.LDS
            assert pitch.value >= tile.value + (ntaps - 1 + R - 1) // R
            assert B.read_conflicts(R, pitch.value) == 0
            if (R, ntaps) in ((8, 65), (16, 129)):
                assert cost.value == 0, (R, ntaps, cs16, cost.value)
            if (R, ntaps) == (32, 257):
                assert cost.value <= 4 * (4 if cs16 else 2)   # one extra cycle in each group
    assert f(1, 8, 0, ctypes.byref(tile), ctypes.byref(pitch), ctypes.byref(cost)) == ERR_ARG
    assert f(8, 1025, 0, ctypes.byref(tile), ctypes.byref(pitch), ctypes.byref(cost)) == ERR_ARG


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bound(cpu, shape, fmt):
    nch, R, ntaps, nout = shape
    set_format(cpu, fmt)
    h = M.make_taps(ntaps)
    for kind in ("noise", "edges"):
        x = signal(kind, nch, nout * R, R)
        cpu.setChannelDecimator(h, R, nch)
        y = cpu.channel_decimate(host_iq(x, fmt))
        assert y.shape == (nch, nout) and y.dtype == np.complex64
        e = M.excess(y, sample_values(x, fmt), h, R)
        print(f"{kind} {fmt} {shape}: |y - y64| - bound <= {e:.3e}")
        assert np.isfinite(y.view(np.float32)).all() and e <= 0.0


@pytest.mark.parametrize("fmt", FORMATS)
def test_impulse_is_the_taps_bit_for_bit(cpu, fmt):
    """x = delta[i - p], amplitude 1.0: y[m] == h[mR - p] where 0 <= mR - p < ntaps, else 0; p = 0, 1,
    R - 1, R pin the orientation and the phase, an impulse in the previous call pins the tail."""
    R, ntaps, nsamp = 4, 11, 24
    h = M.make_taps(ntaps)
    cpu.setOutputFormat(fmt, 1.0)   # CS16: code 1 at cs16_scale 1 is the value 1.0

    def expect(p, first, n):
        k = np.arange(first, first + n) * R - p
        return np.where((k >= 0) & (k < ntaps), h[np.clip(k, 0, ntaps - 1)], np.float32(0)).astype(np.float32)

    for p in (0, 1, R - 1, R):
        cpu.setChannelDecimator(h, R, 2)
        x = M.make_input("impulse", 2, nsamp, R, pos=p)
        y = cpu.channel_decimate(host_iq(x, fmt))
        for c in range(2):
            np.testing.assert_array_equal(bits(y[c].real), bits(expect(p, 0, nsamp // R)))
            np.testing.assert_array_equal(bits(y[c].imag), bits(np.zeros(nsamp // R, np.float32)))
    # the impulse in the previous call, R + 1 samples before its end (so the tail holds it)
    cpu.setChannelDecimator(h, R, 2)
    p = nsamp - R - 1
    cpu.channel_decimate(host_iq(M.make_input("impulse", 2, nsamp, R, pos=p), fmt))
    y = cpu.channel_decimate(host_iq(M.make_input("impulse", 2, nsamp, R, pos=-1), fmt))
    want = expect(p, nsamp // R, nsamp // R)
    assert np.count_nonzero(want) >= 2
    np.testing.assert_array_equal(bits(y[1].real), bits(want))


@pytest.mark.parametrize("fmt", FORMATS)
def test_cuts_are_bit_identical(cpu, fmt):
    """One call against the cuts [R, 3R, rest] and [rest, R], with ntaps - 1 > 3R: the calls shorter
    than the tail leave part of the old tail in the new one."""
    nch, R, ntaps, nout = 3, 5, 21, 40
    assert ntaps - 1 > 3 * R
    set_format(cpu, fmt)
    h = M.make_taps(ntaps)
    x = host_iq(signal("noise", nch, nout * R, R), fmt)
    cpu.setChannelDecimator(h, R, nch)
    whole = cpu.channel_decimate(x)
    assert M.excess(whole, sample_values(signal("noise", nch, nout * R, R), fmt), h, R) <= 0.0
    for cuts in ([R, 3 * R, (nout - 4) * R], [(nout - 1) * R, R]):
        cpu.setChannelDecimator(h, R, nch)
        parts, at = [], 0
        for n in cuts:
            parts.append(cpu.channel_decimate(np.ascontiguousarray(x[:, at:at + n])))
            at += n
        np.testing.assert_array_equal(bits(np.concatenate(parts, axis=1)), bits(whole))


def test_reset_equals_a_fresh_handle_and_a_repeated_set_zeroes_the_tails(cpu):
    nch, R, ntaps, nout = 2, 4, 9, 16
    h = M.make_taps(ntaps)
    x = host_iq(signal("noise", nch, nout * R, R), "CF32")
    cpu.setChannelDecimator(h, R, nch)
    first = cpu.channel_decimate(x)
    second = cpu.channel_decimate(x)
    assert not np.array_equal(bits(first), bits(second))       # the tail entered
    cpu.resetChannelDecimator()
    np.testing.assert_array_equal(bits(cpu.channel_decimate(x)), bits(first))
    cpu.setChannelDecimator(h, R, nch)                           # the same parameters
    np.testing.assert_array_equal(bits(cpu.channel_decimate(x)), bits(first))
    with R2iq(gain=1.0, device=DEVICE_CPU) as fresh:
        fresh.setChannelDecimator(h, R, nch)
        np.testing.assert_array_equal(bits(fresh.channel_decimate(x)), bits(first))


def test_channel_decimate_samples():
    assert channel_decimate_samples(8, 4096) == 512
    assert channel_decimate_samples(3, 9) == 3
    assert channel_decimate_samples(64, 64) == 1
    for factor, nsamp in ((1, 8), (65, 65), (0, 8), (-2, 8), (8, 12)):
        assert channel_decimate_samples(factor, nsamp) == 0


def test_error_returns(cpu):
    L, hd = cpu._L, cpu._h
    setd, host, dev = L.sddc_ddc_set_channel_decimator, L.sddc_ddc_channel_decimate_host, L.sddc_ddc_channel_decimate_device
    nch, R, ntaps, nsamp = 3, 4, 9, 32
    taps = M.make_taps(ntaps)
    tp = taps.ctypes.data
    x = np.ascontiguousarray(M.as_cf32(signal("noise", nch, nsamp, R), 2))       # in_stride = 2 nsamp + 2
    out = np.full((nch, 2 * (nsamp // R) + 2), np.nan, np.float32)
    xi, oi, S, OS = x.ctypes.data, out.ctypes.data, x.shape[1], out.shape[1]
    # nothing set
    assert host(hd, xi, nch, nsamp, S, oi, OS) == ERR_STATE
    assert L.sddc_ddc_channel_decimator_reset(hd) == ERR_STATE
    with pytest.raises(DDCError):
        cpu.channel_decimate(x[:, :2 * nsamp].view(np.complex64))
    # set: the ranges and the finite taps
    big = np.zeros(1025, np.float32)
    assert setd(hd, big.ctypes.data, 1025, R, nch) == ERR_ARG
    assert setd(hd, tp, ntaps, 1, nch) == ERR_ARG
    assert setd(hd, tp, ntaps, 65, nch) == ERR_ARG
    assert setd(hd, tp, ntaps, R, 0) == ERR_ARG
    assert setd(hd, tp, ntaps, R, 1025) == ERR_ARG
    assert setd(hd, tp, -1, R, nch) == ERR_ARG
    for bad in (np.nan, np.inf):
        t = taps.copy()
        t[3] = bad
        assert setd(hd, t.ctypes.data, ntaps, R, nch) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, OS) == ERR_STATE                      # a failed set sets nothing
    assert setd(hd, tp, ntaps, R, nch) == 0
    assert host(hd, xi, nch, nsamp, S, oi, OS) == 0
    good = out.copy()
    assert np.isnan(good[:, -2:]).all() and np.isfinite(good[:, :-2]).all()      # nothing between the streams
    assert setd(hd, tp, ntaps, R, nch) == 0
    # the calls
    out[:] = np.nan
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None) == ERR_STATE                 # a CPU handle has no device path
    assert host(hd, xi, nch - 1, nsamp, S, oi, OS) == ERR_STATE                  # another nch than the set one
    assert host(hd, xi, nch, 0, S, oi, OS) == ERR_ARG
    assert host(hd, xi, nch, nsamp - 1, S, oi, OS) == ERR_ARG
    assert host(hd, xi, nch, nsamp, 2 * nsamp - 2, oi, OS) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S + 1, oi, OS) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, 2 * (nsamp // R) - 2) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, OS + 1) == ERR_ARG
    assert host(hd, xi + 4, nch, nsamp, S, oi, OS) == ERR_ARG                    # CF32: 8-byte samples
    assert host(hd, xi, nch, nsamp, S, oi + 4, OS) == ERR_ARG
    assert host(hd, None, nch, nsamp, S, oi, OS) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, None, OS) == ERR_ARG
    assert np.isnan(out).all()
    # a failed call changed no state: the next valid call is the first call of the stream
    assert host(hd, xi, nch, nsamp, S, oi, OS) == 0
    np.testing.assert_array_equal(bits(out), bits(good))
    # off: the state is gone
    assert setd(hd, None, 0, 0, 0) == 0
    assert host(hd, xi, nch, nsamp, S, oi, OS) == ERR_STATE
    assert ctypes.c_size_t(L.sddc_ddc_channel_decimate_samples(R, nsamp)).value == nsamp // R
