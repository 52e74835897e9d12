"""The channel resampler on the CPU backend (no GPU): the float64 model (tools/channel_resample_model.py)
against the literal definition, sddc_ddc_resample_count against a brute-force count, and
sddc_ddc_channel_resample_host of a CPU handle against the model and its derived bound, the stream
cut into calls, the impulse response bit for bit, the decimator at L = 1, the bank model against the
launch's layout, and the error returns of the C ABI.

The bar: every output component within gamma sum_j |h[p + jL]| |x[s - j]|, gamma = n u / (1 - n u),
n = K + 1, K = ceil(ntaps / L), u = 2^-24, computed per output from the model's own sum.
Pairs (L, M, ntaps): (2, 3, 1), (3, 2, 7), (6, 125, 259), (4, 1, 16), (1, 8, 65).
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


RM = _load("channel_resample_model")
DM = _load("channel_decimate_model")
B = _load("channel_resample_banks")

from extio_sddc_amd import DEVICE_CPU, DDCError, R2iq, resample_count  # noqa: E402
import extio_sddc_amd as pkg  # noqa: E402

CS16_SCALE = 4.0
ERR_ARG, ERR_STATE = -1, -4
FORMATS = ["CF32", "CS16"]
PAIRS = [(2, 3, 1), (3, 2, 7), (6, 125, 259), (4, 1, 16), (1, 8, 65)]
# (nch, L, M, ntaps, nsamp): a few hundred outputs at most, nsamp no multiple of M
SHAPES = [(1, 2, 3, 1, 8), (1, 3, 2, 7, 301), (3, 6, 125, 259, 5003), (2, 3, 250, 3072, 3001), (1, 32, 255, 4096, 2001),
          (1, 4, 1, 16, 97), (2, 1, 8, 65, 1029)]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


def set_format(r, fmt):
    r.setOutputFormat(fmt, CS16_SCALE if fmt == "CS16" else 1.0)


@functools.lru_cache(maxsize=None)
def signal(kind, nch, nsamp):
    x = RM.make_input(kind, nch, nsamp)
    x.setflags(write=False)
    return x


def host_iq(x, fmt):
    if fmt == "CS16":
        return RM.as_cs16(x).reshape(x.shape[0], x.shape[1], 2)
    return RM.as_cf32(x).view(np.complex64)


def sample_values(x, fmt):
    """What the backend reads: the float32 values of the model's input in this format."""
    return RM.cs16_values(RM.as_cs16(x), CS16_SCALE) if fmt == "CS16" else RM.values(x)


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def run_cuts(r, x, fmt, cuts):
    """The stream x in calls of `cuts` samples -> complex64 [nch, total outputs]."""
    assert sum(cuts) == x.shape[1]
    iq, at, outs = host_iq(x, fmt), 0, []
    for n in cuts:
        want = r.channel_resample_samples(n)
        y = r.channel_resample(np.ascontiguousarray(iq[:, at:at + n]))
        assert y.shape == (x.shape[0], want)
        outs.append(y)
        at += n
    return np.concatenate(outs, axis=1)


def literal(x, h, L, M):
    """The definition, word for word: zero-stuff by L, convolve, keep every M-th sample that the
    consumed samples determine (n = mM <= (nsamp - 1) L + L - 1)."""
    nsamp = x.size
    u = np.zeros(nsamp * L, np.complex128)
    u[::L] = x
    v = np.convolve(u, h.astype(np.float64))[:nsamp * L]
    return v[::M]


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_model_against_the_literal_definition(pair):
    L, M, ntaps = pair
    h = RM.make_taps(ntaps)
    for nsamp in (1, 2, M, 3 * M + 1, 401):
        x = RM.values(RM.make_input("noise", 2, nsamp))
        y = RM.resample(x, h, L, M)
        assert y.shape == (2, -(-nsamp * L // M))
        for c in range(2):
            ref = literal(x[c], h, L, M)
            assert ref.shape == y[c].shape
            scale = np.abs(h).sum() * np.abs(x[c]).max()
            assert np.abs(y[c] - ref).max() <= 1e-13 * scale


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_count_against_brute_force(pair):
    L, M, _ = pair
    zeros = 0
    for n0 in range(2 * M):
        for nsamp in range(1, 3 * M + 1):
            # output m exists once sample floor(m M / L) is consumed
            brute = sum(1 for m in range((n0 + nsamp) * L // M + 2) if n0 <= (m * M) // L < n0 + nsamp)
            assert resample_count(L, M, n0, nsamp) == brute == RM.count(L, M, n0, nsamp), (n0, nsamp)
            zeros += brute == 0
    assert (zeros > 0) == (M > L)
    # far out: only the position modulo M counts
    for n0 in (0, 1, M - 1):
        assert resample_count(L, M, n0 + (2 ** 40) * M, 3 * M + 1) == RM.count(L, M, n0, 3 * M + 1)
    assert resample_count(L, M, 2 ** 64 - 1, 7) == RM.count(L, M, 2 ** 64 - 1, 7)
    for bad in ((0, 3), (33, 2), (3, 0), (3, 257), (2, 4), (6, 9), (1, 1)):
        assert resample_count(bad[0], bad[1], 0, 100) == 0


def test_limits_match_the_headers():
    import re
    src = open(os.path.join(ROOT, "include", "sddc_ddc.h")).read()
    for name, val in (("MAX_UP", pkg.CHANNEL_RESAMPLE_MAX_UP), ("MAX_DOWN", pkg.CHANNEL_RESAMPLE_MAX_DOWN),
                      ("MAX_TAPS", pkg.CHANNEL_RESAMPLE_MAX_TAPS), ("MAX_PHASE_TAPS", pkg.CHANNEL_RESAMPLE_MAX_PHASE_TAPS)):
        assert int(re.search(r"#define SDDC_DDC_RESAMPLE_%s\s+(\d+)" % name, src).group(1)) == val


def test_lds_layout_model():
    """tools/channel_resample_banks.py against the launch's own layout: the same tile and pitch, the
    tile inside the LDS with the halo's columns and the last tile's extra one, conflict-free reads
    for every pitch picked (the direct layout: for an odd M alone)."""
    f = pkg._lib.load().sddc_ddc_internal_chres_layout
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)] * 3
    tile, pitch, cost = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cases = [s[1:4] for s in SHAPES] + [(12, 125, 1536), (6, 125, 1536), (1, 16, 129), (1, 256, 1024), (31, 256, 4096),
                                        (32, 1, 4096), (1, 2, 1)]
    for L, M, ntaps in cases:
        K = -(-ntaps // L)
        for cs16 in (0, 1):
            assert f(L, M, ntaps, cs16, ctypes.byref(tile), ctypes.byref(pitch), ctypes.byref(cost)) == 0
            assert (tile.value, pitch.value, cost.value) == B.layout(L, M, ntaps, cs16), (L, M, ntaps, cs16)
            ta = tile.value // L
            assert tile.value == ta * L and 1 <= ta <= B.MAXA and pitch.value * M <= B.LDS
            assert pitch.value >= ta + (K - 1 + M - 1) // M + 1
            assert B.read_conflicts(M, pitch.value, K) == 0
    # the direct layout (slot s) reads conflict-free for an odd M alone
    assert B.read_conflicts(125, 0, 128, transposed=False) == 0
    assert B.read_conflicts(250, 0, 1024, transposed=False) == 2 and B.read_conflicts(16, 0, 129, transposed=False) == 30
    for bad in ((0, 3, 8), (2, 4, 8), (1, 1, 8), (3, 2, 0), (3, 2, 4097), (1, 2, 1025)):
        assert f(*bad, 0, ctypes.byref(tile), ctypes.byref(pitch), ctypes.byref(cost)) == ERR_ARG


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bound(cpu, shape, fmt):
    nch, L, M, ntaps, nsamp = shape
    set_format(cpu, fmt)
    h = RM.make_taps(ntaps)
    for kind in ("noise", "edges"):
        cpu.setChannelResampler(h, L, M, nch)
        x = signal(kind, nch, nsamp)
        y = cpu.channel_resample(host_iq(x, fmt))
        assert y.shape == (nch, RM.count(L, M, 0, nsamp)) and y.shape[1] > 0
        e = RM.excess(y, sample_values(x, fmt), h, L, M)
        print(f"{kind} {fmt} {shape}: |y - y64| - bound <= {e:.3e}")
        assert np.isfinite(y.view(np.float32)).all() and e <= 0.0
    if (L, M, ntaps) == (2, 3, 1):   # phase 1 has no tap: outputs 1, 3, .. (m M mod L = 1) are 0
        assert (y[:, 1::2] == 0).all() and (y[:, 0::2] != 0).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[1]], ids=IDS)
def test_cuts_are_bit_identical(cpu, shape, fmt):
    nch, L, M, ntaps, nsamp = shape
    K = -(-ntaps // L)
    set_format(cpu, fmt)
    h = RM.make_taps(ntaps)
    x = signal("noise", nch, nsamp)
    cpu.setChannelResampler(h, L, M, nch)
    whole = run_cuts(cpu, x, fmt, [nsamp])
    assert RM.excess(whole, sample_values(x, fmt), h, L, M) <= 0.0
    # single-sample calls on the stream's first samples (the same path for every later one)
    few = min(nsamp, 2 * M + K + 3)
    nfew = RM.count(L, M, 0, few)
    cpu.setChannelResampler(h, L, M, nch)
    np.testing.assert_array_equal(bits(run_cuts(cpu, x[:, :few], fmt, [1] * few)), bits(whole[:, :nfew]))
    # cuts shorter than K - 1, then the rest
    short = max(1, (K - 1) // 3)
    cuts = [short, 1, short + 1, max(1, K - 2)]
    cuts.append(nsamp - sum(cuts))
    cpu.resetChannelResampler()
    np.testing.assert_array_equal(bits(run_cuts(cpu, x, fmt, cuts)), bits(whole))
    # seeded random cuts
    rng = np.random.default_rng(5)
    for _ in range(2):
        marks = np.sort(rng.choice(np.arange(1, nsamp), 6, replace=False))
        cuts = np.diff(np.concatenate([[0], marks, [nsamp]])).tolist()
        cpu.resetChannelResampler()
        np.testing.assert_array_equal(bits(run_cuts(cpu, x, fmt, cuts)), bits(whole))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("pair", PAIRS + [(3, 250, 3072)], ids=IDS)
def test_impulse_is_the_taps_bit_for_bit(cpu, pair, fmt):
    """x = delta[i], amplitude 1.0: y[m] == h[mM] while mM < ntaps, 0 beyond; the same with the
    impulse in a first call of one sample."""
    L, M, ntaps = pair
    h = RM.make_taps(ntaps)
    cpu.setOutputFormat(fmt, 1.0)   # CS16: code 1 at cs16_scale 1 is the value 1.0
    nsamp = -(-ntaps // L) + 2 * M + 3
    nout = RM.count(L, M, 0, nsamp)
    k = np.arange(nout) * M
    want = np.where(k < ntaps, h[np.clip(k, 0, ntaps - 1)], np.float32(0)).astype(np.float32)
    assert np.count_nonzero(want) == -(-ntaps // M) and (nout - 1) * M >= ntaps
    x = RM.make_input("impulse", 2, nsamp, pos=0)
    for cuts in ([nsamp], [1, nsamp - 1]):
        cpu.setChannelResampler(h, L, M, 2)
        y = run_cuts(cpu, x, fmt, cuts)
        for c in range(2):
            np.testing.assert_array_equal(bits(y[c].real), bits(want))
            np.testing.assert_array_equal(bits(y[c].imag), bits(np.zeros(nout, np.float32)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_l1_equals_the_decimator_within_the_two_bounds(cpu, fmt):
    nch, R, ntaps, nsamp = 2, 8, 65, 1024
    set_format(cpu, fmt)
    h = RM.make_taps(ntaps)
    x = signal("noise", nch, nsamp)
    cpu.setChannelResampler(h, 1, R, nch)
    cpu.setChannelDecimator(h, R, nch)
    yr = cpu.channel_resample(host_iq(x, fmt))
    yd = cpu.channel_decimate(host_iq(x, fmt))
    assert yr.shape == yd.shape == (nch, nsamp // R)
    xv = sample_values(x, fmt)
    rr, ri = RM.bound(xv, h, 1, R)
    dr, di = DM.bound(xv, h, R)
    d = yr.astype(np.complex128) - yd.astype(np.complex128)
    assert (np.abs(d.real) <= rr + dr).all() and (np.abs(d.imag) <= ri + di).all()
    assert RM.excess(yr, xv, h, 1, R) <= 0.0


def test_error_returns_and_a_failed_call_changes_no_state(cpu):
    L_, hd = cpu._L, cpu._h
    sets, host = L_.sddc_ddc_set_channel_resampler, L_.sddc_ddc_channel_resample_host
    nch, L, M, ntaps, nsamp = 3, 3, 7, 20, 40
    taps = RM.make_taps(ntaps)
    tp = taps.ctypes.data
    x = signal("noise", nch, nsamp)
    xs = np.ascontiguousarray(RM.as_cf32(x, 2, np.nan))
    S, nout = xs.shape[1], RM.count(L, M, 0, nsamp)
    out = np.full((nch, 2 * nout + 2), np.nan, np.float32)
    OS = out.shape[1]
    xi, oi = xs.ctypes.data, out.ctypes.data
    got = ctypes.c_size_t(99)
    gp = ctypes.addressof(got)
    assert host(hd, xi, nch, nsamp, S, oi, OS, gp) == ERR_STATE                 # nothing set
    assert L_.sddc_ddc_channel_resampler_reset(hd) == ERR_STATE
    assert cpu.channel_resample_samples(nsamp) == 0
    with pytest.raises(DDCError):
        cpu.channel_resample(host_iq(x, "CF32"))
    big = np.zeros(4097, np.float32)
    assert sets(hd, big.ctypes.data, 4097, L, M, nch) == ERR_ARG
    assert sets(hd, big.ctypes.data, 1025, 1, 2, nch) == ERR_ARG                # K = 1025
    assert sets(hd, big.ctypes.data, 1024, 1, 2, nch) == 0
    for up, down in ((0, M), (33, M), (L, 0), (L, 257), (2, 4), (6, 9), (1, 1)):
        assert sets(hd, tp, ntaps, up, down, nch) == ERR_ARG
    assert sets(hd, tp, ntaps, L, M, 0) == ERR_ARG
    assert sets(hd, tp, ntaps, L, M, 1025) == ERR_ARG
    t = taps.copy()
    t[ntaps - 1] = np.nan
    assert sets(hd, t.ctypes.data, ntaps, L, M, nch) == ERR_ARG
    cpu.setChannelResampler(None)
    assert host(hd, xi, nch, nsamp, S, oi, OS, gp) == ERR_STATE                 # off again
    cpu.setChannelResampler(taps, L, M, nch)
    good = cpu.channel_resample(host_iq(x, "CF32"))
    cpu.setChannelResampler(taps, L, M, nch)
    assert host(hd, xi, nch - 1, nsamp, S, oi, OS, gp) == ERR_STATE             # another nch than the set one
    assert host(hd, xi, nch, 0, S, oi, OS, gp) == ERR_ARG
    assert host(hd, xi, nch, nsamp, 2 * nsamp - 2, oi, OS, gp) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S + 1, oi, OS, gp) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, 2 * nout - 2, gp) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, OS + 1, gp) == ERR_ARG
    assert host(hd, xi + 4, nch, nsamp, S, oi, OS, gp) == ERR_ARG               # CF32: 8-byte samples
    assert host(hd, xi, nch, nsamp, S, oi + 4, OS, gp) == ERR_ARG
    assert host(hd, None, nch, nsamp, S, oi, OS, gp) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, None, OS, gp) == ERR_ARG
    assert got.value == 99 and np.isnan(out).all()
    # the failed calls changed no state: the next valid call is the first call of the stream
    assert cpu.channel_resample_samples(nsamp) == nout
    assert host(hd, xi, nch, nsamp, S, oi, OS, gp) == 0 and got.value == nout
    assert np.isnan(out[:, 2 * nout:]).all()
    np.testing.assert_array_equal(bits(out[:, :2 * nout]), bits(good).reshape(nch, 2 * nout))
    # a call without an output is legal, writes nothing and advances the stream
    cpu.setChannelResampler(taps, L, M, nch)
    out[:] = np.nan
    assert host(hd, xi, nch, 1, S, oi, OS, gp) == 0 and got.value == 1          # output 0 needs sample 0 alone
    assert cpu.channel_resample_samples(1) == 0                                 # output 1 needs sample 2
    out[:] = np.nan
    assert host(hd, xi + 8, nch, 1, S, oi, OS, None) == 0 and np.isnan(out).all()
    assert cpu.channel_resample_samples(1) == 1
    cpu.resetChannelResampler()
    assert cpu.channel_resample_samples(nsamp) == nout
