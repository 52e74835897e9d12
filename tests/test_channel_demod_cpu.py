"""The channel demodulator on the CPU backend (no GPU): the accuracy sweeps of demod_math.h's two
routines against float64, sddc_ddc_channel_demodulate_host of a CPU handle against the float64 model
and its bounds (tools/channel_demod_model.py), the exact BFO cases, the discriminator's orientation,
the stream cut into calls, S16, the power, and the error returns of the C ABI.

The bars (u = 2^-24; sddc_ddc.h):
  angle        at most 4 ulp of the float32 nearest the true angle
  sincos_word  at most 4 u absolute per component, the rounding of the phase included
  AM           |y - y64| <= 4 u |y64|
  FM           |y - g theta64| <= |g| (4 u + 8 u |theta64|)   where |x[i]| |x[i - 1]| > 0
  BFO          |y - y64| <= |g| (|I| + |Q|) 6 u
  S16          at most 1 code from the model's value converted by the stated rule
  power        |P - P64| <= gamma_n P64, n = nsamp + 3
Shapes (nch, nsamp): those of tests/test_gpu_channel_demod.py, T the GPU kernel's tile.
"""
from __future__ import annotations

import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("channel_demod_model", os.path.join(ROOT, "tools", "channel_demod_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

from extio_sddc_amd import AUDIO_F32, AUDIO_S16, DEMOD_AM, DEMOD_BFO, DEMOD_FM  # noqa: E402
from extio_sddc_amd import CHANNEL_DEMOD_TILE as T  # noqa: E402
from extio_sddc_amd import DEVICE_CPU, DDCError, R2iq, bfo_word, kaiser  # noqa: E402
from extio_sddc_amd import _lib  # noqa: E402

U = 2.0 ** -24
CS16_SCALE = 4.0
ERR_ARG, ERR_STATE = -1, -4
FORMATS = ["CF32", "CS16"]
SHAPES = [(1, 1), (1, T + 1), (1, T - 1), (3, 2 * T + 3), (1024, 2), (2, 65)]
THREE = SHAPES[3]


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


def set_format(r, fmt):
    r.setOutputFormat(fmt, CS16_SCALE if fmt == "CS16" else 1.0)


@functools.lru_cache(maxsize=None)
def signal(kind, nch, nsamp):
    x = M.make_input(kind, nch, nsamp)
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
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chdem_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_int
    return f(r._h, pos)


def test_constants_match_the_headers():
    import re
    src = open(os.path.join(ROOT, "extio_sddc_amd", "csrc", "ddc_kernels.h")).read()
    assert int(re.search(r"constexpr int kChDemTile = (\d+);", src).group(1)) == T <= 8192
    hdr = open(os.path.join(ROOT, "include", "sddc_ddc.h")).read()
    for name, v in (("DEMOD_AM", DEMOD_AM), ("DEMOD_FM", DEMOD_FM), ("DEMOD_BFO", DEMOD_BFO), ("AUDIO_F32", AUDIO_F32),
                    ("AUDIO_S16", AUDIO_S16)):
        assert int(re.search(rf"#define SDDC_DDC_{name}\s+(\d+)", hdr).group(1)) == v
    assert (DEMOD_AM, DEMOD_FM, DEMOD_BFO, AUDIO_F32, AUDIO_S16) == (0, 1, 2, 0, 1)
    assert re.search(r"#define SDDC_DDC_ABI_VERSION 3\b", hdr)


def test_bfo_word():
    assert bfo_word(0.0) == 0 and bfo_word(0.25) == 2 ** 30 and bfo_word(-0.25) == 3 * 2 ** 30
    assert bfo_word(-0.5) == 2 ** 31 and bfo_word(2.0 ** -32) == 1 and bfo_word(-2.0 ** -32) == 2 ** 32 - 1
    assert bfo_word(0.1) == round(0.1 * 2 ** 32)


def test_angle_sweep_against_float64():
    """2^22 + 1 ratios t = k / 2^22 in [0, 1] in all eight octants at seeded magnitudes, the axes and
    (0, 0): at most 4 ulp of the float32 nearest the true angle."""
    f = _lib.load().sddc_ddc_internal_demod_angle
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int
    n = 2 ** 22 + 1
    t = (np.arange(n, dtype=np.float64) / 2 ** 22).astype(np.float32)
    mag = np.exp2(np.random.default_rng(11).uniform(-30, 30, n)).astype(np.float32)
    big, small = mag, (mag * t).astype(np.float32)
    worst = 0.0
    for octant in range(8):
        re, im = (small, big) if octant & 1 else (big, small)
        re = -re if octant & 2 else re
        im = -im if octant & 4 else im
        keep = (im != 0) | (octant & 4 == 0)   # -0 on the axis is read as +0: angle(-0, -1) = +pi
        re, im = np.ascontiguousarray(re[keep]), np.ascontiguousarray(im[keep])
        out = np.empty(re.size, np.float32)
        assert f(im.ctypes.data, re.ctypes.data, re.size, out.ctypes.data) == 0
        ref = np.arctan2(im.astype(np.float64), re.astype(np.float64))
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        nz = ref != 0
        assert (out[~nz] == 0).all()
        worst = max(worst, float((np.abs(out.astype(np.float64) - ref)[nz] / ulp[nz]).max()))
    print(f"angle: worst error {worst:.3f} ulp")
    assert worst <= 4.0
    # the axes and the origin, bit for bit where float32 has the value
    re = np.array([1, 0, -1, 0, 0, 3e-30, 0], np.float32)
    im = np.array([0, 1, 0, -1, 0, 0, 2e30], np.float32)
    out = np.empty(re.size, np.float32)
    assert f(im.ctypes.data, re.ctypes.data, re.size, out.ctypes.data) == 0
    want = np.array([0, np.pi / 2, np.pi, -np.pi / 2, 0, 0, np.pi / 2], np.float32)
    assert (np.abs(out.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
    assert bits(out[[0, 4, 5]]).tolist() == [0, 0, 0]   # +0.0f


def test_sincos_sweep_against_float64():
    """2^22 words spread over the circle by an odd stride, 2^16 seeded ones, and every multiple of
    2^29: at most 4 u per component; the quarter cycles exact with +0 for the zero."""
    f = _lib.load().sddc_ddc_internal_demod_sincos
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    w = np.concatenate([(np.arange(2 ** 22, dtype=np.uint64) * 1023 + 511) & 0xffffffff,
                        np.random.default_rng(12).integers(0, 2 ** 32, 2 ** 16, dtype=np.uint64),
                        np.arange(8, dtype=np.uint64) << 29]).astype(np.uint32)
    c, s = np.empty(w.size, np.float32), np.empty(w.size, np.float32)
    assert f(w.ctypes.data, w.size, c.ctypes.data, s.ctypes.data) == 0
    ph = 2.0 * np.pi * w.astype(np.float64) / 2.0 ** 32
    worst = max(np.abs(c - np.cos(ph)).max(), np.abs(s - np.sin(ph)).max()) / U
    print(f"sincos_word: worst error {worst:.3f} u")
    assert worst <= 4.0
    r = np.float32(np.sqrt(0.5))
    want_c = np.array([1, r, 0, -r, -1, -r, 0, r], np.float32)
    want_s = np.array([0, r, 1, r, 0, -r, -1, -r], np.float32)
    assert (np.abs(c[-8:] - want_c) <= 4 * U).all() and (np.abs(s[-8:] - want_s) <= 4 * U).all()
    for k in (0, 2, 4, 6):
        assert bits(c[-8 + k]) == bits(want_c[k]) and bits(s[-8 + k]) == bits(want_s[k])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bounds_on_a_cpu_handle(cpu, shape, fmt):
    nch, nsamp = shape
    set_format(cpu, fmt)
    m, g, w = M.channel_params(nch)
    for kind in ("noise", "edges"):
        x = signal(kind, nch, nsamp)
        xv = sample_values(x, fmt)
        cpu.setChannelDemodulator(m, g, w)
        y, p = cpu.channel_demodulate(host_iq(x, fmt), power=True)
        e = M.excess(y, xv, m, g, w)
        pe = float((np.abs(p - M.power(xv)) - M.power_bound(xv)).max())
        print(f"{kind} {fmt} {shape}: |y - y64| - bound <= {e:.3e}, |P - P64| - bound <= {pe:.3e}")
        assert np.isfinite(y).all() and e <= 0.0 and pe <= 0.0
        # S16: at most one code from the model's value, none where the F32 result is the CPU backend's own
        cpu.setChannelDemodulator(m, g, w, AUDIO_S16)
        ys = cpu.channel_demodulate(host_iq(x, fmt))
        assert ys.dtype == np.int16
        ref = M.demodulate(xv, m, g, w)[0]
        ok = np.isfinite(M.bound(xv, m, g, w))
        assert (np.abs(ys.astype(np.int32) - M.to_s16(ref).astype(np.int32))[ok] <= 1).all()
        np.testing.assert_array_equal(ys, M.to_s16(y))
        assert np.abs(ys).max() < M.S16_POISON


def test_exact_bfo_sequences_and_the_position(cpu):
    """w = 0: y = g I; w = 2^30: g I, -g Q, -g I, g Q, across a call boundary and across the 2^32 wrap
    of the position."""
    nsamp = 37
    x = signal("noise", 2, nsamp)
    I, Q = x.real.astype(np.float32), x.imag.astype(np.float32)
    g = np.array([1.5, -0.75], np.float32)
    for fmt_x in (host_iq(x, "CF32"),):
        cpu.setChannelDemodulator([DEMOD_BFO] * 2, g, [0, 0])
        np.testing.assert_array_equal(cpu.channel_demodulate(fmt_x), g[:, None] * I)
        seq = np.stack([I, -Q, -I, Q])
        for pos in (0, 1, 2, 3, 2 ** 32 - 5, 2 ** 32 - 18):
            want = g[:, None] * np.stack([seq[(pos + i) % 4, :, i] for i in range(nsamp)], axis=1)
            cpu.setChannelDemodulator([DEMOD_BFO] * 2, g, [2 ** 30] * 2)
            assert set_position(cpu, pos) == 0
            np.testing.assert_array_equal(cpu.channel_demodulate(fmt_x), want)
            # the same in two calls: the position is carried over the boundary (and the wrap)
            cpu.setChannelDemodulator([DEMOD_BFO] * 2, g, [2 ** 30] * 2)
            assert set_position(cpu, pos) == 0
            two = np.concatenate([cpu.channel_demodulate(fmt_x[:, :9]), cpu.channel_demodulate(fmt_x[:, 9:])], axis=1)
            np.testing.assert_array_equal(two, want)
    # a general word next to the wrap against the model
    w = [bfo_word(0.1234), bfo_word(-0.31)]
    cpu.setChannelDemodulator([DEMOD_BFO] * 2, g, w)
    assert set_position(cpu, 2 ** 32 - 11) == 0
    y = cpu.channel_demodulate(host_iq(x, "CF32"))
    assert M.excess(y, M.values(x), [DEMOD_BFO] * 2, g, w, pos=2 ** 32 - 11) <= 0.0
    cpu.setChannelDemodulator(None)
    assert set_position(cpu, 0) == ERR_STATE


def test_discriminator_reads_the_tone_frequency_and_its_sign(cpu):
    """A e^{j 2 pi f i} reads g 2 pi f within the bound, its conjugate the negative; y[0] = 0 after a set."""
    n, f, A, g = 500, 0.0371, 9000.0, np.float32(3.0)
    x = (A * np.exp(2j * np.pi * f * np.arange(n))).astype(np.complex64).reshape(1, n)
    for sign, xx in ((1.0, x), (-1.0, np.conj(x))):
        cpu.setChannelDemodulator([DEMOD_FM], [g])
        y = cpu.channel_demodulate(xx)
        assert bits(y[0, :1]).tolist() == [0]
        assert M.excess(y, M.values(xx), [DEMOD_FM], [g], [0]) <= 0.0
        want = sign * float(g) * 2 * np.pi * f
        # float32 samples of amplitude A move each angle by at most 2 u sqrt(2) beyond the bound's own terms
        assert (np.abs(y[0, 1:] - want) <= float(g) * (8 * U + 8 * U * abs(want) / float(g))).all()
        assert np.sign(y[0, 1:]).tolist() == [sign] * (n - 1)


@pytest.mark.parametrize("out_fmt", [AUDIO_F32, AUDIO_S16])
@pytest.mark.parametrize("fmt", FORMATS)
def test_cuts_are_bit_identical(cpu, fmt, out_fmt):
    nch, nsamp = THREE
    set_format(cpu, fmt)
    m, g, w = M.channel_params(nch)
    iq = host_iq(signal("noise", nch, nsamp), fmt)
    cpu.setChannelDemodulator(m, g, w, out_fmt)
    whole = cpu.channel_demodulate(iq)
    cpu.setChannelDemodulator(m, g, w, out_fmt)
    parts = [cpu.channel_demodulate(iq[:, a:b]) for a, b in ((0, 1), (1, 4), (4, nsamp))]
    np.testing.assert_array_equal(bits(np.concatenate(parts, axis=1)), bits(whole))
    cpu.resetChannelDemodulator()
    parts = [cpu.channel_demodulate(iq[:, i:i + 1]) for i in range(64)]
    np.testing.assert_array_equal(bits(np.concatenate(parts, axis=1)), bits(whole[:, :64]))


def test_s16_rounding_clamping_and_nan(cpu):
    """BFO with w = 0 and g = 1 passes I through: ties to even, the clamps, infinities and NaN."""
    I = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, 32766.5, 32767.5, 1e9, -32768.5, -1e9, np.inf, -np.inf,
                  np.nan, 12345.678], np.float32)
    x = (I + 0j).astype(np.complex64).reshape(1, -1)
    cpu.setChannelDemodulator([DEMOD_BFO], None, None, AUDIO_S16)
    y = cpu.channel_demodulate(x)
    assert y[0].tolist() == [0, 2, 2, 0, -2, -2, 0, 32766, 32767, 32767, -32768, -32768, 32767, -32768, 0, 12346]
    np.testing.assert_array_equal(y[0], M.to_s16(I))


def test_power_is_per_call_and_deterministic(cpu):
    nch, nsamp = THREE
    x = signal("edges", nch, nsamp)
    m, g, w = M.channel_params(nch)
    cpu.setChannelDemodulator(m, g, w)
    _, p1 = cpu.channel_demodulate(host_iq(x, "CF32"), power=True)
    _, p2 = cpu.channel_demodulate(host_iq(x, "CF32"), power=True)
    np.testing.assert_array_equal(bits(p1), bits(p2))
    assert (np.abs(p1 - M.power(M.values(x))) <= M.power_bound(M.values(x))).all()
    _, ph = cpu.channel_demodulate(host_iq(x[:, :100], "CF32"), power=True)
    assert (np.abs(ph - M.power(M.values(x[:, :100]))) <= M.power_bound(M.values(x[:, :100]))).all()


def test_error_returns_and_a_failed_call_changes_no_state(cpu):
    L, hd = cpu._L, cpu._h
    setd, host, dev = L.sddc_ddc_set_channel_demodulator, L.sddc_ddc_channel_demodulate_host, L.sddc_ddc_channel_demodulate_device
    nch, nsamp = 3, 40
    m, g, w = M.channel_params(nch)
    mp, gp, wp = m.ctypes.data, g.ctypes.data, w.ctypes.data
    x = np.ascontiguousarray(M.as_cf32(signal("noise", nch, nsamp), 2, np.nan))
    S = x.shape[1]
    out = np.full((nch, nsamp + 1), np.nan, np.float32)
    pw = np.full(nch, np.nan, np.float32)
    xi, oi, OS = x.ctypes.data, out.ctypes.data, out.shape[1]
    assert host(hd, xi, nch, nsamp, S, oi, OS, None) == ERR_STATE                  # nothing set
    assert L.sddc_ddc_channel_demodulator_reset(hd) == ERR_STATE
    with pytest.raises(DDCError):
        cpu.channel_demodulate(x.view(np.complex64))
    bad = m.copy()
    bad[1] = 3
    assert setd(hd, bad.ctypes.data, gp, wp, nch, AUDIO_F32) == ERR_ARG
    bad[1] = -1
    assert setd(hd, bad.ctypes.data, gp, wp, nch, AUDIO_F32) == ERR_ARG
    for v in (np.inf, np.nan):
        gb = g.copy()
        gb[2] = v
        assert setd(hd, mp, gb.ctypes.data, wp, nch, AUDIO_F32) == ERR_ARG
    assert setd(hd, mp, gp, wp, -1, AUDIO_F32) == ERR_ARG
    assert setd(hd, mp, gp, wp, 1025, AUDIO_F32) == ERR_ARG
    assert setd(hd, mp, gp, wp, nch, 2) == ERR_ARG
    assert setd(hd, mp, gp, wp, nch, -1) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, OS, None) == ERR_STATE                  # a failed set sets nothing
    with pytest.raises(DDCError):
        cpu.setChannelDemodulator(m, g[:2], w)
    cpu.setChannelDemodulator(m, g, w)
    assert host(hd, xi, nch, nsamp, S, oi, OS, pw.ctypes.data) == 0
    good, good_p = out.copy(), pw.copy()
    assert np.isnan(good[:, nsamp:]).all() and np.isfinite(good[:, :nsamp]).all()
    cpu.setChannelDemodulator(m, g, w)
    out[:] = np.nan
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None, None) == ERR_STATE             # a CPU handle has no device path
    assert host(hd, xi, nch - 1, nsamp, S, oi, OS, None) == ERR_STATE              # another nch than the set one
    assert host(hd, xi, nch, 0, S, oi, OS, None) == ERR_ARG
    assert host(hd, xi, nch, 2 ** 40 + 1, 2 ** 42, oi, 2 ** 41, None) == ERR_ARG
    assert host(hd, xi, nch, nsamp, 2 * nsamp - 2, oi, OS, None) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S + 1, oi, OS, None) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, nsamp - 1, None) == ERR_ARG
    assert host(hd, xi + 4, nch, nsamp, S, oi, OS, None) == ERR_ARG                # CF32: 8-byte samples
    assert host(hd, xi, nch, nsamp, S, oi + 2, OS, None) == ERR_ARG                # F32: 4-byte outputs
    assert host(hd, xi, nch, nsamp, S, oi, OS, pw.ctypes.data + 2) == ERR_ARG
    assert host(hd, None, nch, nsamp, S, oi, OS, None) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, None, OS, None) == ERR_ARG
    assert np.isnan(out).all()
    # the failed calls changed no state: the next valid call is the first call of the stream
    assert host(hd, xi, nch, nsamp, S, oi, OS, pw.ctypes.data) == 0
    np.testing.assert_array_equal(bits(out), bits(good))
    np.testing.assert_array_equal(bits(pw), bits(good_p))
    # an odd out_stride and a 2-byte aligned S16 output
    cpu.setChannelDemodulator(m, g, w, AUDIO_S16)
    o16 = np.full(1 + nch * (nsamp + 1), M.S16_POISON, np.int16)
    assert host(hd, xi, nch, nsamp, S, o16.ctypes.data + 2, nsamp + 1, None) == 0
    body = o16[1:].reshape(nch, nsamp + 1)
    assert o16[0] == M.S16_POISON and (body[:, nsamp] == M.S16_POISON).all()
    np.testing.assert_array_equal(body[:, :nsamp], M.to_s16(good[:, :nsamp]))
    cpu.setChannelDemodulator(None)
    assert host(hd, xi, nch, nsamp, S, oi, OS, None) == ERR_STATE


def test_the_three_stages_on_one_handle_keep_independent_states(cpu):
    """Decimator, resampler and demodulator set together: each stream equals the one of a handle that
    has that stage alone, call by call, and a reset of one leaves the others' streams running."""
    nch, n = 2, 240
    x = host_iq(signal("noise", nch, 2 * n), "CF32")
    h = kaiser(33, 60.0, 0.05, 0.125)
    m, g, w = M.channel_params(nch, [DEMOD_FM, DEMOD_BFO])

    def alone(setup, call):
        with R2iq(gain=1.0, device=DEVICE_CPU) as r:
            setup(r)
            return [call(r, x[:, :n]), call(r, x[:, n:])]

    dec = alone(lambda r: r.setChannelDecimator(h, 4, nch), lambda r, v: r.channel_decimate(v))
    res = alone(lambda r: r.setChannelResampler(3 * h, 3, 5, nch), lambda r, v: r.channel_resample(v))
    dem = alone(lambda r: r.setChannelDemodulator(m, g, w), lambda r, v: r.channel_demodulate(v))
    cpu.setChannelDecimator(h, 4, nch)
    cpu.setChannelResampler(3 * h, 3, 5, nch)
    cpu.setChannelDemodulator(m, g, w)
    for k, v in enumerate((x[:, :n], x[:, n:])):
        np.testing.assert_array_equal(cpu.channel_demodulate(v), dem[k])
        np.testing.assert_array_equal(cpu.channel_decimate(v), dec[k])
        np.testing.assert_array_equal(cpu.channel_resample(v), res[k])
        if k == 0:
            cpu.resetChannelDecimator()
            cpu.setChannelDecimator(h, 4, nch)
            cpu.channel_decimate(x[:, :n])
    cpu.resetChannelDemodulator()
    np.testing.assert_array_equal(cpu.channel_demodulate(x[:, :n]), dem[0])
