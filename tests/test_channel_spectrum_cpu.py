"""The channel spectrum without a GPU: the C ABI's new symbols, the n-point windows, the argument
checks and the CPU backend (sddc_ddc_channel_spectrum_host on a CPU handle) against the float64
statement of the definition, tools/channel_spectrum_model.py.

Parity bar (the project's, tests/test_gpu_spectrum.py): per row max_q |psd - model| / max_q model
<= 1e-5.  On the two-tone input with a Hann or Blackman-Harris window the weak tone (80 dB below
the strong one) must read within 0.05 dB of the model, and the quiet bins away from both tones
must stay below the model's highest quiet bin plus the model's own peak-over-mean there (both taken
from the model in the test); that bound must itself lie 20 dB under the weak tone, which a window
that is not applied misses by far.
Shapes (nch, nrows, fpr, hop): (1, 1, 1, n), (3, 2, 3, n/2), (2, 5, 2, n/4 + 1), (1, 2, 2, 2n).
CS16 runs with cs16_scale 4: the samples enter as integers and 1/16 goes into the final scale.
"""
from __future__ import annotations

import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("channel_spectrum_model",
                                               os.path.join(ROOT, "tools", "channel_spectrum_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

TOL = 1e-5
SYMBOLS = ["sddc_ddc_window", "sddc_ddc_set_channel_spectrum_window", "sddc_ddc_channel_spectrum_device",
           "sddc_ddc_channel_spectrum_host"]
INPUTS = ["noise", "twotone", "edges"]
WINDOWS = ["rect", "hann", "blackman_harris"]
FORMATS = ["CF32", "CS16"]
CS16_SCALE = 4.0
ERR_ARG, ERR_STATE = -1, -4


def shapes(n):
    return [(1, 1, 1, n), (3, 2, 3, n // 2), (2, 5, 2, n // 4 + 1), (1, 2, 2, 2 * n)]


@functools.lru_cache(maxsize=None)
def signal(kind, n, nch, nsamp):
    x = M.make_input(kind, n, nch, nsamp)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def lib_window(kind, n):
    from extio_sddc_amd import window
    w = window(kind, n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(kind, win, n, nch, nrows, fpr, hop):
    x = signal(kind, n, nch, M.nsamp_for(n, hop, fpr, nrows))
    ref = M.psd(x, n, hop, fpr, nrows, None if win == "rect" else lib_window(win, n))
    ref.setflags(write=False)
    return ref


def row_errors(psd, ref):
    return (np.abs(psd.astype(np.float64) - ref).max(axis=-1) / ref.max(axis=-1)).reshape(-1)


def host_iq(x, fmt):
    """The array R2iq.channel_spectrum takes; the reference's scale for it."""
    if fmt == "CS16":
        return M.as_cs16(x).reshape(x.shape[0], x.shape[1], 2), 1.0 / CS16_SCALE ** 2
    return M.as_cf32(x).view(np.complex64), 1.0


def set_format(r, fmt):
    r.setOutputFormat(fmt, CS16_SCALE if fmt == "CS16" else 1.0)


def set_window(r, win, n):
    r.setChannelSpectrumWindow(None if win == "rect" else lib_window(win, n))


@pytest.fixture(scope="module")
def cpu(ddc_lib):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


def test_header_declares_and_library_exports_the_symbols(ddc_lib):
    import subprocess
    from extio_sddc_amd._lib import LIB_PATH, SIGNATURES
    with open(os.path.join(ROOT, "include", "sddc_ddc.h")) as f:
        hdr = f.read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (sddc_ddc_\w+)", out))
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), f"{s} is not declared"
        assert s in exported, f"{s} is not exported"
        assert s in SIGNATURES and hasattr(ddc_lib, s)
    assert ddc_lib.sddc_ddc_abi_version() == 3
    with open(os.path.join(ROOT, "extio_sddc_amd", "csrc", "sddc_ddc_internal.h")) as f:
        assert re.search(r"#define\s+SDDC_DDC_PARAM_CHSPEC_MAX_WGS\s+12\b", f.read())


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_window_8192_is_the_spectrum_window(ddc_lib, kind):
    from extio_sddc_amd import spectrum_window, window
    np.testing.assert_array_equal(window(kind, 8192).view(np.uint32), spectrum_window(kind).view(np.uint32))


@pytest.mark.parametrize("n", [32, 256, 512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("win", WINDOWS)
def test_window_within_one_ulp_of_the_double_formula(ddc_lib, win, n):
    from extio_sddc_amd import window
    w = window(win, n)
    ref = M.window(win, n)
    assert w.dtype == np.float32 and w.shape == (n,)
    r32 = ref.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(r32), np.float32(2.0 ** -126)))
    assert (np.abs(w.astype(np.float64) - ref) <= ulp).all()
    if win == "rect":
        assert (w == 1.0).all()
    if win == "hann":
        assert w[0] == 0.0 and w[n // 2] == 1.0 and w[1] == w[-1] != 0.0   # periodic (DFT-even)


def test_window_argument_errors(ddc_lib):
    w = np.zeros(8192, np.float32)
    f = ddc_lib.sddc_ddc_window
    assert f(3, 256, w.ctypes.data) == ERR_ARG and f(-1, 256, w.ctypes.data) == ERR_ARG
    assert f(1, 256, None) == ERR_ARG
    for n in (0, -256, 16, 300, 16384):
        assert f(1, n, w.ctypes.data) == ERR_ARG
    assert (w == 0).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("n", M.SIZES)
def test_cpu_parity(cpu, n, win, fmt):
    set_format(cpu, fmt)
    set_window(cpu, win, n)
    try:
        for kind in INPUTS:
            for nch, nrows, fpr, hop in shapes(n):
                x = signal(kind, n, nch, M.nsamp_for(n, hop, fpr, nrows))
                iq, k = host_iq(x, fmt)
                psd = cpu.channel_spectrum(iq, n, hop, fpr, nrows)
                ref = reference(kind, win, n, nch, nrows, fpr, hop) * k
                assert psd.shape == ref.shape == (nch, nrows, n) and psd.dtype == np.float32
                err = row_errors(psd, ref)
                print(f"{kind} {win} {fmt} n {n} ({nch}, {nrows}, {fpr}, {hop}): max row error {err.max():.3e}")
                assert np.isfinite(psd).all() and (err <= TOL).all(), err
    finally:
        set_format(cpu, "CF32")


def test_defaults_of_hop_and_nrows(cpu):
    """hop = n / 2; nrows = all whole rows of the stream."""
    set_window(cpu, "hann", 256)
    x = signal("noise", 256, 2, 256 + 9 * 128 + 77)        # 10 frames at hop 128, and a remainder
    iq, _ = host_iq(x, "CF32")
    psd = cpu.channel_spectrum(iq, 256, frames_per_row=3)
    assert psd.shape == (2, 3, 256)
    assert (row_errors(psd, M.psd(x, 256, 128, 3, 3, lib_window("hann", 256))) <= TOL).all()
    one = cpu.channel_spectrum(iq[0], 256, frames_per_row=3)   # a single stream without the channel axis
    np.testing.assert_array_equal(one[0], psd[0])


@pytest.mark.parametrize("n", M.SIZES)
def test_edges_peaks_pin_rotation_and_orientation(cpu, n):
    """Tones at bin -n/2, DC and +n/4 read at q = 0, n/2 and 3n/4 with their amplitudes squared."""
    set_window(cpu, "rect", n)
    x = signal("edges", n, 1, M.nsamp_for(n, n, 2, 1))
    psd = cpu.channel_spectrum(host_iq(x, "CF32")[0], n, n, 2, 1)[0, 0]
    top = np.sort(np.argsort(psd)[-3:])
    assert list(top) == [0, n // 2, 3 * n // 4]
    for (b, a) in M.edges_tones(n):
        assert abs(psd[b + n // 2] / a ** 2 - 1.0) < 1e-3    # the input is rounded to integers
    assert psd[n // 4] < 1e-6 * psd[3 * n // 4]              # the mirror of +n/4 is empty


def check_dynamic_range(psd, ref, n, label):
    """psd, ref: [nrows, n] of the two-tone input."""
    _, b2, quiet = M.twotone_bins(n)
    qt, qq = b2 + n // 2, quiet + n // 2
    for r in range(psd.shape[0]):
        tone, tone_m = 10 * np.log10(psd[r, qt]), 10 * np.log10(ref[r, qt])
        level = 10 * np.log10(ref[r, qq].max())                 # the model's highest quiet bin
        margin = level - 10 * np.log10(ref[r, qq].mean())        # the model's own peak over mean there
        floor = 10 * np.log10(psd[r, qq].max())
        print(f"{label} row {r}: weak tone {tone:.4f} dB (model {tone_m:.4f}), quiet bins max {floor:.2f} dB, "
              f"model {level:.2f} dB + margin {margin:.2f} dB")
        assert abs(tone - tone_m) <= 0.05
        assert abs(tone_m - 20 * np.log10(M.TWOTONE_WEAK)) < 0.5   # the model itself: the tone reads A^2
        assert level + margin < tone_m - 20.0
        assert floor <= level + margin


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("win", ["hann", "blackman_harris"])
@pytest.mark.parametrize("n", M.SIZES)
def test_cpu_dynamic_range(cpu, n, win, fmt):
    set_format(cpu, fmt)
    set_window(cpu, win, n)
    try:
        x = signal("twotone", n, 1, M.nsamp_for(n, n // 2, 4, 2))
        iq, k = host_iq(x, fmt)
        psd = cpu.channel_spectrum(iq, n, n // 2, 4, 2)[0].astype(np.float64) / k
        check_dynamic_range(psd, reference("twotone", win, n, 1, 2, 4, n // 2)[0], n, f"{win} {fmt} n {n}")
    finally:
        set_format(cpu, "CF32")


def test_rectangular_window_fails_the_dynamic_range_check(cpu):
    """The check has teeth: without a window the strong tone's leakage covers the quiet bins."""
    n = 1024
    set_window(cpu, "rect", n)
    x = signal("twotone", n, 1, M.nsamp_for(n, n // 2, 4, 2))
    psd = cpu.channel_spectrum(host_iq(x, "CF32")[0], n, n // 2, 4, 2)[0].astype(np.float64)
    with pytest.raises(AssertionError):
        check_dynamic_range(psd, reference("twotone", "hann", n, 1, 2, 4, n // 2)[0], n, "rect")


def test_argument_errors_leave_the_output_untouched(ddc_lib, cpu):
    from extio_sddc_amd import DDCError
    L, h = ddc_lib, cpu._h
    n, nsamp = 256, 1024
    assert L.sddc_ddc_set_channel_spectrum_window(h, None, 0) == 0
    assert L.sddc_ddc_set_output_format(h, 0, 1.0) == 0
    iq = np.zeros(3 * (2 * nsamp + 2) + 4, np.float32)
    guard = np.float32(-12345.5)
    psd = np.full(3 * 4 * n + 1, guard, np.float32)
    xi, pi = iq.ctypes.data, psd.ctypes.data
    host, dev = L.sddc_ddc_channel_spectrum_host, L.sddc_ddc_channel_spectrum_device
    S = 2 * nsamp

    def untouched():
        return (psd == guard).all()

    assert host(None, xi, 1, nsamp, S, n, 128, 1, 1, pi) == ERR_ARG            # null handle
    assert dev(None, xi, 1, nsamp, S, n, 128, 1, 1, pi, None) == ERR_ARG
    assert host(h, None, 1, nsamp, S, n, 128, 1, 1, pi) == ERR_ARG             # null buffers
    assert host(h, xi, 1, nsamp, S, n, 128, 1, 1, None) == ERR_ARG
    for bad_n in (0, 128, 300, 8192, -256):                                     # n outside the five sizes
        assert host(h, xi, 1, nsamp, S, bad_n, 128, 1, 1, pi) == ERR_ARG
    assert host(h, xi, 1, nsamp, S, n, 0, 1, 1, pi) == ERR_ARG                 # hop, fpr, nrows, nch < 1
    assert host(h, xi, 1, nsamp, S, n, -3, 1, 1, pi) == ERR_ARG
    assert host(h, xi, 1, nsamp, S, n, 128, 0, 1, pi) == ERR_ARG
    assert host(h, xi, 1, nsamp, S, n, 128, 1, 0, pi) == ERR_ARG
    assert host(h, xi, 0, nsamp, S, n, 128, 1, 1, pi) == ERR_ARG
    assert host(h, xi, 1025, nsamp, S, n, 128, 1, 1, pi) == ERR_ARG
    assert host(h, xi, 1, nsamp, S, n, 128, 7, 1, pi) == 0                     # (7 - 1) 128 + 256 = 1024: fits
    psd[:] = guard
    assert host(h, xi, 1, nsamp, S, n, 128, 8, 1, pi) == ERR_ARG               # one frame too many
    assert host(h, xi, 1, nsamp, S, n, 128, 4, 2, pi) == ERR_ARG
    assert host(h, xi, 1, nsamp, S, n, 769, 1, 2, pi) == ERR_ARG               # hop > n: 769 + 256 > 1024
    assert host(h, xi, 1, n - 1, S, n, 128, 1, 1, pi) == ERR_ARG               # nsamp < n
    assert host(h, xi, 1, nsamp, S, n, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, pi) == ERR_ARG   # no overflow
    assert host(h, xi, 1024, nsamp, S, n, 1, 1, 2 ** 22, pi) == ERR_ARG        # nch * nrows >= 2^31
    assert host(h, xi, 3, nsamp, S - 2, n, 128, 1, 1, pi) == ERR_ARG           # in_stride < 2 nsamp
    assert host(h, xi, 3, nsamp, S + 1, n, 128, 1, 1, pi) == ERR_ARG           # channels off the sample grid
    assert host(h, xi + 4, 1, nsamp, S, n, 128, 1, 1, pi) == ERR_ARG           # CF32: 8-byte samples
    assert b"aligned" in L.sddc_ddc_last_error()
    assert host(h, xi, 1, nsamp, S, n, 128, 1, 1, pi + 2) == ERR_ARG
    assert untouched()
    assert host(h, xi, 3, nsamp, S + 2, n, 128, 1, 4, pi + 4) == 0             # psd 4-byte aligned, no more
    assert psd[0] == guard and (psd[1:] == 0).all()
    assert host(h, xi, 1, nsamp, 0, n, 128, 1, 1, pi) == 0                     # one channel: no stride needed
    psd[:] = guard
    # CS16 samples are 4 bytes
    assert L.sddc_ddc_set_output_format(h, 1, 2.0) == 0
    assert host(h, xi + 4, 1, nsamp, S, n, 128, 1, 1, pi) == 0
    psd[:] = guard
    assert host(h, xi + 2, 1, nsamp, S, n, 128, 1, 1, pi) == ERR_ARG
    assert L.sddc_ddc_set_output_format(h, 0, 1.0) == 0
    # the device call on a CPU handle
    assert dev(h, xi, 1, nsamp, S, n, 128, 1, 1, pi, None) == ERR_STATE
    # the window: null handle, a non-finite value, sum <= 0, n outside the five sizes
    w = np.ones(8192, np.float32)
    setw = L.sddc_ddc_set_channel_spectrum_window
    assert setw(None, w.ctypes.data, 256) == ERR_ARG
    for bad in (np.nan, np.inf):
        wb = w.copy()
        wb[77] = bad
        assert setw(h, wb.ctypes.data, 256) == ERR_ARG
    assert setw(h, np.zeros(256, np.float32).ctypes.data, 256) == ERR_ARG
    assert setw(h, (-w).ctypes.data, 256) == ERR_ARG
    for bad_n in (0, 128, 300, 8192):
        assert setw(h, w.ctypes.data, bad_n) == ERR_ARG
    # a stored window of another length
    assert setw(h, w.ctypes.data, 512) == 0
    assert host(h, xi, 1, nsamp, S, n, 128, 1, 1, pi) == ERR_STATE
    assert untouched()
    assert host(h, xi, 1, nsamp, S, 512, 128, 1, 1, pi) == 0
    assert setw(h, None, 0) == 0
    assert host(h, xi, 1, nsamp, S, n, 128, 1, 1, pi) == 0                     # rectangular: any n
    # the Python layer's own checks
    with pytest.raises(DDCError):
        cpu.channel_spectrum(np.zeros((1, 1024, 2), np.int16), 256)              # int16 on a CF32 handle
    with pytest.raises(DDCError):
        cpu.channel_spectrum(np.zeros((1, 1024), np.complex128), 256)
    with pytest.raises(DDCError):
        cpu.channel_spectrum(np.zeros((1, 100), np.complex64), 256)              # nsamp < n
    with pytest.raises(DDCError):
        cpu.channel_spectrum(np.zeros((1, 1024), np.complex64), 256, nrows=8)    # more rows than the stream holds
    with pytest.raises(DDCError):
        cpu.channel_spectrum(np.zeros((1, 1024), np.complex64), 300)
    with pytest.raises(DDCError):
        cpu.setChannelSpectrumWindow(np.ones(100, np.float32))


@pytest.mark.parametrize("fmt", FORMATS)
def test_channels_and_rows_are_independent(cpu, fmt):
    """A channel alone = the same channel among others; row r = row 0 of a call on the buffer that
    starts at sample r fpr hop.  Bit for bit."""
    n, nch, nrows, fpr, hop = 512, 3, 4, 3, 131
    set_format(cpu, fmt)
    set_window(cpu, "blackman_harris", n)
    try:
        x = signal("noise", n, nch, M.nsamp_for(n, hop, fpr, nrows))
        iq, _ = host_iq(x, fmt)
        whole = cpu.channel_spectrum(iq, n, hop, fpr, nrows).view(np.uint32)
        for c in range(nch):
            alone = cpu.channel_spectrum(iq[c:c + 1], n, hop, fpr, nrows).view(np.uint32)
            np.testing.assert_array_equal(alone[0], whole[c])
        for r in range(nrows):
            part = cpu.channel_spectrum(iq[:, r * fpr * hop:], n, hop, fpr, 1).view(np.uint32)
            np.testing.assert_array_equal(part[:, 0], whole[:, r])
    finally:
        set_format(cpu, "CF32")


def test_channel_spectrum_leaves_the_host_path_alone(ddc_lib):
    """process_host output and kept history are bit-identical with channel spectrum calls in between."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    rng = np.random.default_rng(5)
    blocks = rng.integers(-3000, 3000, (3, 65536)).astype(np.int16)
    outs = []
    for with_spectrum in (False, True):
        with R2iq(gain=1.0, device=DEVICE_CPU) as r:
            r.setDecimate(2)
            y = [r.process(blocks[0])]
            if with_spectrum:
                r.setChannelSpectrumWindow(lib_window("hann", 4096))
                r.channel_spectrum(y[0], 4096)
            y.append(r.process(blocks[1]))      # starts from block 0's tail: the kept history
            if with_spectrum:
                r.channel_spectrum(y[1], 4096, 100, 3)
            y.append(r.process(blocks[2]))
            outs.append(np.concatenate(y))
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("lsb", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
def test_end_to_end_against_the_ddc(ddc_lib, fmt, lsb):
    """A real ADC tone at wideband bin tb + 10 through process_host at d = 4 with tune bin tb: the
    channel spectrum at n = 1024 peaks (b - tb) 2^(d+1) n / 8192 = 40 bins above the centre, and
    40 bins below it with the sideband inverted (the DDC has conjugated the samples)."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    d, tb, n = 4, 1000, 1024
    t = np.arange(3 * 65536, dtype=np.float64)
    adc = np.rint(20000.0 * np.cos(2.0 * np.pi * (tb + 10) / 8192.0 * t + 0.4)).astype(np.int16)
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        r.setDecimate(d)
        r.setTuneBin(tb)
        r.setSideband(lsb)
        if fmt == "CS16":
            scale = 0.5 * 32767.0 / np.abs(_cf32_peak(adc, d, tb, lsb))
            r.setOutputFormat("CS16", float(scale))
        iq = r.process(adc)
        iq = iq[2048:] if fmt == "CF32" else iq[2048:].reshape(1, -1, 2)     # past the first block's transient
        r.setChannelSpectrumWindow(lib_window("hann", n))
        psd = r.channel_spectrum(iq, n, frames_per_row=4, nrows=1)[0, 0]
    want = n // 2 - 40 if lsb else n // 2 + 40
    assert int(np.argmax(psd)) == want
    assert psd[n - want] < 1e-6 * psd[want]      # nothing at the mirror


def _cf32_peak(adc, d, tb, lsb):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        r.setDecimate(d)
        r.setTuneBin(tb)
        r.setSideband(lsb)
        return np.abs(r.process(adc)).max()
