"""The channel spectrum on the GPU (pytest -m gpu): sddc_ddc_channel_spectrum_device and
sddc_ddc_channel_spectrum_host of a GPU handle against the float64 model
(tools/channel_spectrum_model.py), the bit-exact properties of the kernel's fixed summation order,
and the DDC and the spectrum on one stream and one device buffer.

Bars as in tests/test_channel_spectrum_cpu.py: per row max_q |psd - model| / max_q model <= 1e-5; on
the two-tone input the weak tone within 0.05 dB of the model and the quiet bins below the model's
level plus the model's own margin; GPU against the CPU backend within twice the bar (the sum of the
two bounds against the model).
Shapes (nch, nrows, fpr, hop, unused components between the streams), chosen for where the kernel
can go wrong (a 256-thread workgroup holds 4096 / n items, n / 16 threads each):
  (1, 1, 1, n, 0)              one live sub-group, the rest idle at the barriers
  (1, 4096/n + 1, 3, n/2, 0)   a tail workgroup with one live sub-group (n = 256: 17 items)
  (3, 2, 2, n/4 + 1, 2)        in_stride = 2 nsamp + 2, an odd hop
  (1, 2, 2, 2n, 0)             hop > n
  (2, 1, 16, n/2, 0)           16 frames per row
Every d_psd sits one float into a NaN-filled tensor whose head and tail must stay NaN.
Every test runs under a watchdog that ends the process if a GPU step hangs.
"""
from __future__ import annotations

import ctypes
import faulthandler
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("channel_spectrum_model",
                                               os.path.join(ROOT, "tools", "channel_spectrum_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

TOL = 1e-5
INPUTS = ["noise", "twotone", "edges"]
WINDOWS = ["rect", "hann", "blackman_harris"]
FORMATS = ["CF32", "CS16"]
CS16_SCALE = 4.0
PARAM_CHSPEC_MAX_WGS = 12   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60


def shapes(n):
    return [(1, 1, 1, n, 0), (1, 4096 // n + 1, 3, n // 2, 0), (3, 2, 2, n // 4 + 1, 2), (1, 2, 2, 2 * n, 0),
            (2, 1, 16, n // 2, 0)]


@pytest.fixture(autouse=True)
def step_limit():
    """A hung GPU step ends the run (with a traceback) instead of blocking it."""
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def gpu(torch_dev):
    from extio_sddc_amd import R2iq
    with R2iq(gain=1.0) as r:
        yield r
        torch_dev.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def signal(kind, n, nch, nsamp):
    x = M.make_input(kind, n, nch, nsamp)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dev_signal(kind, n, nch, nsamp, fmt, extra):
    """The streams as the DDC writes them, on the device: [nch, 2 nsamp + extra] components."""
    import torch
    x = signal(kind, n, nch, nsamp)
    return torch.from_numpy(M.as_cs16(x, extra) if fmt == "CS16" else M.as_cf32(x, extra)).to("cuda")


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


def fmt_scale(fmt):
    return 1.0 / CS16_SCALE ** 2 if fmt == "CS16" else 1.0


def host_iq(x, fmt):
    if fmt == "CS16":
        return M.as_cs16(x).reshape(x.shape[0], x.shape[1], 2)
    return M.as_cf32(x).view(np.complex64)


def set_format(r, fmt):
    r.setOutputFormat(fmt, CS16_SCALE if fmt == "CS16" else 1.0)


def set_window(r, win, n):
    r.setChannelSpectrumWindow(None if win == "rect" else lib_window(win, n))


def set_max_wgs(r, cap):
    f = r._L.sddc_ddc_internal_set_param
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    return f(r._h, PARAM_CHSPEC_MAX_WGS, cap)


def run_device(torch, r, d_iq, nch, nsamp, in_stride, n, hop, fpr, nrows, stream_=None):
    """One channel_spectrum_device call -> host array [nch, nrows, n]; d_psd is one float into a
    NaN-filled tensor whose head and tail stay NaN."""
    count = nch * nrows * n
    buf = torch.full((count + 65,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[1:]   # d_psd is 4-byte aligned, no more
    if stream_ is not None:
        stream_.wait_stream(torch.cuda.current_stream())
    r.channel_spectrum_device(d_iq, nch, nsamp, in_stride, n, hop, fpr, nrows, out, stream=stream_)
    torch.cuda.synchronize()
    y = buf.cpu().numpy()
    assert np.isnan(y[0]) and np.isnan(y[1 + count:]).all()
    return y[1:1 + count].reshape(nch, nrows, n).copy()


def run_signal(torch, r, kind, fmt, n, nch, nrows, fpr, hop, extra=0, stream_=None):
    nsamp = M.nsamp_for(n, hop, fpr, nrows)
    d_iq = dev_signal(kind, n, nch, nsamp, fmt, extra)
    return run_device(torch, r, d_iq, nch, nsamp, 2 * nsamp + extra, n, hop, fpr, nrows, stream_)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("n", M.SIZES)
def test_parity_device_and_host(torch_dev, gpu, n, win, fmt):
    set_format(gpu, fmt)
    set_window(gpu, win, n)
    try:
        for kind in INPUTS:
            for nch, nrows, fpr, hop, extra in shapes(n):
                ref = reference(kind, win, n, nch, nrows, fpr, hop) * fmt_scale(fmt)
                dev = run_signal(torch_dev, gpu, kind, fmt, n, nch, nrows, fpr, hop, extra)
                x = signal(kind, n, nch, M.nsamp_for(n, hop, fpr, nrows))
                host = gpu.channel_spectrum(host_iq(x, fmt), n, hop, fpr, nrows)
                e_dev, e_host = row_errors(dev, ref), row_errors(host, ref)
                print(f"{kind} {win} {fmt} n {n} ({nch}, {nrows}, {fpr}, {hop}): device {e_dev.max():.3e} "
                      f"host {e_host.max():.3e}")
                assert np.isfinite(dev).all() and (e_dev <= TOL).all(), e_dev
                assert (e_host <= TOL).all(), e_host
                np.testing.assert_array_equal(dev.view(np.uint32), host.view(np.uint32))   # the same kernel
    finally:
        set_format(gpu, "CF32")


@pytest.mark.parametrize("n", M.SIZES)
def test_edges_peaks(torch_dev, gpu, n):
    set_window(gpu, "rect", n)
    psd = run_signal(torch_dev, gpu, "edges", "CF32", n, 1, 1, 2, n)[0, 0]
    assert list(np.sort(np.argsort(psd)[-3:])) == [0, n // 2, 3 * n // 4]
    for (b, a) in M.edges_tones(n):
        assert abs(psd[b + n // 2] / a ** 2 - 1.0) < 1e-3
    assert psd[n // 4] < 1e-6 * psd[3 * n // 4]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("win", ["hann", "blackman_harris"])
@pytest.mark.parametrize("n", M.SIZES)
def test_dynamic_range(torch_dev, gpu, n, win, fmt):
    set_format(gpu, fmt)
    set_window(gpu, win, n)
    try:
        psd = run_signal(torch_dev, gpu, "twotone", fmt, n, 1, 2, 4, n // 2)[0].astype(np.float64) / fmt_scale(fmt)
    finally:
        set_format(gpu, "CF32")
    ref = reference("twotone", win, n, 1, 2, 4, n // 2)[0]
    _, b2, quiet = M.twotone_bins(n)
    qt, qq = b2 + n // 2, quiet + n // 2
    for r in range(2):
        tone, tone_m = 10 * np.log10(psd[r, qt]), 10 * np.log10(ref[r, qt])
        level = 10 * np.log10(ref[r, qq].max())                 # the model's highest quiet bin
        margin = level - 10 * np.log10(ref[r, qq].mean())        # the model's own peak over mean there
        floor = 10 * np.log10(psd[r, qq].max())
        print(f"{win} {fmt} n {n} row {r}: weak tone {tone:.4f} dB (model {tone_m:.4f}), quiet bins max "
              f"{floor:.2f} dB, model {level:.2f} dB + margin {margin:.2f} dB")
        assert abs(tone - tone_m) <= 0.05
        assert level + margin < tone_m - 20.0
        assert floor <= level + margin


@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_identical_for_any_grid(torch_dev, fmt):
    """40 items at n = 1024 (4 per workgroup): 10 workgroups uncapped; capped at 1 a workgroup takes 10
    rounds; capped at 3 it takes 4 and the last round is partial (4 of 12 items)."""
    from extio_sddc_amd import R2iq
    n, nch, nrows, fpr, hop = 1024, 5, 8, 2, 512
    with R2iq(gain=1.0) as r:
        set_format(r, fmt)
        set_window(r, "blackman_harris", n)
        outs = []
        for cap in (0, 1, 3):
            assert set_max_wgs(r, cap) == 0
            outs.append(run_signal(torch_dev, r, "noise", fmt, n, nch, nrows, fpr, hop).view(np.uint32))
        assert set_max_wgs(r, -1) == ERR_ARG
    ref = reference("noise", "blackman_harris", n, nch, nrows, fpr, hop) * fmt_scale(fmt)
    assert (row_errors(outs[0].view(np.float32), ref) <= TOL).all()
    np.testing.assert_array_equal(outs[1], outs[0])
    np.testing.assert_array_equal(outs[2], outs[0])


def test_bit_identical_runs_streams_channels_rows_and_unrelated_settings(torch_dev, gpu):
    from extio_sddc_amd import R2iq
    torch = torch_dev
    n, nch, nrows, fpr, hop = 512, 3, 4, 3, 131
    set_window(gpu, "hann", n)
    nsamp = M.nsamp_for(n, hop, fpr, nrows)
    d_iq = dev_signal("noise", n, nch, nsamp, "CF32", 2)
    S = 2 * nsamp + 2
    base = run_device(torch, gpu, d_iq, nch, nsamp, S, n, hop, fpr, nrows).view(np.uint32)
    np.testing.assert_array_equal(run_device(torch, gpu, d_iq, nch, nsamp, S, n, hop, fpr, nrows).view(np.uint32), base)
    side = torch.cuda.Stream()
    np.testing.assert_array_equal(
        run_device(torch, gpu, d_iq, nch, nsamp, S, n, hop, fpr, nrows, side).view(np.uint32), base)
    # a channel alone against the same channel among others
    for c in range(nch):
        alone = run_device(torch, gpu, d_iq[c], 1, nsamp, S, n, hop, fpr, nrows).view(np.uint32)
        np.testing.assert_array_equal(alone[0], base[c])
    # row r against row 0 of a call on the buffer that starts at sample r fpr hop
    flat = d_iq.reshape(-1)
    for r in range(nrows):
        off = r * fpr * hop
        sub = flat[2 * off:]
        assert sub.data_ptr() % 8 == 0
        part = run_device(torch, gpu, sub, nch, nsamp - off, S, n, hop, fpr, 1).view(np.uint32)
        np.testing.assert_array_equal(part[:, 0], base[:, r])
    # d, the tune bin, the sideband and both NCOs do not enter
    with R2iq(gain=1.0) as r:
        set_window(r, "hann", n)
        for change in (lambda: r.setDecimate(3), lambda: r.setTuneBin(2000), lambda: r.setSideband(True),
                       lambda: r.setFineTune(0.0123), lambda: r.setChannelFineTune([0.01, -0.02, 0.03]),
                       lambda: r.updateRand(True)):
            change()
            np.testing.assert_array_equal(
                run_device(torch, r, d_iq, nch, nsamp, S, n, hop, fpr, nrows).view(np.uint32), base)


@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_against_the_cpu_backend(torch_dev, gpu, fmt):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    n, nch, nrows, fpr, hop = 2048, 2, 3, 4, 700
    set_format(gpu, fmt)
    set_window(gpu, "blackman_harris", n)
    try:
        with R2iq(gain=1.0, device=DEVICE_CPU) as c:
            set_format(c, fmt)
            set_window(c, "blackman_harris", n)
            for kind in INPUTS:
                g = run_signal(torch_dev, gpu, kind, fmt, n, nch, nrows, fpr, hop)
                x = signal(kind, n, nch, M.nsamp_for(n, hop, fpr, nrows))
                err = row_errors(g, c.channel_spectrum(host_iq(x, fmt), n, hop, fpr, nrows).astype(np.float64))
                print(f"{kind} {fmt}: GPU against CPU backend {err.max():.3e}")
                assert (err <= 2 * TOL).all(), err
    finally:
        set_format(gpu, "CF32")


def test_window_length_mismatch_and_window_change_between_streams(torch_dev, gpu):
    torch = torch_dev
    n, nch, nrows, fpr, hop = 1024, 2, 3, 2, 512
    nsamp = M.nsamp_for(n, hop, fpr, nrows)
    d_iq = dev_signal("twotone", n, nch, nsamp, "CF32", 0)
    args = (d_iq, nch, nsamp, 2 * nsamp, n, hop, fpr, nrows)
    single = {}
    for win in ("hann", "blackman_harris"):
        set_window(gpu, win, n)
        single[win] = run_device(torch, gpu, *args).view(np.uint32)
    assert not np.array_equal(single["hann"], single["blackman_harris"])
    # a stored window of another length
    set_window(gpu, "hann", 512)
    out = torch.full((nch * nrows * n,), float("nan"), dtype=torch.float32, device="cuda")
    rc = gpu._L.sddc_ddc_channel_spectrum_device(gpu._h, d_iq.data_ptr(), nch, nsamp, 2 * nsamp, n, hop, fpr, nrows,
                                                 out.data_ptr(), None)
    assert rc == ERR_STATE
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # each launch keeps its own window's result when the window changes between two streams
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.full((nch * nrows * n,), float("nan"), dtype=torch.float32, device="cuda") for _ in s]
    torch.cuda.synchronize()
    for _ in range(3):
        for i, win in enumerate(("hann", "blackman_harris")):
            set_window(gpu, win, n)
            gpu.channel_spectrum_device(*args, outs[i], stream=s[i])
    torch.cuda.synchronize()
    for i, win in enumerate(("hann", "blackman_harris")):
        np.testing.assert_array_equal(outs[i].cpu().numpy().view(np.uint32).reshape(nch, nrows, n), single[win])


def test_device_argument_errors(torch_dev, gpu):
    from extio_sddc_amd import DDCError
    torch = torch_dev
    set_window(gpu, "rect", 256)
    n, nsamp = 256, 1024
    d_iq = torch.zeros(3 * (2 * nsamp + 2) + 4, dtype=torch.float32, device="cuda")
    out = torch.full((3 * 4 * n + 1,), float("nan"), dtype=torch.float32, device="cuda")
    xi, pi, S = d_iq.data_ptr(), out.data_ptr(), 2 * nsamp
    dev, h = gpu._L.sddc_ddc_channel_spectrum_device, gpu._h
    assert dev(h, None, 1, nsamp, S, n, 128, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 1, nsamp, S, n, 128, 1, 1, None, None) == ERR_ARG
    assert dev(h, xi, 1, nsamp, S, 128, 128, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 1, nsamp, S, 8192, 128, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 0, nsamp, S, n, 128, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 1025, nsamp, S, n, 128, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 1, nsamp, S, n, 0, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 1, nsamp, S, n, 128, 0, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 1, nsamp, S, n, 128, 1, 0, pi, None) == ERR_ARG
    assert dev(h, xi, 1, nsamp, S, n, 128, 8, 1, pi, None) == ERR_ARG           # one frame too many
    assert dev(h, xi, 3, nsamp, S - 2, n, 128, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi, 3, nsamp, S + 1, n, 128, 1, 1, pi, None) == ERR_ARG
    assert dev(h, xi + 4, 1, nsamp, S, n, 128, 1, 1, pi, None) == ERR_ARG       # CF32: 8-byte samples
    assert dev(h, xi, 1, nsamp, S, n, 128, 1, 1, pi + 2, None) == ERR_ARG
    with pytest.raises(DDCError):
        gpu.channel_spectrum_device(d_iq, 1, nsamp, S, n, 128, 1, 4, out[:n])        # d_psd too small
    with pytest.raises(DDCError):
        gpu.channel_spectrum_device(d_iq, 4, nsamp, S + 2, n, 128, 1, 1, out)        # d_iq too small
    with pytest.raises(DDCError):
        gpu.channel_spectrum_device(d_iq.to(torch.int16), 1, nsamp, S, n, 128, 1, 1, out)   # wrong dtype
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_ddc_and_channel_spectrum_on_one_stream(torch_dev, fmt):
    """process_channels_device at d = 4 (3 blocks, 5 channels) and channel_spectrum_device on its
    output buffer, on the same stream: within the bar of the model applied to the IQ copied back, and
    the peaks 4 (b - tb) bins from the centre ((b - tb) 2^(d+1) n / 8192 at n = 1024)."""
    from extio_sddc_amd import R2iq, output_samples
    torch = torch_dev
    d, nblk, n, hop, fpr = 4, 3, 1024, 512, 11
    tones = ((1010, 12000.0), (1200, 8000.0))                     # wideband bins, amplitudes
    tbs = [1000, 1004, 1020, 1180, 1240]
    want = [512 + 4 * (1010 - 1000), 512 + 4 * (1010 - 1004), 512 + 4 * (1010 - 1020), 512 + 4 * (1200 - 1180),
            512 + 4 * (1200 - 1240)]
    t = np.arange(4096 + nblk * 65536, dtype=np.float64)
    adc = sum(a * np.cos(2.0 * np.pi * b / 8192.0 * t + 0.3 * i) for i, (b, a) in enumerate(tones))
    d_in = torch.from_numpy(np.rint(adc).astype(np.int16)).to("cuda")
    nsamp = output_samples(d, nblk)
    assert M.nsamp_for(n, hop, fpr, 1) == nsamp == 6144
    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        r.setChannelSpectrumWindow(lib_window("hann", n))
        scale = 1.0
        if fmt == "CS16":   # half of full scale for the strongest channel
            y = torch.empty((len(tbs), 2 * nsamp), dtype=torch.float32, device="cuda")
            r.process_channels_device(d_in, nblk, tbs, y)
            torch.cuda.synchronize()
            scale = float(0.5 * 32767.0 / y.abs().max().item())
            r.setOutputFormat("CS16", scale)
        d_iq = torch.empty((len(tbs), 2 * nsamp), dtype=torch.int16 if fmt == "CS16" else torch.float32, device="cuda")
        d_psd = torch.full((len(tbs) * n,), float("nan"), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, d_iq, stream=s)
        r.channel_spectrum_device(d_iq, len(tbs), nsamp, d_iq.stride(0), n, hop, fpr, 1, d_psd, stream=s)
        torch.cuda.synchronize()
    iq = d_iq.cpu().numpy().astype(np.float64) / scale
    x = iq[:, 0::2] + 1j * iq[:, 1::2]
    psd = d_psd.cpu().numpy().reshape(len(tbs), 1, n)
    err = row_errors(psd, M.psd(x, n, hop, fpr, 1, lib_window("hann", n)))
    print(f"{fmt}: DDC + channel spectrum against the model on the IQ copied back {err}")
    assert (err <= TOL).all(), err
    assert [int(np.argmax(p[0])) for p in psd] == want
