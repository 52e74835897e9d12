"""The wideband averaged power spectrum on the GPU (pytest -m gpu): sddc_ddc_spectrum_device and
sddc_ddc_spectrum_host of a GPU handle against the float64 model (tools/spectrum_model.py), and the
bit-exact properties of the kernel's fixed summation order.

Bars as in tests/test_spectrum_cpu.py: max_k |psd - ref| / max_k ref <= 1e-5 per row; on the
two-tone input bin 3000 within 0.05 dB of the model and bins 2900..2989 below -110 dBFS.
Shapes: nblk <= 8; (1, 1) one work item, (3, 1) rows stored by the kernel, (4, 2) and (5, 5) the
partial rows and the reduce kernel (5, 5: five blocks in one run each), (8, 2) / (8, 1) with the
grid capped at 1 and 3 workgroups: a workgroup with several items, items that outnumber the grid.
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
_spec = importlib.util.spec_from_file_location("spectrum_model", os.path.join(ROOT, "tools", "spectrum_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

TOL = 1e-5
INPUTS = ["noise", "twotone", "fs4"]
WINDOWS = ["rect", "hann", "blackman_harris"]
SHAPES = [(1, 1), (3, 1), (4, 2), (5, 5)]
PARAM_SPECTRUM_MAX_WGS = 11   # sddc_ddc_internal.h
STEP_LIMIT_S = 60


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
def stream(kind, nblk):
    x = M.make_input(kind, nblk)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dev_stream(kind, nblk):
    import torch
    return torch.from_numpy(np.array(stream(kind, nblk))).to("cuda")


@functools.lru_cache(maxsize=None)
def lib_window(kind):
    from extio_sddc_amd import spectrum_window
    w = spectrum_window(kind)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(kind, win, nblk, bpr):
    ref = M.psd(stream(kind, nblk), nblk, bpr, None if win == "rect" else lib_window(win))
    ref.setflags(write=False)
    return ref


def row_errors(psd, ref):
    return np.abs(psd.astype(np.float64) - ref).max(axis=1) / ref.max(axis=1)


def set_window(r, win):
    r.setSpectrumWindow(None if win == "rect" else lib_window(win))


def run_device(torch, r, d_in, nblk, bpr, stream_=None):
    """One spectrum_device call -> host array [nblk / bpr, 4096]; the tensor's tail stays untouched."""
    rows = nblk // bpr
    buf = torch.full((rows * M.HALF + 65,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[1:]   # d_psd is 4-byte aligned, no more
    if stream_ is not None:
        stream_.wait_stream(torch.cuda.current_stream())
    r.spectrum_device(d_in, nblk, out, bpr, stream=stream_)
    torch.cuda.synchronize()
    y = buf.cpu().numpy()
    assert np.isnan(y[0]) and np.isnan(y[1 + rows * M.HALF:]).all()
    return y[1:1 + rows * M.HALF].reshape(rows, M.HALF).copy()


def set_max_wgs(r, n):
    f = r._L.sddc_ddc_internal_set_param
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    assert f(r._h, PARAM_SPECTRUM_MAX_WGS, n) == 0


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("kind", INPUTS)
def test_parity_device_and_host(torch_dev, gpu, kind, win):
    set_window(gpu, win)
    for nblk, bpr in SHAPES:
        ref = reference(kind, win, nblk, bpr)
        dev = run_device(torch_dev, gpu, dev_stream(kind, nblk), nblk, bpr)
        host = gpu.spectrum(stream(kind, nblk), bpr)
        e_dev, e_host = row_errors(dev, ref), row_errors(host, ref)
        print(f"{kind} {win} nblk {nblk} bpr {bpr}: device {e_dev.max():.3e} host {e_host.max():.3e}")
        assert np.isfinite(dev).all() and (e_dev <= TOL).all(), e_dev
        assert (e_host <= TOL).all(), e_host
        np.testing.assert_array_equal(dev.view(np.uint32), host.view(np.uint32))   # the same kernel


@pytest.mark.parametrize("win", ["hann", "blackman_harris"])
def test_dynamic_range(torch_dev, gpu, win):
    from extio_sddc_amd import psd_to_dbfs
    set_window(gpu, win)
    dbr = M.dbfs(reference("twotone", win, 2, 1))
    for path, psd in (("device", run_device(torch_dev, gpu, dev_stream("twotone", 2), 2, 1)),
                      ("host", gpu.spectrum(stream("twotone", 2)))):
        db = psd_to_dbfs(psd)
        for r in range(2):
            tone, floor = db[r, 3000], db[r, 2900:2990].max()
            print(f"{win} {path} row {r}: bin 3000 {tone:.4f} dBFS (model {dbr[r, 3000]:.4f}), "
                  f"bins 2900..2989 max {floor:.1f} dBFS")
            assert abs(tone - dbr[r, 3000]) <= 0.05
            assert floor < -110.0


@pytest.mark.parametrize("win", ["rect", "hann"])
def test_rand_on_randomised_input_is_bit_identical(torch_dev, gpu, win):
    set_window(gpu, win)
    nblk, bpr = 4, 2
    plain = run_device(torch_dev, gpu, dev_stream("noise", nblk), nblk, bpr)
    d_rnd = torch_dev.from_numpy(M.randomise(stream("noise", nblk))).to("cuda")
    assert not torch_dev.equal(d_rnd, dev_stream("noise", nblk))
    gpu.updateRand(True)
    try:
        rnd = run_device(torch_dev, gpu, d_rnd, nblk, bpr)
    finally:
        gpu.updateRand(False)
    np.testing.assert_array_equal(rnd.view(np.uint32), plain.view(np.uint32))


def test_bit_identical_runs_streams_and_unrelated_settings(torch_dev, gpu):
    from extio_sddc_amd import R2iq
    set_window(gpu, "hann")
    nblk, bpr = 4, 2
    d_in = dev_stream("twotone", nblk)
    base = run_device(torch_dev, gpu, d_in, nblk, bpr).view(np.uint32)
    np.testing.assert_array_equal(run_device(torch_dev, gpu, d_in, nblk, bpr).view(np.uint32), base)
    side = torch_dev.cuda.Stream()
    np.testing.assert_array_equal(run_device(torch_dev, gpu, d_in, nblk, bpr, side).view(np.uint32), base)
    base1 = run_device(torch_dev, gpu, d_in, nblk, 1).view(np.uint32)
    np.testing.assert_array_equal(run_device(torch_dev, gpu, d_in, nblk, 1, side).view(np.uint32), base1)
    # d, sideband, the fine-tune NCO and the output format do not enter
    with R2iq(gain=1.0) as r:
        set_window(r, "hann")
        for change in (lambda: r.setDecimate(3), lambda: r.setSideband(True), lambda: r.setFineTune(0.0123),
                       lambda: r.setOutputFormat("CS16", 100.0)):
            change()
            np.testing.assert_array_equal(run_device(torch_dev, r, d_in, nblk, bpr).view(np.uint32), base)
            np.testing.assert_array_equal(run_device(torch_dev, r, d_in, nblk, 1).view(np.uint32), base1)


@pytest.mark.parametrize("nblk,bpr", [(8, 2), (8, 1)])
def test_bit_identical_for_any_grid(torch_dev, nblk, bpr):
    from extio_sddc_amd import R2iq
    d_in = dev_stream("noise", nblk)
    with R2iq(gain=1.0) as r:
        set_window(r, "blackman_harris")
        outs = []
        for cap in (0, 1, 3):
            set_max_wgs(r, cap)
            outs.append(run_device(torch_dev, r, d_in, nblk, bpr).view(np.uint32))
        f = r._L.sddc_ddc_internal_set_param
        assert f(r._h, PARAM_SPECTRUM_MAX_WGS, -1) != 0
    assert (row_errors(outs[0].view(np.float32), reference("noise", "blackman_harris", nblk, bpr)) <= TOL).all()
    np.testing.assert_array_equal(outs[1], outs[0])
    np.testing.assert_array_equal(outs[2], outs[0])


def test_rows_are_independent(torch_dev, gpu):
    """Row r of (4, 2) = row 0 of a (2, 2) call on the sub-buffer that starts 4096 samples before block 2r."""
    set_window(gpu, "hann")
    d_in = dev_stream("noise", 4)
    whole = run_device(torch_dev, gpu, d_in, 4, 2).view(np.uint32)
    for r in range(2):
        sub = d_in[2 * r * M.BLOCK: M.HALF + (2 * r + 2) * M.BLOCK]
        assert sub.data_ptr() % 4 == 0
        part = run_device(torch_dev, gpu, sub, 2, 2).view(np.uint32)
        np.testing.assert_array_equal(part[0], whole[r])


def test_two_streams_share_the_partial_rows(torch_dev, gpu):
    """Two launches back to back on two streams (bpr = 2: both use the handle's partial rows)."""
    torch = torch_dev
    set_window(gpu, "hann")
    nblk, bpr = 8, 2
    ins = [dev_stream("noise", nblk), dev_stream("twotone", nblk)]
    single = [run_device(torch, gpu, d, nblk, bpr).view(np.uint32) for d in ins]
    assert not np.array_equal(single[0], single[1])
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.full((nblk // bpr * M.HALF,), float("nan"), dtype=torch.float32, device="cuda") for _ in ins]
    torch.cuda.synchronize()
    for _ in range(3):
        for i in range(2):
            gpu.spectrum_device(ins[i], nblk, outs[i], bpr, stream=s[i])
    torch.cuda.synchronize()
    for i in range(2):
        np.testing.assert_array_equal(outs[i].cpu().numpy().view(np.uint32).reshape(-1, M.HALF), single[i])


def test_gpu_row_against_the_cpu_backend(torch_dev, gpu):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    set_window(gpu, "blackman_harris")
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        set_window(c, "blackman_harris")
        for kind in INPUTS:
            g = run_device(torch_dev, gpu, dev_stream(kind, 4), 4, 2)
            err = row_errors(g, c.spectrum(stream(kind, 4), 2).astype(np.float64))
            print(f"{kind}: GPU against CPU backend {err}")
            assert (err <= TOL).all(), err


def test_spectrum_leaves_the_host_path_alone(torch_dev):
    """process_host output and kept history (on the device) are bit-identical with spectrum calls in between."""
    from extio_sddc_amd import R2iq
    x = stream("noise", 3)
    blocks = x[M.HALF:].reshape(3, M.BLOCK)
    outs = []
    for with_spectrum in (False, True):
        with R2iq(gain=1.0) as r:
            r.setDecimate(2)
            y = [r.process(blocks[0])]
            if with_spectrum:
                set_window(r, "hann")
                r.spectrum(stream("twotone", 2), 2)
                run_device(torch_dev, r, dev_stream("fs4", 1), 1, 1)
            y.append(r.process(blocks[1]))      # starts from block 0's tail: the kept history
            if with_spectrum:
                r.spectrum(stream("fs4", 1))
            y.append(r.process(blocks[2]))
            outs.append(np.concatenate(y))
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_device_argument_errors(torch_dev, gpu):
    from extio_sddc_amd import DDCError
    L, h = gpu._L, gpu._h
    d_in = dev_stream("noise", 4)
    out = torch_dev.zeros(4 * M.HALF + 1, dtype=torch_dev.float32, device="cuda")
    xi, pi = d_in.data_ptr(), out.data_ptr()
    dev = L.sddc_ddc_spectrum_device
    assert dev(h, None, 4, 1, pi, None) == -1 and dev(h, xi, 4, 1, None, None) == -1
    assert dev(h, xi, 0, 1, pi, None) == -1 and dev(h, xi, 32769, 1, pi, None) == -1
    assert dev(h, xi, 4, 0, pi, None) == -1 and dev(h, xi, 4, 3, pi, None) == -1
    assert dev(h, xi + 2, 4, 1, pi, None) == -1 and dev(h, xi, 4, 1, pi + 2, None) == -1
    with pytest.raises(DDCError):
        gpu.spectrum_device(d_in, 4, out[:M.HALF], 1)          # d_psd too small
    with pytest.raises(DDCError):
        gpu.spectrum_device(d_in, 8, out, 1)                   # d_in too small
    with pytest.raises(DDCError):
        gpu.spectrum_device(d_in, 4, out.double(), 1)          # wrong dtype
    torch_dev.cuda.synchronize()
