"""The wideband averaged power spectrum without a GPU: the C ABI's new symbols, the windows, the
argument checks and the CPU backend (sddc_ddc_spectrum_host on a CPU handle) against the float64
statement of the definition, tools/spectrum_model.py.

Parity bar: max_k |psd - ref| / max_k ref <= 1e-5 per row, the project's IQ bar (a float32 numpy
port of the definition stays at 2.4e-7 on these inputs).  Dynamic range on the two-tone input with
a Hann or Blackman-Harris window: the -80 dBFS tone at bin 3000 within 0.05 dB of the model, bins
2900..2989 below -110 dBFS (a rectangular window reads -74 dBFS there, so a window that is not
applied fails).
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
_spec = importlib.util.spec_from_file_location("spectrum_model", os.path.join(ROOT, "tools", "spectrum_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

TOL = 1e-5
SYMBOLS = ["sddc_ddc_spectrum_window", "sddc_ddc_set_spectrum_window", "sddc_ddc_spectrum_device",
           "sddc_ddc_spectrum_host"]
INPUTS = ["noise", "twotone", "fs4"]
WINDOWS = ["rect", "hann", "blackman_harris"]
SHAPES = [(1, 1), (3, 1), (4, 2), (5, 5)]
ERR_ARG, ERR_STATE = -1, -4


@functools.lru_cache(maxsize=None)
def stream(kind, nblk):
    x = M.make_input(kind, nblk)
    x.setflags(write=False)
    return x


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
    assert re.search(r"#define\s+SDDC_DDC_SPECTRUM_BINS\s+4096\b", hdr)
    assert ddc_lib.sddc_ddc_abi_version() == 3


@pytest.mark.parametrize("win", WINDOWS)
def test_window_within_one_ulp_of_the_double_formula(win):
    from extio_sddc_amd import spectrum_window
    w = spectrum_window(win)
    ref = M.window(win)
    assert w.dtype == np.float32 and w.shape == (M.FFTN,)
    r32 = ref.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(r32), np.float32(2.0 ** -126)))
    assert (np.abs(w.astype(np.float64) - ref) <= ulp).all()
    if win == "rect":
        assert (w == 1.0).all()
    if win == "hann":
        assert w[0] == 0.0 and w[M.FFTN // 2] == 1.0 and w[1] == w[-1] != 0.0   # periodic (DFT-even)


def test_unknown_window_kind(ddc_lib):
    w = np.zeros(M.FFTN, np.float32)
    assert ddc_lib.sddc_ddc_spectrum_window(3, w.ctypes.data) == ERR_ARG
    assert ddc_lib.sddc_ddc_spectrum_window(-1, w.ctypes.data) == ERR_ARG
    assert ddc_lib.sddc_ddc_spectrum_window(1, None) == ERR_ARG


def test_argument_errors(ddc_lib, cpu):
    from extio_sddc_amd import DDCError
    L, h = ddc_lib, cpu._h
    x = np.zeros(M.HALF + 4 * M.BLOCK + 2, np.int16)
    psd = np.zeros(4 * M.HALF + 1, np.float32)
    xi, pi = x.ctypes.data, psd.ctypes.data
    for fn, extra in ((L.sddc_ddc_spectrum_host, ()), (L.sddc_ddc_spectrum_device, (None,))):
        assert fn(None, xi, 4, 1, pi, *extra) == ERR_ARG                         # null handle
    host = L.sddc_ddc_spectrum_host
    assert host(h, None, 4, 1, pi) == ERR_ARG                                    # null buffers
    assert host(h, xi, 4, 1, None) == ERR_ARG
    assert host(h, xi, 0, 1, pi) == ERR_ARG                                      # nblk outside 1..MAX_BLOCKS
    assert host(h, xi, -1, 1, pi) == ERR_ARG
    assert host(h, xi, 32769, 1, pi) == ERR_ARG
    assert host(h, xi, 4, 0, pi) == ERR_ARG                                      # bpr < 1
    assert host(h, xi, 4, -2, pi) == ERR_ARG
    assert host(h, xi, 4, 3, pi) == ERR_ARG                                      # not a divisor of nblk
    assert host(h, xi, 4, 8, pi) == ERR_ARG
    assert host(h, xi + 2, 4, 1, pi) == ERR_ARG                                  # misaligned
    assert host(h, xi, 4, 1, pi + 2) == ERR_ARG
    assert b"aligned" in L.sddc_ddc_last_error()
    assert host(h, xi, 4, 2, pi) == 0                                            # and the valid call
    # the device call on a CPU handle
    assert L.sddc_ddc_spectrum_device(h, xi, 4, 1, pi, None) == ERR_STATE
    # the window: null handle, a non-finite value, sum <= 0
    w = np.ones(M.FFTN, np.float32)
    assert L.sddc_ddc_set_spectrum_window(None, w.ctypes.data) == ERR_ARG
    for bad in (np.nan, np.inf):
        wb = w.copy()
        wb[77] = bad
        assert L.sddc_ddc_set_spectrum_window(h, wb.ctypes.data) == ERR_ARG
    assert L.sddc_ddc_set_spectrum_window(h, np.zeros(M.FFTN, np.float32).ctypes.data) == ERR_ARG
    assert L.sddc_ddc_set_spectrum_window(h, (-w).ctypes.data) == ERR_ARG
    assert L.sddc_ddc_set_spectrum_window(h, None) == 0
    # the Python layer's own checks
    with pytest.raises(DDCError):
        cpu.spectrum(x[:M.HALF + 4 * M.BLOCK], blocks_per_row=3)
    with pytest.raises(DDCError):
        cpu.spectrum(x[:M.HALF + 100])
    with pytest.raises(DDCError):
        cpu.setSpectrumWindow(np.ones(100, np.float32))


@pytest.mark.parametrize("nblk,bpr", SHAPES, ids=[f"{n}x{b}" for n, b in SHAPES])
@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("kind", INPUTS)
def test_cpu_parity(cpu, kind, win, nblk, bpr):
    cpu.setSpectrumWindow(None if win == "rect" else lib_window(win))
    psd = cpu.spectrum(stream(kind, nblk), bpr)
    ref = reference(kind, win, nblk, bpr)
    assert psd.shape == ref.shape == (nblk // bpr, M.HALF) and psd.dtype == np.float32
    err = row_errors(psd, ref)
    print(f"{kind} {win} nblk {nblk} bpr {bpr}: max row error {err.max():.3e}")
    assert (err <= TOL).all(), err


def check_dynamic_range(psd, ref, win):
    from extio_sddc_amd import psd_to_dbfs
    db, dbr = psd_to_dbfs(psd), M.dbfs(ref)
    for r in range(psd.shape[0]):
        tone, floor = db[r, 3000], db[r, 2900:2990].max()
        print(f"{win} row {r}: bin 3000 {tone:.4f} dBFS (model {dbr[r, 3000]:.4f}), bins 2900..2989 max {floor:.1f} dBFS")
        assert abs(tone - dbr[r, 3000]) <= 0.05
        assert abs(dbr[r, 3000] + 80.0) < 0.05   # the model itself: the tone is at -80 dBFS
        assert floor < -110.0


@pytest.mark.parametrize("win", ["hann", "blackman_harris"])
def test_cpu_dynamic_range(cpu, win):
    cpu.setSpectrumWindow(lib_window(win))
    check_dynamic_range(cpu.spectrum(stream("twotone", 2)), reference("twotone", win, 2, 1), win)


def test_rectangular_window_fails_the_dynamic_range_check(cpu):
    """The check has teeth: without a window the leakage of the strong tone covers bins 2900..2989."""
    cpu.setSpectrumWindow(None)
    from extio_sddc_amd import psd_to_dbfs
    assert psd_to_dbfs(cpu.spectrum(stream("twotone", 2)))[:, 2900:2990].max() > -90.0


def test_cpu_custom_window(cpu):
    """A 7-term flat-top: negative lobes, positive sum."""
    w = M.cosine_window(M.FLATTOP7).astype(np.float32)
    assert w.min() < 0 and w.sum() > 0
    cpu.setSpectrumWindow(w)
    for kind in INPUTS:
        err = row_errors(cpu.spectrum(stream(kind, 4), 2), M.psd(stream(kind, 4), 4, 2, w))
        print(f"flat-top {kind}: {err}")
        assert (err <= TOL).all(), err
    cpu.setSpectrumWindow(None)


def test_cpu_rand(cpu):
    """rand = 1 on the host-randomised input equals rand = 0 on the plain input."""
    x = stream("noise", 2)
    cpu.setSpectrumWindow(lib_window("hann"))
    plain = cpu.spectrum(x)
    cpu.updateRand(True)
    try:
        np.testing.assert_array_equal(cpu.spectrum(M.randomise(x)), plain)
    finally:
        cpu.updateRand(False)


def test_spectrum_leaves_the_host_path_alone(ddc_lib):
    """process_host output and kept history are bit-identical with spectrum calls in between."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    x = stream("noise", 3)
    blocks = x[M.HALF:].reshape(3, M.BLOCK)
    outs = []
    for with_spectrum in (False, True):
        with R2iq(gain=1.0, device=DEVICE_CPU) as r:
            r.setDecimate(2)
            y = [r.process(blocks[0])]
            if with_spectrum:
                r.setSpectrumWindow(lib_window("hann"))
                r.spectrum(stream("twotone", 2), 2)
            y.append(r.process(blocks[1]))      # starts from block 0's tail: the kept history
            if with_spectrum:
                r.spectrum(stream("fs4", 1))
            y.append(r.process(blocks[2]))
            outs.append(np.concatenate(y))
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
