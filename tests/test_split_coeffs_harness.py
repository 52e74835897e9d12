"""The shipped (P, r) coefficient code of the two table-build kernels (extio_sddc_amd/csrc/split_coeffs.h:
build_fs_tables_kernel, build_split_filter_kernel), compiled for the host by
tests/harness/split_coeffs_harness.cpp and run here without a GPU, against numpy in longdouble
at all 4096 bins (Hh = 1).

Bars: P and r carry one float32 rounding each of a double value, so each is held to 2^-23 of
its exact value (2^-24 for the rounding, as much again for the double arithmetic and this
check's own longdouble); and per bin the Q the kernels apply, i r P, to 2^-21 of the exact Q,
the per-bin bar of tests/test_split_pr_model.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "bin", "split_coeffs_harness")
HALF = 4096


@pytest.fixture(scope="module")
def exact():
    ld = np.longdouble
    b = np.arange(HALF).astype(ld)
    pi = ld(np.pi) + ld(1.2246467991473532e-16)        # pi to longdouble: np.pi + its double remainder
    a = pi * (ld(2048) - b) / ld(8192)                 # phi / 2
    s, c = np.sin(a), np.cos(a)
    # 1 - i W = 2 s (s - i c), 1 + i W = 2 c (c + i s), r = c / s
    return {"pr": 2 * s * s, "pi": -2 * s * c, "qr": 2 * c * c, "qi": 2 * c * s, "s": s, "c": c}


def _table(mode):
    assert os.path.exists(EXE), "run make -C extio_sddc_amd/csrc (or __graft_entry__.build())"
    out = subprocess.run([EXE, mode], check=True, capture_output=True, text=True).stdout
    t = np.array([[float(v) for v in line.split()] for line in out.splitlines()])
    assert t.shape == (HALF, 4) and np.array_equal(t[:, 0], np.arange(HALF))
    # 9 significant digits name one float32: back to it, then exactly to double
    return tuple(t[:, k].astype(np.float32).astype(np.float64) for k in (1, 2, 3))


@pytest.mark.parametrize("mode", ["q0", "2p64"])
def test_coeffs_every_bin(exact, mode):
    px, py, r = _table(mode)
    ld = np.longdouble
    ok = np.arange(HALF) != 2048
    absp = np.hypot(exact["pr"], exact["pi"])
    errp = np.hypot(px.astype(ld) - exact["pr"], py.astype(ld) - exact["pi"])
    assert np.all(errp[ok] <= ld(2.0) ** -23 * absp[ok]), int(np.argmax(np.where(ok, errp / np.where(ok, absp, 1), 0)))
    rex = np.where(ok, exact["c"] / np.where(ok, exact["s"], 1), 0)
    errr = np.abs(r.astype(ld) - rex)
    assert np.all(errr[ok] <= ld(2.0) ** -23 * np.abs(rex[ok])), int(np.argmax(np.where(ok, errr, 0)))
    # Q as applied: i r P against the exact Q, per bin
    q = 1j * r[ok] * (px[ok] + 1j * py[ok])
    qex = (exact["qr"] + 1j * exact["qi"]).astype(np.complex128)[ok]
    assert np.max(np.abs(q - qex) / np.abs(qex)) <= 2.0 ** -21
    # bin 2048 (P = 0, Q = 2): the entry of each form, exact
    if mode == "q0":
        assert (px[2048], py[2048], r[2048]) == (2.0, 0.0, 0.0)
    else:
        assert (px[2048], py[2048], r[2048]) == (0.0, -2.0 * 2.0 ** -64, 2.0 ** 64)


def test_both_forms_agree_off_bin_2048():
    a, b = _table("q0"), _table("2p64")
    ok = np.arange(HALF) != 2048
    for u, v in zip(a, b):
        assert np.array_equal(u[ok], v[ok])
