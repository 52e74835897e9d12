"""The d = 0 kernel's split with P of the live pairs held in registers (ddc_fs.hip, fs_cached_pairs)
on the GPU (pytest -m gpu).

The static plain instances with three or more zero rows read P of their bin pairs once per launch
instead of once per frame.  The values and the order of the operations on them do not change, so
the product must give the output of the same launch by the comparison library
(build/lib/libsddc_ddc_recomputed.so, built with -DSDDC_FS_RECOMPUTED=1: the pair counts and the
per-frame P loads as before) bit for bit, into NaN-filled buffers, and stay within the d = 0 path's
bar against the f64 oracle (1e-5 max-rel, test_gpu_fs_packed_bases.py).  Like that test, this one
fails (it does not skip) when the comparison library has not been built.

Tune bins: one per changed instance, tb = 256 (8 - z) for ZR = z = 3..8 (z = 4 is the benchmark's
1024) and tb = 2048 + 256 z for ZR = -z, z = 3..7; the rule is restated from fs_zero_rows
(ddc_fs.hip) and the list is checked against it, so it cannot stop covering an instance unseen.
Shapes: 2 blocks (22 frames: a k = 0 frame, the k = 10 -> next block step, workgroups with one
frame) against the comparison library and the oracle; 96 blocks (1056 frames on at most 1024
workgroups: the slot-weighted split and the share table) against the comparison library only.
RAND + LSB at ZR = 4 and -4: these instances take the plain ones' pair counts (the rule excludes
only the NCO and CS16 outputs).  Tones exactly on bin 2048 and on the self-mirrored columns' bins
(0, 128 + 256 k) at tb = 1024, whose band [0, 3072) holds them all: wave 0's split reads the same
registers."""
from __future__ import annotations

import numpy as np
import pytest

from extio_sddc_amd.synth import make_stream, make_tone_stream
from test_gpu_fs_packed_bases import TOL, H, _both, _device_stream, recomputed_lib, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

TOP = [(256 * (8 - z), z) for z in range(3, 9)]
BOTTOM = [(2048 + 256 * z, -z) for z in range(3, 8)]
BINS = TOP + BOTTOM


def fs_zero_rows(tb):
    """ddc_fs.hip fs_zero_rows: the zero rows of the inverse input the FS instance of tb skips"""
    top = 16 - (tb + 2048 + 255) // 256
    bot = (tb - 2048) // 256 if tb > 2048 else 0
    z = top if top > 0 else -bot if bot > 0 else 0
    z = max(-8, min(8, z))
    return 0 if abs(z) == 1 else z


def fs_cached_pairs(zr):
    """ddc_fs.hip fs_cached_pairs: the bin pairs whose P the static plain instance of ZR holds"""
    return 0 if abs(zr) < 3 else 7 if abs(zr) == 3 else 8


def test_bins_cover_every_changed_instance():
    assert [fs_zero_rows(tb) for tb, _ in BINS] == [zr for _, zr in BINS]
    changed = {zr for zr in {fs_zero_rows(tb) for tb in range(0, 4096, 4)} if fs_cached_pairs(zr) > 0}
    assert changed == {zr for _, zr in BINS} and len(BINS) == 11
    assert fs_zero_rows(1024) == 4   # the benchmark's instance


@pytest.fixture(scope="module")
def stream96(torch_dev):
    return _device_stream(torch_dev, 96, 0x5DDC)


@pytest.mark.parametrize("tb,zr", BINS)
def test_two_blocks_vs_oracle_and_comparison_library(torch_dev, recomputed_lib, oracle, H, tb, zr):
    nblk = 2
    x = make_stream(nblk, "mix")
    y = _both(torch_dev, recomputed_lib, x, nblk, tb).view(np.complex64)
    err = oracle.max_rel_err(y, oracle.r2iq(x, nblk, 0, tb, H=H))
    print(f"tb {tb} (ZR {zr}) nblk {nblk}: max-rel-err {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("tb,zr", BINS)
def test_full_residency_bit_identical_to_comparison_library(torch_dev, recomputed_lib, stream96, tb, zr):
    _both(torch_dev, recomputed_lib, stream96, 96, tb)


@pytest.mark.parametrize("tb", [1024, 3072])
def test_rand_lsb(torch_dev, recomputed_lib, oracle, H, tb):
    nblk = 2
    assert abs(fs_zero_rows(tb)) == 4
    x = make_stream(nblk, "mix")
    y = _both(torch_dev, recomputed_lib, x, nblk, tb, lsb=True, rand=True).view(np.complex64)
    err = oracle.max_rel_err(y, oracle.r2iq(x, nblk, 0, tb, True, True, H=H))
    print(f"rand + lsb tb {tb}: max-rel-err {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("tone", [2048, 0] + [128 + 256 * k for k in range(12)])
def test_tones_on_wave0_bins(torch_dev, recomputed_lib, oracle, H, tone):
    nblk, tb = 2, 1024
    assert 0 <= tone < tb + 2048   # in the band: the reference is the tone, not the filter's leakage
    x = make_tone_stream(nblk, float(tone), noise=30.0)
    y = _both(torch_dev, recomputed_lib, x, nblk, tb).view(np.complex64)
    err = oracle.max_rel_err(y, oracle.r2iq(x, nblk, 0, tb, H=H))
    print(f"tone {tone} tb {tb}: max-rel-err {err:.3e}")
    assert err <= TOL
