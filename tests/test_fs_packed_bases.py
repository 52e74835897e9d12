"""The d = 0 kernel's packed LDS lane bases (extio_sddc_amd/csrc/fs_bases.h), compiled for the host
by tests/harness/fs_bases_harness.cpp and run here without a GPU: for all 256 threads, every base
as the frame loop unpacks it from the four packed words equals the address the loop used to
re-derive per pass (fs_slot of tests/test_fs_model.py, the F2 column formula, the padded twiddle
index), for the LDS placement the kernel has and for one with every array moved."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fs_perm as P  # noqa: E402

EXE = os.path.join(ROOT, "build", "bin", "fs_bases_harness")
LDS_SLOTS, TWL_SLOTS, TW_SLOTS = 4352, 15 * 16, 257   # float2 slots: exchange buffer, F1 / I1 table, one base table


def _slot(R, j):
    return 272 * (R >> 4) + (R >= 128) + 34 * ((R & 15) >> 1) + (R & 1) + 2 * j   # ddc_fs.hip fs_slot


def _run(lds0, twl0, wtab0):
    assert os.path.exists(EXE), "run make -C extio_sddc_amd/csrc (or __graft_entry__.build())"
    out = subprocess.run([EXE, str(lds0), str(twl0), str(wtab0)], check=True, capture_output=True, text=True).stdout
    a = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)
    assert a.shape == (256, 13)
    return a


# the kernel's placement (the arrays in declaration order) and one with gaps and another order;
# the second ends at the 16-bit limit of a packed half
@pytest.mark.parametrize("lds0,twl0,wtab0", [(0, 8 * LDS_SLOTS, 8 * (LDS_SLOTS + TWL_SLOTS)),
                                             (65536 - 8 * LDS_SLOTS, 4136, 16)])
def test_packed_bases_every_lane(lds0, twl0, wtab0):
    a = _run(lds0, twl0, wtab0)
    t = np.arange(256)
    c = np.asarray(P.read_header())
    assert np.array_equal(a[:, 0], t) and np.array_equal(a[:, 1], c)
    row, pair, col, wc, wt, twf, twi, t16, t4, tt, lane = a[:, 2:].T
    assert np.array_equal(row, lds0 + 8 * _slot(t, 0))                       # F0 stores / I2 reads
    u, j = 2 * (t >> 5) + (t & 1), (t >> 1) & 15                             # fs_pair_lane
    assert np.array_equal(pair, lds0 + 8 * _slot(u, j))                      # F1 / I1, block 0
    assert np.array_equal(pair, lds0 + 8 * (t + 2 * (t >> 5)))
    h, cl = c >> 4, c & 15
    assert np.array_equal(col, lds0 + 8 * (272 * h + (h >= 8) + 2 * cl))     # F2 reads / I0 stores
    assert np.array_equal(col, lds0 + 8 * _slot(16 * h, cl))
    assert np.array_equal(wc, wtab0 + 8 * (c + (c >= 128)))                  # W^c (W^{4c}: + 8 * 257)
    assert np.array_equal(wt, wtab0 + 8 * (t + (t >= 128)))                  # W^t
    assert np.array_equal(twf, twl0 + 8 * j)                                 # F1's table column
    assert np.array_equal(twi, twl0 + 8 * u)                                 # I1's table column
    assert np.array_equal(t16, 16 * t) and np.array_equal(t4, 4 * t)
    assert np.array_equal(tt, t) and np.array_equal(lane, t & 63)
    # every access of the loop stays inside its array: base + the largest immediate of its pass
    assert np.all(row + 8 * 2 * 15 + 8 <= lds0 + 8 * LDS_SLOTS)
    assert np.all(pair + 8 * (272 * 15 + 1) + 8 <= lds0 + 8 * LDS_SLOTS)
    assert np.all(col + 8 * (34 * 7 + 1) + 8 <= lds0 + 8 * LDS_SLOTS)
    assert np.all(wc + 8 * TW_SLOTS + 8 <= wtab0 + 8 * 2 * TW_SLOTS) and np.all(wt + 8 * TW_SLOTS + 8 <= wtab0 + 8 * 2 * TW_SLOTS)
    assert np.all(twf + 8 * 14 * 16 + 8 <= twl0 + 8 * TWL_SLOTS) and np.all(twi + 8 * 14 * 16 + 8 <= twl0 + 8 * TWL_SLOTS)
    assert a[:, 2:9].max() < 65536 and a[:, 2:9].min() >= 0


def test_kernel_lds_fits_a_packed_half():
    # the workgroup's LDS (the three arrays + the next-frame word) is 40 852 bytes: every byte
    # address in it fits 16 bits wherever the compiler places the arrays
    assert 8 * (LDS_SLOTS + TWL_SLOTS + 2 * TW_SLOTS) + 4 == 40852 < 65536
