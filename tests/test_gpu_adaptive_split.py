"""The adaptive static frame split of the d = 0 kernel on the GPU: whatever split a launch takes
(learnt, forced, or none), its output is bit-identical to the built-in split's, since a frame's
result is a function of the frame alone.  Shapes: the smallest batch that fills the chip (one
frame per workgroup and a few left over: 94 blocks on 256 CUs) and batches below it."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from extio_sddc_amd.synth import make_stream

pytestmark = pytest.mark.gpu

TOL = 1e-5            # tests/test_gpu_parity.py: IQ within 1e-5 relative of the f64 oracle
FRAMES = 11           # frames per block
PARAM_FS_SLOT_WEIGHTS, PARAM_FS_ADAPTIVE_SPLIT = 8, 10
SLOT_WEIGHTS = (31, 26, 18, 13)   # kFsSlotWeights


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def grid(torch):
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def nblk(grid):
    return -(-grid // FRAMES)   # the smallest batch with a frame for every workgroup


@pytest.fixture(scope="module")
def stream_in(torch, nblk):
    x = make_stream(nblk, "mix")
    return x, torch.from_numpy(x).to("cuda")


class Handle:
    """an R2iq with the development entry points of its handle"""

    def __init__(self, adaptive, d=0, tb=1024, **cfg):
        from extio_sddc_amd import R2iq
        self.r = R2iq(gain=1.0, device=0)
        L = self.L = self.r._L
        L.sddc_ddc_internal_set_param.restype = ctypes.c_int
        L.sddc_ddc_internal_set_param.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.sddc_ddc_internal_fs_set_shares.restype = ctypes.c_int
        L.sddc_ddc_internal_fs_set_shares.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.sddc_ddc_internal_fs_split_state.restype = ctypes.c_int
        L.sddc_ddc_internal_fs_split_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        self.param(PARAM_FS_ADAPTIVE_SPLIT, int(adaptive))
        self.r.setDecimate(d)
        self.r.setTuneBin(tb)
        self.r.updateRand(bool(cfg.get("rand", False)))
        self.r.setSideband(bool(cfg.get("lsb", False)))
        self.cs16 = bool(cfg.get("cs16", False))
        if self.cs16:
            self.r.setOutputFormat("CS16", 0.5)
        if cfg.get("fine_tune"):
            self.r.setFineTune(cfg["fine_tune"])

    def param(self, k, v):
        assert self.L.sddc_ddc_internal_set_param(self.r._h, k, v) == 0

    def shares(self, sh):
        sh = np.ascontiguousarray(sh, np.float32)
        assert self.L.sddc_ddc_internal_fs_set_shares(self.r._h, sh.ctypes.data, sh.size) == 0

    def state(self):
        info = (ctypes.c_long * 5)()
        counts = np.zeros(2048, np.int32)
        n = self.L.sddc_ddc_internal_fs_split_state(self.r._h, info, counts.ctypes.data, counts.size)
        return dict(grid=info[0], measured=info[1], skipped=info[2], table=info[3], logged=info[4]), counts[:n]

    def run(self, torch, d_in, nblk, stream=None):
        from extio_sddc_amd import output_samples
        n = output_samples(0, nblk) * 2
        if self.cs16:
            out = torch.full((n,), -12345, dtype=torch.int16, device="cuda")
        else:
            out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())   # the fill above
        self.r.process_device(d_in, nblk, out, stream)
        return out

    def close(self):
        self.r.close()


def same_bits(torch, a, b):
    if a.dtype == torch.float32:
        return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    return bool(torch.equal(a, b))


@pytest.fixture(scope="module")
def plain_off(torch, stream_in, nblk):
    """the adaptation-off output of the plain configuration at the full-residency batch"""
    h = Handle(False)
    out = h.run(torch, stream_in[1], nblk)
    torch.cuda.synchronize()
    st, _ = h.state()
    h.close()
    assert st["table"] == 0 and st["logged"] == 0 and st["measured"] == 0
    assert not bool(torch.isnan(out).any())
    return out


def test_adapting_launches_are_bit_identical(torch, oracle, stream_in, nblk, grid, plain_off):
    x, d_in = stream_in
    h = Handle(True)
    try:
        for i in range(30):
            out = h.run(torch, d_in, nblk)
            torch.cuda.synchronize()
            assert same_bits(torch, out, plain_off), f"launch {i}"
            st, counts = h.state()
            assert st["logged"] == 1
        # every launch after the first found its predecessor's times complete
        assert st["grid"] == grid and st["measured"] >= 25 and st["table"] == 1, st
        assert counts.size == grid and counts.sum() == nblk * FRAMES
    finally:
        h.close()
    # the first blocks against the f64 oracle (they do not depend on the blocks after them)
    nb = 4
    y = plain_off[: nb * 32768 * 2].cpu().numpy().view(np.complex64)
    ref = oracle.r2iq(x[: 4096 + nb * 65536], nb, 0, 1024)
    assert oracle.max_rel_err(y, ref) <= TOL


def forced_tables(grid):
    w = np.repeat(np.array(SLOT_WEIGHTS, float), grid // 4)
    alt = w * np.where(np.arange(grid) % 2 == 0, 0.75, 1.25)      # all weight at the clamps, alternating
    empty = w.copy()
    empty[[0, 7, grid // 2, grid - 1]] = 0.0                      # workgroups with an empty range
    return {"clamps alternating": alt, "empty ranges": empty, "reversed slots": w[::-1].copy(),
            "one workgroup takes half": np.where(np.arange(grid) == 3, float(grid), 1.0)}


@pytest.mark.parametrize("name", ["clamps alternating", "empty ranges", "reversed slots", "one workgroup takes half"])
def test_forced_share_tables(torch, stream_in, nblk, grid, plain_off, name):
    h = Handle(True)
    try:
        h.shares(forced_tables(grid)[name])
        out = h.run(torch, stream_in[1], nblk)
        torch.cuda.synchronize()
        st, counts = h.state()
        assert st["table"] == 1 and st["logged"] == 0, st   # the given table, nothing measured
        assert counts.sum() == nblk * FRAMES
        if name == "empty ranges":
            assert counts[0] == 0 and counts[grid - 1] == 0
        if name == "one workgroup takes half":
            assert counts[3] >= nblk * FRAMES // 2 - 1
        assert same_bits(torch, out, plain_off)
        h.shares(np.zeros(0, np.float32))   # cleared: back to the controller
        out = h.run(torch, stream_in[1], nblk)
        torch.cuda.synchronize()
        assert same_bits(torch, out, plain_off)
        assert h.state()[0]["logged"] == 1
    finally:
        h.close()


@pytest.mark.parametrize("nb", [1, 8])
def test_below_full_residency_is_untouched(torch, stream_in, nb):
    d_in = stream_in[1][: 4096 + nb * 65536].contiguous()
    outs = []
    for adaptive in (False, True):
        h = Handle(adaptive)
        try:
            for _ in range(3):
                out = h.run(torch, d_in, nb)
                torch.cuda.synchronize()
                st, _ = h.state()
                assert st["table"] == 0 and st["logged"] == 0 and st["measured"] == 0, st
            outs.append(out)
        finally:
            h.close()
    assert not bool(torch.isnan(outs[0]).any())
    assert same_bits(torch, outs[0], outs[1])


def test_explicit_slot_weights_are_untouched(torch, stream_in, nblk, plain_off):
    h = Handle(True)
    try:
        h.param(PARAM_FS_SLOT_WEIGHTS, 20 | (20 << 8) | (20 << 16) | (20 << 24))
        for _ in range(2):
            out = h.run(torch, stream_in[1], nblk)
            torch.cuda.synchronize()
            st, _ = h.state()
            assert st["table"] == 0 and st["logged"] == 0, st
        assert same_bits(torch, out, plain_off)
    finally:
        h.close()


OTHER = {"rand": dict(rand=True), "lsb": dict(lsb=True), "cs16": dict(cs16=True),
         "fused nco": dict(fine_tune=0.0123), "tune bin 0 (8 zero rows)": dict(tb=0),
         "tune bin 2048 (no zero row)": dict(tb=2048), "tune bin 3332 (5 zero rows below)": dict(tb=3332)}


@pytest.mark.parametrize("name", list(OTHER))
def test_other_instances(torch, stream_in, nblk, name):
    """three launches each with the adaptation off and on (the second and third of `on` take a
    learnt table): launch k's outputs agree (the fused NCO's phase runs on from launch to launch)"""
    outs = {}
    for adaptive in (False, True):
        h = Handle(adaptive, **OTHER[name])
        try:
            outs[adaptive] = []
            for k in range(3):
                outs[adaptive].append(h.run(torch, stream_in[1], nblk))
                torch.cuda.synchronize()
            st, _ = h.state()
            assert st["table"] == int(adaptive) and st["logged"] == int(adaptive), st
            assert not adaptive or st["measured"] >= 1
        finally:
            h.close()
    for k in range(3):
        o = outs[False][k]
        assert not bool((o == -12345).all()) if o.dtype == torch.int16 else not bool(torch.isnan(o).any())
        assert same_bits(torch, outs[False][k], outs[True][k]), f"launch {k}"


def test_two_streams_on_one_handle(torch, stream_in, nblk, plain_off):
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    h = Handle(True)
    try:
        for rnd in range(3):
            outs = [h.run(torch, stream_in[1], nblk, s[i % 2]) for i in range(8)]
            torch.cuda.synchronize()
            for i, o in enumerate(outs):
                assert same_bits(torch, o, plain_off), f"round {rnd} launch {i}"
        st, _ = h.state()
        # launches that may have overlapped another one of the handle teach nothing
        assert st["measured"] == 0 and st["logged"] == 1, st
    finally:
        h.close()
