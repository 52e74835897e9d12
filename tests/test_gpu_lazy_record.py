"""The lazily recorded stream event of the single-channel launches (ddc_runtime.cpp Readers, the
handle's `readers`) on the GPU (pytest -m gpu).

A d = 0 launch no longer records its stream's event; the event is recorded when another stream is
about to rebuild the tables the launch reads.  Here stream A is backed up with launches at tune
bin 1024, then the handle is retuned and launched on stream B at once.  The rebuild on B has to
wait for A's last launch: if the pending event were not recorded at that moment (a wait for an
event that was never recorded returns at once), the small rebuild kernel would overtake A's queue
and A's remaining launches would read the tables of the new tune bin.  So A's last output must
equal the quiet tune-bin-1024 result and B's the quiet result of the new tune bin, bit for bit,
with the lazy record on (the default) and off (SDDC_DDC_PARAM_LAZY_RECORD = 0)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK, HIST = 65536, 4096
P_LAZY_RECORD = 20   # sddc_ddc_internal.h


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.mark.parametrize("lazy", [1, 0])
def test_retune_on_second_stream_waits_for_first(torch_dev, lazy):
    torch = torch_dev
    from extio_sddc_amd import R2iq, _lib, output_samples
    nblk, tb_a, tb_b, backlog = 256, 1024, 3072, 12
    g = torch.Generator(device="cuda").manual_seed(0x5DDC)
    d_in = torch.randint(-20000, 20000, (HIST + nblk * BLOCK,), dtype=torch.int16, device="cuda", generator=g)
    n = output_samples(0, nblk) * 2

    def out():
        return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")

    with R2iq(gain=1.0, device=0) as r:
        f = r._L.sddc_ddc_internal_set_param
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        f.restype = ctypes.c_int
        _lib.check(f(r._h, P_LAZY_RECORD, lazy))
        r.setDecimate(0)
        quiet = {}
        for tb in (tb_b, tb_a):   # ends tuned to tb_a, its tables built
            r.setTuneBin(tb)
            o = out()
            r.process_device(d_in, nblk, o)
            torch.cuda.synchronize()
            quiet[tb] = o.cpu().numpy()
        assert np.all(np.isfinite(quiet[tb_a])) and not np.array_equal(quiet[tb_a], quiet[tb_b])
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        scratch, last_a, o_b = out(), out(), out()
        torch.cuda.synchronize()
        for _ in range(backlog):
            r.process_device(d_in, nblk, scratch, stream=sa)
        r.process_device(d_in, nblk, last_a, stream=sa)
        r.setTuneBin(tb_b)
        r.process_device(d_in, nblk, o_b, stream=sb)   # rebuilds the tables on sb
        torch.cuda.synchronize()
        np.testing.assert_array_equal(last_a.cpu().numpy(), quiet[tb_a])
        np.testing.assert_array_equal(o_b.cpu().numpy(), quiet[tb_b])
