"""The d = 0 kernel's frame loop on packed LDS lane bases (ddc_fs.hip, fs_bases.h) on the GPU
(pytest -m gpu).

The packed bases change no floating-point operation or its order, so the product library must give
the output of the same launch by the comparison library (build/lib/libsddc_ddc_recomputed.so: the
same sources built with -DSDDC_FS_RECOMPUTED=1, whose static instances re-derive the bases in every
pass as before; the product itself carries no second set of instances and no switch) bit for bit,
into NaN-filled (CS16: pattern-filled) buffers, and stay within the bars the d = 0 path already has
against the f64 oracle: 1e-5 max-rel for CF32 (test_fs_zero_rows; with the fused NCO against the
oracle DDC followed by the oracle mixer, test_gpu_nco.py), 1 LSB for CS16 (test_gpu_cs16.py).
Shapes: 1 and 3 blocks (11 and 33 frames: a workgroup has one frame or none, the k = 0 frame and a
block boundary), 64 blocks (full residency, several frames per workgroup); the tune bins of ZR = 4
(1024, the benchmark's), 8 (0), 0 (2048, the if / else form), -4 (3072) and 2 (1280, 8-byte P
halves); RAND + LSB, CS16 and the NCO at 1024; tones exactly at bins 0, 2048 + 128 and 2048 (the
self-mirrored columns 0 and 128 of wave 0's lanes 0 and 1, and the b = 2048 entry).
The oracle check runs at 1 and 3 blocks; the 64-block launches (plain, RAND + LSB, CS16, NCO) are
held to the comparison library's output only, which the small cases tie to the oracle (a 64-block
f64 oracle run would take longer than every other case together)."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from extio_sddc_amd.synth import make_stream, make_tone_stream

pytestmark = pytest.mark.gpu

TOL = 1e-5
BLOCK, HIST = 65536, 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECOMPUTED = os.path.join(ROOT, "build", "lib", "libsddc_ddc_recomputed.so")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def H(oracle):
    return oracle.filter_bank(1.0)


@pytest.fixture(scope="module")
def recomputed_lib():
    from extio_sddc_amd import _lib
    _lib.load()   # the product first: both share torch's HIP runtime
    assert os.path.exists(RECOMPUTED), "run make -C extio_sddc_amd/csrc (or __graft_entry__.build())"
    L = ctypes.CDLL(RECOMPUTED)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _handle(lib, tb, lsb=False, rand=False, fc=0.0, cs16_scale=0.0):
    """an R2iq on the product library (lib None) or on the comparison library"""
    from extio_sddc_amd import R2iq, _lib
    product = _lib.load()
    try:
        if lib is not None:
            _lib._lib = lib   # R2iq binds the library that load() returns when it is constructed
        r = R2iq(gain=1.0, device=0)
    finally:
        _lib._lib = product
    assert r._L is (lib if lib is not None else product)
    r.setDecimate(0)
    r.setTuneBin(tb)
    r.setSideband(lsb)
    r.updateRand(rand)
    if fc:
        r.setFineTune(fc)
    if cs16_scale:
        r.setOutputFormat("CS16", cs16_scale)
    return r


def _launch(torch, r, d_in, nblk, cs16=False):
    from extio_sddc_amd import output_samples
    n = output_samples(0, nblk) * 2
    if cs16:
        out = torch.full((n,), -12345, dtype=torch.int16, device="cuda")
    else:
        out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    r.process_device(d_in, nblk, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _both(torch, rlib, x, nblk, tb, **kw):
    """the launch by the product (packed bases) and by the comparison library; asserts they are equal"""
    d_in = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    outs = []
    for lib in (None, rlib):
        with _handle(lib, tb, **kw) as r:
            outs.append(_launch(torch, r, d_in, nblk, cs16=bool(kw.get("cs16_scale"))))
    if not kw.get("cs16_scale"):
        assert np.all(np.isfinite(outs[0]))
    np.testing.assert_array_equal(outs[0], outs[1])
    return outs[0]


def _device_stream(torch, nblk, seed):
    """[4096 zero history | nblk blocks] int16 on the GPU: the synth 'mix' recipe on the device"""
    n = nblk * BLOCK
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64, device="cuda")
    x = 9000 * torch.sin(2 * np.pi * torch.frac(0.0713 * t)) + 3000 * torch.sin(2 * np.pi * torch.frac(0.191 * t))
    x += 300 * torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    x = torch.clamp(torch.round(x), -32768, 32767).to(torch.int16)
    return torch.cat([torch.zeros(HIST, dtype=torch.int16, device="cuda"), x])


@pytest.fixture(scope="module")
def stream64(torch_dev):
    return _device_stream(torch_dev, 64, 0x5DDC)


@pytest.mark.parametrize("tb", [1024, 0, 2048, 3072, 1280])
@pytest.mark.parametrize("nblk", [1, 3])
def test_small_batches_vs_oracle_and_recomputed(torch_dev, recomputed_lib, oracle, H, tb, nblk):
    x = make_stream(nblk, "mix")
    y = _both(torch_dev, recomputed_lib, x, nblk, tb).view(np.complex64)
    err = oracle.max_rel_err(y, oracle.r2iq(x, nblk, 0, tb, H=H))
    print(f"tb {tb} nblk {nblk}: max-rel-err {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("tb", [1024, 0, 2048, 3072, 1280])
def test_full_residency_bit_identical_to_recomputed(torch_dev, recomputed_lib, stream64, tb):
    _both(torch_dev, recomputed_lib, stream64, 64, tb)


def test_rand_lsb(torch_dev, recomputed_lib, oracle, H, stream64):
    nblk, tb = 3, 1024
    x = make_stream(nblk, "uniform")
    y = _both(torch_dev, recomputed_lib, x, nblk, tb, lsb=True, rand=True).view(np.complex64)
    err = oracle.max_rel_err(y, oracle.r2iq(x, nblk, 0, tb, True, True, H=H))
    print(f"rand + lsb: max-rel-err {err:.3e}")
    assert err <= TOL
    _both(torch_dev, recomputed_lib, stream64, 64, tb, lsb=True, rand=True)


def test_cs16(torch_dev, recomputed_lib, oracle, H, stream64):
    nblk, tb = 3, 1024
    x = make_stream(nblk, "mix")
    ref = oracle.r2iq(x, nblk, 0, tb, H=H)
    scale = 30000.0 / float(np.max(np.abs(np.concatenate([ref.real, ref.imag]))))
    c = _both(torch_dev, recomputed_lib, x, nblk, tb, cs16_scale=scale).reshape(-1, 2)
    lsb = np.max(np.abs(c - np.rint(np.stack([ref.real, ref.imag], 1) * scale)))
    print(f"cs16: {lsb} LSB")
    assert lsb <= 1
    _both(torch_dev, recomputed_lib, stream64, 64, tb, cs16_scale=scale)


def test_fused_nco(torch_dev, recomputed_lib, oracle, H, stream64):
    nblk, tb, fc = 3, 1024, 0.0123
    x = make_stream(nblk, "mix")
    y = _both(torch_dev, recomputed_lib, x, nblk, tb, fc=fc).view(np.complex64)
    ref = oracle.Nco(fc).apply(oracle.r2iq(x, nblk, 0, tb, H=H).astype(np.complex64))
    err = oracle.max_rel_err(y, ref)
    print(f"nco: max-rel-err {err:.3e}")
    assert err <= TOL
    _both(torch_dev, recomputed_lib, stream64, 64, tb, fc=fc)


# Tones exactly on the bins of the self-mirrored columns, each at a tune bin that has the tone in
# the passband (so the reference is the tone, not the filter's leakage), and at the benchmark's
# tune bin 1024 (ZR = 4) with a little noise, which has bins 0 and 2176 in its band
@pytest.mark.parametrize("tone,tb,noise", [(0, 0, 0.0), (2048 + 128, 2048, 0.0), (2048, 2048, 0.0),
                                           (0, 1024, 30.0), (2048 + 128, 1024, 30.0)])
def test_tones_on_the_self_mirrored_columns(torch_dev, recomputed_lib, oracle, H, tone, tb, noise):
    nblk = 1
    x = make_tone_stream(nblk, float(tone), noise=noise)
    y = _both(torch_dev, recomputed_lib, x, nblk, tb).view(np.complex64)
    err = oracle.max_rel_err(y, oracle.r2iq(x, nblk, 0, tb, H=H))
    print(f"tone {tone} tb {tb}: max-rel-err {err:.3e}")
    assert err <= TOL
