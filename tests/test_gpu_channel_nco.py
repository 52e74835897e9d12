"""Per-channel fine-tune NCO of the many-channel DDC on the GPU (pytest -m gpu), through the C ABI.

"plain" is the same channels launch with the NCO off; "mixed" must equal
oracle.Nco(fc_c).apply(plain[c]) as uint32 for every channel (the oracle mixer is pinned bit-exact
to the reference's pf_mixer.cpp, tests/test_nco_cpu.py).  The lane-start chain runs on the device
(ddc_channels.hip channel_nco_chain_kernel), so these tests also pin its sqrt / divide against the
host chain the oracle restates.  Shapes: the smallest that reach every store path (v2 direct, v2
staged, the p kernel's LDS and L2X2 forms), frame kind (k = 0 and k >= 1), block boundary, idle
lane and second chunk.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from extio_sddc_amd.synth import make_stream

pytestmark = pytest.mark.gpu
TOL = 1e-5
PARAM_CH_NCO_RUN_BLOCKS = 9   # sddc_ddc_internal.h


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _ddc(d, lsb=False, rand=False):
    from extio_sddc_amd import R2iq
    r = R2iq(gain=1.0)
    r.setDecimate(d)
    r.setSideband(lsb)
    r.updateRand(rand)
    return r


def _fcs(nch, seed=1):
    """Channel 0 unmixed, the last at magnitude 0.4999, the rest distinct in (-0.06, 0.06)."""
    fc = np.random.default_rng(seed).uniform(-0.06, 0.06, nch).astype(np.float32)
    fc[0] = 0.0
    fc[-1] = np.float32(-0.4999 if nch % 2 else 0.4999)
    assert np.unique(fc).size == nch and np.count_nonzero(fc) == nch - 1
    return fc


def _channels(torch, r, x, nblk, d, tbs, pad=0, cs16=False):
    """One process_channels_device call -> host array [nch, nblk*(32768>>d)*2] (float32 or int16).
    pad: extra components per row (out_stride = need + pad)."""
    from extio_sddc_amd import output_samples
    need = output_samples(d, nblk) * 2
    d_in = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    if cs16:
        out = torch.full((len(tbs), need + pad), -12345, dtype=torch.int16, device="cuda")
    else:
        out = torch.full((len(tbs), need + pad), float("nan"), dtype=torch.float32, device="cuda")
    r.process_channels_device(d_in, nblk, tbs, out)
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    if pad:   # the gap between rows stays untouched
        fill = y[:, need:]
        assert (fill == -12345).all() if cs16 else np.isnan(fill).all()
    return np.ascontiguousarray(y[:, :need])


def _assert_mixed(oracle, plain, mixed, fcs):
    assert np.isfinite(plain).all()
    for c, fc in enumerate(fcs):
        p = plain[c].view(np.complex64)
        ref = p if fc == 0 else oracle.Nco(float(fc)).apply(p)
        np.testing.assert_array_equal(mixed[c].view(np.uint32), ref.view(np.float32).view(np.uint32),
                                      err_msg=f"channel {c} fc {fc}")
        if fc != 0:
            assert not np.array_equal(mixed[c].view(np.uint32), plain[c].view(np.uint32))


ADJ5 = [1000 + 4 * c for c in range(5)]
CASES = [
    # id, d, tune bins, lsb, rand, row pad
    ("d4_compact", 4, ADJ5, True, False, 0),
    ("d4_two_chunks", 4, [400 + 4 * c for c in range(131)], False, True, 0),
    ("d4_full_spectrum", 4, [0, 2048, 4092], False, False, 0),
    ("d5_staged", 5, ADJ5, False, True, 0),
    ("d6_staged", 6, ADJ5, True, False, 0),
    ("d5_direct", 5, ADJ5, True, False, 2),
    ("d6_direct", 6, ADJ5, False, True, 2),
    ("d0_lds", 0, [1024, 284, 3000], True, False, 0),
    ("d1_l2", 1, [1024, 1028, 284, 2048, 3500], False, True, 0),
    ("d3_two_chunks", 3, [600 + 4 * c for c in range(37)], True, True, 0),
]


@pytest.mark.parametrize("name,d,tbs,lsb,rand,pad", CASES, ids=[c[0] for c in CASES])
def test_channel_nco_bit_exact(torch_dev, oracle, name, d, tbs, lsb, rand, pad):
    nblk = 2
    x = make_stream(nblk, "uniform" if rand else "mix")
    fcs = _fcs(len(tbs))
    with _ddc(d, lsb, rand) as r:
        plain = _channels(torch_dev, r, x, nblk, d, tbs, pad)
        r.setChannelFineTune(fcs)
        mixed = _channels(torch_dev, r, x, nblk, d, tbs, pad)
    _assert_mixed(oracle, plain, mixed, fcs)


@pytest.mark.parametrize("d", [4, 6])
def test_channel_nco_cs16(torch_dev, d):
    """CS16 = clamp(round(CF32 NCO output * scale)), bit-exact (d = 6: the staged 16-byte stores)."""
    nblk, tbs = 2, ADJ5
    x = make_stream(nblk, "mix")
    fcs = _fcs(len(tbs))
    with _ddc(d) as r:
        r.setChannelFineTune(fcs)
        y = _channels(torch_dev, r, x, nblk, d, tbs)
        scale = np.float32(40000.0 / np.abs(y).max())   # the largest values saturate
        r.setChannelFineTune(None)
        r.setChannelFineTune(fcs)                        # phase 0 again
        r.setOutputFormat("CS16", float(scale))
        c16 = _channels(torch_dev, r, x, nblk, d, tbs, cs16=True)
    ref = np.clip(np.rint(y * scale), -32768, 32767).astype(np.int16)
    np.testing.assert_array_equal(c16, ref)
    assert np.abs(c16.astype(np.int32)).max() >= 32767


def test_channel_nco_vs_f64_oracle_pipeline(torch_dev, oracle):
    d, nblk, tbs = 4, 3, [584, 1564, 1024]
    fcs = np.array([0.0123, -0.271, 0.4999], np.float32)
    x = make_stream(nblk, "mix")
    H = oracle.filter_bank(1.0)
    with _ddc(d) as r:
        r.setChannelFineTune(fcs)
        y = _channels(torch_dev, r, x, nblk, d, tbs)
    for c, (tb, fc) in enumerate(zip(tbs, fcs)):
        ref = oracle.Nco(float(fc)).apply(oracle.r2iq(x, nblk, d, tb, H=H).astype(np.complex64))
        err = oracle.max_rel_err(y[c].view(np.complex64), ref)
        print(f"channel {c} tb {tb} fc {fc}: max-rel-err {err:.3e}")
        assert err <= TOL, f"channel {c}: {err:.3e}"


def test_channel_nco_long_chain(torch_dev, oracle):
    """8192 chain steps per channel in one launch: the device sqrt / divide against the host chain."""
    d, nblk, tbs = 0, 32, [1024, 2000]
    fcs = np.array([0.0123, -0.4999], np.float32)
    x = make_stream(nblk, "mix")
    with _ddc(d) as r:
        plain = _channels(torch_dev, r, x, nblk, d, tbs)
        r.setChannelFineTune(fcs)
        mixed = _channels(torch_dev, r, x, nblk, d, tbs)
    _assert_mixed(oracle, plain, mixed, fcs)


def test_channel_nco_phase_continues_across_calls(torch_dev):
    """Two calls of 2 blocks (with their halos) == one call of 4, bit-exact."""
    d, nblk, tbs = 1, 4, [1024, 284, 3000]
    fcs = _fcs(len(tbs))
    x = make_stream(nblk, "mix")
    with _ddc(d) as r:
        r.setChannelFineTune(fcs)
        one = _channels(torch_dev, r, x, nblk, d, tbs)
    with _ddc(d) as r:
        r.setChannelFineTune(fcs)
        a = _channels(torch_dev, r, x[:4096 + 2 * 65536], 2, d, tbs)
        b = _channels(torch_dev, r, x[2 * 65536:], 2, d, tbs)
    np.testing.assert_array_equal(one.view(np.uint32), np.concatenate([a, b], axis=1).view(np.uint32))


@pytest.mark.parametrize("d,tbs", [(4, ADJ5), (1, [1024, 284, 3000])])
def test_channel_nco_run_cut(torch_dev, d, tbs):
    """The call cut into runs of one block (chain + channels launch each) == the uncut call."""
    nblk = 3
    fcs = _fcs(len(tbs))
    x = make_stream(nblk, "mix")
    with _ddc(d) as r:
        r.setChannelFineTune(fcs)
        whole = _channels(torch_dev, r, x, nblk, d, tbs)
    with _ddc(d) as r:
        f = r._L.sddc_ddc_internal_set_param
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
        assert f(r._h, PARAM_CH_NCO_RUN_BLOCKS, 1) == 0
        r.setChannelFineTune(fcs)
        cut = _channels(torch_dev, r, x, nblk, d, tbs)
    np.testing.assert_array_equal(whole.view(np.uint32), cut.view(np.uint32))


def test_channel_nco_reinit_rule_and_off(torch_dev):
    """Per channel index: the same fc keeps the phase, a changed fc restarts at phase 0
    (RadioHandler.cpp:291-296); off = the plain DDC."""
    d, nblk, tbs = 2, 2, [1024, 284, 3000]
    fcs = np.array([0.1, -0.0371, 0.0123], np.float32)
    x = make_stream(nblk, "mix")
    with _ddc(d) as r:
        plain = _channels(torch_dev, r, x, nblk, d, tbs)
        r.setChannelFineTune(fcs)
        first = _channels(torch_dev, r, x, nblk, d, tbs)
        r.setChannelFineTune(fcs)                       # unchanged: every channel continues
        second = _channels(torch_dev, r, x, nblk, d, tbs)
        for c in range(3):
            assert not np.array_equal(first[c], second[c])
        other = fcs.copy()
        other[1] = 0.2
        r.setChannelFineTune(other)
        r.setChannelFineTune(fcs)                       # channel 1 changed and back: restarts
        third = _channels(torch_dev, r, x, nblk, d, tbs)
        np.testing.assert_array_equal(third[1].view(np.uint32), first[1].view(np.uint32))
        r.setChannelFineTune(None)
        off = _channels(torch_dev, r, x, nblk, d, tbs)
        np.testing.assert_array_equal(off.view(np.uint32), plain.view(np.uint32))
    # channels 0 and 2 of the third call continue from the second: the third call of an unbroken run
    with _ddc(d) as r:
        r.setChannelFineTune(fcs)
        for _ in range(3):
            cont = _channels(torch_dev, r, x, nblk, d, tbs)
    for c in (0, 2):
        np.testing.assert_array_equal(third[c].view(np.uint32), cont[c].view(np.uint32))
    assert not np.array_equal(third[1], cont[1])


def test_channel_nco_rejects_other_channel_count(torch_dev):
    from extio_sddc_amd import DDCError
    d, nblk = 4, 1
    x = make_stream(nblk, "mix")
    with _ddc(d) as r:
        r.setChannelFineTune([0.01, 0.02, 0.03])
        with pytest.raises(DDCError) as e:
            _channels(torch_dev, r, x, nblk, d, [100, 200])
        assert e.value.code == -4
        _channels(torch_dev, r, x, nblk, d, [100, 200, 300])   # the count that was set


def test_channels_still_reject_single_channel_nco(torch_dev):
    from extio_sddc_amd import DDCError
    d, nblk = 4, 1
    x = make_stream(nblk, "mix")
    with _ddc(d) as r:
        r.setFineTune(0.1)
        r.setChannelFineTune([0.01, 0.02])
        with pytest.raises(DDCError) as e:
            _channels(torch_dev, r, x, nblk, d, [100, 200])
        assert e.value.code == -4
        r.setFineTune(0.0)
        _channels(torch_dev, r, x, nblk, d, [100, 200])
