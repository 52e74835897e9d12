"""A strong tone next to fs/4 (8192-point bin 2048) in the passband, on a real MI355X (pytest -m gpu).

At bin b the single-channel kernels evaluate the split x filter as P (Zk + i r conj Zc) with
r = Q / (i P) = cot(pi/4 - pi b / 8192) kept as one real float (split_pr, ddc_frame_common.hpp;
split_v2, ddc_fs.hip).  Towards b = 2048 P vanishes and r grows like 1 / |b - 2048|, and so does
every error of the table: built from the float twiddle table, r was wrong by 1e-5 at bins
2045..2051 (split_coeffs.h).  No other input of the suite has energy there (the sources' tones
sit at bins 128, 584, 1026, 1565 and 3031; white input hides seven bins of 4096 in a maximum
over the frame), so these tests put it there: one tone per entry of TONES, on and off bin, for
every kernel that reads such a table (the d = 0 frame kernel, the persistent kernel at d = 0..6,
their fused NCO and CS16 instances) and for the many-channel kernels, whose plain split does not
amplify the table's rounding.

Bars, per tone, err = max|y - r| / max|r| against the f64 oracle:
  * err <= REF_FLOAT_ERR = 2.6e-6: how far the reference's own float FFTW path is from the f64
    oracle; a drop-in must not be worse than what it replaces at
    a strong in-band tone.
  * at d >= 3, err <= 4 x the error of the oracle's float32 port of the reference algorithm on
    the same input: the float32 model of these kernels (tools/fp32_model.py,
    tests/test_split_pr_model.py::test_r2iq_model_tones_vs_oracle) sits at <= 1.7 x with the
    tables as built now and at >= 20 x with the float-table r.  At d <= 2 the model does not cover
    the kernels: the ratio is recorded (SDDC_PARITY_RECORD, as tests/test_gpu_sweep.py) and
    tabulated in DESIGN.md §3, not asserted.
  * no case is leakage-only: max|r| >= -40 dB of full scale 1024 amp.

Measured (profiles/fs4_tones/): with the float-table r every single-channel case sat at 0.94-1.10e-5
at bins 2045, 2046 and 2051, 6.3-7.1e-6 at 2047 and 2049 and 1.27-1.49e-5 at 2046.4 and 2050.6
(10-68 x the port); with the tables as built now every tone is <= 8.3e-7, the d >= 3 ratios
0.42-1.63, the d <= 2 ratios 0.63-2.87.
"""
from __future__ import annotations

import numpy as np
import pytest

from extio_sddc_amd.synth import make_tone_stream
from test_gpu_sweep import _record

pytestmark = pytest.mark.gpu

TONES = [2045, 2046, 2046.4, 2047, 2047.5, 2048, 2049, 2050.6, 2051]   # 8192-point bins around fs/4
REF_FLOAT_ERR = 2.6e-6
PORT_FACTOR = 4.0        # d >= 3, against the oracle's float32 port
TOL = 1e-5               # the project's bar (channels without the tone in their passband)
AMP = 30000.0
NBLK = 2
IN_BAND = 10 ** (-40 / 20) * 1024 * AMP


@pytest.fixture(scope="module")
def ddc():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from extio_sddc_amd import R2iq
    r = R2iq(gain=1.0, device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def H(oracle):
    return oracle.filter_bank(1.0)


@pytest.fixture(scope="module")
def H32(oracle):
    return oracle.filter_bank(1.0, np.float32)


def _check_tone(oracle, H, H32, y, x, b0, d, tb, lsb, rand, what):
    """the per-tone assertions of one output y of (d, tb, lsb, rand) on the stream x"""
    r = oracle.r2iq(x, NBLK, d, tb, lsb, rand, H=H)
    port = oracle.r2iq(x, NBLK, d, tb, lsb, rand, dtype=np.float32, H=H32)
    assert np.all(np.isfinite(y))
    assert np.max(np.abs(r)) >= IN_BAND, f"{what} tone {b0}: not in the passband"
    err, port_err = oracle.max_rel_err(y, r), oracle.max_rel_err(port, r)
    print(f"{what} d={d} tb={tb} lsb={lsb} rand={rand} tone={b0}: err {err:.3e} port {port_err:.3e} "
          f"ratio {err / port_err:.2f}")
    _record({"test": "fs4 tone", "kernel": what, "d": d, "tunebin": tb, "lsb": lsb, "rand": rand, "tone_bin": b0,
             "max_rel_err": err, "port_f32_max_rel_err": port_err, "ratio": err / port_err})
    assert err <= REF_FLOAT_ERR, f"{what} d={d} tb={tb} tone {b0}: err {err:.3e} > {REF_FLOAT_ERR:.1e}"
    if d >= 3:
        assert err <= PORT_FACTOR * port_err, \
            f"{what} d={d} tb={tb} tone {b0}: err {err:.3e} > {PORT_FACTOR} x port {port_err:.3e}"


def _run(ddc, x, d, cs16=False):
    import torch
    from extio_sddc_amd import output_samples
    d_in = torch.from_numpy(x).to("cuda")
    n = output_samples(d, NBLK) * 2
    if cs16:
        out = torch.full((n,), -12345, dtype=torch.int16, device="cuda")
    else:
        out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    ddc.process_device(d_in, NBLK, out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o.reshape(-1, 2) if cs16 else o.view(np.complex64)


# d = 0 at a multiple of 4: the frame kernel (ddc_fs.hip).  Bins 2045..2047 and 2048..2051 are rows 7
# and 8 of the lane permutation's column pair, the two rows of one P row pair; bin 2048 takes the
# wave-0 (Q, 0) entry.  tb 2048: m small, both signs; tb 3072: the tb - 2048 <= b < tb branch of
# the band test.  d = 0 at tb 2046 and 2049, and d = 1..6: the persistent kernel (ddc_persistent.hip).
SINGLE = [
    (0, 1024, 0, 0), (0, 2048, 0, 0), (0, 3072, 0, 0), (0, 2048, 1, 1),
    (0, 2046, 0, 0), (0, 2049, 0, 0),
    (1, 2048, 0, 0), (1, 1536, 0, 0), (1, 2044, 1, 1),
    (2, 2048, 0, 0), (2, 2300, 0, 0),
    (3, 2048, 0, 0), (3, 1900, 0, 0),
    (4, 2048, 0, 0),
    (5, 2044, 0, 0),
    (6, 2048, 0, 0),
]


@pytest.mark.parametrize("d,tb,lsb,rand", SINGLE)
def test_single_channel_tones(ddc, oracle, H, H32, d, tb, lsb, rand):
    ddc.setDecimate(d)
    ddc.setTuneBin(tb)
    ddc.setSideband(bool(lsb))
    ddc.updateRand(bool(rand))
    for b0 in TONES:
        x = make_tone_stream(NBLK, b0, amp=AMP, rand=bool(rand))
        _check_tone(oracle, H, H32, _run(ddc, x, d), x, b0, d, tb, lsb, rand, "single")


@pytest.mark.parametrize("d", [0, 2, 4])
def test_channels_tones(ddc, oracle, H, H32, d):
    """the many-channel kernels (plain split2 from the float twiddle table: no amplification):
    channels with the tone in their passband (within N/4 of the tune bin) take the tone bars, the
    others the project's 1e-5 where they reach -40 dB"""
    import torch
    from extio_sddc_amd import output_samples
    tbs = [2048, 2044, 2052, 1024, 3000]
    N = 4096 >> d
    ddc.setDecimate(d)
    ddc.setSideband(False)
    ddc.updateRand(False)
    per = output_samples(d, NBLK) * 2
    seen = 0
    for b0 in TONES:
        x = make_tone_stream(NBLK, b0, amp=AMP)
        out = torch.full((len(tbs), per), float("nan"), dtype=torch.float32, device="cuda")
        ddc.process_channels_device(torch.from_numpy(x).to("cuda"), NBLK, tbs, out)
        torch.cuda.synchronize()
        y = out.cpu().numpy()
        assert np.all(np.isfinite(y))
        for c, tb in enumerate(tbs):
            yc = y[c].view(np.complex64)
            if abs(b0 - tb) <= N // 4:
                _check_tone(oracle, H, H32, yc, x, b0, d, tb, 0, 0, "channels")
                seen += 1
            else:
                r = oracle.r2iq(x, NBLK, d, tb, H=H)
                if np.max(np.abs(r)) >= IN_BAND:
                    assert oracle.max_rel_err(yc, r) <= TOL, f"channel tb {tb} tone {b0}"
    assert seen >= 3 * len(TONES)     # 2048, 2044 and 2052 hold every tone at every d here


def test_fused_nco_tones(oracle, H):
    """the NCO instance of the persistent kernel on the same tables (d = 1, tb 2048): the f64 oracle
    followed by the oracle mixer, as tests/test_gpu_nco.py, at the tone bar"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from extio_sddc_amd import R2iq
    d, tb, fc = 1, 2048, 0.0123
    for b0 in TONES:
        x = make_tone_stream(NBLK, b0, amp=AMP)
        with R2iq(gain=1.0) as r:       # a fresh handle: the mixer starts at phase 0
            r.setDecimate(d)
            r.setTuneBin(tb)
            r.setFineTune(fc)
            y = _run(r, x, d)
        plain = oracle.r2iq(x, NBLK, d, tb, H=H)
        assert np.max(np.abs(plain)) >= IN_BAND
        ref = oracle.Nco(fc).apply(plain.astype(np.complex64))
        err = oracle.max_rel_err(y, ref)
        print(f"nco d={d} tb={tb} tone={b0}: err {err:.3e}")
        assert np.all(np.isfinite(y))
        assert err <= REF_FLOAT_ERR, f"tone {b0}: err {err:.3e}"


def test_cs16_tones(oracle, H):
    """the CS16 instance of the d = 0 frame kernel (tb 1024): the f64 oracle followed by the same
    quantisation, as tests/test_gpu_cs16.py.  The scale puts the largest component at 30000; an
    exact input is then within 0.5 LSB of its own rounding, and an output within REF_FLOAT_ERR
    of the oracle adds at most REF_FLOAT_ERR max|r| scale LSB to that."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from extio_sddc_amd import R2iq
    d, tb = 0, 1024
    for b0 in TONES:
        x = make_tone_stream(NBLK, b0, amp=AMP)
        ref = oracle.r2iq(x, NBLK, d, tb, H=H)
        assert np.max(np.abs(ref)) >= IN_BAND
        scale = 30000.0 / float(np.max(np.abs(np.concatenate([ref.real, ref.imag]))))
        with R2iq(gain=1.0) as r:
            r.setDecimate(d)
            r.setTuneBin(tb)
            r.setOutputFormat("CS16", scale)
            c = _run(r, x, d, cs16=True)
        exact = np.stack([ref.real, ref.imag], 1) * scale
        dev = float(np.max(np.abs(c - exact)))
        bound = 0.5 + REF_FLOAT_ERR * float(np.max(np.abs(ref))) * scale
        print(f"cs16 d={d} tb={tb} tone={b0}: max dev {dev:.4f} LSB, bound {bound:.4f}")
        assert np.max(np.abs(c - np.rint(exact))) <= 1
        assert dev <= bound, f"tone {b0}: {dev:.4f} LSB > {bound:.4f}"
