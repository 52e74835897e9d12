"""The persistent kernel's (P, r) split x filter (round 6, ddc_persistent.hip build_split_filter_kernel,
ddc_frame_common.hpp split_pr), in tools/fp32_model.py's float32 model: T = P (Zk + i r conj Zc)
with P and r = Q / (i P) rounded to float32, and at bin 2048 (P = 0, r infinite) r = 2^64,
P = Q / (i 2^64).  Against the exact Zk P + conj(Zc) Q (the reference's split x filter,
fft_mt_r2iq_impl.hpp:84-98) at every d >= 1, with bin 2048 inside the band and at its edges.

The tables are built from W = e^{-2 pi i b / 8192} in double (split_coeffs.h; the model's
w_table="double").  Built from the float post8192 table (w_table="float", what the kernels did
before) the ratio r is wrong by 1e-5 at bins 2045..2051: the per-bin test holds every bin near
2048 to the form's own rounding and asserts that the float table misses it; the tone tests put
the input's energy at those bins, where the frame-maximum form with white input hides them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import fp32_model as F  # noqa: E402
from oracle import oracle as O  # noqa: E402

HALF = 4096
TONES = [2045, 2046, 2046.4, 2047, 2047.5, 2048, 2049, 2050.6, 2051]   # 8192-point bins around fs/4
REF_FLOAT_ERR = 2.6e-6   # the reference's float FFTW path against the f64 oracle


@pytest.fixture(scope="module")
def H():
    return O.filter_bank(1.0)


def _spectrum(seed, frames=2):
    rng = np.random.default_rng(seed)
    z = rng.integers(-32768, 32768, size=(frames, HALF)) + 1j * rng.integers(-32768, 32768, size=(frames, HALF))
    return np.fft.fft(z, axis=1)


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_split_pr_matches_exact(H, d):
    """float32 (P, r) split within 2^-21 of the exact one (relative to the frame's max), at tune
    bins with bin 2048 in band (middle, both edges) and out of band"""
    N = HALF >> d
    Z = _spectrum(d)
    for tb in (2048, 2048 - N // 2, 2048 + N // 2 - 4, 1024, 3000, 0, 4092):
        ex = F.split_filter(Z, d, tb, H[d], exact=True)
        pr = F.split_filter(Z, d, tb, H[d], form="pr")
        scale = np.abs(ex).max()
        assert np.abs(pr - ex).max() <= 2.0 ** -21 * scale, (d, tb)


def test_split_pr_bin_2048_entry(H):
    """the bin-2048 entry alone: Q conj(Zc) to float32 precision, though P = 0 and r is infinite"""
    d, tb = 1, 2048
    N = HALF >> d
    Z = _spectrum(7)
    ex = F.split_filter(Z, d, tb, H[d], exact=True)
    pr = F.split_filter(Z, d, tb, H[d], form="pr")
    m = 0                                  # inverse input 0 holds bin tb = 2048
    assert np.all(np.abs(ex[:, m]) > 0)
    rel = np.abs(pr[:, m] - ex[:, m]) / np.abs(ex[:, m])
    assert rel.max() <= 2.0 ** -21
    # the other bins of the band are unaffected by the special case
    assert np.abs(pr[:, 1:N] - ex[:, 1:N]).max() <= 2.0 ** -21 * np.abs(ex).max()


def _tone_spectrum(b0, frames=2):
    """Z of the packed FFT (z[n] = x[2n] + i x[2n + 1]) of frames of a tone at 8192-point bin b0"""
    from extio_sddc_amd.synth import make_tone_stream
    x = make_tone_stream(1, b0)[HALF:].astype(np.float64)
    fr = np.stack([x[6144 * k: 6144 * k + 2 * HALF] for k in range(1, 1 + frames)])
    return np.fft.fft(fr[:, 0::2] + 1j * fr[:, 1::2], axis=1)


@pytest.mark.parametrize("d,tb", [(0, 1024), (0, 2048), (1, 2048), (2, 2300), (3, 1900), (4, 2048), (5, 2044),
                                  (6, 2048)])
def test_split_pr_per_bin_near_2048(H, d, tb):
    """every in-band bin with |b - 2048| <= 16 on its own: Q as the kernel applies it, i r P from
    the float32 tables, within 2^-21 of the exact Q relative to that bin's |Q| (P and r carry one
    float32 rounding each: <= 2^-23).  The tables built from the float W miss that bar at each of
    the bins 2045..2047 and 2049..2051 (strictly: this test detects the defect, not its absence)."""
    _, bb, _, Q, _ = F.split_coeffs(d, tb, H[d])
    sel = np.flatnonzero(np.abs(bb - 2048) <= 16)
    assert sel.size == 33 and np.all(np.abs(Q[sel]) > 0)       # all of them in band
    rel = {}
    for w_table in ("double", "float"):
        _, _, P32, r32 = F.pr_tables(d, tb, H[d], w_table)
        rel[w_table] = np.abs(1j * r32.astype(np.float64) * P32 - Q)[sel] / np.abs(Q[sel])
    assert rel["double"].max() <= 2.0 ** -21, (d, tb, bb[sel][rel["double"].argmax()], rel["double"].max())
    for b in (2045, 2046, 2047, 2049, 2050, 2051):
        assert rel["float"][bb[sel] == b][0] > 2.0 ** -21, (d, tb, b)


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_split_pr_matches_exact_tones(H, d):
    """test_split_pr_matches_exact with the input's energy at the bins around 2048 (one tone per
    entry of TONES, on and off bin), where r is large and P small: same bar"""
    N = HALF >> d
    for b0 in TONES:
        Z = _tone_spectrum(b0)
        for tb in (2048, 2048 - N // 4, 2048 + N // 4 - 4):
            ex = F.split_filter(Z, d, tb, H[d], exact=True)
            pr = F.split_filter(Z, d, tb, H[d], form="pr")
            assert np.abs(pr - ex).max() <= 2.0 ** -21 * np.abs(ex).max(), (d, tb, b0)


@pytest.mark.parametrize("d,tb", [(3, 2048), (3, 1900), (4, 2048), (5, 2044)])
def test_r2iq_model_tones_vs_oracle(H, d, tb):
    """the float32 model of the d >= 3 kernels end to end on the tones, against the f64 oracle:
    within REF_FLOAT_ERR and within 4x the oracle's float32 port on the same input (the bars of
    tests/test_gpu_fs4_tones.py); with the float W table the on-bin tones next to 2048 miss both"""
    from extio_sddc_amd.synth import make_tone_stream
    H32 = O.filter_bank(1.0, np.float32)
    nblk = 2
    for b0 in TONES:
        x = make_tone_stream(nblk, b0)
        ex = O.r2iq(x, nblk, d, tb, H=H)
        port_err = O.max_rel_err(O.r2iq(x, nblk, d, tb, dtype=np.float32, H=H32), ex)
        err = O.max_rel_err(F.r2iq_model(x, nblk, d, tb, 0, 0, H[d]), ex)
        assert err <= REF_FLOAT_ERR and err <= 4 * port_err, (d, tb, b0, err, port_err)
        if b0 in (2045, 2046, 2047, 2049, 2051):
            bad = O.max_rel_err(F.r2iq_model(x, nblk, d, tb, 0, 0, H[d], w_table="float"), ex)
            assert bad > REF_FLOAT_ERR and bad > 4 * port_err, (d, tb, b0, bad, port_err)
