"""The channel audio resampler on the CPU backend (no GPU): the C ABI's five symbols and their error
returns, sddc_ddc_channel_audio_resample_host of a CPU handle against the numpy model of the definition
(tools/channel_audio_resample_model.py) EXACTLY and against the float64 sum within the derived bound,
the output counts, the stream cut into calls, reset and set, a change of the input format inside a
stream, the S16 rounding, and the kernel's LDS layout against its numpy bank model
(tools/channel_audio_resample_banks.py).

The bars.  Exact: the CPU handle's bits are the model's, the definition's sequence a[j mod 4] =
fmaf(h[p + jL], x[s - j], a[j mod 4]), y = (a0 + a1) + (a2 + a3) in correctly rounded float32.  Bound:
every F32 output within gamma sum_j |h[p + jL]| |x[s - j]|, gamma = n u / (1 - n u), n = K + 1, u = 2^-24,
of the float64 sum, per output from the model's own sum; S16 output within that plus 1/2 of the
clamped sum.
Ratios (L, M, ntaps): 1/6 x 97, 1/4 x 65, 24/125 x 1536, 2/3 x 40, 3/2 x 7 (L > M), 32/1 x 100 (M = 1),
1/256 x 300, 5/7 x 4 (K = 1: ntaps <= L) and 3/250 x 3072 (K = 1024).
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


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


AM = _load("channel_audio_resample_model")
BK = _load("channel_audio_resample_banks")

from extio_sddc_amd import AUDIO_F32, AUDIO_S16, DEVICE_CPU, DDCError, R2iq, _lib, resample_count  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
SYMBOLS = ["sddc_ddc_set_channel_audio_resampler", "sddc_ddc_channel_audio_resampler_reset",
           "sddc_ddc_channel_audio_resample_samples", "sddc_ddc_channel_audio_resample_device",
           "sddc_ddc_channel_audio_resample_host"]
RATIOS = [(1, 6, 97), (1, 4, 65), (24, 125, 1536), (2, 3, 40), (3, 2, 7), (32, 1, 100), (1, 256, 300), (5, 7, 4),
          (3, 250, 3072)]
FORMATS = [(AUDIO_F32, AUDIO_F32), (AUDIO_F32, AUDIO_S16), (AUDIO_S16, AUDIO_F32), (AUDIO_S16, AUDIO_S16)]
FMT_IDS = ["f32-f32", "f32-s16", "s16-f32", "s16-s16"]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
NOUT = 45   # outputs per channel of the model comparisons: every phase of L <= 32 and a ragged end


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def signal(kind, nch, nsamp, fmt):
    x = AM.make_input(kind, nch, nsamp, fmt)
    x.setflags(write=False)
    return x


def taps_for(ntaps, fout):
    """S16 out: the sum of |h| is about sqrt(ntaps) / 2, so noise of sigma 3000 stays inside int16 most
    of the time and clamps now and then."""
    return AM.make_taps(ntaps) * np.float32(0.25 if fout == AUDIO_S16 else 1.0)


def same(y, ref):
    assert y.dtype == ref.dtype and y.shape == ref.shape
    if y.dtype == np.float32:
        y, ref = np.ascontiguousarray(y).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)
    np.testing.assert_array_equal(y, ref)


def run_cuts(r, x, cuts):
    """The stream x in calls of `cuts` samples -> [nch, total outputs]."""
    assert sum(cuts) == x.shape[1]
    at, outs = 0, []
    for n in cuts:
        want = r.channel_audio_resample_samples(n)
        y = r.channel_audio_resample_host(np.ascontiguousarray(x[:, at:at + n]))
        assert y.shape == (x.shape[0], want)
        outs.append(y)
        at += n
    return np.concatenate(outs, axis=1)


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chars_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint64], ctypes.c_int
    return f(r._h, pos)


def test_the_interface_declares_exports_and_binds_the_five_symbols():
    header = open(os.path.join(ROOT, "include", "sddc_ddc.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"#define\s+SDDC_DDC_ABI_VERSION\s+3\b", header) and lib.sddc_ddc_abi_version() == 3
    internal = open(os.path.join(ROOT, "extio_sddc_amd", "csrc", "sddc_ddc_internal.h")).read()
    assert re.search(r"#define\s+SDDC_DDC_PARAM_CHARS_MAX_WGS\s+30\b", internal)


def test_model_against_the_literal_definition():
    """Zero-stuff by L, convolve, keep every M-th sample: the float64 sum of the model; and the float32
    model within the bound of it."""
    for L, M, ntaps in ((2, 3, 40), (3, 2, 7), (5, 7, 4), (1, 4, 65)):
        h = AM.make_taps(ntaps)
        for nsamp in (1, M, 3 * M + 1, 211):
            x = signal("noise", 2, nsamp, AUDIO_F32)
            ref = AM.resample64(x, h, L, M)
            assert ref.shape == (2, AM.count(L, M, 0, nsamp))
            for c in range(2):
                u = np.zeros(nsamp * L)
                u[::L] = x[c]
                v = np.convolve(u, h.astype(np.float64))[:nsamp * L][::M]
                np.testing.assert_allclose(ref[c], v, rtol=0, atol=1e-9 * np.abs(x).max())
            assert AM.excess(AM.resample32(x, h, L, M), x, h, L, M) <= 0.0


@pytest.mark.parametrize("fmts", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("ratio", RATIOS, ids=IDS)
def test_cpu_handle_is_the_model_exactly_and_holds_the_bound(cpu, ratio, fmts):
    L, M, ntaps = ratio
    fin, fout = fmts
    h = taps_for(ntaps, fout)
    nsamp = AM.nsamp_for(L, M, NOUT) + (1 if M > L else 0)
    for kind in ("noise", "edges"):
        x = signal(kind, 2, nsamp, fin)
        cpu.setChannelAudioResampler(h, L, M, 2, fin, fout)
        y = cpu.channel_audio_resample_host(x)
        assert y.shape == (2, AM.count(L, M, 0, nsamp)) and y.shape[1] >= NOUT
        same(y, AM.resample_fmt(x, h, L, M, fout))
        e = AM.excess(y, x, h, L, M, fout)
        print(f"{kind} {IDS(ratio)} {FMT_IDS[FORMATS.index(fmts)]}: |y - y64| - bound <= {e:.3e}")
        assert e <= 0.0 and np.abs(y.astype(np.float64)).max() > 0
    if ntaps <= L:   # K = 1: a phase past the taps has none, its outputs are zero
        p = (np.arange(y.shape[1]) * M) % L
        assert (y[:, p >= ntaps] == 0).all() and (y[:, p < ntaps] != 0).all()


@pytest.mark.parametrize("ratio", [(1, 6, 97), (24, 125, 1536), (3, 2, 7), (1, 256, 300)], ids=IDS)
def test_counts_at_positions_and_the_zero_output_call(cpu, ratio):
    L, M, ntaps = ratio
    h = AM.make_taps(ntaps)
    x = signal("noise", 2, 2 * M + 3, AUDIO_F32)
    for pos in (0, 1, M - 1, 2 ** 32 + 5, 2 ** 40 * M + 1):
        cpu.setChannelAudioResampler(h, L, M, 2)
        assert set_position(cpu, pos) == 0
        for n in (1, 2, M, 2 * M + 3):
            want = AM.count(L, M, pos, n)
            assert resample_count(L, M, pos, n) == want and cpu.channel_audio_resample_samples(n) == want
        y = cpu.channel_audio_resample_host(x)
        assert y.shape == (2, AM.count(L, M, pos, x.shape[1]))
        assert cpu.channel_audio_resample_samples(5) == AM.count(L, M, pos + x.shape[1], 5)
    if M >= 2 and M > L:
        # one sample at position 1: no output, nothing written, and the stream still advances
        cpu.setChannelAudioResampler(h, L, M, 2)
        whole = cpu.channel_audio_resample_host(x)
        cpu.channel_audio_resampler_reset()
        first = cpu.channel_audio_resample_host(x[:, :1])
        assert cpu.channel_audio_resample_samples(1) == 0
        out = np.full((2, 4), np.nan, np.float32)
        got = ctypes.c_size_t(7)
        one = np.ascontiguousarray(x[:, 1:2])
        assert cpu._L.sddc_ddc_channel_audio_resample_host(cpu._h, one.ctypes.data, 2, 1, 1, out.ctypes.data, 4,
                                                           ctypes.addressof(got)) == 0
        assert got.value == 0 and np.isnan(out).all()
        rest = cpu.channel_audio_resample_host(np.ascontiguousarray(x[:, 2:]))
        same(np.concatenate([first, rest], axis=1), whole)


@pytest.mark.parametrize("fmts", [FORMATS[0], FORMATS[3]], ids=[FMT_IDS[0], FMT_IDS[3]])
@pytest.mark.parametrize("ratio", [(1, 6, 97), (24, 125, 1536), (3, 2, 7), (3, 250, 3072)], ids=IDS)
def test_cuts_reset_and_set_give_identical_bits(cpu, ratio, fmts):
    L, M, ntaps = ratio
    fin, fout = fmts
    K = -(-ntaps // L)
    h = taps_for(ntaps, fout)
    nsamp = max(AM.nsamp_for(L, M, NOUT), 2 * K + M + 110)
    x = signal("noise", 2, nsamp, fin)
    cpu.setChannelAudioResampler(h, L, M, 2, fin, fout)
    whole = cpu.channel_audio_resample_host(x)
    same(whole, AM.resample_fmt(x, h, L, M, fout))
    for cuts in ([1, 1, max(K - 2, 1), K], [100, M]):
        cuts = cuts + [nsamp - sum(cuts)]
        cpu.channel_audio_resampler_reset()          # a reset restarts the stream
        same(run_cuts(cpu, x, cuts), whole)
        cpu.setChannelAudioResampler(h, L, M, 2, fin, fout)   # and so does a set
        same(run_cuts(cpu, x, cuts), whole)
    # without either the stream goes on: the second pass is not the first
    again = cpu.channel_audio_resample_host(x)
    assert again.shape[1] != whole.shape[1] or not np.array_equal(again, whole)


def test_the_input_format_may_switch_inside_a_stream(cpu):
    """The tails hold values: integer-valued samples fed as F32, then as S16, then as F32 give the bits
    of the one-format stream."""
    L, M, ntaps = 2, 3, 40
    h = AM.make_taps(ntaps)
    xs = signal("noise", 2, 300, AUDIO_S16)
    xf = xs.astype(np.float32)
    cpu.setChannelAudioResampler(h, L, M, 2, AUDIO_F32, AUDIO_F32)
    whole = cpu.channel_audio_resample_host(xf)
    cpu.channel_audio_resampler_reset()
    parts = [cpu.channel_audio_resample_host(np.ascontiguousarray(xf[:, :7]))]
    cpu.setChannelAudioResamplerFormats(AUDIO_S16, AUDIO_F32)
    parts.append(cpu.channel_audio_resample_host(np.ascontiguousarray(xs[:, 7:150])))
    cpu.setChannelAudioResamplerFormats(AUDIO_F32, AUDIO_F32)
    parts.append(cpu.channel_audio_resample_host(np.ascontiguousarray(xf[:, 150:])))
    same(np.concatenate(parts, axis=1), whole)
    assert cpu._L.sddc_ddc_channel_audio_resampler_formats(cpu._h, 2, 0) == ERR_ARG


def test_s16_output_saturates_and_maps_nan_to_zero(cpu):
    """L = 1, M = 2, one tap of 1.0: y[m] = x[2 m], so the rounding alone shows."""
    x = np.zeros((1, 24), np.float32)
    x[0, ::2] = [32766.5, 32767.0, 32767.5, 1e9, np.inf, -32768.0, -32768.5, -1e9, -np.inf, np.nan, 0.5, 1.5]
    want = np.array([32766, 32767, 32767, 32767, 32767, -32768, -32768, -32768, -32768, 0, 0, 2], np.int16)
    cpu.setChannelAudioResampler(np.ones(1, np.float32), 1, 2, 1, AUDIO_F32, AUDIO_S16)
    y = cpu.channel_audio_resample_host(x)
    np.testing.assert_array_equal(y[0], want)
    np.testing.assert_array_equal(AM.to_s16(x[0, ::2]), want)
    # a gain of 2 on full-scale S16 input: both rails
    cpu.setChannelAudioResampler(np.full(1, 2.0, np.float32), 1, 2, 1, AUDIO_S16, AUDIO_S16)
    y = cpu.channel_audio_resample_host(np.array([[32767, 0, -32768, 0, 16383, 0, -16384, 0]], np.int16))
    np.testing.assert_array_equal(y[0], np.array([32767, -32768, 32766, -32768], np.int16))


def test_error_returns_and_a_failed_call_changes_no_state(cpu):
    L_, hd = cpu._L, cpu._h
    sets, host = L_.sddc_ddc_set_channel_audio_resampler, L_.sddc_ddc_channel_audio_resample_host
    nch, L, M, ntaps, nsamp = 3, 3, 7, 20, 40
    taps = AM.make_taps(ntaps)
    tp = taps.ctypes.data
    x = np.ascontiguousarray(np.concatenate([signal("noise", nch, nsamp, AUDIO_F32), np.full((nch, 3), np.nan, np.float32)], axis=1))
    S, nout = x.shape[1], AM.count(L, M, 0, nsamp)
    out = np.full((nch, nout + 2), np.nan, np.float32)
    OS = out.shape[1]
    xi, oi = x.ctypes.data, out.ctypes.data
    got = ctypes.c_size_t(99)
    gp = ctypes.addressof(got)
    assert host(hd, xi, nch, nsamp, S, oi, OS, gp) == ERR_STATE                       # nothing set
    assert L_.sddc_ddc_channel_audio_resampler_reset(hd) == ERR_STATE
    assert L_.sddc_ddc_channel_audio_resampler_formats(hd, 0, 0) == ERR_STATE
    assert cpu.channel_audio_resample_samples(nsamp) == 0
    with pytest.raises(DDCError):
        cpu.channel_audio_resample_host(x)
    big = np.zeros(4097, np.float32)
    assert sets(hd, big.ctypes.data, 4097, L, M, nch, 0, 0) == ERR_ARG
    assert sets(hd, big.ctypes.data, 1025, 1, 2, nch, 0, 0) == ERR_ARG               # K = 1025
    for up, down in ((0, M), (33, M), (L, 0), (L, 257), (2, 4), (6, 9), (1, 1)):
        assert sets(hd, tp, ntaps, up, down, nch, 0, 0) == ERR_ARG
    assert sets(hd, tp, ntaps, L, M, 0, 0, 0) == ERR_ARG
    assert sets(hd, tp, ntaps, L, M, 1025, 0, 0) == ERR_ARG
    assert sets(hd, tp, ntaps, L, M, nch, 2, 0) == ERR_ARG                           # formats
    assert sets(hd, tp, ntaps, L, M, nch, 0, -1) == ERR_ARG
    for bad in (np.inf, np.nan):
        t = taps.copy()
        t[ntaps - 1] = bad
        assert sets(hd, t.ctypes.data, ntaps, L, M, nch, 0, 0) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, oi, OS, gp) == ERR_STATE                       # a failed set sets nothing
    cpu.setChannelAudioResampler(taps, L, M, nch)
    good = cpu.channel_audio_resample_host(x[:, :nsamp])
    same(good, AM.resample32(x[:, :nsamp], taps, L, M))
    cpu.setChannelAudioResampler(taps, L, M, nch)
    assert host(hd, xi, nch - 1, nsamp, S, oi, OS, gp) == ERR_STATE                   # another nch than the set one
    assert host(hd, xi, nch, 0, S, oi, OS, gp) == ERR_ARG
    assert host(hd, xi, nch, 2 ** 40 + 1, 2 ** 41, oi, 2 ** 41, gp) == ERR_ARG
    assert host(hd, xi, nch, nsamp, nsamp - 1, oi, OS, gp) == ERR_ARG                 # strides
    assert host(hd, xi, nch, nsamp, S, oi, nout - 1, gp) == ERR_ARG
    assert host(hd, xi + 2, nch, nsamp, S, oi, OS, gp) == ERR_ARG                     # F32: 4-byte samples
    assert host(hd, xi, nch, nsamp, S, oi + 2, OS, gp) == ERR_ARG
    assert host(hd, None, nch, nsamp, S, oi, OS, gp) == ERR_ARG
    assert host(hd, xi, nch, nsamp, S, None, OS, gp) == ERR_ARG
    assert L_.sddc_ddc_channel_audio_resample_device(hd, xi, nch, nsamp, S, oi, OS, gp, None) == ERR_STATE   # a CPU handle
    assert got.value == 99 and np.isnan(out).all()
    # the failed calls changed no state: the next valid call is the first call of the stream, with odd
    # strides (any parity) and nothing written between the streams
    assert cpu.channel_audio_resample_samples(nsamp) == nout
    assert host(hd, xi, nch, nsamp, S, oi, OS, gp) == 0 and got.value == nout
    same(np.ascontiguousarray(out[:, :nout]), good)
    assert np.isnan(out[:, nout:]).all()
    # S16 buffers need 2-byte alignment only
    cpu.setChannelAudioResampler(taps, L, M, 1, AUDIO_S16, AUDIO_S16)
    xs = np.zeros(nsamp + 1, np.int16)
    ys = np.zeros(nout + 1, np.int16)
    assert host(hd, xs.ctypes.data + 1, 1, nsamp, 0, ys.ctypes.data, 0, gp) == ERR_ARG
    assert host(hd, xs.ctypes.data, 1, nsamp, 0, ys.ctypes.data + 1, 0, gp) == ERR_ARG
    assert host(hd, xs.ctypes.data + 2, 1, nsamp, 0, ys.ctypes.data + 2, 0, gp) == 0
    cpu.setChannelAudioResampler(None)
    assert host(hd, xi, nch, nsamp, S, oi, OS, gp) == ERR_STATE


def test_both_resamplers_on_one_handle_are_independent(cpu):
    L, M, ntaps = 2, 3, 40
    h = AM.make_taps(ntaps)
    x = signal("noise", 2, 120, AUDIO_F32)
    cpu.setChannelAudioResampler(h, L, M, 2)
    alone = run_cuts(cpu, x, [50, 70])
    cpu.setChannelAudioResampler(h, L, M, 2)
    cpu.setChannelResampler(h, 3, 5, 2)
    first = cpu.channel_audio_resample_host(np.ascontiguousarray(x[:, :50]))
    cpu.channel_resample(np.ascontiguousarray(x[:, :33]).astype(np.complex64))
    cpu.resetChannelResampler()
    second = cpu.channel_audio_resample_host(np.ascontiguousarray(x[:, 50:]))
    same(np.concatenate([first, second], axis=1), alone)


def layout_of(L, M, ntaps, in_s16):
    f = _lib.load().sddc_ddc_internal_chars_layout
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)] * 4
    v = [ctypes.c_int() for _ in range(4)]
    assert f(L, M, ntaps, in_s16, *[ctypes.byref(c) for c in v]) == 0
    return tuple(c.value for c in v)


def test_the_lds_layout_is_the_bank_models(cpu):
    """The launch's tile, LDS instance, pitch and modelled store cycles are the numpy model's; the
    tile fits its LDS; a tap's read is conflict-free for every row."""
    pitch_of = _lib.load().sddc_ddc_internal_chars_pitch
    pitch_of.restype = ctypes.c_int
    pitch_of.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)]
    for L, M, ntaps in RATIOS + [(1, 2, 3), (32, 255, 4096), (1, 16, 129), (7, 64, 500)]:
        K = -(-ntaps // L)
        for s16 in (0, 1):
            ta, lds, pitch, cost = layout_of(L, M, ntaps, s16)
            assert (ta, lds, pitch, cost) == BK.layout(L, M, ntaps, s16)
            hcols = (K - 2 + M) // M + 1
            assert ta >= 1 and pitch >= ta + hcols and pitch * M <= lds and lds in (BK.LDS, BK.LDS_SMALL)
            assert ta * M + K - 1 + M - 1 <= lds   # the last tile's samples
            assert BK.read_conflicts(M, pitch, K) == 0
            c = ctypes.c_int()
            assert pitch_of(M, ta + hcols, pitch, 8 if s16 else 4, ctypes.byref(c)) == pitch and c.value == cost
    assert layout_of(1, 4, 65, 0)[1] == BK.LDS_SMALL and layout_of(24, 125, 1536, 0)[1] == BK.LDS
