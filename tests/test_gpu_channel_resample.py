"""The channel resampler on the GPU (pytest -m gpu): sddc_ddc_channel_resample_device and
sddc_ddc_channel_resample_host of a GPU handle against the float64 model and its derived bound
(tools/channel_resample_model.py), the bit-exact properties of the kernel's fixed summation order,
and the DDC, the decimator and the resampler on one stream and one device buffer.

The bar: every output component within gamma sum_j |h[p + jL]| |x[s - j]|, gamma = n u / (1 - n u),
n = K + 1, K = ceil(ntaps / L), u = 2^-24, computed per output from the model's own sum; GPU against
the CPU backend within twice that.
Shapes (nch, L, M, ntaps, outputs asked for, unused components between the streams), T = the
kernel's outputs per tile of that (L, M, ntaps, format) from sddc_ddc_internal_chres_layout; the
call has the fewest samples that give the outputs asked for:
  (1, 2, 3, 1, 5, 0)            K = 1: no tails, and phase 1 has no tap (its outputs are 0)
  (1, 3, 2, 7, T + 1, 0)        upsampling, ntaps no multiple of L
  (3, 6, 125, 259, 2T + 1, 2)   the 1 MS/s -> 48 kS/s pair, strides with gaps
  (2, 3, 250, 3072, 37, 0)      K = 1024
  (1, 32, 255, 4096, T - 1, 0)  the largest L, an odd M
  (1, 4, 1, 16, 33, 0)          M = 1
  (2, 1, 8, 65, T + 1, 0)       L = 1: a decimator
Input gaps hold NaN (CF32) or 0x7fff (CS16).  Every d_out sits two floats (the call needs 8-byte
alignment) into a NaN-filled tensor whose head, tail and gaps between the streams must stay NaN.
Every test runs under a watchdog that ends the process if a GPU step hangs.
"""
from __future__ import annotations

import ctypes
import faulthandler
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RM = _load("channel_resample_model")
DM = _load("channel_decimate_model")

FORMATS = ["CF32", "CS16"]
CS16_SCALE = 4.0
PARAM_CHRES_MAX_WGS = 14   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
HEAD = 2                   # floats before d_out in its NaN-filled tensor
# (nch, L, M, ntaps, outputs as a function of T, gap)
SHAPES = [(1, 2, 3, 1, lambda T: 5, 0), (1, 3, 2, 7, lambda T: T + 1, 0), (3, 6, 125, 259, lambda T: 2 * T + 1, 2),
          (2, 3, 250, 3072, lambda T: 37, 0), (1, 32, 255, 4096, lambda T: T - 1, 0), (1, 4, 1, 16, lambda T: 33, 0),
          (2, 1, 8, 65, lambda T: T + 1, 0)]
IDS = ["1x2x3x1", "1x3x2x7", "3x6x125x259", "2x3x250x3072", "1x32x255x4096", "1x4x1x16", "2x1x8x65"]
THREE, K1024 = SHAPES[2], SHAPES[3]


@pytest.fixture(autouse=True)
def step_limit():
    """A hung GPU step ends the run (with a traceback) instead of blocking it."""
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture()
def gpu(torch_dev):
    from extio_sddc_amd import R2iq
    with R2iq(gain=1.0) as r:
        yield r
        torch_dev.cuda.synchronize()


def tile_outputs(L, M, ntaps, fmt):
    from extio_sddc_amd import _lib
    f = _lib.load().sddc_ddc_internal_chres_layout
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)] * 3
    t, p, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert f(L, M, ntaps, int(fmt == "CS16"), ctypes.byref(t), ctypes.byref(p), ctypes.byref(c)) == 0
    return t.value


def resolve(shape, fmt):
    """(nch, L, M, ntaps, nsamp, gap): the fewest samples that give the outputs the shape asks for."""
    nch, L, M, ntaps, want, gap = shape
    return nch, L, M, ntaps, RM.nsamp_for(L, M, want(tile_outputs(L, M, ntaps, fmt))), gap


@functools.lru_cache(maxsize=None)
def signal(kind, nch, nsamp, pos=0):
    x = RM.make_input(kind, nch, nsamp, pos)
    x.setflags(write=False)
    return x


def components(x, fmt, extra=0):
    """The streams as the DDC writes them: [nch, 2 nsamp + extra] components, the gaps poisoned."""
    return RM.as_cs16(x, extra, 0x7fff) if fmt == "CS16" else RM.as_cf32(x, extra, np.nan)


@functools.lru_cache(maxsize=None)
def dev_signal(kind, nch, nsamp, fmt, extra, pos=0):
    import torch
    return torch.from_numpy(components(signal(kind, nch, nsamp, pos), fmt, extra)).to("cuda")


@functools.lru_cache(maxsize=None)
def sample_values(kind, nch, nsamp, fmt):
    """What the backend reads: the float32 values of the model's input in this format."""
    x = signal(kind, nch, nsamp)
    return RM.cs16_values(RM.as_cs16(x), CS16_SCALE) if fmt == "CS16" else RM.values(x)


def host_iq(x, fmt):
    if fmt == "CS16":
        return RM.as_cs16(x).reshape(x.shape[0], x.shape[1], 2)
    return RM.as_cf32(x).view(np.complex64)


def set_format(r, fmt):
    r.setOutputFormat(fmt, CS16_SCALE if fmt == "CS16" else 1.0)


def set_max_wgs(r, cap):
    f = r._L.sddc_ddc_internal_set_param
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    return f(r._h, PARAM_CHRES_MAX_WGS, cap)


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chres_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint64], ctypes.c_int
    assert f(r._h, pos) == 0


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def out_tensor(torch, nch, nout, gap):
    """(the NaN-filled tensor, d_out two floats into it, out_stride)."""
    stride = 2 * nout + gap
    buf = torch.full((HEAD + nch * stride + 64,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[HEAD:], stride


def collect(buf, nch, nout, gap):
    """complex64 [nch, nout] of a finished call; the head, the tail and the gaps must still be NaN."""
    stride = 2 * nout + gap
    y = buf.cpu().numpy()
    body = y[HEAD:HEAD + nch * stride].reshape(nch, stride)
    assert np.isnan(y[:HEAD]).all() and np.isnan(y[HEAD + nch * stride:]).all()
    assert np.isnan(body[:, 2 * nout:]).all()
    return np.ascontiguousarray(body[:, :2 * nout]).view(np.complex64).reshape(nch, nout)


def run_device(torch, r, d_iq, nch, nsamp, in_stride, gap=0, stream_=None):
    """One channel_resample_device call -> complex64 [nch, nout]."""
    nout = r.channel_resample_samples(nsamp)
    buf, out, stride = out_tensor(torch, nch, nout, gap)
    if stream_ is not None:
        stream_.wait_stream(torch.cuda.current_stream())
    assert r.channel_resample_device(d_iq, nch, nsamp, in_stride, out, stride, stream=stream_) == nout
    torch.cuda.synchronize()
    return collect(buf, nch, nout, gap)


def run_cuts(torch, r, d_iq, nch, nsamp, in_stride, total, cuts, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of d_iq it covers, every call
    writing behind the one before into one NaN-filled buffer of `total` outputs per channel
    (a call without an output writes nothing); nothing synchronises between the calls."""
    assert sum(cuts) == nsamp
    flat, at, done = d_iq.reshape(-1), 0, 0
    buf, out, stride = out_tensor(torch, nch, total, 2)
    torch.cuda.synchronize()   # the NaN fill is done before a call on another stream writes
    for k, n in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        done += r.channel_resample_device(flat[2 * at:], nch, n, in_stride, out[2 * done:], stride, stream=s)
        at += n
    torch.cuda.synchronize()
    assert done == total
    return collect(buf, nch, total, 2)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bound_device(torch_dev, gpu, shape, fmt):
    nch, L, M, ntaps, nsamp, gap = resolve(shape, fmt)
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    for kind in ("noise", "edges"):
        gpu.setChannelResampler(h, L, M, nch)
        d_iq = dev_signal(kind, nch, nsamp, fmt, gap)
        y = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + gap, gap)
        assert y.shape == (nch, RM.count(L, M, 0, nsamp))
        e = RM.excess(y, sample_values(kind, nch, nsamp, fmt), h, L, M)
        print(f"{kind} {fmt} {IDS[SHAPES.index(shape)]} nsamp {nsamp} nout {y.shape[1]}: |y - y64| - bound <= {e:.3e}")
        assert np.isfinite(y.view(np.float32)).all() and e <= 0.0
    if (L, M, ntaps) == (2, 3, 1):   # phase 1 has no tap
        assert (y[:, 1::2] == 0).all() and (y[:, 0::2] != 0).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("pair", [(2, 3, 1), (3, 2, 7), (6, 125, 259), (4, 1, 16), (1, 8, 65), (3, 250, 3072)],
                         ids=lambda p: "x".join(map(str, p)))
def test_impulse_is_the_taps_bit_for_bit(torch_dev, gpu, pair, fmt):
    """x = delta[i], amplitude 1.0: y[m] == h[mM] while mM < ntaps, 0 beyond; the same with the
    impulse in a first call of one sample (the tail holds it)."""
    L, M, ntaps = pair
    h = RM.make_taps(ntaps)
    gpu.setOutputFormat(fmt, 1.0)   # CS16: code 1 at cs16_scale 1 is the value 1.0
    nsamp = -(-ntaps // L) + 2 * M + 3
    nout = RM.count(L, M, 0, nsamp)
    k = np.arange(nout) * M
    want = np.where(k < ntaps, h[np.clip(k, 0, ntaps - 1)], np.float32(0)).astype(np.float32)
    assert np.count_nonzero(want) == -(-ntaps // M) and (nout - 1) * M >= ntaps
    d_iq = torch_dev.from_numpy(components(RM.make_input("impulse", 2, nsamp, pos=0), fmt)).to("cuda")
    for cuts in ([nsamp], [1, nsamp - 1]):
        gpu.setChannelResampler(h, L, M, 2)
        y = run_cuts(torch_dev, gpu, d_iq, 2, nsamp, 2 * nsamp, nout, cuts)
        for c in range(2):
            np.testing.assert_array_equal(bits(y[c].real), bits(want))
            np.testing.assert_array_equal(bits(y[c].imag), bits(np.zeros(nout, np.float32)))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [THREE, K1024], ids=["3x6x125x259", "2x3x250x3072"])
def test_cuts_are_bit_identical(torch_dev, gpu, shape, fmt):
    """One call against a call per sample (most of them without an output), against cuts shorter
    than K - 1 and against seeded random cuts."""
    nch, L, M, ntaps, nsamp, gap = resolve(shape, fmt)
    K = -(-ntaps // L)
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, fmt, gap)
    S = 2 * nsamp + gap
    gpu.setChannelResampler(h, L, M, nch)
    whole = run_device(torch_dev, gpu, d_iq, nch, nsamp, S)
    total = whole.shape[1]
    assert RM.excess(whole, sample_values("noise", nch, nsamp, fmt), h, L, M) <= 0.0
    gpu.setChannelResampler(h, L, M, nch)
    assert gpu.channel_resample_samples(1) == 1
    one = run_cuts(torch_dev, gpu, d_iq, nch, nsamp, S, total, [1] * nsamp)   # the counts sum to `total`
    np.testing.assert_array_equal(bits(one), bits(whole))
    short = max(1, (K - 1) // 3)
    cuts = [short, 1, short + 1, max(1, K - 2)]
    cuts.append(nsamp - sum(cuts))
    gpu.resetChannelResampler()
    np.testing.assert_array_equal(bits(run_cuts(torch_dev, gpu, d_iq, nch, nsamp, S, total, cuts)), bits(whole))
    rng = np.random.default_rng(5)
    for _ in range(2):
        marks = np.sort(rng.choice(np.arange(1, nsamp), 6, replace=False))
        cuts = np.diff(np.concatenate([[0], marks, [nsamp]])).tolist()
        gpu.resetChannelResampler()
        np.testing.assert_array_equal(bits(run_cuts(torch_dev, gpu, d_iq, nch, nsamp, S, total, cuts)), bits(whole))


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu, fmt):
    nch, L, M, ntaps, nsamp, gap = resolve(THREE, fmt)
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, fmt, gap)
    gpu.setChannelResampler(h, L, M, nch)
    among = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + gap)
    for c in range(nch):
        gpu.setChannelResampler(h, L, M, 1)
        alone = run_device(torch_dev, gpu, d_iq[c], 1, nsamp, 0)
        np.testing.assert_array_equal(bits(alone[0]), bits(among[c]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_identical_for_any_grid_and_from_run_to_run(torch_dev, gpu, fmt):
    """9 items (3 channels x 3 tiles): capped at 1 a workgroup takes 9 rounds, at 2 five, at 3 three."""
    nch, L, M, ntaps, nsamp, gap = resolve(THREE, fmt)
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, fmt, gap)
    outs = []
    for cap in (0, 0, 1, 2, 3):
        assert set_max_wgs(gpu, cap) == 0
        gpu.setChannelResampler(h, L, M, nch)
        first = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + gap, gap)
        second = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + gap, gap)   # the tails and the position too
        outs.append(np.concatenate([first, second], axis=1))
    assert set_max_wgs(gpu, -1) == ERR_ARG
    assert set_max_wgs(gpu, 0) == 0
    x = sample_values("noise", nch, nsamp, fmt)
    assert RM.excess(outs[0], np.concatenate([x, x], axis=1), h, L, M) <= 0.0
    for o in outs[1:]:
        np.testing.assert_array_equal(bits(o), bits(outs[0]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_streams_back_to_back_equal_the_two_call_cut(torch_dev, gpu, fmt):
    """A call on a side stream and a call on the default stream, issued without a sync between them:
    the second waits for the first, whose tails it reads."""
    torch = torch_dev
    nch, L, M, ntaps, nsamp, gap = resolve(THREE, fmt)
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, fmt, gap)
    S = 2 * nsamp + gap
    cuts = [nsamp // 2 + 3, nsamp - nsamp // 2 - 3]
    gpu.setChannelResampler(h, L, M, nch)
    whole = run_device(torch, gpu, d_iq, nch, nsamp, S)
    total = whole.shape[1]
    gpu.setChannelResampler(h, L, M, nch)
    np.testing.assert_array_equal(bits(run_cuts(torch, gpu, d_iq, nch, nsamp, S, total, cuts)), bits(whole))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for streams in ([side, torch.cuda.current_stream()], [torch.cuda.current_stream(), side]):
        gpu.setChannelResampler(h, L, M, nch)
        np.testing.assert_array_equal(bits(run_cuts(torch, gpu, d_iq, nch, nsamp, S, total, cuts, streams)), bits(whole))


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_call_equals_the_device_call_and_shares_its_state(torch_dev, gpu, fmt):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    nch, L, M, ntaps, nsamp, _ = resolve(THREE, fmt)
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    x = signal("noise", nch, nsamp)
    d_iq = dev_signal("noise", nch, nsamp, fmt, 0)
    gpu.setChannelResampler(h, L, M, nch)
    dev = np.concatenate([run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp) for _ in range(2)], axis=1)
    nout = RM.count(L, M, 0, nsamp)
    assert dev.shape[1] == RM.count(L, M, 0, 2 * nsamp) and nsamp * L % M != 0   # the second call starts off phase
    # host then device, device then host: the same stream of two calls
    gpu.setChannelResampler(h, L, M, nch)
    hd = np.concatenate([gpu.channel_resample(host_iq(x, fmt)),
                         run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp)], axis=1)
    np.testing.assert_array_equal(bits(hd), bits(dev))
    gpu.resetChannelResampler()
    dh = np.concatenate([run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp),
                         gpu.channel_resample(host_iq(x, fmt))], axis=1)
    np.testing.assert_array_equal(bits(dh), bits(dev))
    # a strided host output: nothing between the streams
    gpu.resetChannelResampler()
    out = np.full((nch, 2 * nout + 2), np.nan, np.float32)
    xs = np.ascontiguousarray(components(x, fmt, 2))
    got = ctypes.c_size_t(0)
    assert gpu._L.sddc_ddc_channel_resample_host(gpu._h, xs.ctypes.data, nch, nsamp, xs.shape[1], out.ctypes.data,
                                                 out.shape[1], ctypes.addressof(got)) == 0
    assert got.value == nout and np.isnan(out[:, 2 * nout:]).all()
    np.testing.assert_array_equal(bits(out[:, :2 * nout]), bits(dev[:, :nout]).reshape(nch, 2 * nout))
    # against the CPU backend: twice the bound
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        set_format(c, fmt)
        c.setChannelResampler(h, L, M, nch)
        yc = np.concatenate([c.channel_resample(host_iq(x, fmt)) for _ in range(2)], axis=1)
    xv = sample_values("noise", nch, nsamp, fmt)
    br, bi = RM.bound(np.concatenate([xv, xv], axis=1), h, L, M)
    d = dev.astype(np.complex128) - yc.astype(np.complex128)
    print(f"{fmt}: GPU against the CPU backend, worst |difference| / bound "
          f"{max((np.abs(d.real) / br).max(), (np.abs(d.imag) / bi).max()):.3f}")
    assert (np.abs(d.real) <= 2 * br).all() and (np.abs(d.imag) <= 2 * bi).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_position_counts_modulo_m_alone(torch_dev, gpu, fmt):
    """A zero-tail stream started at position r and at r + 2^40 M: the same counts and bits, and the
    outputs of the stream [r zeros | x] from position r on."""
    nch, L, M, ntaps = THREE[:4]
    nsamp = 1501
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, fmt, 0)
    xv = sample_values("noise", nch, nsamp, fmt)
    for r in (0, 1, M - 1):
        ys = []
        for pos in (r, r + (2 ** 40) * M):
            gpu.setChannelResampler(h, L, M, nch)
            set_position(gpu, pos)
            assert gpu.channel_resample_samples(nsamp) == RM.count(L, M, r, nsamp)
            first = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp)
            ys.append(np.concatenate([first, run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp)], axis=1))
        np.testing.assert_array_equal(bits(ys[1]), bits(ys[0]))
        full = np.concatenate([np.zeros((nch, r)), xv, xv], axis=1)
        skip = RM.count(L, M, 0, r)
        ref, (br, bi) = RM.resample(full, h, L, M)[:, skip:], RM.bound(full, h, L, M)
        d = ys[0].astype(np.complex128) - ref
        assert (np.abs(d.real) <= br[:, skip:]).all() and (np.abs(d.imag) <= bi[:, skip:]).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_l1_equals_the_decimator_within_the_two_bounds(torch_dev, gpu, fmt):
    """L = 1: the resampler and the decimator, both set on one handle, on one buffer."""
    nch, L, R, ntaps = SHAPES[6][:4]
    nsamp = (tile_outputs(L, R, ntaps, fmt) + 1) * R
    set_format(gpu, fmt)
    h = RM.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, fmt, 0)
    gpu.setChannelResampler(h, L, R, nch)
    gpu.setChannelDecimator(h, R, nch)
    yr = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp)
    buf, out, stride = out_tensor(torch_dev, nch, nsamp // R, 0)
    gpu.channel_decimate_device(d_iq, nch, nsamp, 2 * nsamp, out, stride)
    torch_dev.cuda.synchronize()
    yd = collect(buf, nch, nsamp // R, 0)
    xv = sample_values("noise", nch, nsamp, fmt)
    rr, ri = RM.bound(xv, h, L, R)
    dr, di = DM.bound(xv, h, R)
    d = yr.astype(np.complex128) - yd.astype(np.complex128)
    assert (np.abs(d.real) <= rr + dr).all() and (np.abs(d.imag) <= ri + di).all()
    assert RM.excess(yr, xv, h, L, R) <= 0.0 and np.abs(yr).max() > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_ddc_decimator_and_resampler_on_one_handle_and_buffer(torch_dev, fmt):
    """process_channels_device at d = 6 (2 blocks, 3 channels), then the decimator (R = 8, 65 taps) and
    the resampler (6/125, 259 taps) interleaved on the two halves of its output buffer, on one
    stream: each equals its stand-alone run on another handle bit for bit, and the resampler holds
    the bound of the model applied to the IQ copied back."""
    from extio_sddc_amd import R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import make_tone_stream
    torch = torch_dev
    d, nblk, R, L, M, tbs = 6, 2, 8, 6, 125, [1000, 1008, 1012]
    hd, hr = kaiser(65, 60.0, 0.04, 0.0625), RM.make_taps(259)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    half = nsamp // 2
    assert half % R == 0
    d_in = torch.from_numpy(make_tone_stream(nblk, 1010.3, amp=20000.0)).to("cuda")
    dtype = torch.int16 if fmt == "CS16" else torch.float32

    def chain(r, d_iq, dec, res):
        """The two halves through the stages asked for -> (decimated, resampled) [nch, .] or None."""
        flat, S = d_iq.reshape(-1), d_iq.stride(0)
        bd, od, sd = out_tensor(torch, nch, nsamp // R, 0)
        nres = RM.count(L, M, 0, nsamp)
        br, orr, sr = out_tensor(torch, nch, nres, 0)
        done = 0
        for k in range(2):
            part = flat[2 * k * half:]
            if dec:
                r.channel_decimate_device(part, nch, half, S, od[2 * k * (half // R):], sd, stream=s)
            if res:
                done += r.channel_resample_device(part, nch, half, S, orr[2 * done:], sr, stream=s)
        torch.cuda.synchronize()
        assert not res or done == nres
        return (collect(bd, nch, nsamp // R, 0) if dec else None), (collect(br, nch, nres, 0) if res else None)

    s = torch.cuda.Stream()
    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        set_format(r, fmt)
        r.setChannelDecimator(hd, R, nch)
        r.setChannelResampler(hr, L, M, nch)
        d_iq = torch.zeros((nch, 2 * nsamp), dtype=dtype, device="cuda")
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, d_iq, stream=s)
        both = chain(r, d_iq, True, True)
    with R2iq(gain=1.0) as r:
        set_format(r, fmt)
        r.setChannelDecimator(hd, R, nch)
        dec_alone = chain(r, d_iq, True, False)[0]
    with R2iq(gain=1.0) as r:
        set_format(r, fmt)
        r.setChannelResampler(hr, L, M, nch)
        res_alone = chain(r, d_iq, False, True)[1]
    np.testing.assert_array_equal(bits(both[0]), bits(dec_alone))
    np.testing.assert_array_equal(bits(both[1]), bits(res_alone))
    iq = d_iq.cpu().numpy()
    assert np.abs(iq.astype(np.float64)).max() > 0
    xv = RM.cs16_values(iq, CS16_SCALE) if fmt == "CS16" else RM.values(np.ascontiguousarray(iq).view(np.complex64))
    e = RM.excess(both[1], xv, hr, L, M)
    print(f"{fmt}: DDC + resampler against the model on the IQ copied back: |y - y64| - bound <= {e:.3e}")
    assert e <= 0.0 and np.abs(both[1]).max() > 0 and np.abs(both[0]).max() > 0


def test_error_returns_and_a_failed_call_changes_no_state(torch_dev, gpu):
    from extio_sddc_amd import DEVICE_CPU, DDCError, R2iq
    torch = torch_dev
    L_, hd = gpu._L, gpu._h
    sets, dev = L_.sddc_ddc_set_channel_resampler, L_.sddc_ddc_channel_resample_device
    nch, L, M, ntaps, nsamp = 3, 3, 7, 20, 40
    taps = RM.make_taps(ntaps)
    tp = taps.ctypes.data
    d_iq = dev_signal("noise", nch, nsamp, "CF32", 2)
    S, nout = 2 * nsamp + 2, RM.count(L, M, 0, nsamp)
    buf, out, OS = out_tensor(torch, nch, nout, 2)
    xi, oi = d_iq.data_ptr(), out.data_ptr()
    got = ctypes.c_size_t(99)
    gp = ctypes.addressof(got)
    assert dev(hd, xi, nch, nsamp, S, oi, OS, gp, None) == ERR_STATE                 # nothing set
    assert L_.sddc_ddc_channel_resampler_reset(hd) == ERR_STATE
    assert gpu.channel_resample_samples(nsamp) == 0
    with pytest.raises(DDCError):
        gpu.channel_resample_device(d_iq, nch, nsamp, S, out, OS)
    big = np.zeros(4097, np.float32)
    assert sets(hd, big.ctypes.data, 4097, L, M, nch) == ERR_ARG
    assert sets(hd, big.ctypes.data, 1025, 1, 2, nch) == ERR_ARG                     # K = 1025
    for up, down in ((0, M), (33, M), (L, 0), (L, 257), (2, 4), (6, 9), (1, 1)):
        assert sets(hd, tp, ntaps, up, down, nch) == ERR_ARG
    assert sets(hd, tp, ntaps, L, M, 0) == ERR_ARG
    assert sets(hd, tp, ntaps, L, M, 1025) == ERR_ARG
    t = taps.copy()
    t[ntaps - 1] = np.inf
    assert sets(hd, t.ctypes.data, ntaps, L, M, nch) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, OS, gp, None) == ERR_STATE                 # a failed set sets nothing
    gpu.setChannelResampler(taps, L, M, nch)
    good = run_device(torch, gpu, d_iq, nch, nsamp, S, 2)
    gpu.setChannelResampler(taps, L, M, nch)
    assert dev(hd, xi, nch - 1, nsamp, S, oi, OS, gp, None) == ERR_STATE             # another nch than the set one
    assert dev(hd, xi, nch, 0, S, oi, OS, gp, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, 2 * nsamp - 2, oi, OS, gp, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S + 1, oi, OS, gp, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, 2 * nout - 2, gp, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, OS + 1, gp, None) == ERR_ARG
    assert dev(hd, xi + 4, nch, nsamp, S, oi, OS, gp, None) == ERR_ARG               # CF32: 8-byte samples
    assert dev(hd, xi, nch, nsamp, S, oi + 4, OS, gp, None) == ERR_ARG
    assert dev(hd, None, nch, nsamp, S, oi, OS, gp, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, None, OS, gp, None) == ERR_ARG
    with pytest.raises(DDCError):
        gpu.channel_resample_device(d_iq, nch, nsamp, S, out[:OS], OS)               # d_out too small
    with pytest.raises(DDCError):
        gpu.channel_resample_device(d_iq, nch + 1, nsamp, S, out, OS)                # d_iq too small
    with pytest.raises(DDCError):
        gpu.channel_resample_device(d_iq.to(torch.int16), nch, nsamp, S, out, OS)    # wrong dtype
    torch.cuda.synchronize()
    assert got.value == 99 and torch.isnan(buf).all()
    # the failed calls changed no state: the next valid call is the first call of the stream
    assert gpu.channel_resample_samples(nsamp) == nout
    np.testing.assert_array_equal(bits(run_device(torch, gpu, d_iq, nch, nsamp, S, 2)), bits(good))
    gpu.setChannelResampler(None)
    assert dev(hd, xi, nch, nsamp, S, oi, OS, gp, None) == ERR_STATE
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:                                     # a CPU handle has no device path
        c.setChannelResampler(taps, L, M, nch)
        assert c._L.sddc_ddc_channel_resample_device(c._h, xi, nch, nsamp, S, oi, OS, gp, None) == ERR_STATE
    assert torch.isnan(buf).all()
