"""The channel decimator on the GPU (pytest -m gpu): sddc_ddc_channel_decimate_device and
sddc_ddc_channel_decimate_host of a GPU handle against the float64 model and its derived bound
(tools/channel_decimate_model.py), the bit-exact properties of the kernel's fixed summation order,
and the DDC and the decimator on one stream and one device buffer.

The bar: every output component within gamma sum_j |h[j]| |x[mR - j]|, gamma = n u / (1 - n u),
n = ntaps + 1, u = 2^-24, computed per output from the model's own sum; GPU against the CPU backend
within twice that.
Shapes (nch, R, ntaps, nsamp / R, unused components between the streams), T = the kernel's outputs
per tile (CHANNEL_DECIMATE_TILE):
  (1, 2, 1, 1, 0)          one output, no halo
  (1, 8, 3, T + 1, 0)      ntaps < R, a tail tile with one output
  (1, 3, 3, T - 1, 0)      ntaps = R, R not a power of two
  (3, 5, 21, 2T + 1, 2)    in_stride = 2 nsamp + 2, out_stride with a gap, odd ntaps
  (2, 64, 1024, 3, 0)      both maxima, a tile that is mostly halo
  (1024, 8, 65, 2, 0)      every channel, almost no samples each
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
_spec = importlib.util.spec_from_file_location("channel_decimate_model",
                                               os.path.join(ROOT, "tools", "channel_decimate_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

from extio_sddc_amd import CHANNEL_DECIMATE_TILE as T  # noqa: E402

FORMATS = ["CF32", "CS16"]
CS16_SCALE = 4.0
PARAM_CHDEC_MAX_WGS = 13   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
HEAD = 2                   # floats before d_out in its NaN-filled tensor
SHAPES = [(1, 2, 1, 1, 0), (1, 8, 3, T + 1, 0), (1, 3, 3, T - 1, 0), (3, 5, 21, 2 * T + 1, 2), (2, 64, 1024, 3, 0),
          (1024, 8, 65, 2, 0)]
THREE = SHAPES[3]


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


@functools.lru_cache(maxsize=None)
def signal(kind, nch, nsamp, R, pos=0):
    x = M.make_input(kind, nch, nsamp, R, pos)
    x.setflags(write=False)
    return x


def components(x, fmt, extra=0):
    """The streams as the DDC writes them: [nch, 2 nsamp + extra] components, the gaps poisoned."""
    return M.as_cs16(x, extra, 0x7fff) if fmt == "CS16" else M.as_cf32(x, extra, np.nan)


@functools.lru_cache(maxsize=None)
def dev_signal(kind, nch, nsamp, R, fmt, extra, pos=0):
    import torch
    return torch.from_numpy(components(signal(kind, nch, nsamp, R, pos), fmt, extra)).to("cuda")


def sample_values(x, fmt):
    """What the backend reads: the float32 values of the model's input in this format."""
    return M.cs16_values(M.as_cs16(x), CS16_SCALE) if fmt == "CS16" else M.values(x)


def host_iq(x, fmt):
    if fmt == "CS16":
        return M.as_cs16(x).reshape(x.shape[0], x.shape[1], 2)
    return M.as_cf32(x).view(np.complex64)


def set_format(r, fmt):
    r.setOutputFormat(fmt, CS16_SCALE if fmt == "CS16" else 1.0)


def set_max_wgs(r, cap):
    f = r._L.sddc_ddc_internal_set_param
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    return f(r._h, PARAM_CHDEC_MAX_WGS, cap)


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
    return np.ascontiguousarray(body[:, :2 * nout]).view(np.complex64)


def run_device(torch, r, d_iq, nch, nsamp, in_stride, R, gap=0, stream_=None):
    """One channel_decimate_device call -> complex64 [nch, nsamp / R]."""
    nout = nsamp // R
    buf, out, stride = out_tensor(torch, nch, nout, gap)
    if stream_ is not None:
        stream_.wait_stream(torch.cuda.current_stream())
    r.channel_decimate_device(d_iq, nch, nsamp, in_stride, out, stride, stream=stream_)
    torch.cuda.synchronize()
    return collect(buf, nch, nout, gap)


def run_cuts(torch, r, d_iq, nch, nsamp, in_stride, R, cuts, fmt, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of d_iq it covers (channel c of
    call k starts at component c in_stride + 2 at); nothing synchronises between the calls."""
    assert sum(cuts) == nsamp
    flat, at = d_iq.reshape(-1), 0
    outs = [out_tensor(torch, nch, n // R, 0) for n in cuts]
    torch.cuda.synchronize()   # the NaN fills are done before a call on another stream writes
    for k, n in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        r.channel_decimate_device(flat[2 * at:], nch, n, in_stride, outs[k][1], outs[k][2], stream=s)
        at += n
    torch.cuda.synchronize()
    return np.concatenate([collect(o[0], nch, n // R, 0) for o, n in zip(outs, cuts)], axis=1)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bound_device(torch_dev, gpu, shape, fmt):
    nch, R, ntaps, nout, extra = shape
    nsamp = nout * R
    set_format(gpu, fmt)
    h = M.make_taps(ntaps)
    for kind in ("noise", "edges"):
        gpu.setChannelDecimator(h, R, nch)
        d_iq = dev_signal(kind, nch, nsamp, R, fmt, extra)
        y = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, R, extra)
        e = M.excess(y, sample_values(signal(kind, nch, nsamp, R), fmt), h, R)
        print(f"{kind} {fmt} {shape}: |y - y64| - bound <= {e:.3e}")
        assert np.isfinite(y.view(np.float32)).all() and e <= 0.0


@pytest.mark.parametrize("fmt", FORMATS)
def test_impulse_is_the_taps_bit_for_bit(torch_dev, gpu, fmt):
    """x = delta[i - p], amplitude 1.0: y[m] == h[mR - p] where 0 <= mR - p < ntaps, else 0; p = 0, 1,
    R - 1, R pin the orientation and the phase, an impulse in the previous call pins the tail."""
    R, ntaps, nsamp = 4, 11, 24
    h = M.make_taps(ntaps)
    gpu.setOutputFormat(fmt, 1.0)   # CS16: code 1 at cs16_scale 1 is the value 1.0

    def expect(p, first, n):
        k = np.arange(first, first + n) * R - p
        return np.where((k >= 0) & (k < ntaps), h[np.clip(k, 0, ntaps - 1)], np.float32(0)).astype(np.float32)

    def dev(p):
        return torch_dev.from_numpy(components(M.make_input("impulse", 2, nsamp, R, pos=p), fmt)).to("cuda")

    for p in (0, 1, R - 1, R):
        gpu.setChannelDecimator(h, R, 2)
        y = run_device(torch_dev, gpu, dev(p), 2, nsamp, 2 * nsamp, R)
        for c in range(2):
            np.testing.assert_array_equal(bits(y[c].real), bits(expect(p, 0, nsamp // R)))
            np.testing.assert_array_equal(bits(y[c].imag), bits(np.zeros(nsamp // R, np.float32)))
    # the impulse in the previous call, R + 1 samples before its end (so the tail holds it)
    gpu.setChannelDecimator(h, R, 2)
    p = nsamp - R - 1
    run_device(torch_dev, gpu, dev(p), 2, nsamp, 2 * nsamp, R)
    y = run_device(torch_dev, gpu, dev(-1), 2, nsamp, 2 * nsamp, R)
    want = expect(p, nsamp // R, nsamp // R)
    assert np.count_nonzero(want) >= 2
    np.testing.assert_array_equal(bits(y[1].real), bits(want))


@pytest.mark.parametrize("fmt", FORMATS)
def test_cuts_are_bit_identical(torch_dev, gpu, fmt):
    """The 3-channel shape in one call against the cuts [R, 3R, rest] and against a call per R
    samples (ntaps - 1 = 4R: the new tail keeps part of the old one)."""
    nch, R, ntaps, nout, extra = THREE
    nsamp = nout * R
    assert ntaps - 1 > 3 * R
    set_format(gpu, fmt)
    h = M.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, R, fmt, extra)
    S = 2 * nsamp + extra
    gpu.setChannelDecimator(h, R, nch)
    whole = run_device(torch_dev, gpu, d_iq, nch, nsamp, S, R)
    assert M.excess(whole, sample_values(signal("noise", nch, nsamp, R), fmt), h, R) <= 0.0
    gpu.setChannelDecimator(h, R, nch)
    np.testing.assert_array_equal(
        bits(run_cuts(torch_dev, gpu, d_iq, nch, nsamp, S, R, [R, 3 * R, nsamp - 4 * R], fmt)), bits(whole))
    # a call per R samples: on the first 64 outputs (the same code path 1025 times proves no more)
    few = 64 * R
    gpu.setChannelDecimator(h, R, nch)
    np.testing.assert_array_equal(bits(run_cuts(torch_dev, gpu, d_iq, nch, few, S, R, [R] * 64, fmt)),
                                  bits(whole[:, :64]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu, fmt):
    nch, R, ntaps, nout, extra = THREE
    nsamp = nout * R
    set_format(gpu, fmt)
    h = M.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, R, fmt, extra)
    gpu.setChannelDecimator(h, R, nch)
    among = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, R)
    for c in range(nch):
        gpu.setChannelDecimator(h, R, 1)
        alone = run_device(torch_dev, gpu, d_iq[c], 1, nsamp, 0, R)
        np.testing.assert_array_equal(bits(alone[0]), bits(among[c]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_identical_for_any_grid_and_from_run_to_run(torch_dev, gpu, fmt):
    """9 items (3 channels x 3 tiles): capped at 1 a workgroup takes 9 rounds, capped at 3 it takes 3."""
    nch, R, ntaps, nout, extra = THREE
    nsamp = nout * R
    set_format(gpu, fmt)
    h = M.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, R, fmt, extra)
    outs = []
    for cap in (0, 0, 1, 3):
        assert set_max_wgs(gpu, cap) == 0
        gpu.setChannelDecimator(h, R, nch)
        first = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, R, extra)
        second = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, R, extra)   # the tails too
        outs.append(np.concatenate([first, second], axis=1))
    assert set_max_wgs(gpu, -1) == ERR_ARG
    assert set_max_wgs(gpu, 0) == 0
    x = sample_values(signal("noise", nch, nsamp, R), fmt)
    assert M.excess(outs[0], np.concatenate([x, x], axis=1), h, R) <= 0.0
    for o in outs[1:]:
        np.testing.assert_array_equal(bits(o), bits(outs[0]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_streams_back_to_back_equal_the_two_call_cut(torch_dev, gpu, fmt):
    """A call on a side stream and a call on the default stream, issued without a sync between them:
    the second waits for the first, whose tails it reads."""
    torch = torch_dev
    nch, R, ntaps, nout, extra = THREE
    nsamp = nout * R
    set_format(gpu, fmt)
    h = M.make_taps(ntaps)
    d_iq = dev_signal("noise", nch, nsamp, R, fmt, extra)
    S = 2 * nsamp + extra
    cuts = [(T + 3) * R, nsamp - (T + 3) * R]
    gpu.setChannelDecimator(h, R, nch)
    same = run_cuts(torch, gpu, d_iq, nch, nsamp, S, R, cuts, fmt)
    gpu.setChannelDecimator(h, R, nch)
    whole = run_device(torch, gpu, d_iq, nch, nsamp, S, R)
    np.testing.assert_array_equal(bits(same), bits(whole))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for streams in ([side, torch.cuda.current_stream()], [torch.cuda.current_stream(), side]):
        gpu.setChannelDecimator(h, R, nch)
        np.testing.assert_array_equal(bits(run_cuts(torch, gpu, d_iq, nch, nsamp, S, R, cuts, fmt, streams)), bits(whole))


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_call_equals_the_device_call_and_shares_its_tails(torch_dev, gpu, fmt):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    nch, R, ntaps, nout, _ = THREE
    nsamp = nout * R
    set_format(gpu, fmt)
    h = M.make_taps(ntaps)
    x = signal("noise", nch, nsamp, R)
    d_iq = dev_signal("noise", nch, nsamp, R, fmt, 0)
    gpu.setChannelDecimator(h, R, nch)
    dev = np.concatenate([run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp, R) for _ in range(2)], axis=1)
    # host then device, device then host: the same stream of two calls
    gpu.setChannelDecimator(h, R, nch)
    hd = np.concatenate([gpu.channel_decimate(host_iq(x, fmt)),
                         run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp, R)], axis=1)
    np.testing.assert_array_equal(bits(hd), bits(dev))
    gpu.resetChannelDecimator()
    dh = np.concatenate([run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp, R),
                         gpu.channel_decimate(host_iq(x, fmt))], axis=1)
    np.testing.assert_array_equal(bits(dh), bits(dev))
    # a strided host output: nothing between the streams
    gpu.resetChannelDecimator()
    out = np.full((nch, 2 * nout + 2), np.nan, np.float32)
    xs = np.ascontiguousarray(components(x, fmt, 2))
    assert gpu._L.sddc_ddc_channel_decimate_host(gpu._h, xs.ctypes.data, nch, nsamp, xs.shape[1], out.ctypes.data,
                                                 out.shape[1]) == 0
    assert np.isnan(out[:, 2 * nout:]).all()
    np.testing.assert_array_equal(bits(out[:, :2 * nout]), bits(dev[:, :nout]).reshape(nch, 2 * nout))
    # against the CPU backend: twice the bound
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        set_format(c, fmt)
        c.setChannelDecimator(h, R, nch)
        yc = np.concatenate([c.channel_decimate(host_iq(x, fmt)) for _ in range(2)], axis=1)
    xv = sample_values(x, fmt)
    br, bi = M.bound(np.concatenate([xv, xv], axis=1), h, R)
    d = dev.astype(np.complex128) - yc.astype(np.complex128)
    print(f"{fmt}: GPU against the CPU backend, worst |difference| / bound "
          f"{max((np.abs(d.real) / br).max(), (np.abs(d.imag) / bi).max()):.3f}")
    assert (np.abs(d.real) <= 2 * br).all() and (np.abs(d.imag) <= 2 * bi).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_ddc_and_decimator_on_one_buffer_and_stream(torch_dev, fmt):
    """process_channels_device at d = 6 (2 blocks, 3 channels) and channel_decimate_device (R = 8, 65
    Kaiser taps) on its output buffer, on the same stream: within the bound of the model applied to
    the IQ copied back, and the IQ itself bit-identical to a run without the decimator set."""
    from extio_sddc_amd import R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import make_tone_stream
    torch = torch_dev
    d, nblk, R, tbs = 6, 2, 8, [1000, 1008, 1012]
    h = kaiser(65, 60.0, 0.04, 0.0625)
    assert h.size == 65
    nsamp, nch = output_samples(d, nblk), len(tbs)
    nout = nsamp // R
    d_in = torch.from_numpy(make_tone_stream(nblk, 1010.3, amp=20000.0)).to("cuda")
    dtype = torch.int16 if fmt == "CS16" else torch.float32
    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        set_format(r, fmt)
        plain = torch.zeros((nch, 2 * nsamp), dtype=dtype, device="cuda")
        r.process_channels_device(d_in, nblk, tbs, plain)
        torch.cuda.synchronize()
        r.setChannelDecimator(h, R, nch)
        d_iq = torch.zeros((nch, 2 * nsamp), dtype=dtype, device="cuda")
        buf, out, stride = out_tensor(torch, nch, nout, 0)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, d_iq, stream=s)
        r.channel_decimate_device(d_iq, nch, nsamp, d_iq.stride(0), out, stride, stream=s)
        torch.cuda.synchronize()
    iq = d_iq.cpu().numpy()
    np.testing.assert_array_equal(iq, plain.cpu().numpy())
    assert np.abs(iq.astype(np.float64)).max() > 0
    xv = M.cs16_values(iq, CS16_SCALE) if fmt == "CS16" else M.values(np.ascontiguousarray(iq).view(np.complex64))
    y = collect(buf, nch, nout, 0)
    e = M.excess(y, xv, h, R)
    print(f"{fmt}: DDC + decimator against the model on the IQ copied back: |y - y64| - bound <= {e:.3e}")
    assert e <= 0.0 and np.abs(y).max() > 0


def test_error_returns_and_a_failed_call_changes_no_state(torch_dev, gpu):
    from extio_sddc_amd import DDCError
    torch = torch_dev
    L, hd = gpu._L, gpu._h
    setd, dev = L.sddc_ddc_set_channel_decimator, L.sddc_ddc_channel_decimate_device
    nch, R, ntaps, nsamp = 3, 4, 9, 32
    taps = M.make_taps(ntaps)
    tp = taps.ctypes.data
    d_iq = dev_signal("noise", nch, nsamp, R, "CF32", 2)
    S, nout = 2 * nsamp + 2, nsamp // R
    buf, out, OS = out_tensor(torch, nch, nout, 2)
    xi, oi = d_iq.data_ptr(), out.data_ptr()
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None) == ERR_STATE                 # nothing set
    assert L.sddc_ddc_channel_decimator_reset(hd) == ERR_STATE
    with pytest.raises(DDCError):
        gpu.channel_decimate_device(d_iq, nch, nsamp, S, out, OS)
    big = np.zeros(1025, np.float32)
    assert setd(hd, big.ctypes.data, 1025, R, nch) == ERR_ARG
    assert setd(hd, tp, ntaps, 1, nch) == ERR_ARG
    assert setd(hd, tp, ntaps, 65, nch) == ERR_ARG
    assert setd(hd, tp, ntaps, R, 0) == ERR_ARG
    assert setd(hd, tp, ntaps, R, 1025) == ERR_ARG
    t = taps.copy()
    t[ntaps - 1] = np.inf
    assert setd(hd, t.ctypes.data, ntaps, R, nch) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None) == ERR_STATE                 # a failed set sets nothing
    gpu.setChannelDecimator(taps, R, nch)
    good = run_device(torch, gpu, d_iq, nch, nsamp, S, R, 2)
    gpu.setChannelDecimator(taps, R, nch)
    assert dev(hd, xi, nch - 1, nsamp, S, oi, OS, None) == ERR_STATE             # another nch than the set one
    assert dev(hd, xi, nch, 0, S, oi, OS, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp - 1, S, oi, OS, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, 2 * nsamp - 2, oi, OS, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S + 1, oi, OS, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, 2 * nout - 2, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, OS + 1, None) == ERR_ARG
    assert dev(hd, xi + 4, nch, nsamp, S, oi, OS, None) == ERR_ARG               # CF32: 8-byte samples
    assert dev(hd, xi, nch, nsamp, S, oi + 4, OS, None) == ERR_ARG
    assert dev(hd, None, nch, nsamp, S, oi, OS, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, None, OS, None) == ERR_ARG
    with pytest.raises(DDCError):
        gpu.channel_decimate_device(d_iq, nch, nsamp, S, out[:OS], OS)               # d_out too small
    with pytest.raises(DDCError):
        gpu.channel_decimate_device(d_iq, nch + 1, nsamp, S, out, OS)                # d_iq too small
    with pytest.raises(DDCError):
        gpu.channel_decimate_device(d_iq.to(torch.int16), nch, nsamp, S, out, OS)    # wrong dtype
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    # the failed calls changed no state: the next valid call is the first call of the stream
    np.testing.assert_array_equal(bits(run_device(torch, gpu, d_iq, nch, nsamp, S, R, 2)), bits(good))
    gpu.setChannelDecimator(None)
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None) == ERR_STATE
