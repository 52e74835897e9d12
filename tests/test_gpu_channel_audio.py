"""The channel audio filter on the GPU (pytest -m gpu): sddc_ddc_channel_audio_filter_device and
sddc_ddc_channel_audio_filter_host of a GPU handle bit for bit against the CPU backend (which
tests/test_channel_audio_cpu.py pins to the definition), within the float64 model's bound
(tools/channel_audio_model.py), the bit-exact properties of the kernels (cuts, streams, grids, run
length, a channel alone), and the DDC, the decimator, the AM demodulator and this stage on one stream.

Shapes (nch, nsamp, nsec), B = the block length (AUDIO_BLOCK):
  (1, 1, 1)            one sample: no full block
  (1, B, 2)            exactly one block
  (1, 3B + 17, 3)      full blocks and a tail
  (3, 2B + 3, 4)       differing filters, one identity channel; input and output gaps poisoned, the first
                       samples off a 16-byte line
  (1024, 2, 2)         every channel, almost no samples each
  (1, 66B + 5, 4)      more blocks than a wave has lanes
  (2, 258B + 1, 1)     more blocks than four waves have
Every d_in starts OFFSET samples into a poisoned tensor (NaN, S16: 0x7fff) and every d_out HEAD samples
into one, so neither is 16-byte aligned; the heads, the tails and the gaps between the streams must stay
untouched.  The bound is checked on the first three channels of a shape (the model is a Python loop).
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


M = _load("channel_audio_model")

from extio_sddc_amd import AUDIO_BLOCK as B  # noqa: E402
from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, BIQUAD_DC_BLOCK, BIQUAD_HIGHPASS, BIQUAD_IDENTITY,  # noqa: E402
                            BIQUAD_LOWPASS, BIQUAD_NOTCH, BIQUAD_ONE_POLE_LP, biquad)

PARAM_CHAUD_MAX_WGS, PARAM_CHAUD_RUN_BLOCKS = 16, 17   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
HEAD, OFFSET = 1, 3        # samples before d_out / d_in in their poisoned tensors
S16_POISON = 0x7fff
S16_SCALE = 2000.0         # float streams in (-1, 1) as int16
SHAPES = [(1, 1, 1), (1, B, 2), (1, 3 * B + 17, 3), (3, 2 * B + 3, 4), (1024, 2, 2), (1, 66 * B + 5, 4), (2, 258 * B + 1, 1)]
THREE = SHAPES[3]
FORMATS = [(AUDIO_F32, AUDIO_F32), (AUDIO_S16, AUDIO_S16), (AUDIO_F32, AUDIO_S16), (AUDIO_S16, AUDIO_F32)]
CUTS = {"edges": lambda n: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n: [100, B, n - B - 100]}


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
def bank():
    return [biquad(BIQUAD_DC_BLOCK, 1e-3), biquad(BIQUAD_HIGHPASS, 0.01, 2.0), biquad(BIQUAD_LOWPASS, 0.2, 5.0),
            biquad(BIQUAD_ONE_POLE_LP, 0.05), biquad(BIQUAD_LOWPASS, 0.01, 30.0), biquad(BIQUAD_NOTCH, 0.07, 8.0),
            biquad(BIQUAD_LOWPASS, 0.1, 100.0)]


@functools.lru_cache(maxsize=None)
def coefs(nch, nsec):
    """[nch, nsec, 5]: the channels' filters differ; channel 1 (of several) is the identity."""
    bk = bank()
    c = np.stack([np.stack([bk[(ch + 3 * k) % len(bk)] for k in range(nsec)]) for ch in range(nch)])
    if nch > 1:
        c[1] = biquad(BIQUAD_IDENTITY)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def signal(nch, nsamp, fin):
    """[nch, nsamp] float32 in (-1, 1), or its int16 form."""
    x = M.make_input(nch, nsamp)
    if fin == AUDIO_S16:
        x = np.round(x * S16_SCALE).astype(np.int16)
    x.setflags(write=False)
    return x


def poison(dtype):
    return S16_POISON if dtype == np.int16 else np.nan


@functools.lru_cache(maxsize=None)
def dev_signal(nch, nsamp, fin, gap):
    """(the device tensor, d_in OFFSET samples into it, in_stride): poison before, between and after."""
    import torch
    x = signal(nch, nsamp, fin)
    body = np.full((nch, nsamp + gap), poison(x.dtype), x.dtype)
    body[:, :nsamp] = x
    pad = np.full(OFFSET, poison(x.dtype), x.dtype)
    buf = torch.from_numpy(np.concatenate([pad, body.reshape(-1), pad])).to("cuda")
    return buf, buf[OFFSET:], nsamp + gap


def out_tensor(torch, nch, nsamp, gap, fout):
    """(the poisoned tensor, d_out HEAD samples into it, out_stride)."""
    stride = nsamp + gap
    if fout == AUDIO_S16:
        buf = torch.full((HEAD + nch * stride + 64,), S16_POISON, dtype=torch.int16, device="cuda")
    else:
        buf = torch.full((HEAD + nch * stride + 64,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[HEAD:], stride


def collect(buf, nch, nsamp, gap, fout):
    """[nch, nsamp] of a finished call; the head, the tail and the gaps must still hold the poison (no
    correct S16 output of these inputs is 0x7fff: cpu_result checks that they stay inside the clamp)."""
    stride = nsamp + gap
    y = buf.cpu().numpy()
    clean = (lambda v: (v == S16_POISON).all()) if fout == AUDIO_S16 else (lambda v: np.isnan(v).all())
    body = y[HEAD:HEAD + nch * stride].reshape(nch, stride)
    assert clean(y[:HEAD]) and clean(y[HEAD + nch * stride:]) and clean(body[:, nsamp:])
    return np.ascontiguousarray(body[:, :nsamp])


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run_device(torch, r, d_in, nch, nsamp, in_stride, fout, gap=0, stream_=None):
    buf, out, stride = out_tensor(torch, nch, nsamp, gap, fout)
    if stream_ is not None:
        stream_.wait_stream(torch.cuda.current_stream())
    r.channel_audio_filter_device(d_in, nch, nsamp, in_stride, out, stride, stream=stream_)
    torch.cuda.synchronize()
    return collect(buf, nch, nsamp, gap, fout)


def run_cuts(torch, r, d_in, nch, nsamp, in_stride, cuts, fout, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of d_in it covers; nothing
    synchronises between the calls."""
    assert sum(cuts) == nsamp and min(cuts) > 0
    at = 0
    outs = [out_tensor(torch, nch, n, 0, fout) for n in cuts]
    torch.cuda.synchronize()   # the poison fills are done before a call on another stream writes
    for k, n in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        r.channel_audio_filter_device(d_in[at:], nch, n, in_stride, outs[k][1], outs[k][2], stream=s)
        at += n
    torch.cuda.synchronize()
    return np.concatenate([collect(o[0], nch, n, 0, fout) for o, n in zip(outs, cuts)], axis=1)


@functools.lru_cache(maxsize=None)
def cpu_result(nch, nsamp, nsec, fin, fout, calls=1):
    """The CPU backend's outputs of `calls` consecutive calls on the same samples: [nch, calls nsamp]."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelAudioFilter(coefs(nch, nsec), fin, fout)
        y = np.concatenate([c.channel_audio_filter(signal(nch, nsamp, fin)) for _ in range(calls)], axis=1)
    assert fout != AUDIO_S16 or np.abs(y.astype(np.int32)).max() < 32767
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def model(nch, nsamp, nsec, fin):
    """(y64, bound) of the first three channels."""
    k = min(nch, 3)
    x = signal(nch, nsamp, fin)[:k].astype(np.float32)
    return M.recurrence64(x, coefs(nch, nsec)[:k]), M.bounds(x, coefs(nch, nsec)[:k])


def set_param(r, param, value):
    f = r._L.sddc_ddc_internal_set_param
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    return f(r._h, param, value)


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chaud_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint64], ctypes.c_int
    return f(r._h, pos)


def gaps(shape):
    return (2, 1) if shape == THREE else (0, 0)


@pytest.mark.parametrize("fin,fout", FORMATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_equals_the_cpu_backend_and_stays_within_the_bound(torch_dev, gpu, shape, fin, fout):
    nch, nsamp, nsec = shape
    gin, gout = gaps(shape)
    _, d_in, in_stride = dev_signal(nch, nsamp, fin, gin)
    gpu.setChannelAudioFilter(coefs(nch, nsec), fin, fout)
    y = run_device(torch_dev, gpu, d_in, nch, nsamp, in_stride, fout, gout)
    want = cpu_result(nch, nsamp, nsec, fin, fout)
    assert np.array_equal(bits(y), bits(want)), f"{np.count_nonzero(bits(y) != bits(want))} samples differ"
    if nch > 1:
        xin = signal(nch, nsamp, fin)[1]
        if fout == fin or fout == AUDIO_F32:
            assert np.array_equal(y[1], xin.astype(y.dtype))     # the identity channel
    y64, bnd = model(nch, nsamp, nsec, fin)
    k = y64.shape[0]
    err = np.abs(y[:k].astype(np.float64) - (np.clip(y64, -32768, 32767) if fout == AUDIO_S16 else y64))
    slack = 0.5 if fout == AUDIO_S16 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):   # a zero sample of the identity channel: 0 / 0
        print(f"{shape} {fin}->{fout}: worst (err - slack) / bound {np.nanmax((err - slack) / bnd):.3f}")
    assert np.all(err <= bnd + slack)


@pytest.mark.parametrize("fin,fout", FORMATS[:2])
@pytest.mark.parametrize("cut", list(CUTS) + ["per-sample", "10+20"])
def test_cuts_and_streams_are_bit_identical(torch_dev, gpu, cut, fin, fout):
    torch = torch_dev
    nch, nsec = 3, 4
    nsamp = {"per-sample": B + 2, "10+20": 30}.get(cut, 3 * B + 40)
    cuts = {"per-sample": [1] * (B + 2), "10+20": [10, 20]}.get(cut) or CUTS[cut](nsamp)
    _, d_in, in_stride = dev_signal(nch, nsamp, fin, 2)
    want = cpu_result(nch, nsamp, nsec, fin, fout)
    gpu.setChannelAudioFilter(coefs(nch, nsec), fin, fout)
    assert np.array_equal(bits(run_device(torch, gpu, d_in, nch, nsamp, in_stride, fout)), bits(want))
    gpu.resetChannelAudioFilter()
    assert np.array_equal(bits(run_cuts(torch, gpu, d_in, nch, nsamp, in_stride, cuts, fout)), bits(want))
    gpu.resetChannelAudioFilter()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = run_cuts(torch, gpu, d_in, nch, nsamp, in_stride, cuts, fout, streams)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("shape", [THREE, SHAPES[5]])
def test_bit_identical_for_any_grid_and_run_length_with_the_carried_state(torch_dev, gpu, shape):
    nch, nsamp, nsec = shape
    _, d_in, in_stride = dev_signal(nch, nsamp, AUDIO_F32, 0)
    want = cpu_result(nch, nsamp, nsec, AUDIO_F32, AUDIO_F32, calls=2)
    for cap, run in [(0, 0), (1, 0), (3, 0), (0, 1), (3, 1)]:
        assert set_param(gpu, PARAM_CHAUD_MAX_WGS, cap) == 0 and set_param(gpu, PARAM_CHAUD_RUN_BLOCKS, run) == 0
        gpu.setChannelAudioFilter(coefs(nch, nsec))
        y = np.concatenate([run_device(torch_dev, gpu, d_in, nch, nsamp, in_stride, AUDIO_F32) for _ in range(2)], axis=1)
        assert np.array_equal(bits(y), bits(want)), f"max_wgs {cap}, run_blocks {run}"
    assert set_param(gpu, PARAM_CHAUD_MAX_WGS, -1) == ERR_ARG and set_param(gpu, PARAM_CHAUD_RUN_BLOCKS, -1) == ERR_ARG


def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu):
    nch, nsamp, nsec = THREE
    want = cpu_result(nch, nsamp, nsec, AUDIO_F32, AUDIO_F32)
    for c in range(nch):
        buf = torch_dev.from_numpy(signal(nch, nsamp, AUDIO_F32)[c].copy()).to("cuda")
        gpu.setChannelAudioFilter(coefs(nch, nsec)[c:c + 1])
        y = run_device(torch_dev, gpu, buf, 1, nsamp, nsamp, AUDIO_F32)
        assert np.array_equal(bits(y[0]), bits(want[c]))


@pytest.mark.parametrize("fin,fout", FORMATS[:2])
def test_host_call_equals_the_device_call_and_shares_its_state(torch_dev, gpu, fin, fout):
    nch, nsamp, nsec = THREE
    cut = B + 9
    x = signal(nch, nsamp, fin)
    want = cpu_result(nch, nsamp, nsec, fin, fout)
    gpu.setChannelAudioFilter(coefs(nch, nsec), fin, fout)
    assert np.array_equal(bits(gpu.channel_audio_filter(x)), bits(want))
    # a device call, then a host call on the rest: one stream of samples
    gpu.resetChannelAudioFilter()
    _, d_in, in_stride = dev_signal(nch, nsamp, fin, 2)
    first = run_device(torch_dev, gpu, d_in, nch, cut, in_stride, fout)
    rest = gpu.channel_audio_filter(np.ascontiguousarray(x[:, cut:]))
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(want))
    # the host call writes the streams alone
    f = gpu._L.sddc_ddc_channel_audio_filter_host
    gpu.resetChannelAudioFilter()
    out = np.full((nch, nsamp + 3), poison(want.dtype), want.dtype)
    assert f(gpu._h, np.ascontiguousarray(x).ctypes.data, nch, nsamp, nsamp, out.ctypes.data, nsamp + 3) == 0
    assert np.array_equal(bits(out[:, :nsamp]), bits(want))
    assert (out[:, nsamp:] == S16_POISON).all() if fout == AUDIO_S16 else np.isnan(out[:, nsamp:]).all()


def test_a_stream_that_starts_inside_a_block(torch_dev, gpu):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    nch, nsamp, nsec = THREE
    _, d_in, in_stride = dev_signal(nch, nsamp, AUDIO_F32, 0)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelAudioFilter(coefs(nch, nsec))
        assert set_position(c, 5 * B + 200) == 0
        want = c.channel_audio_filter(signal(nch, nsamp, AUDIO_F32))
    gpu.setChannelAudioFilter(coefs(nch, nsec))
    assert set_position(gpu, 5 * B + 200) == 0
    assert np.array_equal(bits(run_device(torch_dev, gpu, d_in, nch, nsamp, in_stride, AUDIO_F32)), bits(want))


def test_decay_into_subnormals_is_bit_identical(torch_dev, gpu):
    """An impulse, then 3B zeros, through a double pole at 0.5 and a DC blocker: the first section's
    states fall through the subnormals to zero inside the first block.  Channel 1 starts at 1e-36."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    nsamp = 3 * B + 1
    sec = np.stack([np.array([1, 0, 0, -1.0, 0.25], np.float32), biquad(BIQUAD_DC_BLOCK, 1e-3)])
    coef = np.stack([sec, sec])
    x = np.zeros((2, nsamp), np.float32)
    x[0, 0], x[1, 0] = 1.0, 1e-36
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelAudioFilter(coef)
        want = c.channel_audio_filter(x)
    tiny = np.abs(want) < np.finfo(np.float32).tiny
    assert np.any(tiny & (want != 0)), "the test means to cross the subnormals"
    gpu.setChannelAudioFilter(coef)
    y = run_device(torch_dev, gpu, torch_dev.from_numpy(x).to("cuda"), 2, nsamp, nsamp, AUDIO_F32)
    diff = np.flatnonzero(bits(y).reshape(-1) != bits(want).reshape(-1))
    print(f"decay: {np.count_nonzero(tiny & (want != 0))} subnormal outputs, {diff.size} samples differ")
    assert diff.size == 0


def test_error_returns_leave_the_buffers_and_the_state_untouched(torch_dev, gpu):
    torch = torch_dev
    nch, nsamp, nsec = THREE
    _, d_in, in_stride = dev_signal(nch, nsamp, AUDIO_F32, 2)
    buf, out, stride = out_tensor(torch, nch, nsamp, 0, AUDIO_F32)
    f = gpu._L.sddc_ddc_channel_audio_filter_device
    args = (d_in.data_ptr(), nch, nsamp, in_stride, out.data_ptr(), stride, None)
    assert f(gpu._h, *args) == ERR_STATE                                  # nothing set
    gpu.setChannelAudioFilter(coefs(nch, nsec))
    cut = 100
    first = run_device(torch, gpu, d_in, nch, cut, in_stride, AUDIO_F32)
    bad = coefs(nch, nsec).copy()
    bad[2, 1, 4] = 1.0
    c = np.ascontiguousarray(bad)
    assert gpu._L.sddc_ddc_set_channel_audio_filter(gpu._h, c.ctypes.data, nsec, nch, 0, 0) == ERR_ARG   # sets nothing
    assert f(gpu._h, d_in.data_ptr(), 2, nsamp, in_stride, out.data_ptr(), stride, None) == ERR_STATE
    assert f(gpu._h, d_in.data_ptr(), nch, 0, in_stride, out.data_ptr(), stride, None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, (1 << 40) + 1, 1 << 41, out.data_ptr(), 1 << 41, None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, nsamp - 1, out.data_ptr(), stride, None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, in_stride, out.data_ptr(), nsamp - 1, None) == ERR_ARG
    assert f(gpu._h, None, nch, nsamp, in_stride, out.data_ptr(), stride, None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, in_stride, None, stride, None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr() + 2, nch, nsamp, in_stride, out.data_ptr(), stride, None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, in_stride, out.data_ptr() + 1, stride, None) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    rest = run_device(torch, gpu, d_in[cut:], nch, nsamp - cut, in_stride, AUDIO_F32)
    want = cpu_result(nch, nsamp, nsec, AUDIO_F32, AUDIO_F32)
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(want))
    gpu.setChannelAudioFilter(None)
    assert f(gpu._h, *args) == ERR_STATE


def test_ddc_decimator_am_demodulator_and_dc_blocker_on_one_stream(torch_dev):
    """process_channels_device at d = 6 (6 blocks, 3 channels, a tone) -> channel_decimate_device (R = 8)
    -> channel_demodulate_device in AM -> channel_audio_filter_device with a DC blocker, on one stream and
    on the demodulator's own buffer and stride: within the bound of the model applied to the demodulator
    output copied back; the IQ, the decimator output and the demodulator output bit-identical to a run
    without the stage set; and over the settled part |mean(y)| at most the float64 model's own mean plus
    the mean bound (the carrier's DC is gone)."""
    from extio_sddc_amd import DEMOD_AM, R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import make_tone_stream
    torch = torch_dev
    d, nblk, R, tbs = 6, 6, 8, [1000, 1008, 1012]
    h = kaiser(65, 60.0, 0.04, 0.0625)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    nout = nsamp // R   # 384: a full block and a tail
    coef = np.stack([np.stack([biquad(BIQUAD_DC_BLOCK, 0.01)])] * nch)
    d_in = torch.from_numpy(make_tone_stream(nblk, 1010.3, amp=20000.0)).to("cuda")

    def chain(r, audio):
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device="cuda")
        nb = torch.zeros((nch, 2 * nout), dtype=torch.float32, device="cuda")
        am = torch.zeros((nch, nout + 5), dtype=torch.float32, device="cuda")
        buf, out, stride = out_tensor(torch, nch, nout, 1, AUDIO_F32)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=s)
        r.channel_decimate_device(iq, nch, nsamp, iq.stride(0), nb, nb.stride(0), stream=s)
        r.channel_demodulate_device(nb, nch, nout, nb.stride(0), am, am.stride(0), stream=s)
        if audio:
            r.channel_audio_filter_device(am, nch, nout, am.stride(0), out, stride, stream=s)
        torch.cuda.synchronize()
        return iq.cpu().numpy(), nb.cpu().numpy(), am.cpu().numpy(), (collect(buf, nch, nout, 1, AUDIO_F32) if audio else None)

    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        r.setChannelDecimator(h, R, nch)
        r.setChannelDemodulator([DEMOD_AM] * nch, np.full(nch, 1e-3, np.float32))
        iq0, nb0, am0, _ = chain(r, False)
        r.setChannelDecimator(h, R, nch)
        r.setChannelDemodulator([DEMOD_AM] * nch, np.full(nch, 1e-3, np.float32))
        r.setChannelAudioFilter(coef)
        iq1, nb1, am1, y = chain(r, True)
    np.testing.assert_array_equal(bits(iq1), bits(iq0))
    np.testing.assert_array_equal(bits(nb1), bits(nb0))
    np.testing.assert_array_equal(bits(am1), bits(am0))
    x = np.ascontiguousarray(am1[:, :nout])
    assert np.abs(x).max() > 0
    y64, bnd = M.recurrence64(x, coef), M.bounds(x, coef)
    err = np.abs(y.astype(np.float64) - y64)
    print(f"DDC + decimator + AM + DC blocker, {nout} samples: worst err / bound {np.max(err / bnd):.3f}")
    assert np.all(err <= bnd)
    settled = slice(nout // 2, nout)
    for c in range(nch):
        got, own = abs(float(y[c, settled].astype(np.float64).mean())), abs(float(y64[c, settled].mean()))
        print(f"  channel {c}: carrier {x[c, settled].mean():.4f}, |mean y| {got:.3e}, the model's {own:.3e}")
        assert got <= own + bnd[c, settled].mean()
