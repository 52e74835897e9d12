"""The channel AGC on the GPU (pytest -m gpu): sddc_ddc_channel_agc_device and sddc_ddc_channel_agc_host
of a GPU handle bit for bit against the CPU backend (which tests/test_channel_agc_cpu.py pins to the
definition), outputs and envelopes, within the float64 recurrence's bound (tools/channel_agc_model.py),
the bit-exact properties of the kernels (cuts, streams, grids, run length, a channel alone), and the
DDC, the decimator, the AM demodulator, this stage and a DC blocker on one stream.

Shapes (nch, nsamp), B = the block length (AGC_BLOCK):
  (1, 1)            one sample: no full block
  (1, B)            exactly one block
  (1, 3B + 17)      full blocks and a tail
  (3, 2B + 3)       differing parameters, one bypassed channel; input and output gaps poisoned
  (1024, 2)         every channel, almost no samples each
  (1, 66B + 5)      more blocks than a wave has lanes
  (2, 258B + 1)     more blocks than four waves have
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


M = _load("channel_agc_model")

from extio_sddc_amd import AGC_BLOCK as B  # noqa: E402
from extio_sddc_amd import AUDIO_F32, AUDIO_S16, BIQUAD_DC_BLOCK, biquad  # noqa: E402

PARAM_CHAGC_MAX_WGS, PARAM_CHAGC_RUN_BLOCKS = 18, 19   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
U = 2.0 ** -24
STEP_LIMIT_S = 60
HEAD, OFFSET = 1, 3        # samples before d_out / d_in in their poisoned tensors
S16_POISON = 0x7fff
S16_SCALE = 2000.0         # float streams as int16
SHAPES = [(1, 1), (1, B), (1, 3 * B + 17), (3, 2 * B + 3), (1024, 2), (1, 66 * B + 5), (2, 258 * B + 1)]
THREE = SHAPES[3]
FORMATS = [(AUDIO_F32, AUDIO_F32), (AUDIO_S16, AUDIO_S16), (AUDIO_F32, AUDIO_S16), (AUDIO_S16, AUDIO_F32)]
CUTS = {"edges": lambda n: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n: [100, B, n - B - 100]}
FEW = [27, 3, 44]          # rows of make_params(48) for shapes of up to three channels: (T, d, F) all differ


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
def params(nch):
    """[nch, 3] = (T, d, F): the channels differ; channel 1 (of several) is bypassed."""
    p = M.make_params(nch) if nch > 3 else M.make_params(48)[FEW[:nch]].copy()
    if nch > 1:
        p[1, 0] = 0.0
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def signal(nch, nsamp, fin):
    """[nch, nsamp] float32 (loud, then 40 dB down), or its int16 form."""
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


def env_tensor(torch, nch):
    """nch floats one float into a poisoned tensor."""
    buf = torch.full((nch + 2,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[1:]


def collect(buf, nch, nsamp, gap, fout):
    """[nch, nsamp] of a finished call; the head, the tail and the gaps must still hold the poison (no
    correct S16 output of these inputs is 0x7fff: the targets are 16384 at most)."""
    stride = nsamp + gap
    y = buf.cpu().numpy()
    clean = (lambda v: (v == S16_POISON).all()) if fout == AUDIO_S16 else (lambda v: np.isnan(v).all())
    body = y[HEAD:HEAD + nch * stride].reshape(nch, stride)
    assert clean(y[:HEAD]) and clean(y[HEAD + nch * stride:]) and clean(body[:, nsamp:])
    return np.ascontiguousarray(body[:, :nsamp])


def collect_env(ebuf, nch):
    e = ebuf.cpu().numpy()
    assert np.isnan(e[0]) and np.isnan(e[nch + 1])
    return np.ascontiguousarray(e[1:nch + 1])


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run_device(torch, r, d_in, nch, nsamp, in_stride, fout, gap=0, stream_=None):
    """(outputs [nch, nsamp], envelopes [nch]) of one device call."""
    buf, out, stride = out_tensor(torch, nch, nsamp, gap, fout)
    ebuf, env = env_tensor(torch, nch)
    if stream_ is not None:
        stream_.wait_stream(torch.cuda.current_stream())
    r.channel_agc_device(d_in, nch, nsamp, in_stride, out, stride, d_env=env, stream=stream_)
    torch.cuda.synchronize()
    return collect(buf, nch, nsamp, gap, fout), collect_env(ebuf, nch)


def run_cuts(torch, r, d_in, nch, nsamp, in_stride, cuts, fout, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of d_in it covers; nothing
    synchronises between the calls.  Returns the outputs and the last call's envelopes."""
    assert sum(cuts) == nsamp and min(cuts) > 0
    at = 0
    outs = [out_tensor(torch, nch, n, 0, fout) for n in cuts]
    ebuf, env = env_tensor(torch, nch)
    torch.cuda.synchronize()   # the poison fills are done before a call on another stream writes
    for k, n in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        r.channel_agc_device(d_in[at:], nch, n, in_stride, outs[k][1], outs[k][2],
                             d_env=env if k == len(cuts) - 1 else None, stream=s)
        at += n
    torch.cuda.synchronize()
    return np.concatenate([collect(o[0], nch, n, 0, fout) for o, n in zip(outs, cuts)], axis=1), collect_env(ebuf, nch)


@functools.lru_cache(maxsize=None)
def cpu_result(nch, nsamp, fin, fout, calls=1):
    """The CPU backend's outputs of `calls` consecutive calls on the same samples, [nch, calls nsamp],
    and the envelopes after the last."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelAgc(params(nch), fin, fout)
        parts = [c.channel_agc(signal(nch, nsamp, fin), envelope=True) for _ in range(calls)]
    y, env = np.concatenate([p[0] for p in parts], axis=1), parts[-1][1]
    y.setflags(write=False)
    env.setflags(write=False)
    return y, env


@functools.lru_cache(maxsize=None)
def model(nch, nsamp, fin):
    """(y64, bound) of the first three channels."""
    k = min(nch, 3)
    x, p = signal(nch, nsamp, fin)[:k], params(nch)[:k]
    return M.recurrence64(x, p)[0], M.bounds(x, p)


def set_param(r, param, value):
    f = r._L.sddc_ddc_internal_set_param
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    return f(r._h, param, value)


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chagc_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint64], ctypes.c_int
    return f(r._h, pos)


def gaps(shape):
    return (2, 1) if shape == THREE else (0, 0)


@pytest.mark.parametrize("fin,fout", FORMATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_equals_the_cpu_backend_and_stays_within_the_bound(torch_dev, gpu, shape, fin, fout):
    nch, nsamp = shape
    gin, gout = gaps(shape)
    _, d_in, in_stride = dev_signal(nch, nsamp, fin, gin)
    gpu.setChannelAgc(params(nch), fin, fout)
    y, env = run_device(torch_dev, gpu, d_in, nch, nsamp, in_stride, fout, gout)
    want, wenv = cpu_result(nch, nsamp, fin, fout)
    assert np.array_equal(bits(y), bits(want)), f"{np.count_nonzero(bits(y) != bits(want))} samples differ"
    assert np.array_equal(bits(env), bits(wenv))
    if nch > 1:   # the bypassed channel: the sample as it is, and its envelope still moves
        xin = signal(nch, nsamp, fin)[1]
        if fout == fin or fout == AUDIO_F32:
            assert np.array_equal(bits(y[1]), bits(xin.astype(y.dtype)))
        assert env[1] > 0
    y64, bnd = model(nch, nsamp, fin)
    k = y64.shape[0]
    err = np.abs(y[:k].astype(np.float64) - (np.clip(y64, -32768, 32767) if fout == AUDIO_S16 else y64))
    slack = 0.5 if fout == AUDIO_S16 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):   # the bypassed channel: 0 / 0
        print(f"{shape} {fin}->{fout}: worst (err - slack) / bound {np.nanmax((err - slack) / bnd):.3f}")
    assert np.all(err <= bnd + slack)


@pytest.mark.parametrize("fin,fout", FORMATS[:2])
@pytest.mark.parametrize("cut", list(CUTS) + ["per-sample", "10+20"])
def test_cuts_and_streams_are_bit_identical(torch_dev, gpu, cut, fin, fout):
    torch = torch_dev
    nch = 3
    nsamp = {"per-sample": B + 2, "10+20": 30}.get(cut, 3 * B + 40)
    cuts = {"per-sample": [1] * (B + 2), "10+20": [10, 20]}.get(cut) or CUTS[cut](nsamp)
    _, d_in, in_stride = dev_signal(nch, nsamp, fin, 2)
    want, wenv = cpu_result(nch, nsamp, fin, fout)
    gpu.setChannelAgc(params(nch), fin, fout)
    y, env = run_device(torch, gpu, d_in, nch, nsamp, in_stride, fout)
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(env), bits(wenv))
    gpu.resetChannelAgc()
    y, env = run_cuts(torch, gpu, d_in, nch, nsamp, in_stride, cuts, fout)
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(env), bits(wenv))
    gpu.resetChannelAgc()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    y, env = run_cuts(torch, gpu, d_in, nch, nsamp, in_stride, cuts, fout, streams)
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(env), bits(wenv))


@pytest.mark.parametrize("shape", [THREE, SHAPES[5]])
def test_bit_identical_for_any_grid_and_run_length_with_the_carried_state(torch_dev, gpu, shape):
    nch, nsamp = shape
    _, d_in, in_stride = dev_signal(nch, nsamp, AUDIO_F32, 0)
    want, wenv = cpu_result(nch, nsamp, AUDIO_F32, AUDIO_F32, calls=2)
    for cap, run in [(0, 0), (1, 0), (3, 0), (0, 1), (3, 1)]:
        assert set_param(gpu, PARAM_CHAGC_MAX_WGS, cap) == 0 and set_param(gpu, PARAM_CHAGC_RUN_BLOCKS, run) == 0
        gpu.setChannelAgc(params(nch))
        parts = [run_device(torch_dev, gpu, d_in, nch, nsamp, in_stride, AUDIO_F32) for _ in range(2)]
        y = np.concatenate([p[0] for p in parts], axis=1)
        assert np.array_equal(bits(y), bits(want)), f"max_wgs {cap}, run_blocks {run}"
        assert np.array_equal(bits(parts[-1][1]), bits(wenv)), f"max_wgs {cap}, run_blocks {run}"
    assert set_param(gpu, PARAM_CHAGC_MAX_WGS, -1) == ERR_ARG and set_param(gpu, PARAM_CHAGC_RUN_BLOCKS, -1) == ERR_ARG


def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu):
    nch, nsamp = THREE
    want, wenv = cpu_result(nch, nsamp, AUDIO_F32, AUDIO_F32)
    for c in range(nch):
        buf = torch_dev.from_numpy(signal(nch, nsamp, AUDIO_F32)[c].copy()).to("cuda")
        gpu.setChannelAgc(params(nch)[c:c + 1])
        y, env = run_device(torch_dev, gpu, buf, 1, nsamp, nsamp, AUDIO_F32)
        assert np.array_equal(bits(y[0]), bits(want[c])) and np.array_equal(bits(env), bits(wenv[c:c + 1]))


@pytest.mark.parametrize("fin,fout", FORMATS[:2])
def test_host_call_equals_the_device_call_and_shares_its_state(torch_dev, gpu, fin, fout):
    nch, nsamp = THREE
    cut = B + 9
    x = signal(nch, nsamp, fin)
    want, wenv = cpu_result(nch, nsamp, fin, fout)
    gpu.setChannelAgc(params(nch), fin, fout)
    y, env = gpu.channel_agc(x, envelope=True)
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(env), bits(wenv))
    # a device call, then a host call on the rest: one stream of samples
    gpu.resetChannelAgc()
    _, d_in, in_stride = dev_signal(nch, nsamp, fin, 2)
    first, _ = run_device(torch_dev, gpu, d_in, nch, cut, in_stride, fout)
    rest, env = gpu.channel_agc(np.ascontiguousarray(x[:, cut:]), envelope=True)
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(want)) and np.array_equal(bits(env), bits(wenv))
    # the host call writes the streams alone, and env may be null
    f = gpu._L.sddc_ddc_channel_agc_host
    gpu.resetChannelAgc()
    out = np.full((nch, nsamp + 3), poison(want.dtype), want.dtype)
    assert f(gpu._h, np.ascontiguousarray(x).ctypes.data, nch, nsamp, nsamp, out.ctypes.data, nsamp + 3, None) == 0
    assert np.array_equal(bits(out[:, :nsamp]), bits(want))
    assert (out[:, nsamp:] == S16_POISON).all() if fout == AUDIO_S16 else np.isnan(out[:, nsamp:]).all()


def test_a_stream_that_starts_inside_a_block(torch_dev, gpu):
    from extio_sddc_amd import DEVICE_CPU, R2iq
    nch, nsamp = THREE
    _, d_in, in_stride = dev_signal(nch, nsamp, AUDIO_F32, 0)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelAgc(params(nch))
        assert set_position(c, 5 * B + 200) == 0
        want, wenv = c.channel_agc(signal(nch, nsamp, AUDIO_F32), envelope=True)
    gpu.setChannelAgc(params(nch))
    assert set_position(gpu, 5 * B + 200) == 0
    y, env = run_device(torch_dev, gpu, d_in, nch, nsamp, in_stride, AUDIO_F32)
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(env), bits(wenv))


def test_decay_into_subnormals_is_bit_identical(torch_dev, gpu):
    """An impulse, then zeros, d = 0.5 (dB underflows to 0), F = 2^-60, calls that end at samples 130,
    140 and 200: the envelope is subnormal after the first two and 0 after the third."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    p = np.array([[0.5, 0.5, 2.0 ** -60]], np.float32)
    x = np.zeros((1, 200), np.float32)
    x[0, 0] = 1.0
    d_x = torch_dev.from_numpy(x.reshape(-1)).to("cuda")
    tiny = float(np.finfo(np.float32).tiny)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelAgc(p)
        gpu.setChannelAgc(p)
        at = 0
        for end in (130, 140, 200):
            want, wenv = c.channel_agc(x[:, at:end], envelope=True)
            y, env = run_device(torch_dev, gpu, d_x[at:], 1, end - at, end - at, AUDIO_F32)
            print(f"decay: the envelope after sample {end - 1}: {env[0]!r} (the CPU backend: {wenv[0]!r})")
            assert (0 < wenv[0] < tiny) if end < 200 else wenv[0] == 0
            assert np.array_equal(bits(env), bits(wenv)) and np.array_equal(bits(y), bits(want))
            at = end


def test_error_returns_leave_the_buffers_and_the_state_untouched(torch_dev, gpu):
    torch = torch_dev
    nch, nsamp = THREE
    _, d_in, in_stride = dev_signal(nch, nsamp, AUDIO_F32, 2)
    buf, out, stride = out_tensor(torch, nch, nsamp, 0, AUDIO_F32)
    ebuf, env = env_tensor(torch, nch)
    f = gpu._L.sddc_ddc_channel_agc_device
    args = (d_in.data_ptr(), nch, nsamp, in_stride, out.data_ptr(), stride, env.data_ptr(), None)
    assert f(gpu._h, *args) == ERR_STATE                                  # nothing set
    assert gpu._L.sddc_ddc_channel_agc_reset(gpu._h) == ERR_STATE and set_position(gpu, 3) == ERR_STATE
    gpu.setChannelAgc(params(nch))
    cut = 100
    first, _ = run_device(torch, gpu, d_in, nch, cut, in_stride, AUDIO_F32)
    for col, v in [(0, -0.5), (0, 2.0 ** 61), (1, 1.0), (1, -0.1), (2, 0.0), (2, float("nan"))]:
        bad = np.ascontiguousarray(params(nch).copy())
        bad[2, col] = v
        assert gpu._L.sddc_ddc_set_channel_agc(gpu._h, bad.ctypes.data, nch, 0, 0) == ERR_ARG   # sets nothing
    good = np.ascontiguousarray(params(nch))
    assert gpu._L.sddc_ddc_set_channel_agc(gpu._h, good.ctypes.data, nch, 2, 0) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), 2, nsamp, in_stride, out.data_ptr(), stride, env.data_ptr(), None) == ERR_STATE
    assert f(gpu._h, d_in.data_ptr(), nch, 0, in_stride, out.data_ptr(), stride, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, (1 << 40) + 1, 1 << 41, out.data_ptr(), 1 << 41, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, nsamp - 1, out.data_ptr(), stride, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, in_stride, out.data_ptr(), nsamp - 1, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, None, nch, nsamp, in_stride, out.data_ptr(), stride, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, in_stride, None, stride, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr() + 2, nch, nsamp, in_stride, out.data_ptr(), stride, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, in_stride, out.data_ptr() + 1, stride, env.data_ptr(), None) == ERR_ARG
    assert f(gpu._h, d_in.data_ptr(), nch, nsamp, in_stride, out.data_ptr(), stride, env.data_ptr() + 2, None) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(buf).all() and torch.isnan(ebuf).all()
    rest, e = run_device(torch, gpu, d_in[cut:], nch, nsamp - cut, in_stride, AUDIO_F32)
    want, wenv = cpu_result(nch, nsamp, AUDIO_F32, AUDIO_F32)
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(want)) and np.array_equal(bits(e), bits(wenv))
    gpu.setChannelAgc(None)
    assert f(gpu._h, *args) == ERR_STATE


def test_ddc_decimator_am_demodulator_agc_and_dc_blocker_on_one_stream(torch_dev):
    """process_channels_device at d = 6 (6 blocks, 3 channels, a tone) -> channel_decimate_device (R = 8)
    -> channel_demodulate_device in AM -> channel_agc_device (d = 0.999, T = 0.5) on the demodulator's
    own buffer and stride -> channel_audio_filter_device with a DC blocker, on one stream, at two input
    levels 20 dB apart.  The IQ, the decimator output and the demodulator output are bit-identical to a
    run without the AGC set; the AGC output is within the bound of the model applied to the demodulator
    output copied back; over the second half both levels sit on T at their new-peak samples (within
    2 u T) and never exceed T (1 + 2 u); the DC blocker's output is the CPU backend's on the AGC output."""
    from extio_sddc_amd import DEMOD_AM, DEVICE_CPU, R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import make_tone_stream
    torch = torch_dev
    d, nblk, R, tbs = 6, 6, 8, [1000, 1008, 1012]
    h = kaiser(65, 60.0, 0.04, 0.0625)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    nout = nsamp // R   # 384: a full block and a tail
    T = 0.5
    p = np.tile(np.array([[T, 0.999, 1e-9]], np.float32), (nch, 1))
    coef = np.stack([np.stack([biquad(BIQUAD_DC_BLOCK, 0.01)])] * nch)

    def chain(r, d_in, agc):
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device="cuda")
        nb = torch.zeros((nch, 2 * nout), dtype=torch.float32, device="cuda")
        am = torch.zeros((nch, nout + 5), dtype=torch.float32, device="cuda")
        buf, out, stride = out_tensor(torch, nch, nout, 1, AUDIO_F32)
        dc = torch.zeros((nch, nout), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=s)
        r.channel_decimate_device(iq, nch, nsamp, iq.stride(0), nb, nb.stride(0), stream=s)
        r.channel_demodulate_device(nb, nch, nout, nb.stride(0), am, am.stride(0), stream=s)
        if agc:
            r.channel_agc_device(am, nch, nout, am.stride(0), out, stride, stream=s)
            r.channel_audio_filter_device(out, nch, nout, stride, dc, dc.stride(0), stream=s)
        torch.cuda.synchronize()
        return (iq.cpu().numpy(), nb.cpu().numpy(), am.cpu().numpy(),
                collect(buf, nch, nout, 1, AUDIO_F32) if agc else None, dc.cpu().numpy())

    for amp in (20000.0, 2000.0):
        d_in = torch.from_numpy(make_tone_stream(nblk, 1010.3, amp=amp)).to("cuda")
        with R2iq(gain=1.0) as r:
            r.setDecimate(d)
            r.setChannelDecimator(h, R, nch)
            r.setChannelDemodulator([DEMOD_AM] * nch, np.full(nch, 1e-3, np.float32))
            iq0, nb0, am0, _, _ = chain(r, d_in, False)
            r.setChannelDecimator(h, R, nch)
            r.setChannelDemodulator([DEMOD_AM] * nch, np.full(nch, 1e-3, np.float32))
            r.setChannelAgc(p)
            r.setChannelAudioFilter(coef)
            iq1, nb1, am1, y, dc = chain(r, d_in, True)
        np.testing.assert_array_equal(bits(iq1), bits(iq0))
        np.testing.assert_array_equal(bits(nb1), bits(nb0))
        np.testing.assert_array_equal(bits(am1), bits(am0))
        x = np.ascontiguousarray(am1[:, :nout])
        assert np.abs(x).max() > 0
        y64, bnd = M.recurrence64(x, p)[0], M.bounds(x, p)
        err = np.abs(y.astype(np.float64) - y64)
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"amp {amp:g}: demodulated level {np.abs(x[:, nout // 2:]).max():.4g}, worst err / bound "
                  f"{np.nanmax(np.where(bnd > 0, err / bnd, 0)):.3f}")
        assert np.all(err <= bnd)
        _, _, Rt = M.definition32(x, p, trace=True)
        late = np.zeros(x.shape, bool)
        late[:, nout // 2:] = True
        peak = (Rt == np.abs(x)) & (np.abs(x) > p[:, 2:]) & late     # the step took the sample: den = |x|
        ya = np.abs(y.astype(np.float64))
        print(f"amp {amp:g}: {np.count_nonzero(peak)} new peaks in the second half, max |y| {ya[late].max():.9g}")
        # channel 0 holds the tone in the decimator's stop band: after the filter's transient its envelope
        # only decays, so it may have no new peak; the two channels with the tone in band have them throughout
        assert peak[1:].sum(axis=1).min() > nout // 4
        assert np.all(np.abs(ya[peak] - T) <= 2 * U * T) and np.all(ya <= T * (1 + 2 * U))
        assert abs(ya[late].max() - T) <= 2 * U * T
        with R2iq(gain=1.0, device=DEVICE_CPU) as c:
            c.setChannelAudioFilter(coef)
            np.testing.assert_array_equal(bits(dc), bits(c.channel_audio_filter(y)))
