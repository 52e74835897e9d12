"""The channel demodulator on the GPU (pytest -m gpu): sddc_ddc_channel_demodulate_device and
sddc_ddc_channel_demodulate_host of a GPU handle against the float64 model and its bounds
(tools/channel_demod_model.py), bit for bit against the CPU backend, the bit-exact properties of the
kernel (cuts, grids, a channel alone), and the DDC, the decimator and the demodulator on one stream.

The bars (u = 2^-24; sddc_ddc.h): AM |y - y64| <= 4 u |y64|; FM |y - g theta64| <= |g| (4 u + 8 u
|theta64|) where |x[i]| |x[i - 1]| > 0; BFO |y - y64| <= |g| (|I| + |Q|) 6 u; power |P - P64| <=
gamma_n P64 with n = nsamp + 3, GPU against the CPU backend within twice that; the demodulated
samples of a GPU handle and a CPU handle bit-identical in F32 and S16.
Shapes (nch, nsamp, input gap in components, output gap in samples, first-sample offset in samples),
T = the kernel's samples per tile (CHANNEL_DEMOD_TILE):
  (1, 1, 0, 0, 0)          one sample
  (1, T + 1, 0, 0, 1)      a tail tile with one sample, the first sample 1 past a 16-byte line
  (1, T - 1, 0, 0, 3)      CS16: 3 past a line
  (3, 2T + 3, 2, 1, 0)     modes AM, FM, BFO; the channels' alignments differ; an odd out_stride
  (1024, 2, 0, 0, 0)       every channel, almost no samples each, the modes cycling
  (2, 65, 0, 1, 2)         crosses a wave edge
Channels of one or two streams run every rotation of the modes.  Input gaps hold NaN (CF32) or
0x7fff (CS16).  Every d_out sits one output sample into a poisoned tensor (NaN, S16: a code that no
correct output of these inputs equals), so S16 starts 2-byte but not 4-byte aligned; its head, tail
and the gaps between the streams must stay untouched.  Every test runs under a watchdog that ends
the process if a GPU step hangs.
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


M = _load("channel_demod_model")

from extio_sddc_amd import AUDIO_F32, AUDIO_S16, DEMOD_BFO, DEMOD_FM  # noqa: E402
from extio_sddc_amd import CHANNEL_DEMOD_TILE as T  # noqa: E402

FORMATS = ["CF32", "CS16"]
OUT_FORMATS = [AUDIO_F32, AUDIO_S16]
CS16_SCALE = 4.0
PARAM_CHDEM_MAX_WGS = 15   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
HEAD = 1                   # output samples before d_out in its poisoned tensor
SHAPES = [(1, 1, 0, 0, 0), (1, T + 1, 0, 0, 1), (1, T - 1, 0, 0, 3), (3, 2 * T + 3, 2, 1, 0), (1024, 2, 0, 0, 0),
          (2, 65, 0, 1, 2)]
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


def mode_sets(nch):
    """One or two streams run every rotation of (AM, FM, BFO), more streams the cycle alone."""
    return [[(c + r) % 3 for c in range(nch)] for r in range(3 if nch <= 2 else 1)]


@functools.lru_cache(maxsize=None)
def signal(kind, nch, nsamp):
    x = M.make_input(kind, nch, nsamp)
    x.setflags(write=False)
    return x


def components(x, fmt, extra=0):
    """The streams as the DDC writes them: [nch, 2 nsamp + extra] components, the gaps poisoned."""
    return M.as_cs16(x, extra, 0x7fff) if fmt == "CS16" else M.as_cf32(x, extra, np.nan)


@functools.lru_cache(maxsize=None)
def dev_signal(kind, nch, nsamp, fmt, extra, offset=0):
    """(the device tensor, d_iq `offset` samples into it): poison before the first sample too."""
    import torch
    body = components(signal(kind, nch, nsamp), fmt, extra).reshape(-1)
    head = np.full(2 * offset, 0x7fff if fmt == "CS16" else np.nan, body.dtype)
    buf = torch.from_numpy(np.concatenate([head, body])).to("cuda")
    return buf, buf[2 * offset:]


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
    return f(r._h, PARAM_CHDEM_MAX_WGS, cap)


def set_position(r, pos):
    f = r._L.sddc_ddc_internal_chdem_set_position
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_int
    return f(r._h, pos)


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def out_tensor(torch, nch, nsamp, gap, s16):
    """(the poisoned tensor, d_out one output sample into it, out_stride)."""
    stride = nsamp + gap
    if s16:
        buf = torch.full((HEAD + nch * stride + 64,), M.S16_POISON, dtype=torch.int16, device="cuda")
    else:
        buf = torch.full((HEAD + nch * stride + 64,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[HEAD:], stride


def collect(buf, nch, nsamp, gap, s16):
    """[nch, nsamp] of a finished call; the head, the tail and the gaps must still hold the poison."""
    stride = nsamp + gap
    y = buf.cpu().numpy()
    clean = (lambda v: (v == M.S16_POISON).all()) if s16 else (lambda v: np.isnan(v).all())
    body = y[HEAD:HEAD + nch * stride].reshape(nch, stride)
    assert clean(y[:HEAD]) and clean(y[HEAD + nch * stride:]) and clean(body[:, nsamp:])
    return np.ascontiguousarray(body[:, :nsamp])


def run_device(torch, r, d_iq, nch, nsamp, in_stride, gap=0, s16=False, power=True, stream_=None):
    """One channel_demodulate_device call -> ([nch, nsamp], power [nch] or None)."""
    buf, out, stride = out_tensor(torch, nch, nsamp, gap, s16)
    pbuf = torch.full((nch + 2,), float("nan"), dtype=torch.float32, device="cuda") if power else None
    if stream_ is not None:
        stream_.wait_stream(torch.cuda.current_stream())
    r.channel_demodulate_device(d_iq, nch, nsamp, in_stride, out, stride, None if pbuf is None else pbuf[1:], stream=stream_)
    torch.cuda.synchronize()
    p = None
    if power:
        p = pbuf.cpu().numpy()
        assert np.isnan(p[0]) and np.isnan(p[nch + 1])
        p = p[1:nch + 1].copy()
    return collect(buf, nch, nsamp, gap, s16), p


def run_cuts(torch, r, d_iq, nch, nsamp, in_stride, cuts, s16, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of d_iq it covers; nothing
    synchronises between the calls."""
    assert sum(cuts) == nsamp
    flat, at = d_iq.reshape(-1), 0
    outs = [out_tensor(torch, nch, n, 0, s16) for n in cuts]
    torch.cuda.synchronize()   # the poison fills are done before a call on another stream writes
    for k, n in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        r.channel_demodulate_device(flat[2 * at:], nch, n, in_stride, outs[k][1], outs[k][2], stream=s)
        at += n
    torch.cuda.synchronize()
    return np.concatenate([collect(o[0], nch, n, 0, s16) for o, n in zip(outs, cuts)], axis=1)


@functools.lru_cache(maxsize=None)
def cpu_result(kind, nch, nsamp, fmt, out_fmt, modes, calls=1):
    """The CPU backend's outputs and powers of `calls` consecutive calls on the same samples."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    m, g, w = M.channel_params(nch, list(modes))
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        set_format(c, fmt)
        c.setChannelDemodulator(m, g, w, out_fmt)
        res = [c.channel_demodulate(host_iq(signal(kind, nch, nsamp), fmt), power=True) for _ in range(calls)]
    return np.concatenate([y for y, _ in res], axis=1), np.stack([p for _, p in res])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bounds_device(torch_dev, gpu, shape, fmt):
    nch, nsamp, extra, gap, off = shape
    set_format(gpu, fmt)
    for modes in mode_sets(nch):
        m, g, w = M.channel_params(nch, modes)
        for kind in ("noise", "edges"):
            gpu.setChannelDemodulator(m, g, w)
            _, d_iq = dev_signal(kind, nch, nsamp, fmt, extra, off)
            y, p = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, gap)
            xv = sample_values(signal(kind, nch, nsamp), fmt)
            e = M.excess(y, xv, m, g, w)
            pe = float((np.abs(p - M.power(xv)) - M.power_bound(xv)).max())
            print(f"{kind} {fmt} {shape} {modes[:3]}: |y - y64| - bound <= {e:.3e}, |P - P64| - bound <= {pe:.3e}")
            assert np.isfinite(y).all() and e <= 0.0 and pe <= 0.0


@pytest.mark.parametrize("out_fmt", OUT_FORMATS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_equals_the_cpu_backend_bit_for_bit(torch_dev, gpu, shape, fmt, out_fmt):
    nch, nsamp, extra, gap, off = shape
    s16 = out_fmt == AUDIO_S16
    set_format(gpu, fmt)
    for modes in mode_sets(nch):
        m, g, w = M.channel_params(nch, modes)
        for kind in ("noise", "edges"):
            gpu.setChannelDemodulator(m, g, w, out_fmt)
            _, d_iq = dev_signal(kind, nch, nsamp, fmt, extra, off)
            y, p = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, gap, s16)
            yc, pc = cpu_result(kind, nch, nsamp, fmt, out_fmt, tuple(modes))
            np.testing.assert_array_equal(bits(y), bits(yc))
            xv = sample_values(signal(kind, nch, nsamp), fmt)
            assert (np.abs(p.astype(np.float64) - pc[0]) <= M.power_bound(xv, 2.0)).all()
            if s16:   # at most one code from the model's value
                ok = np.isfinite(M.bound(xv, m, g, w))
                ref = M.to_s16(M.demodulate(xv, m, g, w)[0]).astype(np.int32)
                assert (np.abs(y.astype(np.int32) - ref)[ok] <= 1).all() and np.abs(y).max() < M.S16_POISON


@pytest.mark.parametrize("out_fmt", OUT_FORMATS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_cuts_are_bit_identical(torch_dev, gpu, fmt, out_fmt):
    """The 3-channel shape in one call against the cuts [1, T, rest] and against a call per sample on
    the first 64 samples; the same cuts with consecutive calls alternating between two streams."""
    torch = torch_dev
    nch, nsamp, extra, _, _ = THREE
    s16 = out_fmt == AUDIO_S16
    set_format(gpu, fmt)
    m, g, w = M.channel_params(nch)
    _, d_iq = dev_signal("noise", nch, nsamp, fmt, extra)
    S = 2 * nsamp + extra
    gpu.setChannelDemodulator(m, g, w, out_fmt)
    whole, _ = run_device(torch, gpu, d_iq, nch, nsamp, S, 0, s16)
    np.testing.assert_array_equal(bits(whole), bits(cpu_result("noise", nch, nsamp, fmt, out_fmt, tuple(m.tolist()))[0]))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for streams in (None, [side, torch.cuda.current_stream()]):
        gpu.setChannelDemodulator(m, g, w, out_fmt)
        got = run_cuts(torch, gpu, d_iq, nch, nsamp, S, [1, T, nsamp - T - 1], s16, streams)
        np.testing.assert_array_equal(bits(got), bits(whole))
        gpu.resetChannelDemodulator()
        got = run_cuts(torch, gpu, d_iq, nch, 64, S, [1] * 64, s16, streams)
        np.testing.assert_array_equal(bits(got), bits(whole[:, :64]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu, fmt):
    nch, nsamp, extra, _, _ = THREE
    set_format(gpu, fmt)
    m, g, w = M.channel_params(nch)
    _, d_iq = dev_signal("noise", nch, nsamp, fmt, extra)
    gpu.setChannelDemodulator(m, g, w)
    among, p_among = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra)
    rows = d_iq.reshape(nch, 2 * nsamp + extra)
    for c in range(nch):
        gpu.setChannelDemodulator(m[c:c + 1], g[c:c + 1], w[c:c + 1])
        alone, p_alone = run_device(torch_dev, gpu, rows[c], 1, nsamp, 0)
        np.testing.assert_array_equal(bits(alone[0]), bits(among[c]))
        np.testing.assert_array_equal(bits(p_alone), bits(p_among[c:c + 1]))


@pytest.mark.parametrize("out_fmt", OUT_FORMATS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_identical_for_any_grid_and_from_run_to_run(torch_dev, gpu, fmt, out_fmt):
    """9 items (3 channels x 3 tiles): capped at 1 a workgroup takes all 9, capped at 3 it takes 3."""
    nch, nsamp, extra, gap, _ = THREE
    s16 = out_fmt == AUDIO_S16
    set_format(gpu, fmt)
    m, g, w = M.channel_params(nch)
    _, d_iq = dev_signal("noise", nch, nsamp, fmt, extra)
    outs = []
    for cap in (0, 0, 1, 3):
        assert set_max_wgs(gpu, cap) == 0
        gpu.setChannelDemodulator(m, g, w, out_fmt)
        first = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, gap, s16)
        second = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp + extra, gap, s16)   # the carried state too
        outs.append((np.concatenate([first[0], second[0]], axis=1), np.stack([first[1], second[1]])))
    assert set_max_wgs(gpu, -1) == ERR_ARG
    assert set_max_wgs(gpu, 0) == 0
    np.testing.assert_array_equal(bits(outs[0][0]), bits(cpu_result("noise", nch, nsamp, fmt, out_fmt, tuple(m.tolist()), 2)[0]))
    for y, p in outs[1:]:
        np.testing.assert_array_equal(bits(y), bits(outs[0][0]))
        np.testing.assert_array_equal(bits(p), bits(outs[0][1]))


@pytest.mark.parametrize("out_fmt", OUT_FORMATS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_call_equals_the_device_call_and_shares_its_state(torch_dev, gpu, fmt, out_fmt):
    nch, nsamp, _, _, _ = THREE
    s16 = out_fmt == AUDIO_S16
    set_format(gpu, fmt)
    m, g, w = M.channel_params(nch)
    x = signal("noise", nch, nsamp)
    _, d_iq = dev_signal("noise", nch, nsamp, fmt, 0)
    gpu.setChannelDemodulator(m, g, w, out_fmt)
    runs = [run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp, 0, s16) for _ in range(2)]
    dev = np.concatenate([r[0] for r in runs], axis=1)
    # host then device, device then host: the same stream of two calls (position and last samples)
    gpu.setChannelDemodulator(m, g, w, out_fmt)
    yh, ph = gpu.channel_demodulate(host_iq(x, fmt), power=True)
    hd = np.concatenate([yh, run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp, 0, s16)[0]], axis=1)
    np.testing.assert_array_equal(bits(hd), bits(dev))
    np.testing.assert_array_equal(bits(ph), bits(runs[0][1]))
    gpu.resetChannelDemodulator()
    dh = np.concatenate([run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp, 0, s16)[0],
                         gpu.channel_demodulate(host_iq(x, fmt))], axis=1)
    np.testing.assert_array_equal(bits(dh), bits(dev))
    # a strided host output: nothing between the streams
    gpu.resetChannelDemodulator()
    out = np.full((nch, nsamp + 3), M.S16_POISON, np.int16) if s16 else np.full((nch, nsamp + 3), np.nan, np.float32)
    xs = np.ascontiguousarray(components(x, fmt, 2))
    assert gpu._L.sddc_ddc_channel_demodulate_host(gpu._h, xs.ctypes.data, nch, nsamp, xs.shape[1], out.ctypes.data,
                                                   out.shape[1], None) == 0
    assert (out[:, nsamp:] == M.S16_POISON).all() if s16 else np.isnan(out[:, nsamp:]).all()
    np.testing.assert_array_equal(bits(out[:, :nsamp]), bits(dev[:, :nsamp]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_bfo_sequences_and_the_position_next_to_the_wrap(torch_dev, gpu, fmt):
    """w = 0: y = g I; w = 2^30: g I, -g Q, -g I, g Q exactly, over a tile edge, a call boundary and
    the 2^32 wrap of the position; a general word next to the wrap against the model."""
    nch, nsamp = 2, T + 70
    set_format(gpu, fmt)
    x = signal("noise", nch, nsamp)
    xv = sample_values(x, fmt)
    I, Q = xv.real.astype(np.float32), xv.imag.astype(np.float32)
    _, d_iq = dev_signal("noise", nch, nsamp, fmt, 0)
    g = np.array([1.5, -0.75], np.float32)
    gpu.setChannelDemodulator([DEMOD_BFO] * 2, g, [0, 0])
    np.testing.assert_array_equal(run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp)[0], g[:, None] * I)
    seq = np.stack([I, -Q, -I, Q])
    for pos in (0, 3, 2 ** 32 - 5, 2 ** 32 - T - 18):
        want = g[:, None] * seq[(pos + np.arange(nsamp)) % 4, :, np.arange(nsamp)].T
        gpu.setChannelDemodulator([DEMOD_BFO] * 2, g, [2 ** 30] * 2)
        assert set_position(gpu, pos) == 0
        np.testing.assert_array_equal(run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp)[0], want)
        gpu.setChannelDemodulator([DEMOD_BFO] * 2, g, [2 ** 30] * 2)
        assert set_position(gpu, pos) == 0
        np.testing.assert_array_equal(run_cuts(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp, [9, nsamp - 9], False), want)
    from extio_sddc_amd import bfo_word
    w = [bfo_word(0.1234), bfo_word(-0.31)]
    gpu.setChannelDemodulator([DEMOD_BFO] * 2, g, w)
    assert set_position(gpu, 2 ** 32 - 11) == 0
    y = run_device(torch_dev, gpu, d_iq, nch, nsamp, 2 * nsamp)[0]
    assert M.excess(y, xv, [DEMOD_BFO] * 2, g, w, pos=2 ** 32 - 11) <= 0.0


@pytest.mark.parametrize("fmt", FORMATS)
def test_ddc_decimator_and_demodulator_on_one_buffer_and_stream(torch_dev, fmt):
    """process_channels_device at d = 6 (2 blocks, 3 channels, a tone) -> channel_decimate_device (R = 8,
    65 Kaiser taps) -> channel_demodulate_device in FM, on one stream: within the FM bound of the model
    applied to the decimator output copied back; the IQ and the decimator output bit-identical to a
    run without the demodulator set; the discriminator's mean over the settled part equal to
    g 2 pi (tone offset / channel rate) within the bound plus the tone's own leakage, both taken from
    the float64 model on the same copied-back data."""
    from extio_sddc_amd import R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import make_tone_stream
    torch = torch_dev
    d, nblk, R, tbs = 6, 2, 8, [1000, 1008, 1012]
    tone_bin = 1010.3
    h = kaiser(65, 60.0, 0.04, 0.0625)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    nout = nsamp // R
    gain = np.full(nch, 100.0, np.float32)
    d_in = torch.from_numpy(make_tone_stream(nblk, tone_bin, amp=20000.0)).to("cuda")
    dtype = torch.int16 if fmt == "CS16" else torch.float32

    def chain(r, demod):
        iq = torch.zeros((nch, 2 * nsamp), dtype=dtype, device="cuda")
        nb = torch.zeros((nch, 2 * nout), dtype=torch.float32, device="cuda")
        buf, out, stride = out_tensor(torch, nch, nout, 0, False)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=s)
        r.channel_decimate_device(iq, nch, nsamp, iq.stride(0), nb, nb.stride(0), stream=s)
        if demod:   # the decimator's output is CF32 whatever the DDC wrote: the format is read per call
            r.setOutputFormat("CF32", 1.0)
            r.channel_demodulate_device(nb, nch, nout, nb.stride(0), out, stride, stream=s)
            set_format(r, fmt)
        torch.cuda.synchronize()
        return iq.cpu().numpy(), nb.cpu().numpy(), (collect(buf, nch, nout, 0, False) if demod else None)

    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        set_format(r, fmt)
        r.setChannelDecimator(h, R, nch)
        iq0, nb0, _ = chain(r, False)
        r.setChannelDecimator(h, R, nch)
        r.setChannelDemodulator([DEMOD_FM] * nch, gain)
        iq1, nb1, y = chain(r, True)
    np.testing.assert_array_equal(iq1, iq0)
    np.testing.assert_array_equal(bits(nb1), bits(nb0))
    assert np.abs(nb1).max() > 0
    xv = M.values(np.ascontiguousarray(nb1).view(np.complex64))
    e = M.excess(y, xv, [DEMOD_FM] * nch, gain, [0] * nch)
    print(f"{fmt}: DDC + decimator + FM against the model on the decimator output copied back: |y - y64| - bound <= {e:.3e}")
    assert e <= 0.0
    # the tone sits (tone_bin - tunebin) / 8192 of the ADC rate above each channel's centre; the channel
    # rate after d = 6 and R = 8 is fs / (128 R): offset / rate = (tone_bin - tb) * 128 R / 8192 cycles
    settled = slice(nout // 4, nout)
    y64, _, _ = M.demodulate(xv, [DEMOD_FM] * nch, gain, [0] * nch)
    b = M.bound(xv, [DEMOD_FM] * nch, gain, [0] * nch)
    for c, tb in enumerate(tbs):
        f = (tone_bin - tb) * 128 * R / 8192.0
        f -= np.rint(f)
        want = float(gain[c]) * 2 * np.pi * f
        leak = np.abs(y64[c, settled].mean() - want)          # the model's own mean against the ideal tone
        got = float(y[c, settled].astype(np.float64).mean())
        print(f"  channel {c}: mean {got:.6f}, g 2 pi f {want:.6f}, model leakage {leak:.3e}")
        assert abs(got - want) <= b[c, settled].mean() + leak
        if c == 1:   # the tone lies in this channel's pass band: it dominates, so the reading pins the orientation
            assert leak <= 0.01 * abs(want)


def test_error_returns_and_a_failed_call_changes_no_state(torch_dev, gpu):
    from extio_sddc_amd import DDCError
    torch = torch_dev
    L, hd = gpu._L, gpu._h
    setd, dev = L.sddc_ddc_set_channel_demodulator, L.sddc_ddc_channel_demodulate_device
    nch, nsamp = 3, 40
    m, g, w = M.channel_params(nch)
    mp, gp, wp = m.ctypes.data, g.ctypes.data, w.ctypes.data
    _, d_iq = dev_signal("noise", nch, nsamp, "CF32", 2)
    S = 2 * nsamp + 2
    buf, out, OS = out_tensor(torch, nch, nsamp, 1, False)
    pw = torch.full((nch,), float("nan"), dtype=torch.float32, device="cuda")
    xi, oi, pi = d_iq.data_ptr(), out.data_ptr(), pw.data_ptr()
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None, None) == ERR_STATE               # nothing set
    assert L.sddc_ddc_channel_demodulator_reset(hd) == ERR_STATE
    with pytest.raises(DDCError):
        gpu.channel_demodulate_device(d_iq, nch, nsamp, S, out, OS)
    bad = m.copy()
    bad[0] = 3
    assert setd(hd, bad.ctypes.data, gp, wp, nch, AUDIO_F32) == ERR_ARG
    gb = g.copy()
    gb[1] = np.nan
    assert setd(hd, mp, gb.ctypes.data, wp, nch, AUDIO_F32) == ERR_ARG
    assert setd(hd, mp, gp, wp, 1025, AUDIO_F32) == ERR_ARG
    assert setd(hd, mp, gp, wp, -2, AUDIO_F32) == ERR_ARG
    assert setd(hd, mp, gp, wp, nch, 2) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None, None) == ERR_STATE               # a failed set sets nothing
    gpu.setChannelDemodulator(m, g, w)
    good, good_p = run_device(torch, gpu, d_iq, nch, nsamp, S, 1)
    gpu.setChannelDemodulator(m, g, w)
    assert dev(hd, xi, nch - 1, nsamp, S, oi, OS, pi, None) == ERR_STATE             # another nch than the set one
    assert dev(hd, xi, nch, 0, S, oi, OS, pi, None) == ERR_ARG
    assert dev(hd, xi, nch, 2 ** 40 + 1, 2 ** 42, oi, 2 ** 41, pi, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, 2 * nsamp - 2, oi, OS, pi, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S + 1, oi, OS, pi, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, oi, nsamp - 1, pi, None) == ERR_ARG
    assert dev(hd, xi + 4, nch, nsamp, S, oi, OS, pi, None) == ERR_ARG               # CF32: 8-byte samples
    assert dev(hd, xi, nch, nsamp, S, oi + 2, OS, pi, None) == ERR_ARG               # F32: 4-byte outputs
    assert dev(hd, xi, nch, nsamp, S, oi, OS, pi + 2, None) == ERR_ARG
    assert dev(hd, None, nch, nsamp, S, oi, OS, pi, None) == ERR_ARG
    assert dev(hd, xi, nch, nsamp, S, None, OS, pi, None) == ERR_ARG
    with pytest.raises(DDCError):
        gpu.channel_demodulate_device(d_iq, nch, nsamp, S, out[:OS], OS)                 # d_out too small
    with pytest.raises(DDCError):
        gpu.channel_demodulate_device(d_iq, nch + 1, nsamp, S, out, OS)                  # d_iq too small
    with pytest.raises(DDCError):
        gpu.channel_demodulate_device(d_iq.to(torch.int16), nch, nsamp, S, out, OS)      # wrong input dtype
    with pytest.raises(DDCError):
        gpu.channel_demodulate_device(d_iq, nch, nsamp, S, out.to(torch.int16), OS)      # wrong output dtype
    with pytest.raises(DDCError):
        gpu.channel_demodulate_device(d_iq, nch, nsamp, S, out, OS, pw[:nch - 1])        # d_power too small
    torch.cuda.synchronize()
    assert torch.isnan(buf).all() and torch.isnan(pw).all()
    # the failed calls changed no state: the next valid call is the first call of the stream
    y, p = run_device(torch, gpu, d_iq, nch, nsamp, S, 1)
    np.testing.assert_array_equal(bits(y), bits(good))
    np.testing.assert_array_equal(bits(p), bits(good_p))
    gpu.setChannelDemodulator(None)
    assert dev(hd, xi, nch, nsamp, S, oi, OS, None, None) == ERR_STATE
