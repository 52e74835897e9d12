"""The channel noise blanker on the GPU (pytest -m gpu): sddc_ddc_channel_blank_device and
sddc_ddc_channel_blank_host of a GPU handle bit for bit against the CPU backend (which
tests/test_channel_blanker_cpu.py pins to the definition), outputs and counts, the bit-exact properties of
the kernels (cuts, streams, grids, run length, a channel alone), and the DDC, this stage and the channel
decimator on one stream.

Shapes (nch, nsamp), B = the block length (BLANKER_BLOCK):
  (1, 1)            one sample: no full block
  (1, B)            exactly one block
  (1, 3B + 17)      full blocks and a tail
  (3, 2B + 3)       one bypassed channel; input and output gaps poisoned
  (1024, 2)         every channel, almost no samples each
  (1, 66B + 5)      more blocks than a default run has
  (2, 258B + 1)     several runs per channel
Every d_iq starts OFFSET samples into a poisoned tensor (NaN, CS16: 0x7fff) and every d_out HEAD samples
into one; the heads, the tails and the gaps between the streams must stay untouched.  The model's
impulses lie on block boundaries that are also boundaries of runs of 1, 2 and 3 blocks.  Every test runs
under a watchdog that ends the process if a GPU step hangs.
"""
from __future__ import annotations

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


M = _load("channel_blanker_model")

from extio_sddc_amd import BLANKER_BLOCK as B  # noqa: E402
from extio_sddc_amd import BLANKER_MEAN, BLANKER_MEDIAN, blanker_threshold  # noqa: E402
from extio_sddc_amd.r2iq import FMT_CF32, FMT_CS16  # noqa: E402

PARAM_CHNB_MAX_WGS, PARAM_CHNB_RUN_BLOCKS = 21, 22   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
HEAD, OFFSET = 1, 3        # samples before d_out / d_iq in their poisoned tensors
S16_POISON = 0x7fff
SHAPES = [(1, 1), (1, B), (1, 3 * B + 17), (3, 2 * B + 3), (1024, 2), (1, 66 * B + 5), (2, 258 * B + 1)]
THREE = SHAPES[3]
CONFIGS = [(0, 1), (5, 3), (64, 16), (8, 8)]   # (g, M)
MODES = [BLANKER_MEAN, BLANKER_MEDIAN]
FORMATS = [FMT_CF32, FMT_CS16]
NAN_PAYLOAD = 0x7FC12345


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


def poison(fmt):
    return S16_POISON if fmt == FMT_CS16 else np.nan


def params(nch, fmt=FMT_CF32):
    return M.make_params(nch, qmin=1e-6 if fmt == FMT_CF32 else 1.0)


@functools.lru_cache(maxsize=None)
def signal(nch, nsamp, g, fmt):
    """make_input's streams as components [nch, 2 nsamp]; in CF32 the bypassed channel carries a NaN payload."""
    x, _ = M.make_input(nch, nsamp, g)
    if fmt == FMT_CS16:
        c = M.to_cs16(x).reshape(nch, 2 * nsamp)
    else:
        c = np.ascontiguousarray(x).view(np.float32).reshape(nch, 2 * nsamp).copy()
        if nch > 1 and nsamp > 1:
            c.view(np.uint32)[1, 2 * (nsamp // 3)] = NAN_PAYLOAD
    c.setflags(write=False)
    return c


def host_form(c, fmt):
    """components [nch, 2 n] as channel_blank takes them"""
    nch, n2 = c.shape
    return c.reshape(nch, n2 // 2, 2) if fmt == FMT_CS16 else np.ascontiguousarray(c).view(np.complex64)


def comps(y, fmt):
    y = np.ascontiguousarray(y)
    return y.reshape(y.shape[0], -1) if fmt == FMT_CS16 else y.view(np.float32).reshape(y.shape[0], -1)


@functools.lru_cache(maxsize=None)
def dev_signal(nch, nsamp, g, fmt, gap):
    """(the device tensor, d_iq OFFSET samples into it, in_stride): poison before, between and after."""
    import torch
    c = signal(nch, nsamp, g, fmt)
    body = np.full((nch, 2 * (nsamp + gap)), poison(fmt), c.dtype)
    body[:, :2 * nsamp] = c
    pad = np.full(2 * OFFSET, poison(fmt), c.dtype)
    buf = torch.from_numpy(np.concatenate([pad, body.reshape(-1), pad])).to("cuda")
    return buf, buf[2 * OFFSET:], 2 * (nsamp + gap)


def out_tensor(torch, nch, nsamp, gap, fmt):
    """(the poisoned tensor, d_out HEAD samples into it, out_stride)."""
    stride = 2 * (nsamp + gap)
    if fmt == FMT_CS16:
        buf = torch.full((2 * HEAD + nch * stride + 64,), S16_POISON, dtype=torch.int16, device="cuda")
    else:
        buf = torch.full((2 * HEAD + nch * stride + 64,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[2 * HEAD:], stride


def count_tensor(torch, nch):
    buf = torch.full((nch + 2,), -1, dtype=torch.int32, device="cuda")
    return buf, buf[1:]


def collect(buf, nch, nsamp, gap, fmt):
    """components [nch, 2 nsamp] of a finished call; the head, the tail and the gaps must still hold the
    poison (no output is 0x7fff: the codes stay below 30001)."""
    stride = 2 * (nsamp + gap)
    y = buf.cpu().numpy()
    clean = (lambda v: (v == S16_POISON).all()) if fmt == FMT_CS16 else (lambda v: np.isnan(v).all())
    body = y[2 * HEAD:2 * HEAD + nch * stride].reshape(nch, stride)
    assert clean(y[:2 * HEAD]) and clean(y[2 * HEAD + nch * stride:]) and clean(body[:, 2 * nsamp:])
    return np.ascontiguousarray(body[:, :2 * nsamp])


def collect_count(cbuf, nch):
    c = cbuf.cpu().numpy()
    assert c[0] == -1 and c[nch + 1] == -1
    return np.ascontiguousarray(c[1:nch + 1]).view(np.uint32)


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run_cuts(torch, r, d_iq, nch, nsamp, in_stride, cuts, fmt, gap=0, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of d_iq it covers; nothing synchronises
    between the calls.  Returns the outputs [nch, 2 nsamp] and the counts of every call."""
    assert sum(cuts) == nsamp and min(cuts) > 0
    at = 0
    outs = [out_tensor(torch, nch, n, gap, fmt) for n in cuts]
    cnts = [count_tensor(torch, nch) for _ in cuts]
    torch.cuda.synchronize()   # the poison fills are done before a call on another stream writes
    for k, n in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        r.channel_blank_device(d_iq[2 * at:], nch, n, in_stride, outs[k][1], outs[k][2], d_count=cnts[k][1], stream=s)
        at += n
    torch.cuda.synchronize()
    y = np.concatenate([collect(o[0], nch, n, gap, fmt) for o, n in zip(outs, cuts)], axis=1)
    return y, [collect_count(c[0], nch) for c in cnts]


@functools.lru_cache(maxsize=None)
def cpu_result(nch, nsamp, g, m, mode, fmt, cuts=None):
    """The CPU backend's outputs [nch, 2 nsamp] and per-call counts of the stream cut into `cuts`."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    x = host_form(signal(nch, nsamp, g, fmt), fmt)
    p = params(nch, fmt)
    ys, cs, at = [], [], 0
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelBlanker(p, g, m, mode, fmt)
        for n in (cuts or (nsamp,)):
            y, cnt = c.channel_blank(x[:, at:at + n], count=True)
            ys.append(comps(y, fmt))
            cs.append(cnt)
            at += n
    y = np.concatenate(ys, axis=1)
    y.setflags(write=False)
    return y, cs


def set_param(r, param, value):
    return r._L.sddc_ddc_internal_set_param(r._h, param, value)


def same(y, cs, ref, what=None):
    np.testing.assert_array_equal(bits(y), bits(ref[0]), err_msg=str(what))
    assert len(cs) == len(ref[1])
    for a, b in zip(cs, ref[1]):
        np.testing.assert_array_equal(a, b, err_msg=str(what))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_equals_the_cpu_backend(torch_dev, gpu, shape, mode, fmt):
    nch, nsamp = shape
    gap = 1 if nch > 1 else 0
    blanked = 0
    for g, m in CONFIGS:
        ref = cpu_result(nch, nsamp, g, m, mode, fmt)
        _, d_iq, stride = dev_signal(nch, nsamp, g, fmt, gap)
        gpu.setChannelBlanker(params(nch, fmt), g, m, mode, fmt)
        y, cs = run_cuts(torch_dev, gpu, d_iq, nch, nsamp, stride, [nsamp], fmt, gap=gap)
        same(y, cs, ref, ("device", g, m))
        gpu.resetChannelBlanker()
        yh, ch = gpu.channel_blank(host_form(signal(nch, nsamp, g, fmt), fmt), count=True)
        same(comps(yh, fmt), [ch], ref, ("host", g, m))
        blanked += int(cs[0].sum())
    if nsamp > B + 1:
        assert blanked > 0


CUTS = {"edges": lambda n, g: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n, g: [100, B, n - B - 100],
        "short-first": lambda n, g: [max(1, g - 2), 7, n - 7 - max(1, g - 2)]}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_cuts_are_bit_identical(torch_dev, gpu, cut, fmt):
    for (nch, nsamp), (g, m), mode in ((THREE, (5, 3), BLANKER_MEAN), (SHAPES[5], (64, 16), BLANKER_MEDIAN),
                                       (SHAPES[2], (8, 8), BLANKER_MEAN)):
        cuts = tuple(CUTS[cut](nsamp, g))
        ref = cpu_result(nch, nsamp, g, m, mode, fmt, cuts)
        same(ref[0], [], (cpu_result(nch, nsamp, g, m, mode, fmt)[0], []))   # the CPU backend's own cut invariance
        _, d_iq, stride = dev_signal(nch, nsamp, g, fmt, 0)
        gpu.setChannelBlanker(params(nch, fmt), g, m, mode, fmt)
        y, cs = run_cuts(torch_dev, gpu, d_iq, nch, nsamp, stride, list(cuts), fmt)
        same(y, cs, ref, (nch, nsamp, g, m))


@pytest.mark.parametrize("shape", [THREE, SHAPES[5]], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_identical_for_any_grid_and_run_length(torch_dev, gpu, shape):
    nch, nsamp = shape
    k = 0
    for cap in (1, 3, 0):
        for run in (1, 2, 3, 0):
            g, m = CONFIGS[1 + k % 3]
            mode, fmt = MODES[k % 2], FORMATS[(k // 2) % 2]
            k += 1
            assert set_param(gpu, PARAM_CHNB_MAX_WGS, cap) == 0 and set_param(gpu, PARAM_CHNB_RUN_BLOCKS, run) == 0
            cuts = (100, nsamp - 100)   # the second call starts inside a block, from the carried state
            ref = cpu_result(nch, nsamp, g, m, mode, fmt, cuts)
            _, d_iq, stride = dev_signal(nch, nsamp, g, fmt, 0)
            gpu.setChannelBlanker(params(nch, fmt), g, m, mode, fmt)
            y, cs = run_cuts(torch_dev, gpu, d_iq, nch, nsamp, stride, list(cuts), fmt)
            same(y, cs, ref, (cap, run, g, m, mode, fmt))
    assert set_param(gpu, PARAM_CHNB_MAX_WGS, -1) == ERR_ARG and set_param(gpu, PARAM_CHNB_RUN_BLOCKS, -1) == ERR_ARG


def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu):
    nch, nsamp = THREE
    g, m, mode, fmt = 5, 3, BLANKER_MEDIAN, FMT_CF32
    among = cpu_result(nch, nsamp, g, m, mode, fmt)
    _, d_iq, stride = dev_signal(nch, nsamp, g, fmt, 0)
    for c in range(nch):
        gpu.setChannelBlanker(params(nch, fmt)[c:c + 1], g, m, mode, fmt)
        y, cs = run_cuts(torch_dev, gpu, d_iq[c * stride:], 1, nsamp, stride, [nsamp], fmt)
        np.testing.assert_array_equal(bits(y[0]), bits(among[0][c]))
        assert cs[0][0] == among[1][0][c]


def test_a_side_stream_equals_the_default_stream(torch_dev, gpu):
    torch = torch_dev
    nch, nsamp = SHAPES[6]
    g, m, mode, fmt = 8, 8, BLANKER_MEAN, FMT_CF32
    ref = cpu_result(nch, nsamp, g, m, mode, fmt)
    _, d_iq, stride = dev_signal(nch, nsamp, g, fmt, 0)
    gpu.setChannelBlanker(params(nch, fmt), g, m, mode, fmt)
    same(*run_cuts(torch, gpu, d_iq, nch, nsamp, stride, [nsamp], fmt), ref)
    gpu.resetChannelBlanker()
    same(*run_cuts(torch, gpu, d_iq, nch, nsamp, stride, [nsamp], fmt, streams=[torch.cuda.Stream()]), ref)
    # calls of one stream of samples on alternating streams run in call order
    cuts = (300, 1000, nsamp - 1300)
    gpu.resetChannelBlanker()
    y, cs = run_cuts(torch, gpu, d_iq, nch, nsamp, stride, list(cuts), fmt, streams=[torch.cuda.Stream(), torch.cuda.Stream()])
    same(y, cs, cpu_result(nch, nsamp, g, m, mode, fmt, cuts))


def test_reset_and_failed_calls(torch_dev, gpu):
    torch = torch_dev
    nch, nsamp = THREE
    g, m, mode, fmt = 5, 3, BLANKER_MEAN, FMT_CF32
    ref = cpu_result(nch, nsamp, g, m, mode, fmt)
    _, d_iq, stride = dev_signal(nch, nsamp, g, fmt, 0)
    f = gpu._L.sddc_ddc_channel_blank_device
    buf, out, ostride = out_tensor(torch, nch, nsamp, 0, fmt)
    assert f(gpu._h, d_iq.data_ptr(), nch, nsamp, stride, out.data_ptr(), ostride, None, None) == ERR_STATE   # nothing set
    gpu.setChannelBlanker(params(nch, fmt), g, m, mode, fmt)
    y1, _ = run_cuts(torch, gpu, d_iq, nch, 300, stride, [300], fmt)
    # failed calls: they write nothing and change no state
    assert f(gpu._h, d_iq.data_ptr(), 2, nsamp, stride, out.data_ptr(), ostride, None, None) == ERR_STATE
    assert f(gpu._h, d_iq.data_ptr(), nch, 0, stride, out.data_ptr(), ostride, None, None) == ERR_ARG
    assert f(gpu._h, d_iq.data_ptr(), nch, nsamp, stride - 2, out.data_ptr(), ostride, None, None) == ERR_ARG
    assert f(gpu._h, d_iq.data_ptr(), nch, nsamp, stride, out.data_ptr(), ostride + 1, None, None) == ERR_ARG
    assert f(gpu._h, d_iq.data_ptr() + 4, nch, nsamp - 1, stride, out.data_ptr(), ostride, None, None) == ERR_ARG
    assert f(gpu._h, d_iq.data_ptr(), nch, nsamp, stride, d_iq.data_ptr(), stride, None, None) == ERR_ARG    # in place
    torch.cuda.synchronize()
    assert np.isnan(buf.cpu().numpy()).all()
    y2, _ = run_cuts(torch, gpu, d_iq[2 * 300:], nch, nsamp - 300, stride, [nsamp - 300], fmt)
    np.testing.assert_array_equal(bits(np.concatenate([y1, y2], axis=1)), bits(ref[0]))
    gpu.resetChannelBlanker()   # a new stream
    same(*run_cuts(torch, gpu, d_iq, nch, nsamp, stride, [nsamp], fmt), ref)
    gpu.setChannelBlanker(None, 0, 0)
    assert f(gpu._h, d_iq.data_ptr(), nch, nsamp, stride, out.data_ptr(), ostride, None, None) == ERR_STATE


@functools.lru_cache(maxsize=None)
def chain_results():
    """process_channels_device at d = 6 (6 blocks, 3 channels; a weak noisy tone and four two-sample
    impulses in the ADC stream) -> channel_blank_device (10 dB over the mean of 4 blocks, g = 4) ->
    channel_decimate_device (R = 8, 65 taps), on one stream, with the blanker on and with every channel
    bypassed (the same delay); and the blanker and the decimator of a CPU handle fed the DDC's output."""
    import torch
    from extio_sddc_amd import DEVICE_CPU, R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import HALF_FFT, make_tone_stream
    d, nblk, R, tbs = 6, 6, 8, [1000, 1008, 1012]
    g, m = 4, 4
    h = kaiser(65, 60.0, 0.04, 0.0625)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    nout = nsamp // R
    adc = make_tone_stream(nblk, 1010.3, amp=20.0, noise=10.0).copy()
    where = [HALF_FFT + 65536 + 20000 + k * 70001 for k in range(4)]
    for p in where:
        adc[p], adc[p + 1] = 32000, -32000
    d_in = torch.from_numpy(adc).to("cuda")
    on = np.tile(np.float32([blanker_threshold(10.0), 0.0]), (nch, 1))
    off = np.zeros((nch, 2), np.float32)

    def chain(r, p):
        r.setChannelBlanker(p, g, m)
        r.setChannelDecimator(h, R, nch)
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device="cuda")
        bl = torch.zeros((nch, 2 * nsamp + 2), dtype=torch.float32, device="cuda")
        nb = torch.zeros((nch, 2 * nout), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(nch, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=s)
        r.channel_blank_device(iq, nch, nsamp, iq.stride(0), bl, bl.stride(0), d_count=cnt, stream=s)
        r.channel_decimate_device(bl, nch, nsamp, bl.stride(0), nb, nb.stride(0), stream=s)
        torch.cuda.synchronize()
        return iq.cpu().numpy(), bl.cpu().numpy()[:, :2 * nsamp], nb.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)

    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        with_blanker = chain(r, on)
        bypassed = chain(r, off)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelBlanker(on, g, m)
        c.setChannelDecimator(h, R, nch)
        yb, cc = c.channel_blank(np.ascontiguousarray(with_blanker[0]).view(np.complex64), count=True)
        cpu = (comps(yb, FMT_CF32), comps(c.channel_decimate(yb), FMT_CF32), cc)
    # the spans of the decimated stream that an impulse's ringing reaches
    ring = np.zeros(nout, bool)
    for p in where:
        i = (p - HALF_FFT) >> 7   # the DDC's output sample, within its filter delay
        ring[max(0, (i - 8) // R):(i + 24 + g + 65) // R + 2] = True
    return with_blanker, bypassed, cpu, ring, h, R


def test_ddc_blanker_and_decimator_on_one_stream(torch_dev):
    """The chain of chain_results: the DDC's output does not depend on the blanker; the blanker's output
    and counts on the device are the CPU backend's bit for bit; the decimator's output is within its own
    float64 bound (tools/channel_decimate_model.py) of the model applied to the blanked stream; the
    decimated power inside the impulses' ringing spans is lower with the blanker than without."""
    D = _load("channel_decimate_model")
    (iq, bl, nb, cnt), (iq0, bl0, nb0, cnt0), (cpu_bl, cpu_nb, cpu_cnt), ring, h, R = chain_results()
    nch = iq.shape[0]
    np.testing.assert_array_equal(bits(iq), bits(iq0))
    assert (cnt0 == 0).all() and (cnt > 0).all()
    np.testing.assert_array_equal(bits(bl0[:, 8:]), bits(iq[:, :-8]))      # bypassed: the input delayed by g = 4
    np.testing.assert_array_equal(bits(bl), bits(cpu_bl))
    np.testing.assert_array_equal(cnt, cpu_cnt)
    z, z0 = np.ascontiguousarray(nb).view(np.complex64), np.ascontiguousarray(nb0).view(np.complex64)
    e = D.excess(z, D.values(np.ascontiguousarray(bl).view(np.complex64)), h, R)
    print(f"decimator on the blanked stream against its model: |y - y64| - bound <= {e:.3e}")
    assert e <= 0.0
    pw = lambda a: float(np.mean(np.abs(a.astype(np.complex128)) ** 2))  # noqa: E731
    for ch in range(nch):
        print(f"channel {ch}: ringing-span power {pw(z[ch, ring]):.4g} with the blanker, {pw(z0[ch, ring]):.4g} without; "
              f"elsewhere {pw(z[ch, ~ring]):.4g} / {pw(z0[ch, ~ring]):.4g}; {cnt[ch]} outputs blanked")
        assert pw(z[ch, ring]) < pw(z0[ch, ring])


def test_chain_decimated_output_equals_the_cpu_chain_bit_for_bit(torch_dev):
    """The decimated output of the chain on the device is bit-identical to the decimator of a CPU handle fed
    the CPU blanker's output: the blanker's two backends agree bit for bit (the test above), and the CPU
    backend's decimator adds its taps in the device kernel's order (k = q R + r: fma into sum q mod 4, phase
    by phase, then (a0 + a1) + (a2 + a3))."""
    (_, _, nb, _), _, (_, cpu_nb, _), _, _, _ = chain_results()
    differ = int((bits(nb) != bits(cpu_nb)).sum())
    print(f"decimated output, device chain against CPU chain: {differ} of {nb.size} words differ")
    assert np.abs(nb).max() > 0
    np.testing.assert_array_equal(bits(nb), bits(cpu_nb))
