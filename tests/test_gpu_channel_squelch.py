"""The channel squelch on the GPU (pytest -m gpu): sddc_ddc_channel_squelch_device and
sddc_ddc_channel_squelch_host of a GPU handle bit for bit against the CPU backend (which
tests/test_channel_squelch_cpu.py pins to the definition), outputs and the three side outputs, the bit-exact
properties of the kernels (cuts, streams, grids, run length, a channel alone), and the DDC, the decimator, the
demodulator and this stage on one stream.

Shapes (nch, nsamp), B = the block length (SQUELCH_BLOCK):
  (1, 1)            one sample: no full block
  (1, B)            exactly one block
  (1, 3B + 17)      full blocks and a tail
  (3, 2B + 3)       LEVEL, NOISE and OFF in one call
  (1024, 2)         every channel (all four modes), almost no samples each
  (1, 66B + 5)      more blocks than the gates kernel's 64-block step
  (2, 258B + 1)     several steps, and several launch sets when the run length is small
Two layouts: ALIGNED puts every stream on a 16-byte boundary with strides that are multiples of four samples
(the outputs kernel's four-samples-per-lane path), SHIFTED starts the inputs three samples and the outputs one
sample into their tensors with odd gaps (its sample-per-lane path).  Every buffer lies in a poisoned tensor
(NaN, int16: 0x7fff); the heads, the tails and the gaps between the streams must stay untouched.  Every test
runs under a watchdog that ends the process if a GPU step hangs.
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


M = _load("channel_squelch_model")

from extio_sddc_amd import SQUELCH_BLOCK as B  # noqa: E402
from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, DEMOD_FM, SQUELCH_LEVEL, SQUELCH_OFF, SQUELCH_SENSE_CF32,  # noqa: E402
                            SQUELCH_SENSE_CS16, SQUELCH_SENSE_F32, SQUELCH_SENSE_S16, SQUELCH_SENSE_SELF)

PARAM_CHSQ_MAX_WGS, PARAM_CHSQ_RUN_BLOCKS = 23, 24   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
S16_POISON = 0x7fff
SHAPES = [(1, 1), (1, B), (1, 3 * B + 17), (3, 2 * B + 3), (1024, 2), (1, 66 * B + 5), (2, 258 * B + 1)]
THREE, SIXTYSIX = SHAPES[3], SHAPES[5]
CONFIGS = [(1, 0, 0), (3, 2, 1), (16, 70, 1), (1, 65535, 0)]   # (A, H, fade)
SELF, F32, S16, CF32, CS16 = (SQUELCH_SENSE_SELF, SQUELCH_SENSE_F32, SQUELCH_SENSE_S16, SQUELCH_SENSE_CF32,
                              SQUELCH_SENSE_CS16)
# (sense kind, audio in, audio out): every pair of values of two of the three occurs
COMBOS = [(SELF, AUDIO_F32, AUDIO_F32), (SELF, AUDIO_S16, AUDIO_S16), (F32, AUDIO_F32, AUDIO_S16), (F32, AUDIO_S16, AUDIO_F32),
          (S16, AUDIO_F32, AUDIO_F32), (S16, AUDIO_S16, AUDIO_S16), (CF32, AUDIO_F32, AUDIO_S16), (CF32, AUDIO_S16, AUDIO_F32),
          (CS16, AUDIO_F32, AUDIO_F32), (CS16, AUDIO_S16, AUDIO_S16)]
ALIGNED, SHIFTED = 0, 1


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
def case(nch, n, A, H, kind, in16):
    """(audio [nch, n], sense as components [nch, per * n] or None, modes, thresholds, per)."""
    audio, sense, modes, thr = M.make_case(nch, n, A, H, kind, in16)
    per = 2 if kind in (CF32, CS16) else 1
    if sense is not None:
        sense = np.ascontiguousarray(sense)
        sense = (sense.view(np.float32) if sense.dtype == np.complex64 else sense).reshape(nch, per * n)
    for a in (audio, sense, modes, thr):
        if a is not None:
            a.setflags(write=False)
    return audio, sense, modes, thr, per


def host_sense(sense, kind):
    """components [nch, per * n] as channel_squelch takes the sense stream"""
    if sense is None:
        return None
    if kind == CF32:
        return np.ascontiguousarray(sense).view(np.complex64)
    return sense.reshape(sense.shape[0], -1, 2) if kind == CS16 else sense


def stride_of(n, layout):
    """samples (or complex samples) from a channel's stream to the next one's"""
    return (n + 3) // 4 * 4 if layout == ALIGNED else n + 1 + (n % 2)


def to_dev(torch, a, per, n, layout):
    """a [nch, per * n] in a poisoned tensor: (the tensor, the view at the first stream, the stride in
    components)."""
    nch = a.shape[0]
    poison = S16_POISON if a.dtype == np.int16 else np.nan
    stride = per * stride_of(n, layout)
    off = 0 if layout == ALIGNED else 3 * per
    buf = np.full(off + nch * stride + 8, poison, a.dtype)
    buf[off:off + nch * stride].reshape(nch, stride)[:, :per * n] = a
    t = torch.from_numpy(buf).to("cuda")
    return t, t[off:], stride


def out_tensor(torch, nch, n, layout, out16):
    stride = stride_of(n, layout)
    head = 0 if layout == ALIGNED else 1
    if out16:
        buf = torch.full((head + nch * stride + 8,), S16_POISON, dtype=torch.int16, device="cuda")
    else:
        buf = torch.full((head + nch * stride + 8,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[head:], stride, head


def collect(o, nch, n):
    """[nch, n] of a finished call; the head, the tail and the gaps must still hold the poison."""
    buf, _, stride, head = o
    y = buf.cpu().numpy()
    clean = (lambda v: (v == S16_POISON).all()) if y.dtype == np.int16 else (lambda v: np.isnan(v).all())
    body = y[head:head + nch * stride].reshape(nch, stride)
    assert clean(y[:head]) and clean(y[head + nch * stride:]) and clean(body[:, n:])
    return np.ascontiguousarray(body[:, :n])


def side_tensors(torch, nch):
    o = torch.full((nch + 2,), -1, dtype=torch.int32, device="cuda")
    c = torch.full((nch + 2,), -1, dtype=torch.int32, device="cuda")
    lv = torch.full((nch + 2,), float("nan"), dtype=torch.float32, device="cuda")
    return o, c, lv


def collect_sides(s, nch):
    o, c, lv = (t.cpu().numpy() for t in s)
    assert o[0] == -1 and o[nch + 1] == -1 and c[0] == -1 and c[nch + 1] == -1
    assert np.isnan(lv[0]) and np.isnan(lv[nch + 1])
    return o[1:nch + 1].view(np.uint32).copy(), c[1:nch + 1].view(np.uint32).copy(), lv[1:nch + 1].copy()


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run_cuts(torch, r, audio, sense, per, nch, n, cuts, out16, layout=ALIGNED, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of the inputs it covers; nothing synchronises
    between the calls.  Returns the outputs [nch, n] and the side outputs of every call."""
    assert sum(cuts) == n and min(cuts) > 0
    _, d_a, a_stride = to_dev(torch, audio, 1, n, layout)
    d_s, s_stride = None, 0
    if sense is not None:
        _, d_s, s_stride = to_dev(torch, sense, per, n, layout)
    outs = [out_tensor(torch, nch, k, layout, out16) for k in cuts]
    sides = [side_tensors(torch, nch) for _ in cuts]
    torch.cuda.synchronize()   # the uploads and poison fills are done before a call on another stream runs
    at = 0
    for k, ln in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        r.channel_squelch_device(d_a[at:], None if d_s is None else d_s[per * at:], nch, ln, a_stride, s_stride, outs[k][1],
                                 outs[k][2], d_open=sides[k][0][1:], d_count=sides[k][1][1:], d_level=sides[k][2][1:], stream=s)
        at += ln
    torch.cuda.synchronize()
    y = np.concatenate([collect(o, nch, ln) for o, ln in zip(outs, cuts)], axis=1)
    return y, [collect_sides(s, nch) for s in sides]


@functools.lru_cache(maxsize=None)
def cpu_result(nch, n, A, H, fade, kind, fin, fout, cuts=None):
    """The CPU backend's outputs [nch, n] and per-call side outputs of the stream cut into `cuts`."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    audio, sense, modes, thr, _ = case(nch, n, A, H, kind, fin == AUDIO_S16)
    hs = host_sense(sense, kind)
    ys, sides, at = [], [], 0
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelSquelch(modes, thr, A, H, fade, kind, fin, fout)
        for ln in (cuts or (n,)):
            y, o, cnt, lv = c.channel_squelch(audio[:, at:at + ln], None if hs is None else hs[:, at:at + ln], open=True,
                                              count=True, level=True)
            ys.append(y)
            sides.append((o, cnt, lv))
            at += ln
    y = np.concatenate(ys, axis=1)
    y.setflags(write=False)
    return y, sides


def set_param(r, param, value):
    return r._L.sddc_ddc_internal_set_param(r._h, param, value)


def same(y, sides, ref, what=None):
    assert y.dtype == ref[0].dtype
    np.testing.assert_array_equal(bits(y), bits(ref[0]), err_msg=str(what))
    assert len(sides) == len(ref[1])
    for a, b in zip(sides, ref[1]):
        for got, want, name in zip(a, b, ("open", "count", "level")):
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{name} {what}")


def setup(r, nch, n, A, H, fade, kind, fin, fout):
    audio, sense, modes, thr, per = case(nch, n, A, H, kind, fin == AUDIO_S16)
    r.setChannelSquelch(modes, thr, A, H, fade, kind, fin, fout)
    return audio, sense, per


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_equals_the_cpu_backend(torch_dev, gpu, shape):
    nch, n = shape
    opened = 0
    for ci, (A, H, fade) in enumerate(CONFIGS):
        for ki, (kind, fin, fout) in enumerate(COMBOS):
            ref = cpu_result(nch, n, A, H, fade, kind, fin, fout)
            audio, sense, per = setup(gpu, nch, n, A, H, fade, kind, fin, fout)
            layout = (ci + ki) % 2
            y, sides = run_cuts(torch_dev, gpu, audio, sense, per, nch, n, [n], fout == AUDIO_S16, layout)
            same(y, sides, ref, ("device", A, H, fade, kind, fin, fout, layout))
            if ki % 3 == ci % 3:   # the host entry on a third of them
                gpu.resetChannelSquelch()
                yh, o, c, lv = gpu.channel_squelch(audio, host_sense(sense, kind), open=True, count=True, level=True)
                same(yh, [(o, c, lv)], ref, ("host", A, H, fade, kind, fin, fout))
            opened += int(sides[0][1][:2].sum()) if nch > 1 else int(sides[0][1].sum())
    if n >= 66 * B:
        assert opened > 0


# k: the first block whose gate differs from the block before it (2 where no gate moves)
CUTS = {"edges": lambda n, k: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n, k: [100, B, n - B - 100],
        "samples": lambda n, k: [k * B - 2, 1, 1, 1, 1, n - k * B - 2]}


def first_transition(nch, n, A, H, fade, kind, fin):
    audio, sense, modes, thr, _ = case(nch, n, A, H, kind, fin == AUDIO_S16)
    g = M.definition(audio, host_sense(sense, kind), kind, modes, thr, A, H, fade)["G"]
    moved = np.flatnonzero((np.diff(g.astype(np.int8), axis=1) != 0).any(axis=0))
    return int(moved[0]) + 1 if len(moved) and (int(moved[0]) + 1) * B + 2 < n else 2


@pytest.mark.parametrize("layout", [ALIGNED, SHIFTED])
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_cuts_are_bit_identical(torch_dev, gpu, cut, layout):
    k = 0
    for nch, n in (THREE, SIXTYSIX):
        for A, H, fade in CONFIGS[:3]:
            kind, fin, fout = COMBOS[(3 * k + layout) % len(COMBOS)]
            k += 1
            cuts = tuple(CUTS[cut](n, first_transition(nch, n, A, H, fade, kind, fin)))
            ref = cpu_result(nch, n, A, H, fade, kind, fin, fout, cuts)
            whole = cpu_result(nch, n, A, H, fade, kind, fin, fout)
            np.testing.assert_array_equal(bits(ref[0]), bits(whole[0]))   # the CPU backend's own cut invariance
            assert sum(int(s[1].sum()) for s in ref[1]) == int(whole[1][0][1].sum())   # the counts add up
            audio, sense, per = setup(gpu, nch, n, A, H, fade, kind, fin, fout)
            y, sides = run_cuts(torch_dev, gpu, audio, sense, per, nch, n, list(cuts), fout == AUDIO_S16, layout)
            same(y, sides, ref, (nch, n, A, H, fade, kind, fin, fout))


@pytest.mark.parametrize("shape", [THREE, SIXTYSIX, SHAPES[6]], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_identical_for_any_grid_and_run_length(torch_dev, gpu, shape):
    nch, n = shape
    k = 0
    for cap in (1, 3, 0):
        for run in (1, 2, 3, 0):
            A, H, fade = CONFIGS[k % 3]
            kind, fin, fout = COMBOS[(k * 3) % len(COMBOS)]
            k += 1
            assert set_param(gpu, PARAM_CHSQ_MAX_WGS, cap) == 0 and set_param(gpu, PARAM_CHSQ_RUN_BLOCKS, run) == 0
            cuts = (100, n - 100)   # the second call starts inside a block, from the carried state
            ref = cpu_result(nch, n, A, H, fade, kind, fin, fout, cuts)
            audio, sense, per = setup(gpu, nch, n, A, H, fade, kind, fin, fout)
            y, sides = run_cuts(torch_dev, gpu, audio, sense, per, nch, n, list(cuts), fout == AUDIO_S16, k % 2)
            same(y, sides, ref, (cap, run, A, H, fade, kind, fin, fout))
    assert set_param(gpu, PARAM_CHSQ_MAX_WGS, -1) == ERR_ARG and set_param(gpu, PARAM_CHSQ_RUN_BLOCKS, -1) == ERR_ARG
    assert set_param(gpu, PARAM_CHSQ_RUN_BLOCKS, (1 << 20) + 1) == ERR_ARG


def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu):
    nch, n = 3, 30 * B + 3
    A, H, fade, kind, fin, fout = 3, 2, 1, CF32, AUDIO_F32, AUDIO_F32
    among = cpu_result(nch, n, A, H, fade, kind, fin, fout)
    audio, sense, modes, thr, per = case(nch, n, A, H, kind, False)
    for c in range(nch):
        gpu.setChannelSquelch(modes[c:c + 1], thr[c:c + 1], A, H, fade, kind, fin, fout)
        y, sides = run_cuts(torch_dev, gpu, audio[c:c + 1], sense[c:c + 1], per, 1, n, [n], False)
        np.testing.assert_array_equal(bits(y[0]), bits(among[0][c]))
        for got, want in zip(sides[0], among[1][0]):
            assert bits(got)[0] == bits(want)[c]


def test_a_side_stream_equals_the_default_stream(torch_dev, gpu):
    torch = torch_dev
    nch, n = SHAPES[6]
    A, H, fade, kind, fin, fout = 3, 2, 1, SELF, AUDIO_F32, AUDIO_F32
    ref = cpu_result(nch, n, A, H, fade, kind, fin, fout)
    audio, sense, per = setup(gpu, nch, n, A, H, fade, kind, fin, fout)
    same(*run_cuts(torch, gpu, audio, sense, per, nch, n, [n], False), ref)
    gpu.resetChannelSquelch()
    same(*run_cuts(torch, gpu, audio, sense, per, nch, n, [n], False, streams=[torch.cuda.Stream()]), ref)
    # calls of one stream of samples on alternating streams run in call order
    cuts = (300, 1000, n - 1300)
    gpu.resetChannelSquelch()
    y, sides = run_cuts(torch, gpu, audio, sense, per, nch, n, list(cuts), False, streams=[torch.cuda.Stream(), torch.cuda.Stream()])
    same(y, sides, cpu_result(nch, n, A, H, fade, kind, fin, fout, cuts))


def test_reset_and_failed_calls(torch_dev, gpu):
    torch = torch_dev
    nch, n = 3, 30 * B + 3
    A, H, fade, kind, fin, fout = 3, 2, 1, CF32, AUDIO_F32, AUDIO_F32
    ref = cpu_result(nch, n, A, H, fade, kind, fin, fout)
    audio, sense, modes, thr, per = case(nch, n, A, H, kind, False)
    _, d_a, a_stride = to_dev(torch, audio, 1, n, ALIGNED)
    _, d_s, s_stride = to_dev(torch, sense, per, n, ALIGNED)
    f = gpu._L.sddc_ddc_channel_squelch_device
    o = out_tensor(torch, nch, n, ALIGNED, False)
    buf, out, ostride = o[0], o[1], o[2]
    ap, sp, op = d_a.data_ptr(), d_s.data_ptr(), out.data_ptr()
    assert f(gpu._h, ap, sp, nch, n, a_stride, s_stride, op, ostride, None, None, None, None) == ERR_STATE   # nothing set
    gpu.setChannelSquelch(modes, thr, A, H, fade, kind, fin, fout)
    y1, _ = run_cuts(torch, gpu, audio[:, :1300], sense[:, :2 * 1300], per, nch, 1300, [1300], False)
    # failed calls: they write nothing and change no state
    assert f(gpu._h, ap, sp, 2, n, a_stride, s_stride, op, ostride, None, None, None, None) == ERR_STATE
    assert f(gpu._h, ap, sp, nch, 0, a_stride, s_stride, op, ostride, None, None, None, None) == ERR_ARG
    assert f(gpu._h, ap, sp, nch, n, n - 1, s_stride, op, ostride, None, None, None, None) == ERR_ARG
    assert f(gpu._h, ap, sp, nch, n, a_stride, s_stride + 1, op, ostride, None, None, None, None) == ERR_ARG
    assert f(gpu._h, ap, sp, nch, n, a_stride, s_stride, op, n - 1, None, None, None, None) == ERR_ARG
    assert f(gpu._h, ap, None, nch, n, a_stride, s_stride, op, ostride, None, None, None, None) == ERR_ARG
    assert f(gpu._h, ap, sp + 4, nch, n - 1, a_stride, s_stride, op, ostride, None, None, None, None) == ERR_ARG
    assert f(gpu._h, ap, sp, nch, n, a_stride, s_stride, ap, a_stride, None, None, None, None) == ERR_ARG    # in place
    assert f(gpu._h, ap, sp, nch, n, a_stride, s_stride, sp, a_stride, None, None, None, None) == ERR_ARG    # on the sense stream
    torch.cuda.synchronize()
    assert np.isnan(buf.cpu().numpy()).all()
    y2, sides = run_cuts(torch, gpu, audio[:, 1300:], sense[:, 2 * 1300:], per, nch, n - 1300, [n - 1300], False)
    np.testing.assert_array_equal(bits(np.concatenate([y1, y2], axis=1)), bits(ref[0]))
    np.testing.assert_array_equal(sides[0][0], ref[1][0][0])
    gpu.resetChannelSquelch()   # a new, closed stream
    same(*run_cuts(torch, gpu, audio, sense, per, nch, n, [n], False), ref)
    gpu.setChannelSquelch(None, None)
    assert f(gpu._h, ap, sp, nch, n, a_stride, s_stride, op, ostride, None, None, None, None) == ERR_STATE


@functools.lru_cache(maxsize=None)
def chain_results():
    """process_channels_device at d = 6 (6 blocks, 3 channels; a noisy tone 10.3, 2.3 and -1.7 bins from the
    channels' centres) -> channel_decimate_device (R = 4, 65 taps: the first channel's tone falls into the stop
    band) -> channel_demodulate_device (FM) -> channel_squelch_device with the decimator's CF32 output as the
    sense stream, on one stream: first with every channel OFF to read d_level (how thresholds are calibrated),
    then as a carrier squelch (LEVEL, A = 1, H = 0, fade) with every threshold at the geometric mean of the
    largest and the smallest level; and the decimator, the demodulator and the squelch of a CPU handle fed
    the DDC's output."""
    import torch
    from extio_sddc_amd import DEVICE_CPU, R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import make_tone_stream
    d, nblk, R, tbs = 6, 6, 4, [1000, 1008, 1012]
    h = kaiser(65, 60.0, 0.08, 0.125)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    n = nsamp // R
    adc = make_tone_stream(nblk, 1010.3, amp=20.0, noise=10.0).copy()
    d_in = torch.from_numpy(adc).to("cuda")
    off = (np.full(nch, SQUELCH_OFF, np.int32), np.zeros((nch, 2), np.float32))

    def tail(r, modes, thr, iq_host=None):
        """decimator -> demodulator -> squelch of handle r; on the device, or on the host from iq_host"""
        r.setChannelDecimator(h, R, nch)
        r.setChannelDemodulator([DEMOD_FM] * nch)
        r.setChannelSquelch(modes, thr, 1, 0, 1, SQUELCH_SENSE_CF32)
        if iq_host is not None:
            z = r.channel_decimate(iq_host)
            a = r.channel_demodulate(z)
            return (z.view(np.float32).reshape(nch, -1), a) + r.channel_squelch(a, z, open=True, count=True, level=True)
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device="cuda")
        z = torch.zeros((nch, 2 * n), dtype=torch.float32, device="cuda")
        a = torch.zeros((nch, n), dtype=torch.float32, device="cuda")
        y = torch.full((nch, n), float("nan"), dtype=torch.float32, device="cuda")
        o, c = (torch.zeros(nch, dtype=torch.int32, device="cuda") for _ in range(2))
        lv = torch.zeros(nch, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=s)
        r.channel_decimate_device(iq, nch, nsamp, iq.stride(0), z, z.stride(0), stream=s)
        r.channel_demodulate_device(z, nch, n, z.stride(0), a, a.stride(0), stream=s)
        r.channel_squelch_device(a, z, nch, n, a.stride(0), z.stride(0), y, y.stride(0), d_open=o, d_count=c, d_level=lv,
                                 stream=s)
        torch.cuda.synchronize()
        return (iq.cpu().numpy(), z.cpu().numpy(), a.cpu().numpy(), y.cpu().numpy(), o.cpu().numpy().view(np.uint32),
                c.cpu().numpy().view(np.uint32), lv.cpu().numpy())

    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        calib = tail(r, *off)
        level = calib[6].astype(np.float64)
        t = np.float32(np.sqrt(level.max() * level.min()) / 256.0)
        modes, thr = np.full(nch, SQUELCH_LEVEL, np.int32), np.full((nch, 2), t, np.float32)
        dev = tail(r, modes, thr)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        cpu = tail(c, modes, thr, np.ascontiguousarray(dev[0]).view(np.complex64))
    return calib, dev, cpu, n


def test_ddc_decimator_demodulator_and_squelch_on_one_stream(torch_dev):
    """The chain of chain_results: with every channel OFF the squelch passes the demodulator's audio bit for
    bit and reports the levels; the levels of the channels with the tone in the decimator's pass band are at
    least 12 dB above the one without; as a carrier squelch the device chain's outputs, open, count and level
    are the CPU chain's bit for bit; a channel opens (fade in block 1, audio as it is from block 2) and one
    stays closed (+0)."""
    calib, dev, cpu, n = chain_results()
    nch = dev[0].shape[0]
    assert n == 3 * B
    np.testing.assert_array_equal(bits(calib[3]), bits(calib[2]))                  # OFF: y = x
    assert list(calib[4]) == [1] * nch and list(calib[5]) == [n] * nch
    level = calib[6]
    print(f"levels of the last block: {level}, largest / smallest {level.max() / level.min():.1f}")
    assert level.max() >= 16.0 * level.min() > 0.0
    iq, z, a, y, o, c, lv = dev
    np.testing.assert_array_equal(bits(iq), bits(calib[0]))
    np.testing.assert_array_equal(bits(z), bits(cpu[0]))
    np.testing.assert_array_equal(bits(a), bits(cpu[1]))
    np.testing.assert_array_equal(bits(y), bits(cpu[2]))
    np.testing.assert_array_equal(o, cpu[3])
    np.testing.assert_array_equal(c, cpu[4])
    np.testing.assert_array_equal(bits(lv), bits(cpu[5]))
    np.testing.assert_array_equal(bits(lv), bits(level))
    opened, closed = np.flatnonzero(o == 1), np.flatnonzero(o == 0)
    print(f"open {o}, samples in open blocks {c}")
    assert len(opened) >= 1 and len(closed) >= 1
    for ch in opened:
        assert c[ch] == 2 * B and (bits(y[ch, :B]) == 0).all()
        np.testing.assert_array_equal(bits(y[ch, 2 * B:]), bits(a[ch, 2 * B:]))
        w = (np.arange(B, dtype=np.float32) + 1) / np.float32(256.0)
        np.testing.assert_array_equal(bits(y[ch, B:2 * B]), bits(a[ch, B:2 * B] * w))
    for ch in closed:
        assert c[ch] == 0 and (bits(y[ch]) == 0).all()
