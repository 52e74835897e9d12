"""The channel stereo decoder on the GPU (pytest -m gpu): sddc_ddc_channel_stereo_device and
sddc_ddc_channel_stereo_host of a GPU handle bit for bit against the CPU backend (which
tests/test_channel_stereo_cpu.py pins to the definition), both outputs and the four side outputs, the bit-exact
properties of the kernels (cuts, streams, grids, run lengths, a channel alone, the position next to the phase
wrap, reset), and the DDC, the FM demodulator, this stage and the audio resampler on one stream.

Shapes (nch, nsamp, W, run length), B = the block length (STEREO_BLOCK):
  (1, 1)            one sample
  (1, B)            exactly one block
  (1, 3B + 17)      full blocks and a tail
  (3, 2 W B + 3)    AUTO with a pilot, MONO and AUTO without a pilot in one call
  (1024, 2)         every channel, almost no samples each
  (1, 66B + 5)      W = 1: a window per block, more windows than a wave has lanes
  (2, 258B + 1)     W = 3, run length 8: several launch sets, and a window cut by every one
Two layouts: ALIGNED puts every stream on a 16-byte boundary with strides that are multiples of four samples
(the four-samples-per-lane paths), SHIFTED starts the inputs three samples and the outputs one sample into
their tensors with odd gaps (the sample-per-lane paths).  Every buffer lies in a poisoned tensor (NaN, int16:
0x7fff); the heads, the tails and the gaps between the streams must stay untouched.  Every test runs under a
watchdog that ends the process if a GPU step hangs.
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


M = _load("channel_stereo_model")

from extio_sddc_amd import STEREO_BLOCK as B  # noqa: E402
from extio_sddc_amd import AUDIO_F32, AUDIO_S16, DEMOD_FM, STEREO_AUTO, stereo_pilot_word  # noqa: E402

PARAM_CHST_MAX_WGS, PARAM_CHST_RUN_BLOCKS = 31, 32   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
S16_POISON = 0x7fff
# (nch, nsamp, W, run length or 0)
SHAPES = [(1, 1, 3, 0), (1, B, 3, 0), (1, 3 * B + 17, 3, 0), (3, 2 * 8 * B + 3, 8, 0), (1024, 2, 8, 0), (1, 66 * B + 5, 1, 0),
          (2, 258 * B + 1, 3, 8)]
F, S = AUDIO_F32, AUDIO_S16
COMBOS = [(F, F), (F, S), (S, F), (S, S)]   # (input, outputs)
ALIGNED, SHIFTED = 0, 1
A_H = (1, 1)
SIDES = ("stereo", "count", "level", "phase")


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
def case(nch, n, W, in16):
    x, w, modes, params = M.make_case(nch, n, W, in16)
    for a in (x, modes, params):
        a.setflags(write=False)
    return x, w, modes, params


def stride_of(n, layout):
    return (n + 3) // 4 * 4 if layout == ALIGNED else n + 1 + (n % 2)


def to_dev(torch, a, n, layout):
    """a [nch, n] in a poisoned tensor: (the tensor, the view at the first stream, the stride)."""
    nch = a.shape[0]
    poison = S16_POISON if a.dtype == np.int16 else np.nan
    stride = stride_of(n, layout)
    off = 0 if layout == ALIGNED else 3
    buf = np.full(off + nch * stride + 8, poison, a.dtype)
    buf[off:off + nch * stride].reshape(nch, stride)[:, :n] = a
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
    ints = [torch.full((nch + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    flts = [torch.full((2 * nch + 2,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    return ints + flts


def collect_sides(s, nch):
    st, c, lv, ph = (v.cpu().numpy() for v in s)
    for v in (st, c):
        assert v[0] == -7 and v[-1] == -7
    for v in (lv, ph):
        assert np.isnan(v[0]) and np.isnan(v[-1])
    return {"stereo": st[1:-1].view(np.uint32).copy(), "count": c[1:-1].view(np.uint32).copy(),
            "level": lv[1:-1].reshape(nch, 2).copy(), "phase": ph[1:-1].reshape(nch, 2).copy()}


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run_cuts(torch, r, x, nch, n, cuts, out16, layout=ALIGNED, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of the input it covers; nothing synchronises
    between the calls.  Returns (left, right) [nch, n] and the side outputs of every call."""
    assert sum(cuts) == n and min(cuts) > 0
    _, d_x, x_stride = to_dev(torch, x, n, layout)
    outs = [(out_tensor(torch, nch, k, layout, out16), out_tensor(torch, nch, k, layout, out16)) for k in cuts]
    sides = [side_tensors(torch, nch) for _ in cuts]
    torch.cuda.synchronize()   # the uploads and poison fills are done before a call on another stream runs
    at = 0
    for k, ln in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        sd = sides[k]
        r.channel_stereo_device(d_x[at:], nch, ln, x_stride, outs[k][0][1], outs[k][1][1], outs[k][0][2], d_stereo=sd[0][1:],
                                d_count=sd[1][1:], d_level=sd[2][1:], d_phase=sd[3][1:], stream=s)
        at += ln
    torch.cuda.synchronize()
    y = tuple(np.concatenate([collect(o[i], nch, ln) for o, ln in zip(outs, cuts)], axis=1) for i in range(2))
    return y, [collect_sides(s, nch) for s in sides]


@functools.lru_cache(maxsize=None)
def cpu_result(nch, n, W, combo, cuts=None, pos0=0):
    """The CPU backend's outputs (left, right) [nch, n] and per-call side outputs of the stream cut into `cuts`."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    x, w, modes, params = case(nch, n, W, combo[0] == S)
    ls, rs, sides, at = [], [], [], 0
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelStereoDecoder(w, modes, params, W, *A_H, *combo)
        if pos0:
            assert c._L.sddc_ddc_internal_chst_set_position(c._h, pos0) == 0
        for ln in (cuts or (n,)):
            o = c.channel_stereo(x[:, at:at + ln])
            ls.append(o.pop("left"))
            rs.append(o.pop("right"))
            sides.append(o)
            at += ln
    return (np.concatenate(ls, axis=1), np.concatenate(rs, axis=1)), sides


def set_param(r, param, value):
    return r._L.sddc_ddc_internal_set_param(r._h, param, value)


def same(y, sides, ref, what=None):
    for a, b, name in zip(y, ref[0], ("left", "right")):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{name} {what}")
    assert len(sides) == len(ref[1])
    for a, b in zip(sides, ref[1]):
        for name in SIDES:
            np.testing.assert_array_equal(bits(a[name]), bits(b[name]), err_msg=f"{name} {what}")


def setup(r, nch, n, W, combo):
    x, w, modes, params = case(nch, n, W, combo[0] == S)
    r.setChannelStereoDecoder(w, modes, params, W, *A_H, *combo)
    return x


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-W{s[2]}")
def test_gpu_equals_the_cpu_backend(torch_dev, gpu, shape):
    nch, n, W, run = shape
    assert set_param(gpu, PARAM_CHST_RUN_BLOCKS, run) == 0
    stereo = 0
    for ki, combo in enumerate(COMBOS):
        for layout in (ALIGNED, SHIFTED):
            if nch == 1024 and (ki + layout) % 2:     # the widest shape on half of the pairings
                continue
            ref = cpu_result(nch, n, W, combo)
            x = setup(gpu, nch, n, W, combo)
            y, sides = run_cuts(torch_dev, gpu, x, nch, n, [n], combo[1] == S, layout)
            same(y, sides, ref, ("device", shape, combo, layout))
            stereo += int(sides[0]["count"].sum())
        gpu.resetChannelStereoDecoder()
        o = gpu.channel_stereo(x)
        same((o.pop("left"), o.pop("right")), [o], cpu_result(nch, n, W, combo), ("host", shape, combo))
    if n >= 2 * 8 * B:
        assert stereo > 0


CUTS = {"edges": lambda n, W: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n, W: [100, B, n - B - 100],
        "window": lambda n, W: [W * B - 2, 1, 1, 1, 1, n - W * B - 2]}


@pytest.mark.parametrize("layout", [ALIGNED, SHIFTED])
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_cuts_are_bit_identical(torch_dev, gpu, cut, layout):
    k = 0
    for nch, n, W, _ in (SHAPES[3], SHAPES[5], SHAPES[6]):
        combo = COMBOS[(k + layout) % len(COMBOS)]
        k += 1
        cuts = tuple(CUTS[cut](n, W))
        ref = cpu_result(nch, n, W, combo, cuts)
        whole = cpu_result(nch, n, W, combo)
        for a, b in zip(ref[0], whole[0]):
            np.testing.assert_array_equal(bits(a), bits(b))   # the CPU backend's own cut invariance
        assert sum(int(s["count"].sum()) for s in ref[1]) == int(whole[1][0]["count"].sum())   # the counts add up
        x = setup(gpu, nch, n, W, combo)
        y, sides = run_cuts(torch_dev, gpu, x, nch, n, list(cuts), combo[1] == S, layout)
        same(y, sides, ref, (nch, n, W, combo))


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5], SHAPES[6]], ids=lambda s: f"{s[0]}x{s[1]}-W{s[2]}")
def test_bit_identical_for_any_grid_and_run_length(torch_dev, gpu, shape):
    nch, n, W, _ = shape
    k = 0
    for cap in (1, 7, 0):
        for run in (1, 8, 33, 0):
            combo = COMBOS[k % len(COMBOS)]
            k += 1
            assert set_param(gpu, PARAM_CHST_MAX_WGS, cap) == 0 and set_param(gpu, PARAM_CHST_RUN_BLOCKS, run) == 0
            cuts = (100, n - 100)   # the second call starts inside a block, from the carried state
            ref = cpu_result(nch, n, W, combo, cuts)
            x = setup(gpu, nch, n, W, combo)
            y, sides = run_cuts(torch_dev, gpu, x, nch, n, list(cuts), combo[1] == S, k % 2)
            same(y, sides, ref, (cap, run, combo))
    assert set_param(gpu, PARAM_CHST_MAX_WGS, -1) == ERR_ARG and set_param(gpu, PARAM_CHST_RUN_BLOCKS, -1) == ERR_ARG
    assert set_param(gpu, PARAM_CHST_RUN_BLOCKS, (1 << 20) + 1) == ERR_ARG


def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu):
    nch, n, W, combo = 3, 30 * B + 3, 3, (F, F)
    among = cpu_result(nch, n, W, combo)
    x, w, modes, params = case(nch, n, W, False)
    for c in range(nch):
        gpu.setChannelStereoDecoder(w, modes[c:c + 1], params[c:c + 1], W, *A_H)
        y, sides = run_cuts(torch_dev, gpu, x[c:c + 1], 1, n, [n], False)
        for i in range(2):
            np.testing.assert_array_equal(bits(y[i][0]), bits(among[0][i][c]))
        for name in SIDES:
            np.testing.assert_array_equal(bits(sides[0][name][0]), bits(among[1][0][name][c]), err_msg=name)


def test_a_side_stream_equals_the_default_stream(torch_dev, gpu):
    torch = torch_dev
    nch, n, W, _ = SHAPES[6]
    combo = (F, F)
    ref = cpu_result(nch, n, W, combo)
    x = setup(gpu, nch, n, W, combo)
    same(*run_cuts(torch, gpu, x, nch, n, [n], False), ref)
    gpu.resetChannelStereoDecoder()
    same(*run_cuts(torch, gpu, x, nch, n, [n], False, streams=[torch.cuda.Stream()]), ref)
    # calls of one stream of samples on alternating streams run in call order
    cuts = (300, 1000, n - 1300)
    gpu.resetChannelStereoDecoder()
    y, sides = run_cuts(torch, gpu, x, nch, n, list(cuts), False, streams=[torch.cuda.Stream(), torch.cuda.Stream()])
    same(y, sides, cpu_result(nch, n, W, combo, cuts))


@pytest.mark.parametrize("W", [3, 8])
def test_the_position_next_to_the_phase_wrap(torch_dev, gpu, W):
    WB = W * B
    pos0 = (2 ** 32 // WB - 2) * WB
    nch, n, combo = 3, 4 * WB + 17, (F, F)
    cuts = (WB + 5, WB, n - 2 * WB - 5)
    ref = cpu_result(nch, n, W, combo, cuts, pos0)
    assert not np.array_equal(bits(ref[1][-1]["phase"]), bits(cpu_result(nch, n, W, combo, cuts)[1][-1]["phase"]))
    x = setup(gpu, nch, n, W, combo)
    f = gpu._L.sddc_ddc_internal_chst_set_position
    assert f(gpu._h, pos0 + B) == ERR_ARG and f(gpu._h, pos0) == 0
    same(*run_cuts(torch_dev, gpu, x, nch, n, list(cuts), False), ref)


def test_reset_and_failed_calls(torch_dev, gpu):
    torch = torch_dev
    nch, n, W, combo = 3, 30 * B + 3, 3, (F, F)
    ref = cpu_result(nch, n, W, combo)
    x, w, modes, params = case(nch, n, W, False)
    _, d_x, x_stride = to_dev(torch, x, n, ALIGNED)
    f = gpu._L.sddc_ddc_channel_stereo_device
    ol, orr = out_tensor(torch, nch, n, ALIGNED, False), out_tensor(torch, nch, n, ALIGNED, False)
    ostride = ol[2]
    xp, lp, rp = d_x.data_ptr(), ol[1].data_ptr(), orr[1].data_ptr()
    none = (None,) * 5

    def call(x_=xp, c=nch, m=n, xs=x_stride, left=lp, right=rp, ost=ostride):
        return f(gpu._h, x_, c, m, xs, left, right, ost, *none)

    assert call() == ERR_STATE                                   # nothing set
    gpu.setChannelStereoDecoder(w, modes, params, W, *A_H)
    y1, _ = run_cuts(torch, gpu, x[:, :1300], nch, 1300, [1300], False)
    # failed calls: they write nothing and change no state
    assert call(c=2) == ERR_STATE and call(m=0) == ERR_ARG and call(xs=n - 1) == ERR_ARG and call(ost=n - 1) == ERR_ARG
    assert call(x_=None) == ERR_ARG and call(left=None) == ERR_ARG and call(right=None) == ERR_ARG
    assert call(x_=xp + 2, m=n - 1) == ERR_ARG
    assert call(left=xp, ost=x_stride) == ERR_ARG                # in place
    assert call(right=lp) == ERR_ARG and call(right=lp + 4 * n) == ERR_ARG   # the outputs on each other
    torch.cuda.synchronize()
    assert np.isnan(ol[0].cpu().numpy()).all() and np.isnan(orr[0].cpu().numpy()).all()
    y2, sides = run_cuts(torch, gpu, x[:, 1300:], nch, n - 1300, [n - 1300], False)
    for i in range(2):
        np.testing.assert_array_equal(bits(np.concatenate([y1[i], y2[i]], axis=1)), bits(ref[0][i]))
    for name in ("stereo", "level", "phase"):
        np.testing.assert_array_equal(bits(sides[0][name]), bits(ref[1][0][name]), err_msg=name)
    gpu.resetChannelStereoDecoder()   # a new stream
    same(*run_cuts(torch, gpu, x, nch, n, [n], False), ref)
    gpu.setChannelStereoDecoder(0, None, None)
    assert call() == ERR_STATE


@functools.lru_cache(maxsize=None)
def chain_results():
    """Two WFM carriers of amplitude 12000 in noise at the centres of two channels 400 bins apart, 75 kHz deviation,
    the first modulated by a stereo multiplex (a 1 kHz tone left, a 3 kHz tone right, the pilot), the second by a
    mono 1 kHz tone: process_channels_device at d = 6 (16 blocks, 500 kS/s per channel with the ADC at 64 MS/s) ->
    channel_demodulate_device (FM) -> channel_stereo_device (W = 2, A = 2, H = 0) -> channel_audio_resample_device
    of a second handle on the 2 nch output streams (1/4, a 65-tap Kaiser low-pass), on one stream; and the same
    stages of CPU handles fed the DDC's output."""
    import torch
    from extio_sddc_amd import DEVICE_CPU, R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import BLOCK, HALF_FFT
    d, nblk, tbs, W = 6, 16, [1000, 1400], 2
    fa = 500000.0
    fadc = fa * 128
    ha = kaiser(65, 60.0, 0.03, 0.1)
    n, nch = output_samples(d, nblk), len(tbs)
    m = n // 4
    t = np.arange(nblk * BLOCK, dtype=np.float64)
    left, right = 0.8 * np.sin(2 * np.pi * 1000.0 / fadc * t), 0.8 * np.sin(2 * np.pi * 3000.0 / fadc * t)
    mpx0 = M.mpx(left, right, fadc, 0.1, 0.4)
    x = 12000.0 * np.cos(2 * np.pi * tbs[0] / (2 * HALF_FFT) * t + 2 * np.pi * 75000.0 / fadc * np.cumsum(mpx0))
    x += 12000.0 * np.cos(2 * np.pi * tbs[1] / (2 * HALF_FFT) * t + 2 * np.pi * 75000.0 / fadc * np.cumsum(left) + 1.0)
    x += np.random.default_rng(11).normal(0, 10.0, x.shape[0])
    adc = np.concatenate([np.zeros(HALF_FFT, np.int16), np.clip(np.round(x), -32767, 32767).astype(np.int16)])
    d_in = torch.from_numpy(adc).to("cuda")
    word = stereo_pilot_word(fa)
    modes = [STEREO_AUTO] * nch
    params = np.tile(np.float32([0.004, 0.002, 0.0, 1.0]), (nch, 1))

    def tail(r, r2, iq_host=None):
        r.setChannelDemodulator([DEMOD_FM] * nch)
        r.setChannelStereoDecoder(word, modes, params, W, 2, 0)
        r2.setChannelAudioResampler(ha, 1, 4, 2 * nch)
        if iq_host is not None:
            a = r.channel_demodulate(iq_host)
            o = r.channel_stereo(a)
            lr = np.concatenate([o.pop("left"), o.pop("right")], axis=0)
            return a, lr, r2.channel_audio_resample_host(lr), o
        iq = torch.zeros((nch, 2 * n), dtype=torch.float32, device="cuda")
        a = torch.zeros((nch, n), dtype=torch.float32, device="cuda")
        lr = torch.full((2 * nch, n), float("nan"), dtype=torch.float32, device="cuda")
        y = torch.full((2 * nch, m), float("nan"), dtype=torch.float32, device="cuda")
        sd, cn = (torch.zeros(nch, dtype=torch.int32, device="cuda") for _ in range(2))
        lv, ph = (torch.zeros((nch, 2), dtype=torch.float32, device="cuda") for _ in range(2))
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=st)
        r.channel_demodulate_device(iq, nch, n, iq.stride(0), a, a.stride(0), stream=st)
        flat = lr.view(-1)   # the right streams follow the left ones: 2 nch streams of one stride
        r.channel_stereo_device(a, nch, n, a.stride(0), flat[:nch * n], flat[nch * n:], n, d_stereo=sd, d_count=cn, d_level=lv,
                                d_phase=ph, stream=st)
        assert r2.channel_audio_resample_device(lr, 2 * nch, n, n, y, y.stride(0), stream=st) == m
        torch.cuda.synchronize()
        o = {"stereo": sd.cpu().numpy().view(np.uint32), "count": cn.cpu().numpy().view(np.uint32), "level": lv.cpu().numpy(),
             "phase": ph.cpu().numpy()}
        return iq.cpu().numpy(), a.cpu().numpy(), lr.cpu().numpy(), y.cpu().numpy(), o

    with R2iq(gain=1.0) as r, R2iq(gain=1.0) as r2:
        r.setDecimate(d)
        dev = tail(r, r2)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c, R2iq(gain=1.0, device=DEVICE_CPU) as c2:
        cpu = tail(c, c2, np.ascontiguousarray(dev[0]).view(np.complex64))
    return dev[1:], cpu, n, W


def test_ddc_to_audio_resampler_through_the_stereo_decoder_on_one_stream(torch_dev):
    """The chain of chain_results: the device chain's MPX, its 2 nch decoded streams, their resampled audio and the
    side outputs are the CPU chain's bit for bit; the channel with the pilot ends in stereo with a pilot share of
    the window's energy above rho_open, its mono neighbour does not."""
    dev, cpu, n, W = chain_results()
    a, lr, y, o = dev
    np.testing.assert_array_equal(bits(a), bits(cpu[0]))
    np.testing.assert_array_equal(bits(lr), bits(cpu[1]))
    np.testing.assert_array_equal(bits(y), bits(cpu[2]))
    for name in SIDES:
        np.testing.assert_array_equal(bits(o[name]), bits(cpu[3][name]), err_msg=name)
    rho = o["level"][:, 0].astype(np.float64) / (W * B * o["level"][:, 1].astype(np.float64))
    print(f"stereo {o['stereo']}, count {o['count']} of {n}, P / (256 W E) {rho}, phase {o['phase']}")
    assert np.isfinite(y).all() and list(o["stereo"]) == [1, 0] and o["count"][1] == 0
    assert rho[0] > 0.004 and rho[1] < 0.002
    nch = a.shape[0]
    assert not np.array_equal(bits(lr[0]), bits(lr[nch])) and np.array_equal(bits(lr[1]), bits(lr[nch + 1]))
