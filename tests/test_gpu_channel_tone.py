"""The channel tone detector on the GPU (pytest -m gpu): sddc_ddc_channel_tone_device and
sddc_ddc_channel_tone_host of a GPU handle bit for bit against the CPU backend (which
tests/test_channel_tone_cpu.py pins to the definition), outputs and the five side outputs, the bit-exact
properties of the kernels (cuts, streams, grids, run lengths, a channel alone, the position next to the phase
wrap, reset), and the DDC, the decimator, the FM demodulator, the audio filter and this stage on one stream.

Shapes (nch, nsamp, W), B = the block length (TONE_BLOCK):
  (1, 1)            one sample
  (1, B)            exactly one block
  (1, 3B + 17)      full blocks and a tail
  (3, 2 W B + 3)    masks 0, one tone and all tones in one call
  (1024, 2)         every channel, almost no samples each
  (1, 66B + 5)      W = 1: more windows than the gates kernel's 64-window step
  (2, 258B + 1)     W = 3, run length 8: several launch sets, and a window cut by every one
Masks of 1 tone (the windows kernel's small shape), 9 tones (one more than the large shape's chunk) and 64
tones, and of 4 and 5 tones, either side of the threshold between the two shapes.  Two layouts: ALIGNED puts
every stream on a 16-byte boundary with strides that are multiples of four samples (the four-samples-per-lane
paths), SHIFTED starts the inputs three samples and the outputs one sample into their tensors with odd gaps
(the sample-per-lane paths).  Every buffer lies in a poisoned tensor (NaN, int16: 0x7fff); the heads, the tails
and the gaps between the streams must stay untouched.  Every test runs under a watchdog that ends the process
if a GPU step hangs.
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


M = _load("channel_tone_model")

from extio_sddc_amd import TONE_BLOCK as B  # noqa: E402
from extio_sddc_amd import AUDIO_F32, AUDIO_S16, BIQUAD_LOWPASS, DEMOD_FM, biquad, tone_word  # noqa: E402

PARAM_CHTONE_MAX_WGS, PARAM_CHTONE_RUN_BLOCKS = 25, 26   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
S16_POISON = 0x7fff
# (nch, nsamp, W, run length or 0)
SHAPES = [(1, 1, 3, 0), (1, B, 3, 0), (1, 3 * B + 17, 3, 0), (3, 2 * 16 * B + 3, 16, 0), (1024, 2, 16, 0), (1, 66 * B + 5, 1, 0),
          (2, 258 * B + 1, 3, 8)]
MASKS = [1, 9, 64]
F, S = AUDIO_F32, AUDIO_S16
# (sense, audio in, audio out; None: detect only): every pairing at least once
COMBOS = [(F, None, None), (S, None, None), (F, F, F), (F, F, S), (F, S, F), (F, S, S), (S, F, F), (S, F, S), (S, S, F), (S, S, S)]
ALIGNED, SHIFTED = 0, 1
A_H = (2, 1)
SIDES = ("tone", "open", "count", "level", "powers")


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
def case(nch, n, W, mask_tones, sense16, in16):
    arrs = M.make_case(nch, n, W, 64, mask_tones, sense16, in16)
    for a in arrs:
        a.setflags(write=False)
    return arrs


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


def side_tensors(torch, nch, nt):
    ints = [torch.full((nch + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    lv = torch.full((2 * nch + 2,), float("nan"), dtype=torch.float32, device="cuda")
    pw = torch.full((nt * nch + 2,), float("nan"), dtype=torch.float32, device="cuda")
    return ints + [lv, pw]


def collect_sides(s, nch, nt):
    t, o, c, lv, pw = (v.cpu().numpy() for v in s)
    for v in (t, o, c):
        assert v[0] == -7 and v[-1] == -7
    assert np.isnan(lv[0]) and np.isnan(lv[-1]) and np.isnan(pw[0]) and np.isnan(pw[-1])
    return {"tone": t[1:-1].copy(), "open": o[1:-1].view(np.uint32).copy(), "count": c[1:-1].view(np.uint32).copy(),
            "level": lv[1:-1].reshape(nch, 2).copy(), "powers": pw[1:-1].reshape(nch, nt).copy()}


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run_cuts(torch, r, sense, audio, nch, n, cuts, out16, layout=ALIGNED, streams=None, nt=64):
    """The stream in calls of `cuts` samples, each on the columns of the inputs it covers; nothing synchronises
    between the calls.  Returns the outputs [nch, n] (None without audio) and the side outputs of every call."""
    assert sum(cuts) == n and min(cuts) > 0
    _, d_s, s_stride = to_dev(torch, sense, n, layout)
    d_a, a_stride = None, 0
    if audio is not None:
        _, d_a, a_stride = to_dev(torch, audio, n, layout)
    outs = [out_tensor(torch, nch, k, layout, out16) if audio is not None else None for k in cuts]
    sides = [side_tensors(torch, nch, nt) for _ in cuts]
    torch.cuda.synchronize()   # the uploads and poison fills are done before a call on another stream runs
    at = 0
    for k, ln in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        sd = sides[k]
        r.channel_tone_device(d_s[at:], s_stride, None if d_a is None else d_a[at:], nch, ln, a_stride,
                              None if d_a is None else outs[k][1], 0 if d_a is None else outs[k][2], d_tone=sd[0][1:],
                              d_open=sd[1][1:], d_count=sd[2][1:], d_level=sd[3][1:], d_powers=sd[4][1:], stream=s)
        at += ln
    torch.cuda.synchronize()
    y = None if audio is None else np.concatenate([collect(o, nch, ln) for o, ln in zip(outs, cuts)], axis=1)
    return y, [collect_sides(s, nch, nt) for s in sides]


@functools.lru_cache(maxsize=None)
def cpu_result(nch, n, W, mt, combo, cuts=None, pos0=0):
    """The CPU backend's outputs [nch, n] and per-call side outputs of the stream cut into `cuts`."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    fs, fin, fout = combo
    sense, audio, words, masks, thr = case(nch, n, W, mt, fs == S, fin == S)
    ys, sides, at = [], [], 0
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelToneDetector(words, masks, thr, W, *A_H, fs, fin or F, fout or F)
        if pos0:
            assert c._L.sddc_ddc_internal_chtone_set_position(c._h, pos0) == 0
        for ln in (cuts or (n,)):
            o = c.channel_tone(sense[:, at:at + ln], None if fin is None else audio[:, at:at + ln])
            ys.append(o.pop("out"))
            sides.append(o)
            at += ln
    y = None if fin is None else np.concatenate(ys, axis=1)
    return y, sides


def set_param(r, param, value):
    return r._L.sddc_ddc_internal_set_param(r._h, param, value)


def same(y, sides, ref, what=None):
    if ref[0] is None:
        assert y is None
    else:
        assert y.dtype == ref[0].dtype
        np.testing.assert_array_equal(bits(y), bits(ref[0]), err_msg=str(what))
    assert len(sides) == len(ref[1])
    for a, b in zip(sides, ref[1]):
        for name in SIDES:
            np.testing.assert_array_equal(bits(a[name]), bits(b[name]), err_msg=f"{name} {what}")


def setup(r, nch, n, W, mt, combo):
    fs, fin, fout = combo
    sense, audio, words, masks, thr = case(nch, n, W, mt, fs == S, fin == S)
    r.setChannelToneDetector(words, masks, thr, W, *A_H, fs, fin or F, fout or F)
    return sense, (None if fin is None else audio)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-W{s[2]}")
def test_gpu_equals_the_cpu_backend(torch_dev, gpu, shape):
    nch, n, W, run = shape
    assert set_param(gpu, PARAM_CHTONE_RUN_BLOCKS, run) == 0
    opened = 0
    for mi, mt in enumerate(MASKS):
        for ki, combo in enumerate(COMBOS):
            if nch == 1024 and (ki + mi) % 3:     # the widest shape on a third of the pairings
                continue
            ref = cpu_result(nch, n, W, mt, combo)
            sense, audio = setup(gpu, nch, n, W, mt, combo)
            layout = (mi + ki) % 2
            y, sides = run_cuts(torch_dev, gpu, sense, audio, nch, n, [n], combo[2] == S, layout)
            same(y, sides, ref, ("device", shape, mt, combo, layout))
            if ki % 3 == mi % 3:   # the host entry on a third of them
                gpu.resetChannelToneDetector()
                o = gpu.channel_tone(sense, audio)
                same(o.pop("out"), [o], ref, ("host", shape, mt, combo))
            opened += int(sides[0]["count"][1:].sum()) if nch > 1 else int(sides[0]["count"].sum())
    if n >= 66 * B:
        assert opened > 0


CUTS = {"edges": lambda n, W: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n, W: [100, B, n - B - 100],
        "window": lambda n, W: [W * B - 2, 1, 1, 1, 1, n - W * B - 2]}


@pytest.mark.parametrize("layout", [ALIGNED, SHIFTED])
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_cuts_are_bit_identical(torch_dev, gpu, cut, layout):
    k = 0
    for nch, n, W, _ in (SHAPES[3], SHAPES[5], SHAPES[6]):
        for mt in MASKS:
            combo = COMBOS[(3 * k + layout) % len(COMBOS)]
            k += 1
            cuts = tuple(CUTS[cut](n, W))
            ref = cpu_result(nch, n, W, mt, combo, cuts)
            whole = cpu_result(nch, n, W, mt, combo)
            if whole[0] is not None:
                np.testing.assert_array_equal(bits(ref[0]), bits(whole[0]))   # the CPU backend's own cut invariance
            assert sum(int(s["count"].sum()) for s in ref[1]) == int(whole[1][0]["count"].sum())   # the counts add up
            sense, audio = setup(gpu, nch, n, W, mt, combo)
            y, sides = run_cuts(torch_dev, gpu, sense, audio, nch, n, list(cuts), combo[2] == S, layout)
            same(y, sides, ref, (nch, n, W, mt, combo))


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5], SHAPES[6]], ids=lambda s: f"{s[0]}x{s[1]}-W{s[2]}")
def test_bit_identical_for_any_grid_and_run_length(torch_dev, gpu, shape):
    nch, n, W, _ = shape
    k = 0
    for cap in (1, 7, 0):
        for run in (1, 8, 33, 0):
            mt = MASKS[k % 3]
            combo = COMBOS[(k * 3 + 2) % len(COMBOS)]
            k += 1
            assert set_param(gpu, PARAM_CHTONE_MAX_WGS, cap) == 0 and set_param(gpu, PARAM_CHTONE_RUN_BLOCKS, run) == 0
            cuts = (100, n - 100)   # the second call starts inside a block, from the carried state
            ref = cpu_result(nch, n, W, mt, combo, cuts)
            sense, audio = setup(gpu, nch, n, W, mt, combo)
            y, sides = run_cuts(torch_dev, gpu, sense, audio, nch, n, list(cuts), combo[2] == S, k % 2)
            same(y, sides, ref, (cap, run, mt, combo))
    assert set_param(gpu, PARAM_CHTONE_MAX_WGS, -1) == ERR_ARG and set_param(gpu, PARAM_CHTONE_RUN_BLOCKS, -1) == ERR_ARG
    assert set_param(gpu, PARAM_CHTONE_RUN_BLOCKS, (1 << 20) + 1) == ERR_ARG


@pytest.mark.parametrize("mt", [4, 5])
def test_masks_either_side_of_the_shape_threshold(torch_dev, gpu, mt):
    """Four tones on every channel take the windows kernel's small shape, five the large one."""
    nch, n, W, _ = SHAPES[6]
    for k, combo in enumerate(((F, F, F), (S, None, None))):
        cuts = (100, n - 100)
        ref = cpu_result(nch, n, W, mt, combo, cuts)
        sense, audio = setup(gpu, nch, n, W, mt, combo)
        same(*run_cuts(torch_dev, gpu, sense, audio, nch, n, list(cuts), False, k), ref, (mt, combo))


def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu):
    nch, n, W, mt, combo = 3, 30 * B + 3, 3, 9, (F, F, F)
    among = cpu_result(nch, n, W, mt, combo)
    sense, audio, words, masks, thr = case(nch, n, W, mt, False, False)
    for c in range(nch):
        gpu.setChannelToneDetector(words, masks[c:c + 1], thr[c:c + 1], W, *A_H)
        y, sides = run_cuts(torch_dev, gpu, sense[c:c + 1], audio[c:c + 1], 1, n, [n], False)
        np.testing.assert_array_equal(bits(y[0]), bits(among[0][c]))
        for name in SIDES:
            np.testing.assert_array_equal(bits(sides[0][name][0]), bits(among[1][0][name][c]), err_msg=name)


def test_a_side_stream_equals_the_default_stream(torch_dev, gpu):
    torch = torch_dev
    nch, n, W, _ = SHAPES[6]
    mt, combo = 9, (F, F, F)
    ref = cpu_result(nch, n, W, mt, combo)
    sense, audio = setup(gpu, nch, n, W, mt, combo)
    same(*run_cuts(torch, gpu, sense, audio, nch, n, [n], False), ref)
    gpu.resetChannelToneDetector()
    same(*run_cuts(torch, gpu, sense, audio, nch, n, [n], False, streams=[torch.cuda.Stream()]), ref)
    # calls of one stream of samples on alternating streams run in call order
    cuts = (300, 1000, n - 1300)
    gpu.resetChannelToneDetector()
    y, sides = run_cuts(torch, gpu, sense, audio, nch, n, list(cuts), False, streams=[torch.cuda.Stream(), torch.cuda.Stream()])
    same(y, sides, cpu_result(nch, n, W, mt, combo, cuts))


@pytest.mark.parametrize("W", [3, 16])
def test_the_position_next_to_the_phase_wrap(torch_dev, gpu, W):
    WB = W * B
    pos0 = (2 ** 32 // WB - 2) * WB
    nch, n, mt, combo = 3, 4 * WB + 17, 64, (F, F, F)
    cuts = (WB + 5, WB, n - 2 * WB - 5)
    ref = cpu_result(nch, n, W, mt, combo, cuts, pos0)
    assert not np.array_equal(bits(ref[1][-1]["powers"]), bits(cpu_result(nch, n, W, mt, combo, cuts)[1][-1]["powers"]))
    sense, audio = setup(gpu, nch, n, W, mt, combo)
    f = gpu._L.sddc_ddc_internal_chtone_set_position
    assert f(gpu._h, pos0 + B) == ERR_ARG and f(gpu._h, pos0) == 0
    same(*run_cuts(torch_dev, gpu, sense, audio, nch, n, list(cuts), False), ref)


def test_reset_and_failed_calls(torch_dev, gpu):
    torch = torch_dev
    nch, n, W, mt, combo = 3, 30 * B + 3, 3, 9, (F, F, F)
    ref = cpu_result(nch, n, W, mt, combo)
    sense, audio, words, masks, thr = case(nch, n, W, mt, False, False)
    _, d_s, s_stride = to_dev(torch, sense, n, ALIGNED)
    _, d_a, a_stride = to_dev(torch, audio, n, ALIGNED)
    f = gpu._L.sddc_ddc_channel_tone_device
    o = out_tensor(torch, nch, n, ALIGNED, False)
    buf, out, ostride = o[0], o[1], o[2]
    sp, ap, op = d_s.data_ptr(), d_a.data_ptr(), out.data_ptr()
    none = (None,) * 6

    def call(s=sp, ss=s_stride, a=ap, c=nch, m=n, ast=a_stride, out_=op, ost=ostride):
        return f(gpu._h, s, ss, a, c, m, ast, out_, ost, *none)

    assert call() == ERR_STATE                                   # nothing set
    gpu.setChannelToneDetector(words, masks, thr, W, *A_H)
    y1, _ = run_cuts(torch, gpu, sense[:, :1300], audio[:, :1300], nch, 1300, [1300], False)
    # failed calls: they write nothing and change no state
    assert call(c=2) == ERR_STATE and call(m=0) == ERR_ARG and call(ss=n - 1) == ERR_ARG and call(ast=n - 1) == ERR_ARG
    assert call(ost=n - 1) == ERR_ARG and call(s=None) == ERR_ARG and call(a=None) == ERR_ARG and call(out_=None) == ERR_ARG
    assert call(s=sp + 2, m=n - 1) == ERR_ARG
    assert call(out_=ap, ost=a_stride) == ERR_ARG                # in place
    assert call(out_=sp, ost=s_stride) == ERR_ARG                # on the sense stream
    torch.cuda.synchronize()
    assert np.isnan(buf.cpu().numpy()).all()
    y2, sides = run_cuts(torch, gpu, sense[:, 1300:], audio[:, 1300:], nch, n - 1300, [n - 1300], False)
    np.testing.assert_array_equal(bits(np.concatenate([y1, y2], axis=1)), bits(ref[0]))
    for name in ("tone", "open", "level", "powers"):
        np.testing.assert_array_equal(bits(sides[0][name]), bits(ref[1][0][name]), err_msg=name)
    gpu.resetChannelToneDetector()   # a new, closed stream
    same(*run_cuts(torch, gpu, sense, audio, nch, n, [n], False), ref)
    gpu.setChannelToneDetector(None, None, None)
    assert call() == ERR_STATE


FA = 125000.0     # the audio rate of the chain below with the ADC at 64 MS/s
CHAIN_TONES = (67.0, 100.0, 151.4, 203.5, 254.1)


@functools.lru_cache(maxsize=None)
def chain_results():
    """Two NBFM carriers of amplitude 12000 in noise at the centres of two channels 24 bins apart, both modulated
    by a 1 kHz tone (3 kHz deviation), the first also by a 100.0 Hz sub-tone (600 Hz deviation):
    process_channels_device at d = 6 (96 blocks) -> channel_decimate_device (R = 4, 65 taps) ->
    channel_demodulate_device (FM) -> channel_audio_filter_device of a second handle (two low-pass sections at
    300 Hz) -> channel_tone_device (five CTCSS tones, W = 16, A = 1, H = 0) gating the demodulator's audio, on one
    stream; and the same stages of CPU handles fed the DDC's output."""
    import torch
    from extio_sddc_amd import DEVICE_CPU, R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import BLOCK, HALF_FFT
    d, nblk, R, tbs, W = 6, 96, 4, [1000, 1024], 16
    h = kaiser(65, 60.0, 0.08, 0.125)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    n = nsamp // R
    fadc = FA * R * 128
    t = np.arange(nblk * BLOCK, dtype=np.float64)
    voice = (3000.0 / 1000.0) * np.sin(2 * np.pi * 1000.0 / fadc * t)
    sub = (600.0 / 100.0) * np.sin(2 * np.pi * 100.0 / fadc * t)
    x = 12000.0 * np.cos(2 * np.pi * tbs[0] / (2 * HALF_FFT) * t + voice + sub)
    x += 12000.0 * np.cos(2 * np.pi * tbs[1] / (2 * HALF_FFT) * t + voice + 1.0)
    x += np.random.default_rng(11).normal(0, 10.0, x.shape[0])
    adc = np.concatenate([np.zeros(HALF_FFT, np.int16), np.clip(np.round(x), -32767, 32767).astype(np.int16)])
    d_in = torch.from_numpy(adc).to("cuda")
    lp = np.tile(biquad(BIQUAD_LOWPASS, 300.0 / FA), (nch, 2, 1))
    words = [tone_word(f, FA) for f in CHAIN_TONES]
    masks = np.full(nch, (1 << len(words)) - 1, np.uint64)
    thr = np.tile(np.float32([0.2, 0.1, 0.0]), (nch, 1))

    def tail(r, r2, iq_host=None):
        r.setChannelDecimator(h, R, nch)
        r.setChannelDemodulator([DEMOD_FM] * nch)
        r2.setChannelAudioFilter(lp)
        r.setChannelToneDetector(words, masks, thr, W, 1, 0)
        if iq_host is not None:
            a = r.channel_demodulate(r.channel_decimate(iq_host))
            s = r2.channel_audio_filter(a)
            o = r.channel_tone(s, a)
            return a, s, o
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device="cuda")
        z = torch.zeros((nch, 2 * n), dtype=torch.float32, device="cuda")
        a, s = (torch.zeros((nch, n), dtype=torch.float32, device="cuda") for _ in range(2))
        y = torch.full((nch, n), float("nan"), dtype=torch.float32, device="cuda")
        tn, op, cn = (torch.zeros(nch, dtype=torch.int32, device="cuda") for _ in range(3))
        lv = torch.zeros((nch, 2), dtype=torch.float32, device="cuda")
        pw = torch.zeros((nch, len(words)), dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=st)
        r.channel_decimate_device(iq, nch, nsamp, iq.stride(0), z, z.stride(0), stream=st)
        r.channel_demodulate_device(z, nch, n, z.stride(0), a, a.stride(0), stream=st)
        r2.channel_audio_filter_device(a, nch, n, a.stride(0), s, s.stride(0), stream=st)
        r.channel_tone_device(s, s.stride(0), a, nch, n, a.stride(0), y, y.stride(0), d_tone=tn, d_open=op, d_count=cn, d_level=lv,
                              d_powers=pw, stream=st)
        torch.cuda.synchronize()
        o = {"out": y.cpu().numpy(), "tone": tn.cpu().numpy(), "open": op.cpu().numpy().view(np.uint32),
             "count": cn.cpu().numpy().view(np.uint32), "level": lv.cpu().numpy(), "powers": pw.cpu().numpy()}
        return iq.cpu().numpy(), a.cpu().numpy(), s.cpu().numpy(), o

    with R2iq(gain=1.0) as r, R2iq(gain=1.0) as r2:
        r.setDecimate(d)
        dev = tail(r, r2)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c, R2iq(gain=1.0, device=DEVICE_CPU) as c2:
        cpu = tail(c, c2, np.ascontiguousarray(dev[0]).view(np.complex64))
    return dev, cpu, n, W


def test_ddc_to_tone_detector_on_one_stream(torch_dev):
    """The chain of chain_results: the device chain's audio, sense stream, gated audio and side outputs are the
    CPU chain's bit for bit; the channel with the sub-tone reports tone 1 (100.0 Hz) and is open from its
    third window at the latest, its neighbour reports -1 and is closed there (+0)."""
    dev, cpu, n, W = chain_results()
    _, a, s, o = dev
    assert n == 3 * W * B
    np.testing.assert_array_equal(bits(a), bits(cpu[0]))
    np.testing.assert_array_equal(bits(s), bits(cpu[1]))
    for name in ("out",) + SIDES:
        np.testing.assert_array_equal(bits(o[name]), bits(cpu[2][name]), err_msg=name)
    rho = o["level"][:, 0].astype(np.float64) / (W * B * o["level"][:, 1].astype(np.float64))
    print(f"tone {o['tone']}, open {o['open']}, count {o['count']}, P / (256 W E) {rho}")
    assert list(o["tone"]) == [1, -1] and list(o["open"]) == [1, 0]
    # window 0 holds the chain's start-up transient; window 1 is clean, so window 2 is open on channel 0 alone
    assert o["count"][0] in (W * B, 2 * W * B) and o["count"][1] in (0, W * B)
    assert rho[0] > 0.3 and rho[1] < 0.05
    assert (bits(o["out"][0, :W * B]) == 0).all() and (bits(o["out"][1, 2 * W * B:]) == 0).all()
    np.testing.assert_array_equal(bits(o["out"][0, 2 * W * B:]), bits(a[0, 2 * W * B:]))
