"""The channel DCS decoder on the GPU (pytest -m gpu): sddc_ddc_channel_dcs_device and sddc_ddc_channel_dcs_host of
a GPU handle bit for bit against the CPU backend (which tests/test_channel_dcs_cpu.py pins to the definition),
outputs and the four side outputs, the bit-exact properties of the kernels (cuts, streams, grids, run lengths, a
channel alone, reset), and the DDC, the decimator, the FM demodulator, the audio filter and this stage on one
stream.

Shapes (nch, nsamp), B = the block length (DCS_BLOCK), w = 2^29 and W = 6 unless stated:
  (1, 1)              one sample
  (1, B)              exactly one block
  (1, 6B)             exactly one window
  (1, 6B + 1)         a window and one sample
  (3, 12B + 3)        OFF, one code and ANY in one call
  (1024, 2)           every channel, almost no samples each
  (1, 396B + 5)       66 windows: more than the gates kernel's 64-window step
  (2, 258B + 1)       run length 8: several launch sets, and a window cut by every one
  (1, 65536 + 300)    W = 256 with its smallest w
  (3, 20B + 9)        w = 72155451 (134.4 bit/s at 8 kS/s): sub-bin edges that fall irregularly
Two layouts: ALIGNED puts every stream on a 16-byte boundary with strides that are multiples of four samples (the
four-samples-per-lane paths), SHIFTED starts the inputs three samples and the outputs one sample into their tensors
with odd gaps (the sample-per-lane paths).  Every buffer lies in a poisoned tensor (NaN, int16: 0x7fff); the heads,
the tails and the gaps between the streams must stay untouched.  Every test runs under a watchdog that ends the
process if a GPU step hangs.
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


M = _load("channel_dcs_model")

from extio_sddc_amd import DCS_BLOCK as B  # noqa: E402
from extio_sddc_amd import AUDIO_F32, AUDIO_S16, BIQUAD_LOWPASS, DCS_ANY, DEMOD_FM, biquad, dcs_codeword  # noqa: E402

PARAM_CHDCS_MAX_WGS, PARAM_CHDCS_RUN_BLOCKS, PARAM_CHDCS_BALLOT = 27, 28, 29   # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
S16_POISON = 0x7fff
WMAX, W8K = 1 << 29, 72155451
WLONG = M.smallest_word(256)
# (nch, nsamp, W, w, run length or 0)
SHAPES = [(1, 1, 6, WMAX, 0), (1, B, 6, WMAX, 0), (1, 6 * B, 6, WMAX, 0), (1, 6 * B + 1, 6, WMAX, 0), (3, 12 * B + 3, 6, WMAX, 0),
          (1024, 2, 6, WMAX, 0), (1, 396 * B + 5, 6, WMAX, 0), (2, 258 * B + 1, 6, WMAX, 8), (1, 65536 + 300, 256, WLONG, 0),
          (3, 20 * B + 9, 6, W8K, 0)]
F, S = AUDIO_F32, AUDIO_S16
# (sense, audio in, audio out; None: detect only): every pairing
COMBOS = [(F, None, None), (S, None, None), (F, F, F), (F, F, S), (F, S, F), (F, S, S), (S, F, F), (S, F, S), (S, S, F), (S, S, S)]
ALIGNED, SHIFTED = 0, 1
LIMITS = (1, 2, 2, 1)   # e_open, e_close, A, H
SIDES = ("code", "open", "count", "info")


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
def case(nch, n, W, w, ncodes, sense16, in16):
    arrs = M.make_case(nch, n, W, w, ncodes, sense16, in16)
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


def side_tensors(torch, nch):
    return [torch.full((k * nch + 2,), -7, dtype=torch.int32, device="cuda") for k in (1, 1, 1, 4)]


def collect_sides(s, nch):
    c, o, n, i = (v.cpu().numpy() for v in s)
    for v in (c, o, n, i):
        assert v[0] == -7 and v[-1] == -7
    return {"code": c[1:-1].copy(), "open": o[1:-1].view(np.uint32).copy(), "count": n[1:-1].view(np.uint32).copy(),
            "info": i[1:-1].view(np.uint32).reshape(nch, 4).copy()}


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def run_cuts(torch, r, sense, audio, nch, n, cuts, out16, layout=ALIGNED, streams=None):
    """The stream in calls of `cuts` samples, each on the columns of the inputs it covers; nothing synchronises
    between the calls.  Returns the outputs [nch, n] (None without audio) and the side outputs of every call."""
    assert sum(cuts) == n and min(cuts) > 0
    _, d_s, s_stride = to_dev(torch, sense, n, layout)
    d_a, a_stride = None, 0
    if audio is not None:
        _, d_a, a_stride = to_dev(torch, audio, n, layout)
    outs = [out_tensor(torch, nch, k, layout, out16) if audio is not None else None for k in cuts]
    sides = [side_tensors(torch, nch) for _ in cuts]
    torch.cuda.synchronize()   # the uploads and poison fills are done before a call on another stream runs
    at = 0
    for k, ln in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        sd = sides[k]
        r.channel_dcs_device(d_s[at:], s_stride, None if d_a is None else d_a[at:], nch, ln, a_stride,
                             None if d_a is None else outs[k][1], 0 if d_a is None else outs[k][2], d_code=sd[0][1:],
                             d_open=sd[1][1:], d_count=sd[2][1:], d_info=sd[3][1:], stream=s)
        at += ln
    torch.cuda.synchronize()
    y = None if audio is None else np.concatenate([collect(o, nch, ln) for o, ln in zip(outs, cuts)], axis=1)
    return y, [collect_sides(s, nch) for s in sides]


@functools.lru_cache(maxsize=None)
def cpu_result(nch, n, W, w, ncodes, combo, cuts=None):
    """The CPU backend's outputs [nch, n] and per-call side outputs of the stream cut into `cuts`."""
    from extio_sddc_amd import DEVICE_CPU, R2iq
    fs, fin, fout = combo
    sense, audio, cws, params = case(nch, n, W, w, ncodes, fs == S, fin == S)
    ys, sides, at = [], [], 0
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        c.setChannelDcsDecoder(cws, params, w, W, *LIMITS, fs, fin or F, fout or F)
        for ln in (cuts or (n,)):
            o = c.channel_dcs_host(sense[:, at:at + ln], None if fin is None else audio[:, at:at + ln])
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
            np.testing.assert_array_equal(a[name], b[name], err_msg=f"{name} {what}")


def setup(r, nch, n, W, w, ncodes, combo):
    fs, fin, fout = combo
    sense, audio, cws, params = case(nch, n, W, w, ncodes, fs == S, fin == S)
    r.setChannelDcsDecoder(cws, params, w, W, *LIMITS, fs, fin or F, fout or F)
    return sense, (None if fin is None else audio)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-W{s[2]}-w{s[3]}")
def test_gpu_equals_the_cpu_backend(torch_dev, gpu, shape):
    """Every shape with four format pairings (every pairing over the shapes), both layouts, the device and the host call."""
    nch, n, W, w, run = shape
    assert set_param(gpu, PARAM_CHDCS_RUN_BLOCKS, run) == 0
    si = SHAPES.index(shape)
    opened = 0
    for ki in range(4):
        combo = COMBOS[(si + 3 * ki) % len(COMBOS)] if ki else (F, F, F)
        ref = cpu_result(nch, n, W, w, 104, combo)
        sense, audio = setup(gpu, nch, n, W, w, 104, combo)
        layout = (si + ki) % 2
        y, sides = run_cuts(torch_dev, gpu, sense, audio, nch, n, [n], combo[2] == S, layout)
        same(y, sides, ref, ("device", shape, combo, layout))
        if ki < 2:
            gpu.resetChannelDcsDecoder()
            o = gpu.channel_dcs_host(sense, audio)
            same(o.pop("out"), [o], ref, ("host", shape, combo))
        opened += int(sides[0]["count"][1:].sum()) if nch > 1 else int(sides[0]["count"].sum())
    if n // (W * B) >= 40:   # long enough for the case's code segments to open a gate
        assert opened > 0


@pytest.mark.parametrize("layout", [ALIGNED, SHIFTED])
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "-".join("n" if v is None else "fs"[v] for v in c))
def test_every_format_pairing_in_both_layouts(torch_dev, gpu, combo, layout):
    nch, n, W, w = 3, 20 * B + 9, 6, W8K
    ref = cpu_result(nch, n, W, w, 104, combo)
    sense, audio = setup(gpu, nch, n, W, w, 104, combo)
    same(*run_cuts(torch_dev, gpu, sense, audio, nch, n, [n], combo[2] == S, layout), ref, (combo, layout))


@pytest.mark.parametrize("ncodes", [1, 64, 65, 128])
def test_tables_of_every_size(torch_dev, gpu, ncodes):
    nch, n, W, w = 5, 36 * B + 3, 6, W8K
    for k, combo in enumerate(((F, F, F), (S, None, None))):
        ref = cpu_result(nch, n, W, w, ncodes, combo)
        sense, audio = setup(gpu, nch, n, W, w, ncodes, combo)
        same(*run_cuts(torch_dev, gpu, sense, audio, nch, n, [n], False, k), ref, (ncodes, combo))
        found = np.concatenate([s["code"] for s in ref[1]])
        assert (found >= -1).all() and (found < ncodes).all()


CUTS = {"edges": lambda n, W: [1, B - 1, 1, B, n - 2 * B - 1], "100": lambda n, W: [100, B, n - B - 100],
        "window": lambda n, W: [W * B - 2, 1, 1, 1, 1, n - W * B - 2]}


@pytest.mark.parametrize("layout", [ALIGNED, SHIFTED])
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_cuts_are_bit_identical(torch_dev, gpu, cut, layout):
    """Cuts at block edges, inside blocks, and one sample at a time over a window's edge."""
    k = 0
    for nch, n, W, w, _ in (SHAPES[4], SHAPES[7], SHAPES[9]):
        combo = COMBOS[(3 * k + layout + 2) % len(COMBOS)]
        k += 1
        cuts = tuple(CUTS[cut](n, W))
        ref = cpu_result(nch, n, W, w, 104, combo, cuts)
        whole = cpu_result(nch, n, W, w, 104, combo)
        if whole[0] is not None:
            np.testing.assert_array_equal(bits(ref[0]), bits(whole[0]))   # the CPU backend's own cut invariance
        assert sum(int(s["count"].sum()) for s in ref[1]) == int(whole[1][0]["count"].sum())   # the counts add up
        sense, audio = setup(gpu, nch, n, W, w, 104, combo)
        y, sides = run_cuts(torch_dev, gpu, sense, audio, nch, n, list(cuts), combo[2] == S, layout)
        same(y, sides, ref, (nch, n, W, combo))


@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[7], SHAPES[9]], ids=lambda s: f"{s[0]}x{s[1]}-w{s[3]}")
def test_bit_identical_for_any_grid_and_run_length(torch_dev, gpu, shape):
    nch, n, W, w, _ = shape
    k = 0
    for cap in (1, 7, 0):
        for run in (1, 8, 33, 0):
            combo = COMBOS[(k * 3 + 2) % len(COMBOS)]
            k += 1
            assert set_param(gpu, PARAM_CHDCS_MAX_WGS, cap) == 0 and set_param(gpu, PARAM_CHDCS_RUN_BLOCKS, run) == 0
            cuts = (100, n - 100)   # the second call starts inside a block, from the carried sums
            ref = cpu_result(nch, n, W, w, 104, combo, cuts)
            sense, audio = setup(gpu, nch, n, W, w, 104, combo)
            y, sides = run_cuts(torch_dev, gpu, sense, audio, nch, n, list(cuts), combo[2] == S, k % 2)
            same(y, sides, ref, (cap, run, combo))
    assert set_param(gpu, PARAM_CHDCS_MAX_WGS, -1) == ERR_ARG and set_param(gpu, PARAM_CHDCS_RUN_BLOCKS, -1) == ERR_ARG
    assert set_param(gpu, PARAM_CHDCS_RUN_BLOCKS, (1 << 20) + 1) == ERR_ARG


@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[7], SHAPES[8], SHAPES[9]], ids=lambda s: f"{s[0]}x{s[1]}-w{s[3]}")
def test_the_ballot_route_gives_the_same_bits(torch_dev, gpu, shape):
    """The windows kernel's other order-free route (ballots and masked popcounts, no atomics), both layouts."""
    nch, n, W, w, run = shape
    assert set_param(gpu, PARAM_CHDCS_BALLOT, 2) == ERR_ARG and set_param(gpu, PARAM_CHDCS_BALLOT, 1) == 0
    assert set_param(gpu, PARAM_CHDCS_RUN_BLOCKS, run) == 0
    for k, combo in enumerate(((F, F, F), (S, None, None), (S, S, S), (F, None, None))):
        cuts = (100, n - 100)
        ref = cpu_result(nch, n, W, w, 104, combo, cuts)
        sense, audio = setup(gpu, nch, n, W, w, 104, combo)
        same(*run_cuts(torch_dev, gpu, sense, audio, nch, n, list(cuts), combo[2] == S, k % 2), ref, (shape, combo))


def test_a_channel_alone_equals_the_channel_among_five(torch_dev, gpu):
    nch, n, W, w, combo = 5, 60 * B + 3, 6, W8K, (F, F, F)
    among = cpu_result(nch, n, W, w, 104, combo)
    sense, audio, cws, params = case(nch, n, W, w, 104, False, False)
    for c in range(nch):
        gpu.setChannelDcsDecoder(cws, params[c:c + 1], w, W, *LIMITS)
        y, sides = run_cuts(torch_dev, gpu, sense[c:c + 1], audio[c:c + 1], 1, n, [n], False)
        np.testing.assert_array_equal(bits(y[0]), bits(among[0][c]))
        for name in SIDES:
            np.testing.assert_array_equal(sides[0][name][0], among[1][0][name][c], err_msg=name)


def test_a_side_stream_equals_the_default_stream(torch_dev, gpu):
    torch = torch_dev
    nch, n, W, w, _ = SHAPES[7]
    combo = (F, F, F)
    ref = cpu_result(nch, n, W, w, 104, combo)
    sense, audio = setup(gpu, nch, n, W, w, 104, combo)
    same(*run_cuts(torch, gpu, sense, audio, nch, n, [n], False), ref)
    gpu.resetChannelDcsDecoder()
    same(*run_cuts(torch, gpu, sense, audio, nch, n, [n], False, streams=[torch.cuda.Stream()]), ref)
    # calls of one stream of samples on alternating streams run in call order
    cuts = (300, 1000, n - 1300)
    gpu.resetChannelDcsDecoder()
    y, sides = run_cuts(torch, gpu, sense, audio, nch, n, list(cuts), False, streams=[torch.cuda.Stream(), torch.cuda.Stream()])
    same(y, sides, cpu_result(nch, n, W, w, 104, combo, cuts))


def test_reset_and_failed_calls(torch_dev, gpu):
    torch = torch_dev
    nch, n, W, w, combo = 3, 60 * B + 3, 6, W8K, (F, F, F)
    ref = cpu_result(nch, n, W, w, 104, combo)
    sense, audio, cws, params = case(nch, n, W, w, 104, False, False)
    _, d_s, s_stride = to_dev(torch, sense, n, ALIGNED)
    _, d_a, a_stride = to_dev(torch, audio, n, ALIGNED)
    f = gpu._L.sddc_ddc_channel_dcs_device
    o = out_tensor(torch, nch, n, ALIGNED, False)
    buf, out, ostride = o[0], o[1], o[2]
    sp, ap, op = d_s.data_ptr(), d_a.data_ptr(), out.data_ptr()
    none = (None,) * 5

    def call(s=sp, ss=s_stride, a=ap, c=nch, m=n, ast=a_stride, out_=op, ost=ostride):
        return f(gpu._h, s, ss, a, c, m, ast, out_, ost, *none)

    assert call() == ERR_STATE                                   # nothing set
    gpu.setChannelDcsDecoder(cws, params, w, W, *LIMITS)
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
    for name in ("code", "open", "info"):
        np.testing.assert_array_equal(sides[0][name], ref[1][0][name], err_msg=name)
    gpu.resetChannelDcsDecoder()   # a new, closed stream
    same(*run_cuts(torch, gpu, sense, audio, nch, n, [n], False), ref)
    gpu.setChannelDcsDecoder(None, None, 0, 0)
    assert call() == ERR_STATE


FA = 125000.0     # the audio rate of the chain below with the ADC at 64 MS/s


@functools.lru_cache(maxsize=None)
def chain_results():
    """Three FM carriers of amplitude 9000 in noise at the centres of three channels 24 bins apart, each modulated
    (600 Hz deviation) by the NRZ stream of code 023 at its own bit offset, a bit being 512 / 3 audio samples (the
    smallest phase word of W = 16): process_channels_device at d = 6 (96 blocks) -> channel_decimate_device (R = 4, 65
    taps) -> channel_demodulate_device (FM) -> channel_audio_filter_device of a second handle (two low-pass sections
    at 2 kHz) -> channel_dcs_device (table 023, 754; the channels set to 023, ANY and 754; eye 128, e = 1, 2, A = 1, H =
    0) gating the demodulator's audio, on one stream; and the same stages of CPU handles fed the DDC's output."""
    import torch
    from extio_sddc_amd import DEVICE_CPU, R2iq, kaiser, output_samples
    from extio_sddc_amd.synth import BLOCK, HALF_FFT
    d, nblk, R, tbs, W = 6, 96, 4, [1000, 1024, 1048], 16
    w = M.smallest_word(W)
    h = kaiser(65, 60.0, 0.08, 0.125)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    n = nsamp // R
    per_audio = BLOCK * nblk // n                      # ADC samples per audio sample
    assert w % per_audio == 0
    cws = np.array([dcs_codeword("023"), dcs_codeword("754")], np.uint32)
    x = np.zeros(nblk * BLOCK)
    for k, tb in enumerate(tbs):
        msg = M.nrz(int(cws[0]), w // per_audio, nblk * BLOCK, offset=0.3 + 5.41 * k)
        x += M.fm(msg, tb / (2.0 * HALF_FFT), 600.0 / (FA * per_audio), 9000.0, phase=1.0 * k)
    x += np.random.default_rng(11).normal(0, 10.0, x.shape[0])
    adc = np.concatenate([np.zeros(HALF_FFT, np.int16), np.clip(np.round(x), -32767, 32767).astype(np.int16)])
    d_in = torch.from_numpy(adc).to("cuda")
    lp = np.tile(biquad(BIQUAD_LOWPASS, 2000.0 / FA), (nch, 2, 1))
    params = np.array([[0, 0, 128], [DCS_ANY, 0, 128], [1, 0, 128]], np.int32)

    def tail(r, r2, iq_host=None):
        r.setChannelDecimator(h, R, nch)
        r.setChannelDemodulator([DEMOD_FM] * nch)
        r2.setChannelAudioFilter(lp)
        r.setChannelDcsDecoder(cws, params, w, W, 1, 2, 1, 0)
        if iq_host is not None:
            a = r.channel_demodulate(r.channel_decimate(iq_host))
            s = r2.channel_audio_filter(a)
            o = r.channel_dcs_host(s, a)
            return a, s, o
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device="cuda")
        z = torch.zeros((nch, 2 * n), dtype=torch.float32, device="cuda")
        a, s = (torch.zeros((nch, n), dtype=torch.float32, device="cuda") for _ in range(2))
        y = torch.full((nch, n), float("nan"), dtype=torch.float32, device="cuda")
        cd, op, cn = (torch.zeros(nch, dtype=torch.int32, device="cuda") for _ in range(3))
        nf = torch.zeros((nch, 4), dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=st)
        r.channel_decimate_device(iq, nch, nsamp, iq.stride(0), z, z.stride(0), stream=st)
        r.channel_demodulate_device(z, nch, n, z.stride(0), a, a.stride(0), stream=st)
        r2.channel_audio_filter_device(a, nch, n, a.stride(0), s, s.stride(0), stream=st)
        r.channel_dcs_device(s, s.stride(0), a, nch, n, a.stride(0), y, y.stride(0), d_code=cd, d_open=op, d_count=cn, d_info=nf,
                             stream=st)
        torch.cuda.synchronize()
        o = {"out": y.cpu().numpy(), "code": cd.cpu().numpy(), "open": op.cpu().numpy().view(np.uint32),
             "count": cn.cpu().numpy().view(np.uint32), "info": nf.cpu().numpy().view(np.uint32)}
        return iq.cpu().numpy(), a.cpu().numpy(), s.cpu().numpy(), o

    with R2iq(gain=1.0) as r, R2iq(gain=1.0) as r2:
        r.setDecimate(d)
        dev = tail(r, r2)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c, R2iq(gain=1.0, device=DEVICE_CPU) as c2:
        cpu = tail(c, c2, np.ascontiguousarray(dev[0]).view(np.complex64))
    return dev, cpu, n, W


def test_ddc_to_dcs_decoder_on_one_stream(torch_dev):
    """The chain of chain_results: the device chain's audio, sense stream, gated audio and side outputs are the CPU
    chain's bit for bit; the channels set to 023 and to ANY report index 0 without a bit error and are open from
    their third window at the latest, the channel set to 754 reports -1 and stays closed (+0)."""
    dev, cpu, n, W = chain_results()
    _, a, s, o = dev
    assert n == 3 * W * B
    np.testing.assert_array_equal(bits(a), bits(cpu[0]))
    np.testing.assert_array_equal(bits(s), bits(cpu[1]))
    for name in ("out",) + SIDES:
        np.testing.assert_array_equal(bits(o[name]), bits(cpu[2][name]), err_msg=name)
    q, nn, dd, tt = (o["info"][:, k].astype(np.int64) for k in range(4))
    print(f"code {o['code']}, open {o['open']}, count {o['count']}, Q {q}, N {nn}, d {dd}, t {tt}, 256 Q / N {256 * q // nn}")
    assert list(o["code"]) == [0, 0, -1] and list(o["open"]) == [1, 1, 0]
    assert list(dd[:2]) == [0, 0] and dd[2] > 3 and (256 * q >= 192 * nn).all()
    # window 0 holds the chain's start-up transient; window 1 is clean, so window 2 is open on channels 0 and 1
    assert o["count"][0] in (W * B, 2 * W * B) and o["count"][1] in (W * B, 2 * W * B) and o["count"][2] == 0
    assert (bits(o["out"][2]) == 0).all()
    np.testing.assert_array_equal(bits(o["out"][:2, 2 * W * B:]), bits(a[:2, 2 * W * B:]))
