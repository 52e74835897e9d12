"""The channel audio resampler on the GPU (pytest -m gpu): sddc_ddc_channel_audio_resample_device and
sddc_ddc_channel_audio_resample_host of a GPU handle bit for bit against the CPU backend (which
tests/test_channel_audio_resample_cpu.py pins to the definition's numpy model exactly), an independent
cross-check against the device IQ resampler on the stream (x, 0), the bit-exact properties of the fixed
summation order, a change of the formats between two device calls of one stream, and the chain DDC -> decimator -> FM demodulator -> audio resampler -> tone detector on
one stream.

Ratios (L, M, ntaps): 1/6 x 97, 1/4 x 65, 24/125 x 1536, 2/3 x 40, 3/2 x 7, 32/1 x 100, 1/256 x 300, 5/7 x 4
(K = 1) and 3/250 x 3072 (K = 1024); the four format pairs F32 / S16 in and out.
Shapes (nch, nsamp), with K = ceil(ntaps / L): (1, 1); (1, K - 1), shorter than the tail; (1, 32 M + 3), half
a wave unit and a ragged end; (3, 128 M + 17), other data per channel; (1024, 2); and, at M = 125 and M = 1,
two tiles and a bit, the tile's length taken from sddc_ddc_internal_chars_layout.
Layout of every device call: d_in starts 3 samples into a tensor poisoned with NaN (S16: 0x7fff) and
d_out 1 sample into one poisoned with NaN (S16: a sentinel); the channels' strides are odd, so their
bases take every alignment modulo 16 bytes; the gaps between the streams are poisoned too, and the
heads, tails and gaps of d_out must come back untouched.
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


AM = _load("channel_audio_resample_model")

F, S = 0, 1                      # AUDIO_F32, AUDIO_S16
FORMATS = [(F, F), (F, S), (S, F), (S, S)]
FMT_IDS = ["f32-f32", "f32-s16", "s16-f32", "s16-s16"]
RATIOS = [(1, 6, 97), (1, 4, 65), (24, 125, 1536), (2, 3, 40), (3, 2, 7), (32, 1, 100), (1, 256, 300), (5, 7, 4),
          (3, 250, 3072)]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
PARAM_CHARS_MAX_WGS = 30         # sddc_ddc_internal.h
ERR_ARG, ERR_STATE = -1, -4
STEP_LIMIT_S = 60
IN_HEAD, OUT_HEAD = 3, 1         # samples before d_in / d_out in their poisoned tensors
SENTINEL = -21555                # the S16 output poison


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


@pytest.fixture(scope="module")
def cpu():
    from extio_sddc_amd import DEVICE_CPU, R2iq
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


@functools.lru_cache(maxsize=None)
def signal(nch, nsamp, fmt):
    x = AM.make_input("noise", nch, nsamp, fmt)
    x.setflags(write=False)
    return x


def taps_for(ntaps, fout):
    return AM.make_taps(ntaps) * np.float32(0.25 if fout == S else 1.0)


def layout_of(L, M, ntaps, in_s16):
    """(values of a per tile, LDS slots, pitch, store cycles) of the kernel's tile."""
    from extio_sddc_amd import _lib
    f = _lib.load().sddc_ddc_internal_chars_layout
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)] * 4
    v = [ctypes.c_int() for _ in range(4)]
    assert f(L, M, ntaps, in_s16, *[ctypes.byref(c) for c in v]) == 0
    return tuple(c.value for c in v)


def odd(n):
    return n | 1


def dev_input(torch, x, stride):
    """x [nch, nsamp] on the device at `stride` samples per channel, IN_HEAD samples into a poisoned tensor."""
    nch, nsamp = x.shape
    poison = 0x7fff if x.dtype == np.int16 else np.nan
    buf = np.full(IN_HEAD + (nch - 1) * stride + nsamp + 5, poison, x.dtype)
    for c in range(nch):
        buf[IN_HEAD + c * stride:IN_HEAD + c * stride + nsamp] = x[c]
    return torch.from_numpy(buf).to("cuda")[IN_HEAD:]


def out_tensor(torch, nch, nout, stride, fout):
    """(the poisoned tensor, d_out OUT_HEAD samples into it)."""
    n = OUT_HEAD + (nch - 1) * stride + nout + 7
    if fout == S:
        buf = torch.full((n,), SENTINEL, dtype=torch.int16, device="cuda")
    else:
        buf = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[OUT_HEAD:]


def collect(buf, nch, nout, stride, fout):
    """[nch, nout] of finished calls; the head, the tail and the gaps must still hold the poison."""
    y = buf.cpu().numpy()
    untouched = (lambda v: (v == SENTINEL).all()) if fout == S else (lambda v: np.isnan(v).all())
    out = np.empty((nch, nout), y.dtype)
    at = OUT_HEAD
    assert untouched(y[:at])
    for c in range(nch):
        out[c] = y[at:at + nout]
        nxt = OUT_HEAD + (c + 1) * stride if c + 1 < nch else y.size
        assert untouched(y[at + nout:nxt]), f"the gap after channel {c} was written"
        at = nxt
    return out


def same(y, ref, what=""):
    assert y.dtype == ref.dtype and y.shape == ref.shape, what
    if y.dtype == np.float32:
        y, ref = np.ascontiguousarray(y).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)
    np.testing.assert_array_equal(y, ref, err_msg=what)


def run_device(torch, r, x, lm, cuts=None, streams=None, pos=0):
    """The stream x [nch, nsamp], whose first sample is stream sample `pos` of the ratio lm = (L, M), through
    channel_audio_resample_device in calls of `cuts` samples (one call by default), every call writing behind
    the one before into one poisoned buffer; nothing synchronises between the calls.  -> [nch, total outputs]."""
    nch, nsamp = x.shape
    fout = r._aresamp[2]
    cuts = [nsamp] if cuts is None else cuts
    assert sum(cuts) == nsamp
    in_stride = odd(nsamp + 5) if nch > 1 else 0
    d_in = dev_input(torch, x, in_stride)
    total = AM.count(lm[0], lm[1], pos, nsamp)
    out_stride = odd(total + 4) if nch > 1 else 0
    buf, d_out = out_tensor(torch, nch, total, out_stride, fout)
    torch.cuda.synchronize()   # the fills are done before a call on another stream writes
    at = done = 0
    for k, n in enumerate(cuts):
        s = streams[k % len(streams)] if streams else None
        done += r.channel_audio_resample_device(d_in[at:], nch, n, in_stride, d_out[done:], out_stride, stream=s)
        at += n
    torch.cuda.synchronize()
    assert done == total
    return collect(buf, nch, total, out_stride, fout)


def setup(r, h, L, M, nch, fin, fout):
    r.setChannelAudioResampler(h, L, M, nch, fin, fout)


def cpu_ref(cpu, x, h, L, M, fin, fout):
    cpu.setChannelAudioResampler(h, L, M, x.shape[0], fin, fout)
    return cpu.channel_audio_resample_host(x)


def shapes_of(L, M, ntaps):
    K = -(-ntaps // L)
    s = [(1, 1), (1, 32 * M + 3), (3, 128 * M + 17), (1024, 2)]
    if K > 1:
        s.insert(1, (1, K - 1))
    return s


@pytest.mark.parametrize("fmts", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("ratio", RATIOS, ids=IDS)
def test_gpu_equals_the_cpu_backend(torch_dev, gpu, cpu, ratio, fmts):
    L, M, ntaps = ratio
    fin, fout = fmts
    h = taps_for(ntaps, fout)
    for nch, nsamp in shapes_of(L, M, ntaps):
        x = signal(nch, nsamp, fin)
        ref = cpu_ref(cpu, x, h, L, M, fin, fout)
        assert ref.shape == (nch, AM.count(L, M, 0, nsamp))
        setup(gpu, h, L, M, nch, fin, fout)
        same(run_device(torch_dev, gpu, x, (L, M)), ref, f"device {nch} x {nsamp}")
        gpu.channel_audio_resampler_reset()
        same(gpu.channel_audio_resample_host(x), ref, f"host {nch} x {nsamp}")
        if nch == 3:
            assert np.abs(ref.astype(np.float64)).max() > 0 and not np.array_equal(ref[0], ref[1])


@pytest.mark.parametrize("fmts", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("ratio", [(24, 125, 1536), (32, 1, 100)], ids=IDS)
def test_more_than_one_tile_per_channel(torch_dev, gpu, cpu, ratio, fmts):
    """Two tiles and a bit per channel, the tile from the kernel's constants; a second call continues the
    stream from the tails the last tile wrote; the host call shares the state."""
    L, M, ntaps = ratio
    fin, fout = fmts
    ta = layout_of(L, M, ntaps, int(fin == S))[0]
    nsamp = 2 * ta * M + 3 * M + 5
    h = taps_for(ntaps, fout)
    x = signal(2, 2 * nsamp, fin)
    ref = cpu_ref(cpu, x, h, L, M, fin, fout)
    assert -(-AM.count(L, M, 0, nsamp) // L) > 2 * ta
    setup(gpu, h, L, M, 2, fin, fout)
    same(run_device(torch_dev, gpu, x, (L, M), cuts=[nsamp, nsamp]), ref)
    setup(gpu, h, L, M, 2, fin, fout)
    first = gpu.channel_audio_resample_host(np.ascontiguousarray(x[:, :nsamp]))
    second = run_device(torch_dev, gpu, np.ascontiguousarray(x[:, nsamp:]), (L, M), pos=nsamp)
    same(np.concatenate([first, second], axis=1), ref)


@pytest.mark.parametrize("ratio", RATIOS, ids=IDS)
def test_f32_equals_the_real_part_of_the_iq_resampler_on_x_0(torch_dev, gpu, ratio):
    """The device IQ resampler runs the same fixed order on float2: on the CF32 stream (x, 0), with the same
    taps and ratio, its real part is this stage's output bit for bit and its imaginary part is zero."""
    torch = torch_dev
    L, M, ntaps = ratio
    nch, nsamp = 3, 128 * M + 17
    h = AM.make_taps(ntaps)
    x = signal(nch, nsamp, F)
    setup(gpu, h, L, M, nch, F, F)
    y = run_device(torch, gpu, x, (L, M))
    gpu.setChannelResampler(h, L, M, nch)
    iq = np.zeros((nch, 2 * nsamp), np.float32)
    iq[:, 0::2] = x
    nout = gpu.channel_resample_samples(nsamp)
    assert nout == y.shape[1]
    d_out = torch.full((nch, 2 * nout), float("nan"), dtype=torch.float32, device="cuda")
    assert gpu.channel_resample_device(torch.from_numpy(iq).to("cuda"), nch, nsamp, 2 * nsamp, d_out, 2 * nout) == nout
    torch.cuda.synchronize()
    z = d_out.cpu().numpy()
    same(np.ascontiguousarray(z[:, 0::2]), y)
    assert (z[:, 1::2] == 0).all()


@pytest.mark.parametrize("fmts", [FORMATS[0], FORMATS[3]], ids=[FMT_IDS[0], FMT_IDS[3]])
@pytest.mark.parametrize("ratio", [(1, 6, 97), (24, 125, 1536), (3, 250, 3072)], ids=IDS)
def test_cuts_are_bit_identical(torch_dev, gpu, cpu, ratio, fmts):
    """One call against [1, 1, K - 2, K, rest], [100, M, rest] and a cut at every tile boundary - 1, + 0, + 1."""
    L, M, ntaps = ratio
    fin, fout = fmts
    K = -(-ntaps // L)
    T = layout_of(L, M, ntaps, int(fin == S))[0] * M   # samples per tile
    nsamp = 2 * T + 2 * K + M + 110
    h = taps_for(ntaps, fout)
    x = signal(2, nsamp, fin)
    setup(gpu, h, L, M, 2, fin, fout)
    whole = run_device(torch_dev, gpu, x, (L, M))
    same(whole, cpu_ref(cpu, x, h, L, M, fin, fout))
    for cuts in ([1, 1, K - 2, K], [100, M], [T - 1, 1, 1, T - 2, 1, 1]):
        gpu.channel_audio_resampler_reset()
        same(run_device(torch_dev, gpu, x, (L, M), cuts=cuts + [nsamp - sum(cuts)]), whole, str(cuts))


@pytest.mark.parametrize("fmts", [FORMATS[0], FORMATS[3]], ids=[FMT_IDS[0], FMT_IDS[3]])
def test_bit_identical_for_any_grid(torch_dev, gpu, fmts):
    """9 items (3 channels x 3 tiles) at 24/125: capped at 1 a workgroup takes 9 rounds, at 3 three."""
    L, M, ntaps = 24, 125, 1536
    fin, fout = fmts
    f = gpu._L.sddc_ddc_internal_set_param
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    ta = layout_of(L, M, ntaps, int(fin == S))[0]
    nsamp = 2 * ta * M + 3 * M + 5
    h = taps_for(ntaps, fout)
    x = signal(3, nsamp, fin)
    outs = []
    for cap in (0, 1, 3):
        assert f(gpu._h, PARAM_CHARS_MAX_WGS, cap) == 0
        setup(gpu, h, L, M, 3, fin, fout)
        outs.append(run_device(torch_dev, gpu, x, (L, M), cuts=[nsamp // 2, nsamp - nsamp // 2]))   # the tails too
    assert f(gpu._h, PARAM_CHARS_MAX_WGS, -1) == ERR_ARG
    assert f(gpu._h, PARAM_CHARS_MAX_WGS, 0) == 0
    for o in outs[1:]:
        same(o, outs[0])


def test_two_streams_back_to_back_equal_the_two_call_cut(torch_dev, gpu):
    """A call on a side stream and a call on the default stream, issued without a sync between them: the
    second waits for the first, whose tails it reads."""
    torch = torch_dev
    L, M, ntaps = 1, 6, 97
    h = AM.make_taps(ntaps)
    x = signal(3, 128 * M + 17, F)
    cuts = [x.shape[1] // 2 + 3, x.shape[1] - x.shape[1] // 2 - 3]
    setup(gpu, h, L, M, 3, F, F)
    whole = run_device(torch, gpu, x, (L, M))
    side = torch.cuda.Stream()
    for streams in (None, [side, torch.cuda.current_stream()], [torch.cuda.current_stream(), side]):
        gpu.channel_audio_resampler_reset()
        same(run_device(torch, gpu, x, (L, M), cuts=cuts, streams=streams), whole)


@pytest.mark.parametrize("fmts", [FORMATS[0], FORMATS[3]], ids=[FMT_IDS[0], FMT_IDS[3]])
def test_a_channel_alone_equals_the_channel_among_three(torch_dev, gpu, fmts):
    L, M, ntaps = 24, 125, 1536
    fin, fout = fmts
    h = taps_for(ntaps, fout)
    x = signal(3, 128 * M + 17, fin)
    setup(gpu, h, L, M, 3, fin, fout)
    among = run_device(torch_dev, gpu, x, (L, M))
    setup(gpu, h, L, M, 1, fin, fout)
    same(run_device(torch_dev, gpu, np.ascontiguousarray(x[1:2]), (L, M))[0], among[1])


def test_the_formats_may_switch_between_two_device_calls(torch_dev, gpu, cpu):
    """The device tails hold values: integer-valued samples fed as F32, then as S16 (with S16 out), then as F32
    again, each a device call of one stream, give the one-format stream's bits (S16 out: its rounded values)."""
    L, M, ntaps = 1, 4, 65
    h = taps_for(ntaps, S)
    xs = signal(3, 128 * M + 17, S)
    xf = xs.astype(np.float32)
    a, b = 2 * M + 3, 70 * M + 1
    whole = cpu_ref(cpu, xf, h, L, M, F, F)
    setup(gpu, h, L, M, 3, F, F)
    first = run_device(torch_dev, gpu, np.ascontiguousarray(xf[:, :a]), (L, M))
    gpu.setChannelAudioResamplerFormats(S, S)
    second = run_device(torch_dev, gpu, np.ascontiguousarray(xs[:, a:b]), (L, M), pos=a)
    gpu.setChannelAudioResamplerFormats(F, F)
    third = run_device(torch_dev, gpu, np.ascontiguousarray(xf[:, b:]), (L, M), pos=b)
    n1, n2 = first.shape[1], second.shape[1]
    same(first, np.ascontiguousarray(whole[:, :n1]))
    same(second, AM.to_s16(whole[:, n1:n1 + n2]))
    same(third, np.ascontiguousarray(whole[:, n1 + n2:]))


def test_error_returns_and_a_failed_call_changes_no_state(torch_dev, gpu):
    from extio_sddc_amd import DDCError
    torch = torch_dev
    dev = gpu._L.sddc_ddc_channel_audio_resample_device
    nch, L, M, ntaps, nsamp = 3, 3, 7, 20, 40
    h = AM.make_taps(ntaps)
    x = signal(nch, nsamp, F)
    S_ = odd(nsamp + 5)
    d_in = dev_input(torch, x, S_)
    nout = AM.count(L, M, 0, nsamp)
    OS = odd(nout + 4)
    buf, d_out = out_tensor(torch, nch, nout, OS, F)
    xi, oi = d_in.data_ptr(), d_out.data_ptr()
    got = ctypes.c_size_t(99)
    gp = ctypes.addressof(got)
    assert dev(gpu._h, xi, nch, nsamp, S_, oi, OS, gp, None) == ERR_STATE              # nothing set
    with pytest.raises(DDCError):
        gpu.channel_audio_resample_device(d_in, nch, nsamp, S_, d_out, OS)
    setup(gpu, h, L, M, nch, F, F)
    good = run_device(torch, gpu, x, (L, M))
    gpu.channel_audio_resampler_reset()
    assert dev(gpu._h, xi, nch - 1, nsamp, S_, oi, OS, gp, None) == ERR_STATE          # another nch than the set one
    assert dev(gpu._h, xi, nch, 0, S_, oi, OS, gp, None) == ERR_ARG
    assert dev(gpu._h, xi, nch, nsamp, nsamp - 1, oi, OS, gp, None) == ERR_ARG
    assert dev(gpu._h, xi, nch, nsamp, S_, oi, nout - 1, gp, None) == ERR_ARG
    assert dev(gpu._h, xi + 2, nch, nsamp, S_, oi, OS, gp, None) == ERR_ARG            # F32: 4-byte samples
    assert dev(gpu._h, xi, nch, nsamp, S_, oi + 2, OS, gp, None) == ERR_ARG
    assert dev(gpu._h, None, nch, nsamp, S_, oi, OS, gp, None) == ERR_ARG
    assert dev(gpu._h, xi, nch, nsamp, S_, None, OS, gp, None) == ERR_ARG
    with pytest.raises(DDCError):
        gpu.channel_audio_resample_device(d_in, nch, nsamp, S_, d_out[:OS], OS)        # d_out too small
    with pytest.raises(DDCError):
        gpu.channel_audio_resample_device(d_in.to(torch.int16), nch, nsamp, S_, d_out, OS)   # wrong dtype
    torch.cuda.synchronize()
    assert got.value == 99 and torch.isnan(buf).all()
    assert gpu.channel_audio_resample_samples(nsamp) == nout
    assert dev(gpu._h, xi, nch, nsamp, S_, oi, OS, gp, None) == 0 and got.value == nout
    torch.cuda.synchronize()
    same(collect(buf, nch, nout, OS, F), good)


@functools.lru_cache(maxsize=None)
def chain_results():
    """An NBFM carrier of amplitude 12000 in noise at the centre of the first of two channels, modulated by
    a 254.1 Hz sub-tone (600 Hz deviation), and an unmodulated one in the second: process_channels_device at
    d = 6 (48 blocks) -> channel_decimate_device (R = 4, 65 taps) -> channel_demodulate_device (FM) ->
    channel_audio_resample_device (1/4, a 65-tap Kaiser low-pass: the 31.25 kS/s sense stream) ->
    channel_tone_device (three tones, W = 2, detect only), on one stream; and the same stages of a CPU
    handle fed the DDC's output."""
    import torch
    from extio_sddc_amd import DEMOD_FM, DEVICE_CPU, R2iq, kaiser, output_samples, tone_word
    from extio_sddc_amd.synth import BLOCK, HALF_FFT
    d, nblk, R, tbs, W = 6, 48, 4, [1000, 1024], 2
    fa = 125000.0
    h = kaiser(65, 60.0, 0.08, 0.125)
    ha = kaiser(65, 60.0, 0.04, 0.125)
    nsamp, nch = output_samples(d, nblk), len(tbs)
    n = nsamp // R
    m = n // 4
    fadc = fa * R * 128
    t = np.arange(nblk * BLOCK, dtype=np.float64)
    sub = (600.0 / 254.1) * np.sin(2 * np.pi * 254.1 / fadc * t)
    x = 12000.0 * np.cos(2 * np.pi * tbs[0] / (2 * HALF_FFT) * t + sub)
    x += 12000.0 * np.cos(2 * np.pi * tbs[1] / (2 * HALF_FFT) * t + 1.0)
    x += np.random.default_rng(11).normal(0, 10.0, x.shape[0])
    adc = np.concatenate([np.zeros(HALF_FFT, np.int16), np.clip(np.round(x), -32767, 32767).astype(np.int16)])
    d_in = torch.from_numpy(adc).to("cuda")
    words = [tone_word(f, fa / 4) for f in (67.0, 151.4, 254.1)]
    masks = np.full(nch, (1 << len(words)) - 1, np.uint64)
    thr = np.tile(np.float32([0.2, 0.1, 0.0]), (nch, 1))

    def tail(r, iq_host=None):
        r.setChannelDecimator(h, R, nch)
        r.setChannelDemodulator([DEMOD_FM] * nch)
        r.setChannelAudioResampler(ha, 1, 4, nch)
        r.setChannelToneDetector(words, masks, thr, W, 1, 0)
        if iq_host is not None:
            z = r.channel_decimate(iq_host)
            a = r.channel_demodulate(z)
            s = r.channel_audio_resample_host(a)
            o = r.channel_tone(s)
            return z, a, s, {k: o[k] for k in ("tone", "open", "level", "powers")}
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device="cuda")
        z = torch.zeros((nch, 2 * n), dtype=torch.float32, device="cuda")
        a = torch.zeros((nch, n), dtype=torch.float32, device="cuda")
        s = torch.full((nch, m), float("nan"), dtype=torch.float32, device="cuda")
        tn, op = (torch.zeros(nch, dtype=torch.int32, device="cuda") for _ in range(2))
        lv = torch.zeros((nch, 2), dtype=torch.float32, device="cuda")
        pw = torch.zeros((nch, len(words)), dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        r.process_channels_device(d_in, nblk, tbs, iq, stream=st)
        r.channel_decimate_device(iq, nch, nsamp, iq.stride(0), z, z.stride(0), stream=st)
        r.channel_demodulate_device(z, nch, n, z.stride(0), a, a.stride(0), stream=st)
        assert r.channel_audio_resample_device(a, nch, n, a.stride(0), s, s.stride(0), stream=st) == m
        r.channel_tone_device(s, s.stride(0), None, nch, m, 0, None, 0, d_tone=tn, d_open=op, d_level=lv, d_powers=pw,
                              stream=st)
        torch.cuda.synchronize()
        o = {"tone": tn.cpu().numpy(), "open": op.cpu().numpy().view(np.uint32), "level": lv.cpu().numpy(),
             "powers": pw.cpu().numpy()}
        return iq.cpu().numpy(), z.cpu().numpy(), a.cpu().numpy(), s.cpu().numpy(), o

    with R2iq(gain=1.0) as r:
        r.setDecimate(d)
        dev = tail(r)
    with R2iq(gain=1.0, device=DEVICE_CPU) as c:
        host = tail(c, np.ascontiguousarray(dev[0]).view(np.complex64))
    return dev[1:], host, m, W


def test_ddc_to_tone_detector_through_the_audio_resampler_on_one_stream(torch_dev):
    """The chain of chain_results: every stage's output after the DDC is the CPU chain's bit for bit; the
    channel with the sub-tone has most of its sense stream's energy in tone 2 (254.1 Hz)."""
    dev, host, m, W = chain_results()
    assert m == 3 * W * 256
    same(dev[0].view(np.uint32), np.ascontiguousarray(host[0]).view(np.float32).view(np.uint32), "decimator")
    same(dev[1], host[1], "demodulator")
    same(dev[2], host[2], "audio resampler")
    for name in ("tone", "open", "level", "powers"):
        same(np.ascontiguousarray(dev[3][name]).view(np.uint32), np.ascontiguousarray(host[3][name]).view(np.uint32), name)
    print(f"tone {dev[3]['tone']}, open {dev[3]['open']}, powers {dev[3]['powers']}, level {dev[3]['level']}")
    assert np.isfinite(dev[2]).all() and np.abs(dev[2][0]).max() > 0
    assert int(np.argmax(dev[3]["powers"][0])) == 2 and dev[3]["tone"][0] == 2
