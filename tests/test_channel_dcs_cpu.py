"""The channel DCS decoder without a GPU: the stateless helpers (sddc_ddc_dcs_codeword, sddc_ddc_dcs_window, the
104 standard codes), and the CPU backend's sddc_ddc_channel_dcs_host against the numpy model of the definition
(tools/channel_dcs_model.py).  Every comparison is an exact integer or bitwise one: after the sign test the
definition holds integers alone, so no tolerance appears anywhere.
"""
from __future__ import annotations

import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load("channel_dcs_model")

from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, DCS_ANY, DCS_BLOCK, DCS_CODES, DCS_OFF, DEVICE_CPU, DDCError, R2iq,  # noqa: E402
                            dcs_codeword, dcs_window, load)

B = DCS_BLOCK
ERR_ARG, ERR_STATE = -1, -4
F, S = AUDIO_F32, AUDIO_S16
W8K = 72155451                  # 134.4 bit/s at 8 kS/s
WMAX = 1 << 29                  # a bit of 8 samples
# (sense, audio in, audio out; None: detect only): every pairing
COMBOS = [(F, None, None), (S, None, None), (F, F, F), (F, F, S), (F, S, F), (F, S, S), (S, F, F), (S, F, S), (S, S, F), (S, S, S)]
SIDES = ("code", "open", "count", "info")


@pytest.fixture()
def cpu():
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        yield r


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.uint32) if y.dtype == np.float32 else y


def model_sides(m, a, b):
    return {"code": M.code_at(m, b), "open": M.open_at(m, b), "count": M.count(m, a, b), "info": M.info_at(m, b)}


def run_cpu(r, sense, audio, cuts):
    ys, sides, at = [], [], 0
    for ln in cuts:
        o = r.channel_dcs_host(sense[:, at:at + ln], None if audio is None else audio[:, at:at + ln])
        ys.append(o.pop("out"))
        sides.append(o)
        at += ln
    return (None if audio is None else np.concatenate(ys, axis=1)), sides


def check_against_model(r, sense, audio, cws, params, w, W, eo, ec, A, H, combo, cuts=None, what=None):
    fs, fin, fout = combo
    n = sense.shape[1]
    cuts = list(cuts or [n])
    r.setChannelDcsDecoder(cws, params, w, W, eo, ec, A, H, fs, fin or F, fout or F)
    m = M.definition(sense, audio if fin is not None else None, cws, params, w, W, eo, ec, A, H, fout or F)
    y, sides = run_cpu(r, sense, audio if fin is not None else None, cuts)
    if fin is None:
        assert y is None
    else:
        assert y.dtype == m["y"].dtype
        np.testing.assert_array_equal(bits(y), bits(m["y"]), err_msg=str(what))
    at = 0
    for ln, sd in zip(cuts, sides):
        ref = model_sides(m, at, at + ln)
        for name in SIDES:
            np.testing.assert_array_equal(sd[name], ref[name], err_msg=f"{name} {what} ending at {at + ln}")
        at += ln
    return m


@functools.lru_cache(maxsize=None)
def case(nch, n, W, w, ncodes, sense16, in16):
    arrs = M.make_case(nch, n, W, w, ncodes, sense16, in16)
    for a in arrs:
        a.setflags(write=False)
    return arrs


# ---- the helpers ---------------------------------------------------------------------------------
def test_the_codeword_of_023():
    assert dcs_codeword("023") == 0x763813 == dcs_codeword(0o023) == M.codeword("023")
    for c in range(512):
        assert dcs_codeword(c) == M.codeword(c)
    cw = np.zeros(1, np.uint32)
    L = load()
    assert L.sddc_ddc_dcs_codeword(-1, cw.ctypes.data) == ERR_ARG and L.sddc_ddc_dcs_codeword(512, cw.ctypes.data) == ERR_ARG
    assert L.sddc_ddc_dcs_codeword(19, None) == ERR_ARG


def test_the_four_facts_of_the_standard_codes():
    """No codeword of the list is a rotation of another; any rotations of two different ones differ in at least
    7 bits; a codeword and its own rotations in at least 8; the complement of each is a rotation of another one
    of the list (023 inverted is 047).  Hence e <= 3 is unambiguous under ANY and invert is a setting."""
    assert len(DCS_CODES) == 104 == len(set(DCS_CODES)) and DCS_CODES == M.DCS_CODES
    cws = [dcs_codeword(c) for c in DCS_CODES]
    rots = [M.rotations(c) for c in cws]
    owner = {}
    for i, rr in enumerate(rots):
        for r in rr:
            assert owner.setdefault(r, i) == i, "a rotation of another codeword of the list"
    allr = np.array(rots, np.uint32)                                # [104, 23]
    dmin, dself = 23, 23
    for i, c in enumerate(cws):
        d = M.popcount(np.uint32(c) ^ allr)                         # [104, 23]: rotating one of a pair covers both
        dself = min(dself, int(d[i, 1:].min()))
        dmin = min(dmin, int(np.delete(d, i, axis=0).min()))
    assert dmin == 7 and dself == 8
    for i, c in enumerate(cws):
        assert owner.get(c ^ M.MASK, i) != i, "the complement is no rotation of another codeword of the list"
    assert DCS_CODES[owner[cws[0] ^ M.MASK]] == "047"
    # the codewords of all 512 codes (unrotated) differ in at least 7 bits: the (23, 12) code's minimum distance
    allw = np.array([M.codeword(c) for c in range(512)], np.uint32)
    assert min(int(M.popcount(np.uint32(a) ^ allw)[np.arange(512) != i].min()) for i, a in enumerate(allw)) >= 7


def test_dcs_window_values_and_errors():
    assert dcs_window(8000.0) == (W8K, 6) == M.window(8000.0)
    assert dcs_window(48000.0) == (12025908, 34) == M.window(48000.0)
    assert dcs_window(8.0, 1.0) == (WMAX, 1)                          # the largest word: 192 sub-bins in 256 samples
    assert dcs_window(65536.0 * 4, 96.0) == (M.smallest_word(256), 256)
    for fs, br in ((8000.0, 1001.0), (8000.0, 0.0), (0.0, 134.4), (-1.0, 134.4), (np.nan, 134.4), (8000.0, np.inf),
                   (1e12, 134.4), (65536.0 * 4, 95.0)):
        with pytest.raises(DDCError) as e:
            dcs_window(fs, br)
        assert e.value.code == ERR_ARG, (fs, br)
    w = np.zeros(1, np.uint32)
    b = np.zeros(1, np.int32)
    assert load().sddc_ddc_dcs_window(8000.0, 134.4, None, b.ctypes.data) == ERR_ARG
    assert load().sddc_ddc_dcs_window(8000.0, 134.4, w.ctypes.data, None) == ERR_ARG


# ---- the definition ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,W", [(WMAX, 1), (WMAX, 6), (W8K, 6), (M.smallest_word(256), 256)], ids=["2^29-W1", "2^29-W6", "8k", "W256"])
def test_the_sliding_sums_equal_the_floor_form(w, W):
    """c[t][b] from the sub-bins equals the sum of s over floor((w n - t 2^29) / 2^32) = b, and N[t] counts those n."""
    rng = np.random.default_rng(W)
    s = rng.integers(-1, 2, W * B)
    c = M.bit_sums(M.subbin_sums(s[None, :], w, W))[0, 0]
    np.testing.assert_array_equal(c, M.bit_sums_direct(s, w, W))
    np.testing.assert_array_equal(M.counts(w, W), M.bit_sums_direct(np.ones(W * B, np.int64), w, W).sum(axis=1))
    assert M.counts(w, W).max() <= W * B and M.counts(w, W).min() >= 184


def test_argument_errors(cpu):
    cws = M.table(4)
    good = np.array([[0, 0, 128], [DCS_ANY, 1, 0], [DCS_OFF, 0, 256]], np.int32)
    f = cpu._L.sddc_ddc_set_channel_dcs_decoder

    def call(cw=cws, n=4, p=good, c=3, w=W8K, W=6, rest=(1, 2, 1, 0, 0, 0, 0)):
        p = np.ascontiguousarray(p, np.int32)
        cw = np.ascontiguousarray(cw, np.uint32)
        return f(cpu._h, cw.ctypes.data, n, p.ctypes.data, c, w, W, *rest)

    assert cpu._L.sddc_ddc_channel_dcs_reset(cpu._h) == ERR_STATE          # nothing set
    with pytest.raises(DDCError) as ex:
        cpu.channel_dcs_host(np.zeros((3, 10), np.float32))
    assert ex.value.code == ERR_STATE
    assert call() == 0
    assert call(n=0) == ERR_ARG and call(n=129) == ERR_ARG and call(c=-1) == ERR_ARG and call(c=1025) == ERR_ARG
    assert call(w=0) == ERR_ARG and call(w=WMAX + 1) == ERR_ARG
    assert call(W=0) == ERR_ARG and call(W=257) == ERR_ARG and call(W=5) == ERR_ARG        # 5 blocks hold fewer than 24 bits
    assert call(w=M.smallest_word(256) - 1, W=256) == ERR_ARG and call(w=M.smallest_word(256), W=256) == 0
    for col, bad in ((0, (4, -3, 128)), (1, (-1, 2)), (2, (-1, 257))):
        for v in bad:
            p = good.copy()
            p[1, col] = v
            assert call(p=p) == ERR_ARG, (col, v)
    assert call(cw=np.array([1 << 23, 1, 2, 3])) == ERR_ARG
    for rest in ((-1, 2, 1, 0, 0, 0, 0), (2, 1, 1, 0, 0, 0, 0), (0, 4, 1, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0, 0), (1, 2, 256, 0, 0, 0, 0),
                 (1, 2, 1, -1, 0, 0, 0), (1, 2, 1, 65536, 0, 0, 0), (1, 2, 1, 0, 2, 0, 0), (1, 2, 1, 0, 0, -1, 0), (1, 2, 1, 0, 0, 0, 7)):
        assert call(rest=rest) == ERR_ARG, rest
    assert call(rest=(0, 0, 255, 65535, 1, 1, 1)) == 0 and call(rest=(3, 3, 1, 0, 0, 0, 0)) == 0
    # a failed set call sets nothing: the stage is as the last good call left it
    assert call(n=0) == ERR_ARG and cpu._L.sddc_ddc_channel_dcs_reset(cpu._h) == 0
    with pytest.raises(DDCError):
        cpu.setChannelDcsDecoder(cws, good[:, :2], W8K, 6)
    cpu.setChannelDcsDecoder(None, None, 0, 0)                                 # off
    assert cpu._L.sddc_ddc_channel_dcs_reset(cpu._h) == ERR_STATE


def test_call_errors_change_no_state(cpu):
    nch, n, W, w = 2, 7 * B + 5, 6, W8K
    sense, audio, cws, params = case(nch, 2 * n, W, w, 8, False, False)
    f = cpu._L.sddc_ddc_channel_dcs_host
    s = np.ascontiguousarray(sense[:, :n])
    a = np.ascontiguousarray(audio[:, :n])
    out = np.full((nch, 2 * n), np.nan, np.float32)
    side = np.zeros(16, np.int32)
    sp, ap, op, d = s.ctypes.data, a.ctypes.data, out.ctypes.data, side.ctypes.data
    none = (None,) * 4
    assert f(cpu._h, sp, n, ap, nch, n, n, op, 2 * n, *none) == ERR_STATE                     # nothing set
    cpu.setChannelDcsDecoder(cws, params, w, W, 1, 2, 1, 1)
    first = run_cpu(cpu, sense[:, :n], audio[:, :n], [n])
    assert f(cpu._h, sp, n, ap, 3, n, n, op, 2 * n, *none) == ERR_STATE                       # another nch
    assert f(cpu._h, sp, n, None, nch, n, 0, op, 2 * n, *none) == ERR_ARG                     # an output without audio
    assert f(cpu._h, sp, n, ap, nch, n, n, None, 2 * n, *none) == ERR_ARG                     # audio without an output
    assert f(cpu._h, None, n, ap, nch, n, n, op, 2 * n, *none) == ERR_ARG
    assert f(cpu._h, sp, n, ap, nch, 0, n, op, 2 * n, *none) == ERR_ARG
    assert f(cpu._h, sp, 1 << 42, ap, nch, (1 << 40) + 1, 1 << 42, op, 1 << 42, *none) == ERR_ARG
    for strides in ((n - 1, n, 2 * n), (n, n - 1, 2 * n), (n, n, n - 1)):
        assert f(cpu._h, sp, strides[0], ap, nch, n, strides[1], op, strides[2], *none) == ERR_ARG
    assert f(cpu._h, sp + 2, n, ap, nch, n - 1, n, op, 2 * n, *none) == ERR_ARG               # misaligned
    for k in range(4):
        ptrs = [None] * 4
        ptrs[k] = d + 2
        assert f(cpu._h, sp, n, ap, nch, n, n, op, 2 * n, *ptrs) == ERR_ARG
    assert f(cpu._h, sp, n, ap, nch, n, n, ap + 4 * (n - 1), n, *none) == ERR_ARG             # on the audio
    assert f(cpu._h, sp, n, ap, nch, n, n, sp + 4 * (n - 1), n, *none) == ERR_ARG             # on the sense stream
    assert np.isnan(out).all()
    # the stream goes on as if no failed call had been made
    second = run_cpu(cpu, sense[:, n:], audio[:, n:], [n])
    m = M.definition(sense, audio, cws, params, w, W, 1, 2, 1, 1)
    np.testing.assert_array_equal(bits(np.concatenate([first[0], second[0]], axis=1)), bits(m["y"]))
    ref = model_sides(m, n, 2 * n)
    for name in SIDES:
        np.testing.assert_array_equal(second[1][0][name], ref[name], err_msg=name)
    # a CPU handle has no device path
    assert cpu._L.sddc_ddc_channel_dcs_device(cpu._h, sp, n, None, nch, n, 0, None, 0, *none, None) == ERR_STATE


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "-".join("n" if v is None else "fs"[v] for v in c))
def test_every_format_pairing_against_the_model(cpu, combo):
    nch, W, w = 5, 6, W8K
    n = 9 * W * B + 77
    sense, audio, cws, params = case(nch, n, W, w, 104, combo[0] == S, combo[1] == S)
    m = check_against_model(cpu, sense, audio, cws, params, w, W, 1, 2, 1, 1, combo, what=combo)
    # the case exercises the stage: bypass, a channel that opens and closes, found codes under ANY
    assert m["bypass"][0] and m["G"][1].any() and not m["G"][1].all() and (m["best"][2][m["v"][2]] >= 0).any()


@pytest.mark.parametrize("eo,ec", [(0, 0), (0, 3), (3, 3), (1, 2)])
@pytest.mark.parametrize("A,H", [(1, 0), (2, 1), (255, 0), (1, 65535), (3, 2)])
def test_error_limits_and_gate_edges(cpu, eo, ec, A, H):
    nch, W, w = 10, 6, W8K
    n = 14 * W * B + 3
    sense, audio, cws, params = case(nch, n, W, w, 64, False, False)
    check_against_model(cpu, sense, audio, cws, params, w, W, eo, ec, A, H, (F, F, F), what=(eo, ec, A, H))


@pytest.mark.parametrize("eye", [0, 256])
def test_eye_edges_and_both_polarities(cpu, eye):
    """eye = 0 accepts every window (256 Q >= 0), eye = 256 only a window whose every sample agrees with its bit;
    a clean NRZ at w = 2^29 (one sample per sub-bin) has Q = N.  invert = 1 finds the complemented stream."""
    W, w = 6, WMAX
    n = 4 * W * B
    cws = M.table(8)
    clean = M.nrz(int(cws[3]), w, n)
    sense = np.stack([clean, -clean, clean + 0.6 * np.random.default_rng(3).standard_normal(n), clean]).astype(np.float32)
    params = np.array([[3, 0, eye], [3, 1, eye], [3, 0, eye], [3, 1, eye]], np.int32)
    m = check_against_model(cpu, sense, None, cws, params, w, W, 0, 0, 1, 0, (F, None, None), what=eye)
    assert (m["Q"][:2] == m["N"][:2]).all() and (m["d"][:2] == 0).all() and m["G"][:2, 1:].all()
    assert (m["Q"][2] < m["N"][2]).all() and m["G"][2, 1:].all() == (eye == 0)
    assert (m["d"][3] > 3).all() and not m["G"][3].any()               # the wrong polarity never matches


def test_special_samples(cpu):
    """NaN, +-Inf and +-0 in F32 (the signs 0, +1, -1, 0, 0) and -32768 in S16 (-1), placed where they decide a bit."""
    W, w = 6, WMAX
    n = 3 * W * B
    cws = M.table(2)
    base = M.nrz(int(cws[1]), w, n)
    for sense16 in (False, True):
        x = (base * (1000 if sense16 else 1)).astype(np.int16 if sense16 else np.float32)[None, :].repeat(2, axis=0)
        k = np.arange(0, n, 5)
        if sense16:
            x[1, k] = np.where(base[k] > 0, 32767, -32768).astype(np.int16)
            x[1, 3::8] = 0
        else:
            x[1, k] = np.where(base[k] > 0, np.inf, -np.inf).astype(np.float32)
            x[1, 3::8] = np.nan
            x[1, 4::8] = -0.0
        params = np.array([[1, 0, 200], [1, 0, 200]], np.int32)
        m = check_against_model(cpu, x, None, cws, params, w, W, 0, 0, 1, 0, (S if sense16 else F, None, None), what=sense16)
        assert (m["d"] == 0).all()
        assert (m["Q"][0] == m["N"][0]).all() and (m["Q"][1] < m["N"][1]).all()   # the zeros thin the eye, nothing else


def test_every_cut_of_a_short_stream(cpu):
    """w = 2^29, W = 1: windows of 256 samples, so a stream of three windows and a tail has every kind of cut."""
    nch, W, w = 3, 1, WMAX
    n = 3 * B + 40
    sense, audio, cws, params = case(nch, n, W, w, 16, False, False)
    cpu.setChannelDcsDecoder(cws, params, w, W, 1, 2, 1, 1)
    whole = run_cpu(cpu, sense, audio, [n])
    m = M.definition(sense, audio, cws, params, w, W, 1, 2, 1, 1)
    np.testing.assert_array_equal(bits(whole[0]), bits(m["y"]))
    for k in range(1, n):
        cpu.resetChannelDcsDecoder()
        y, sides = run_cpu(cpu, sense, audio, [k, n - k])
        np.testing.assert_array_equal(bits(y), bits(whole[0]), err_msg=str(k))
        for a, b, sd in ((0, k, sides[0]), (k, n, sides[1])):
            ref = model_sides(m, a, b)
            for name in SIDES:
                np.testing.assert_array_equal(sd[name], ref[name], err_msg=f"{name} cut at {k}")


@pytest.mark.parametrize("combo", [(F, F, F), (S, S, S), (F, None, None)], ids=["f32", "s16", "detect"])
def test_random_cuts_into_many_calls(cpu, combo):
    nch, W, w = 4, 6, W8K
    n = 11 * W * B + 123
    sense, audio, cws, params = case(nch, n, W, w, 104, combo[0] == S, combo[1] == S)
    rng = np.random.default_rng(5)
    for trial in range(3):
        edges = np.sort(rng.choice(np.arange(1, n), size=40, replace=False))
        cuts = np.diff(np.concatenate([[0], edges, [n]])).tolist()
        check_against_model(cpu, sense, audio, cws, params, w, W, 1, 2, 2, 1, combo, cuts, what=trial)


def test_a_channel_alone_and_reset(cpu):
    nch, W, w = 5, 6, W8K
    n = 8 * W * B + 9
    sense, audio, cws, params = case(nch, n, W, w, 104, False, False)
    cpu.setChannelDcsDecoder(cws, params, w, W, 1, 2, 1, 1)
    among = run_cpu(cpu, sense, audio, [n])
    cpu.channel_dcs_host(sense[:, :1000], audio[:, :1000])
    cpu.resetChannelDcsDecoder()                       # a new, closed stream
    again = run_cpu(cpu, sense, audio, [n])
    np.testing.assert_array_equal(bits(again[0]), bits(among[0]))
    for c in range(nch):
        cpu.setChannelDcsDecoder(cws, params[c:c + 1], w, W, 1, 2, 1, 1)
        y, sides = run_cpu(cpu, sense[c:c + 1], audio[c:c + 1], [n])
        np.testing.assert_array_equal(bits(y[0]), bits(among[0][c]))
        for name in SIDES:
            np.testing.assert_array_equal(sides[0][name][0], among[1][0][name][c], err_msg=name)


def test_tables_of_every_size(cpu):
    W, w = 6, W8K
    n = 6 * W * B
    for ncodes in (1, 64, 65, 128):
        sense, audio, cws, params = case(4, n, W, w, ncodes, False, False)
        assert cws.shape[0] == ncodes
        check_against_model(cpu, sense, audio, cws, params, w, W, 1, 2, 1, 0, (F, F, F), what=ncodes)


def test_the_largest_window(cpu):
    W = 256
    w = M.smallest_word(W)
    n = 2 * W * B + 300
    sense, audio, cws, params = case(2, n, W, w, 16, False, False)
    check_against_model(cpu, sense, audio, cws, params, w, W, 1, 2, 1, 0, (F, F, F), cuts=[W * B - 1, 2, n - W * B - 1])


# ---- what it is for ------------------------------------------------------------------------------
def test_it_decodes_023_in_noise_and_gates(cpu):
    """NRZ +-1 of code 023 at 8 kS/s (W = 6) at random fractional bit offsets in Gaussian noise of sigma 0.5, with
    eye = 128.  The model decides first: every window of 40 draws decodes with d = 0 and Q / N >= 0.90, never as the
    other table entry; pure sigma = 1 noise has Q / N <= 0.19 and d >= 3.  Then the backend equals the model, and the
    gate opens after A windows, holds, and closes H + 1 windows after the signal stops."""
    w, W = dcs_window(8000.0)
    WB = W * B
    cws = np.array([dcs_codeword("023"), dcs_codeword("754")], np.uint32)
    rng = np.random.default_rng(2024)
    draws = 40
    sig = np.stack([M.nrz(int(cws[0]), w, WB, offset=rng.uniform(0, 23)) + 0.5 * rng.standard_normal(WB) for _ in range(draws)])
    noise = rng.standard_normal((draws, WB))
    params1 = np.array([[DCS_ANY, 0, 128]], np.int32)
    for k in range(draws):
        ms = M.definition(sig[k:k + 1], None, cws, params1, w, W, 1, 2, 1, 0)
        mn = M.definition(noise[k:k + 1], None, cws, params1, w, W, 1, 2, 1, 0)
        assert ms["d"][0, 0] == 0 and ms["best"][0, 0] == 0 and ms["Q"][0, 0] >= 0.90 * ms["N"][0, 0], k
        assert mn["Q"][0, 0] <= 0.19 * mn["N"][0, 0] and mn["d"][0, 0] >= 3 and not mn["v"][0, 0], k
    # one stream: 2 windows of noise, 6 of the code (starting off the window grid), 7 of noise
    A, H = 2, 3
    n = 15 * WB
    x = rng.standard_normal(n)
    a0 = 2 * WB + 1234
    x[a0:a0 + 6 * WB] = M.nrz(int(cws[0]), w, 6 * WB, offset=0.37) + 0.5 * rng.standard_normal(6 * WB)
    sense = np.stack([x, x, x]).astype(np.float32)
    audio = (0.25 * rng.standard_normal((3, n))).astype(np.float32)
    params = np.array([[0, 0, 128], [DCS_ANY, 0, 128], [1, 0, 128]], np.int32)   # 023, scan, 754
    m = check_against_model(cpu, sense, audio, cws, params, w, W, 1, 2, A, H, (F, F, F), cuts=[5 * WB + 7, n - 5 * WB - 7])
    # windows 3..7 hold the code alone (window 2 and window 8 hold its edges)
    assert m["u"][0, 3:8].all() and not m["u"][0, :2].any() and not m["v"][0, 9:].any()
    first = 3 if not m["u"][0, 2] else 2
    last = 8 if m["v"][0, 8] else 7                       # the last window that still matched
    G = m["G"][0]
    assert not G[:first + A].any() and G[first + A:last + H + 2].all() and not G[last + H + 2:].any()
    np.testing.assert_array_equal(m["G"][1], G)           # the scan finds the same code
    assert (m["best"][1, 3:8] == 0).all() and not m["G"][2].any()
    assert (bits(m["y"][0, :(first + A) * WB]) == 0).all()
    np.testing.assert_array_equal(bits(m["y"][0, (first + A) * WB:(last + H + 2) * WB]), bits(audio[0, (first + A) * WB:(last + H + 2) * WB]))
