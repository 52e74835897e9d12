#!/usr/bin/env python3
"""Timing of the channel DCS decoder on one GPU (bench.py stays the flagship benchmark).

Workloads: Gaussian noise of rms 0.5 as the sense stream, with the NRZ +-1 stream of code 023 at 134.4 bit/s and
48 kS/s (the phase word of dcs_window(48000), W = 34) on every other channel (S16: times 8000 as int16 codes), and
Gaussian audio, generated on the device.
  c5     1024 channels x 524288 samples
  d6     128 channels x 131072 samples
  short  1024 channels x 960 samples
Sense F32 and S16 (the audio in and out alike); a table of one code with every channel set to it, and the 104
standard codes with every channel on ANY; eye = 128, e = (1, 2), A = 1, H = 0: every other channel is open in the
steady state.  Runs detect-only (d_audio = None) and with audio.  Legs on the same device buffers, timed with HIP
events in interleaved rounds in ONE process:
  (a) sddc_ddc_channel_dcs_device with all four side outputs (the integer-atomics route, the default);
  (a') the same with the ballot route (SDDC_DDC_PARAM_CHDCS_BALLOT = 1);
  (b) a torch device copy_ that moves the floor: bytes(sense) once, and with audio bytes(out) and the open
      channels' bytes(audio);
  (c) sddc_ddc_channel_squelch_device with the sense buffer as the audio and SENSE_SELF (LEVEL, A = 2, H = 4,
      every channel open);
  (d) sddc_ddc_channel_tone_device with one tone (134.4 Hz, W = 16) on the sense buffer, detect-only or gating the
      same audio.
Leg (a)'s first call after a set is checked bit for bit against the numpy model on two channels' first two windows.
Prints a line per row and one JSON line: ms (median of the rounds), spread (max - min), and the ratios.  Nothing is
gated.

  python tools/channel_dcs_bench.py [--rounds 5] [--reps 5] [--out FILE] [--txt FILE]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM_CHDCS_BALLOT = 29   # sddc_ddc_internal.h


def _model():
    spec = importlib.util.spec_from_file_location("channel_dcs_model", os.path.join(ROOT, "tools", "channel_dcs_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--txt", help="also write the printed rows to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, DCS_ANY, DCS_CODES, SQUELCH_LEVEL, SQUELCH_SENSE_SELF, R2iq, dcs_codeword,
                                dcs_window, tone_word)
    assert torch.cuda.is_available(), "channel_dcs_bench needs a GPU"
    M = _model()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)
    FS, A, H = 48000.0, 1, 0
    w, W = dcs_window(FS)
    WB = W * 256
    table = np.array([dcs_codeword(c) for c in DCS_CODES], np.uint32)
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def median(v):
        return sorted(v)[len(v) // 2]

    res = {"word": w, "window": W, "configs": []}
    for name, nch, nsamp in (("c5", 1024, 524288), ("d6", 128, 131072), ("short", 1024, 960)):
        i = torch.arange(nsamp, dtype=torch.int64, device=dev)
        k = ((i * w) >> 32) % 23
        nrz = ((torch.bitwise_right_shift(torch.full_like(k, int(table[0])), k) & 1) * 2 - 1).to(torch.float32)
        s = torch.randn((nch, nsamp), dtype=torch.float32, device=dev, generator=gen) * 0.5
        s[0::2] += nrz
        s16 = (s * 8000.0).round().clamp(-32768, 32767).to(torch.int16)
        x = torch.randn((nch, nsamp), dtype=torch.float32, device=dev, generator=gen) * 0.25
        x16 = (x * 8000.0).round().clamp(-32768, 32767).to(torch.int16)
        del i, k, nrz
        r = R2iq(gain=1.0)
        d_code, d_open, d_count = (torch.zeros(nch, dtype=torch.int32, device=dev) for _ in range(3))
        d_info = torch.zeros((nch, 4), dtype=torch.int32, device=dev)
        d_level = torch.zeros((nch, 2), dtype=torch.float32, device=dev)
        d_powers = torch.zeros((nch, 1), dtype=torch.float32, device=dev)
        sq_modes, sq_thr = np.full(nch, SQUELCH_LEVEL, np.int32), np.tile(np.float32([1e-9, 5e-10]), (nch, 1))
        tone_words = np.array([tone_word(134.4, FS)], np.uint32)
        tone_masks, tone_thr = np.ones(nch, np.uint64), np.tile(np.float32([0.2, 0.1, 0.0]), (nch, 1))
        for fmt, fname, sense, audio in ((AUDIO_F32, "F32", s, x), (AUDIO_S16, "S16", s16, x16)):
            d_out = torch.zeros((nch, nsamp), dtype=sense.dtype, device=dev)
            r.setChannelSquelch(sq_modes, sq_thr, 2, 4, 0, SQUELCH_SENSE_SELF, fmt, fmt)
            r.setChannelToneDetector(tone_words, tone_masks, tone_thr, 16, A, H, fmt, fmt, fmt)
            size = sense.numel() * sense.element_size()
            for tname, cws, code in (("1 code", table[:1], 0), ("ANY/104", table, DCS_ANY)):
                params = np.tile(np.int32([code, 0, 128]), (nch, 1))
                for with_audio in (False, True):
                    floor = size + (size + size // 2 if with_audio else 0)
                    cp_a = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
                    cp_b = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
                    r.setChannelDcsDecoder(cws, params, w, W, 1, 2, A, H, fmt, fmt, fmt)

                    def leg_a():
                        r.channel_dcs_device(sense, nsamp, audio if with_audio else None, nch, nsamp, nsamp,
                                             d_out if with_audio else None, nsamp, d_code=d_code, d_open=d_open, d_count=d_count,
                                             d_info=d_info)

                    def leg_a2():
                        r._L.sddc_ddc_internal_set_param(r._h, PARAM_CHDCS_BALLOT, 1)
                        leg_a()
                        r._L.sddc_ddc_internal_set_param(r._h, PARAM_CHDCS_BALLOT, 0)

                    def leg_b():
                        cp_b.copy_(cp_a)

                    def leg_c():
                        r.channel_squelch_device(sense, None, nch, nsamp, nsamp, 0, d_out, nsamp)

                    def leg_d():
                        r.channel_tone_device(sense, nsamp, audio if with_audio else None, nch, nsamp, nsamp,
                                              d_out if with_audio else None, nsamp, d_tone=d_code, d_open=d_open, d_count=d_count,
                                              d_level=d_level, d_powers=d_powers)

                    leg_a()   # the check of leg (a): its first call after the set
                    torch.cuda.synchronize()
                    kk = min(nsamp, 2 * WB)
                    want = M.definition(sense[:2, :kk].cpu().numpy(), audio[:2, :kk].cpu().numpy() if with_audio else None,
                                        cws, params[:2], w, W, 1, 2, A, H, fmt)
                    if with_audio:
                        got = d_out[:2, :kk].cpu().numpy()
                        word = np.uint32 if fmt == AUDIO_F32 else np.int16
                        assert np.array_equal(np.ascontiguousarray(got).view(word), np.ascontiguousarray(want["y"]).view(word))
                    if nsamp == kk:
                        assert np.array_equal(d_code[:2].cpu().numpy(), M.code_at(want, kk))
                        assert np.array_equal(d_info[:2].cpu().numpy().view(np.uint32), M.info_at(want, kk))
                    leg_a(), leg_a2(), leg_b(), leg_c(), leg_d()   # warm-up; the gates are in their steady state from here on
                    leg_a()
                    torch.cuda.synchronize()
                    share = float(d_count.to(torch.int64).sum().item()) / (nch * nsamp)
                    named = int((d_code == 0).sum().item())
                    ta, ta2, tb, tc, td = [], [], [], [], []
                    for rnd in range(args.rounds + 1):
                        v = [timed(f, args.reps) for f in (leg_a, leg_a2, leg_b, leg_c, leg_d)]
                        if rnd:
                            for lst, t in zip((ta, ta2, tb, tc, td), v):
                                lst.append(t)
                    ma, ma2, mb, mc, md = (median(t) for t in (ta, ta2, tb, tc, td))
                    cfg = {"workload": name, "channels": nch, "nsamp": nsamp, "format": fname, "table": tname, "audio": with_audio,
                           "open_share": share, "channels_naming_code_0": named, "floor_bytes": floor, "dcs_ms": ma,
                           "dcs_spread_ms": max(ta) - min(ta), "dcs_ballot_ms": ma2, "dcs_ballot_spread_ms": max(ta2) - min(ta2),
                           "copy_ms": mb, "copy_spread_ms": max(tb) - min(tb), "squelch_ms": mc, "squelch_spread_ms": max(tc) - min(tc),
                           "tone1_ms": md, "tone1_spread_ms": max(td) - min(td), "dcs_over_copy": ma / mb, "dcs_over_tone1": ma / md,
                           "rounds_ms": {"dcs": ta, "dcs_ballot": ta2, "copy": tb, "squelch": tc, "tone1": td}}
                    res["configs"].append(cfg)
                    say(f"{name:5s} {fname} {nch:4d} ch x {nsamp:6d} {tname:7s} {'audio ' if with_audio else 'detect'} "
                        f"(open {100 * share:5.1f} %, code 0 on {named}): (a) DCS atomics {ma:8.4f} ms (+-{cfg['dcs_spread_ms']:.4f})  "
                        f"(a') DCS ballots {ma2:8.4f} ms (+-{cfg['dcs_ballot_spread_ms']:.4f})  (b) copy of the floor {mb:8.4f} ms "
                        f"(+-{cfg['copy_spread_ms']:.4f})  (c) squelch SELF {mc:8.4f} ms  (d) tone detector, 1 tone {md:8.4f} ms "
                        f"(+-{cfg['tone1_spread_ms']:.4f})  a/b {ma / mb:5.2f}  a/d {ma / md:5.2f}")
                    del cp_a, cp_b
            del d_out
        r.close()
        del s, s16, x, x16
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.txt, "\n".join(rows) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
