#!/usr/bin/env python3
"""Timing of the channel tone detector on one GPU (bench.py stays the flagship benchmark).

Workloads: Gaussian noise of rms 0.05 as the sense stream, with a tone of amplitude 0.2 at the table's first
frequency on every other channel (S16: times 8000 as int16 codes), and Gaussian audio, generated on the device.
  c5     1024 channels x 524288 samples
  d6     128 channels x 131072 samples
  short  1024 channels x 960 samples
Sense F32 and S16 (the audio in and out alike), masks of the first 1, 8 and 50 CTCSS tones (fs = 12 kS/s) on
every channel, W = 16, A = 1, H = 0, rho = (0.2, 0.1): every other channel is open in the steady state.  Runs
detect-only (d_audio = None) and with audio.  Three legs on the same device buffers, timed with HIP events in
interleaved rounds in ONE process:
  (a) sddc_ddc_channel_tone_device with all five side outputs;
  (b) a torch device copy_ that moves the floor: bytes(sense) once, and with audio bytes(out) and the open
      channels' bytes(audio);
  (c) sddc_ddc_channel_squelch_device with the sense buffer as the audio and SENSE_SELF (LEVEL, A = 2, H = 4,
      every channel open): the stage with the same three-launch shape reading the same buffer.
Leg (a)'s first call after a set is checked bit for bit against the numpy model on two channels' first 8192
samples.  Prints a line per row and one JSON line: ms (median of the rounds), spread (max - min), and the
ratios.  Nothing is gated.

  --trace-row  runs legs (a) (detect-only, F32, the three masks) and (c) on the c5 buffers alone, --reps times
               each, and nothing else: the run a kernel trace splits into the kernels

  python tools/channel_tone_bench.py [--rounds 5] [--reps 5] [--out FILE] [--txt FILE]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model():
    spec = importlib.util.spec_from_file_location("channel_tone_model", os.path.join(ROOT, "tools", "channel_tone_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--trace-row", action="store_true")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--txt", help="also write the printed rows to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import AUDIO_F32, AUDIO_S16, CTCSS_TONES, SQUELCH_LEVEL, SQUELCH_SENSE_SELF, R2iq, tone_word
    assert torch.cuda.is_available(), "channel_tone_bench needs a GPU"
    M = _model()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)
    FS, W, A, H = 12000.0, 16, 1, 0
    words = np.array([tone_word(f, FS) for f in CTCSS_TONES], np.uint32)
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

    res = {"configs": []}
    plans = [("c5", 1024, 524288)] + ([] if args.trace_row else [("d6", 128, 131072), ("short", 1024, 960)])
    for name, nch, nsamp in plans:
        t = torch.arange(nsamp, dtype=torch.float64, device=dev)
        tone = (0.2 * torch.cos(2 * np.pi * CTCSS_TONES[0] / FS * t)).to(torch.float32)
        s = torch.randn((nch, nsamp), dtype=torch.float32, device=dev, generator=gen) * 0.05
        s[0::2] += tone
        s16 = (s * 8000.0).round().clamp(-32768, 32767).to(torch.int16)
        x = torch.randn((nch, nsamp), dtype=torch.float32, device=dev, generator=gen) * 0.25
        x16 = (x * 8000.0).round().clamp(-32768, 32767).to(torch.int16)
        del t, tone
        r = R2iq(gain=1.0)
        d_tone, d_open, d_count = (torch.zeros(nch, dtype=torch.int32, device=dev) for _ in range(3))
        d_level = torch.zeros((nch, 2), dtype=torch.float32, device=dev)
        thr = np.tile(np.float32([0.2, 0.1, 0.0]), (nch, 1))
        sq_modes, sq_thr = np.full(nch, SQUELCH_LEVEL, np.int32), np.tile(np.float32([1e-9, 5e-10]), (nch, 1))
        for fmt, fname, sense, audio in ((AUDIO_F32, "F32", s, x), (AUDIO_S16, "S16", s16, x16)):
            if args.trace_row and fmt != AUDIO_F32:
                continue
            d_out = torch.zeros((nch, nsamp), dtype=sense.dtype, device=dev)
            r.setChannelSquelch(sq_modes, sq_thr, 2, 4, 0, SQUELCH_SENSE_SELF, fmt, fmt)
            size = sense.numel() * sense.element_size()
            for nt in (1, 8, 50):
                masks = np.full(nch, (1 << nt) - 1, np.uint64)
                d_powers = torch.zeros((nch, nt), dtype=torch.float32, device=dev)
                for with_audio in (False, True):
                    if args.trace_row and with_audio:
                        continue
                    floor = size + (size + size // 2 if with_audio else 0)
                    cp_a = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
                    cp_b = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
                    r.setChannelToneDetector(words[:nt], masks, thr, W, A, H, fmt, fmt, fmt)

                    def leg_a():
                        r.channel_tone_device(sense, nsamp, audio if with_audio else None, nch, nsamp, nsamp,
                                              d_out if with_audio else None, nsamp, d_tone=d_tone, d_open=d_open, d_count=d_count,
                                              d_level=d_level, d_powers=d_powers)

                    def leg_b():
                        cp_b.copy_(cp_a)

                    def leg_c():
                        r.channel_squelch_device(sense, None, nch, nsamp, nsamp, 0, d_out, nsamp)

                    if args.trace_row:
                        for _ in range(args.reps):
                            leg_a()
                        if nt == 50:
                            for _ in range(args.reps):
                                leg_c()
                        torch.cuda.synchronize()
                        continue
                    leg_a()   # the check of leg (a): its first call after the set
                    torch.cuda.synchronize()
                    k = min(nsamp, 8192)
                    want = M.definition(sense[:2, :k].cpu().numpy(), audio[:2, :k].cpu().numpy() if with_audio else None,
                                        words[:nt], masks[:2], thr[:2], W, A, H, fmt)
                    if with_audio:
                        got = d_out[:2, :k].cpu().numpy()
                        word = np.uint32 if fmt == AUDIO_F32 else np.int16
                        assert np.array_equal(np.ascontiguousarray(got).view(word), np.ascontiguousarray(want["y"]).view(word))
                    if nsamp == k:
                        assert np.array_equal(d_tone[:2].cpu().numpy(), M.tone_at(want, k))
                        assert np.array_equal(d_powers[:2].cpu().numpy().view(np.uint32), M.powers_at(want, k).view(np.uint32))
                    leg_a(), leg_b(), leg_c()   # warm-up; the gates are in their steady state from here on
                    torch.cuda.synchronize()
                    share = float(d_count.to(torch.int64).sum().item()) / (nch * nsamp)
                    named = int((d_tone == 0).sum().item())
                    ta, tb, tc = [], [], []
                    for rnd in range(args.rounds + 1):
                        a, b, c = timed(leg_a, args.reps), timed(leg_b, args.reps), timed(leg_c, args.reps)
                        if rnd:
                            ta.append(a), tb.append(b), tc.append(c)
                    ma, mb, mc = median(ta), median(tb), median(tc)
                    cfg = {"workload": name, "channels": nch, "nsamp": nsamp, "format": fname, "tones": nt, "audio": with_audio,
                           "open_share": share, "channels_naming_tone_0": named, "floor_bytes": floor, "tone_ms": ma,
                           "tone_spread_ms": max(ta) - min(ta), "copy_ms": mb, "copy_spread_ms": max(tb) - min(tb), "squelch_ms": mc,
                           "squelch_spread_ms": max(tc) - min(tc), "tone_over_copy": ma / mb, "tone_over_squelch": ma / mc,
                           "rounds_ms": {"tone": ta, "copy": tb, "squelch": tc}}
                    res["configs"].append(cfg)
                    say(f"{name:5s} {fname} {nch:4d} ch x {nsamp:6d} {nt:2d} tones {'audio ' if with_audio else 'detect'} "
                        f"(open {100 * share:5.1f} %, tone 0 on {named}): (a) tone detector {ma:8.4f} ms (+-{cfg['tone_spread_ms']:.4f})  "
                        f"(b) copy of the floor {mb:8.4f} ms (+-{cfg['copy_spread_ms']:.4f})  (c) squelch SELF {mc:8.4f} ms "
                        f"(+-{cfg['squelch_spread_ms']:.4f})  a/b {ma / mb:5.2f}  a/c {ma / mc:5.2f}")
                    del cp_a, cp_b
                del d_powers
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
