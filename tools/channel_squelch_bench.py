#!/usr/bin/env python3
"""Timing of the channel squelch on one GPU (bench.py stays the flagship benchmark).

Workloads: Gaussian audio (rms 0.25; S16: times 8000 as int16 codes) and, for the CF32 sense kind, complex
Gaussian noise of mean square 1 as the sense stream, generated on the device.
  c5     1024 channels x 524288 samples
  d6     128 channels x 131072 samples
  short  1024 channels x 960 samples
F32 and S16 audio (in and out alike), sense SELF and CF32, LEVEL mode with A = 2, H = 4 and fade, and three
threshold sets on the same data: every channel closed, every channel open, every other channel open (the
gates move only in the first blocks after the set call; the timed calls run in the steady state).  Three legs
on the same device buffers, timed with HIP events in interleaved rounds in ONE process:
  (a) sddc_ddc_channel_squelch_device with d_open, d_count and d_level;
  (b) a torch device copy_ that moves the floor: bytes(sense) + bytes(audio) + bytes(out), each once (SELF:
      the audio is its own sense stream and counts once);
  (c) sddc_ddc_channel_agc_device on the same audio buffers: the stage with the same three-launch shape.
Leg (a)'s first call after a set is checked bit for bit against the numpy model on two channels' first 4096
samples.  Prints a line per row and one JSON line: ms (median of the rounds), spread (max - min), and the
ratios.  Nothing is gated.

  --trace-row  runs leg (a) on the c5 buffers alone, --reps times per row, and nothing else: the run a kernel
               trace splits into the three kernels

  python tools/channel_squelch_bench.py [--rounds 7] [--reps 10] [--out FILE] [--txt FILE]
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
    spec = importlib.util.spec_from_file_location("channel_squelch_model", os.path.join(ROOT, "tools", "channel_squelch_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed window")
    ap.add_argument("--trace-row", action="store_true")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--txt", help="also write the printed rows to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, SQUELCH_LEVEL, SQUELCH_SENSE_CF32, SQUELCH_SENSE_SELF, R2iq,
                                agc_decay)
    assert torch.cuda.is_available(), "channel_squelch_bench needs a GPU"
    M = _model()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)
    A, H, FADE = 2, 4, 1
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
        x = torch.randn((nch, nsamp), dtype=torch.float32, device=dev, generator=gen) * 0.25
        x16 = (x * 8000.0).round().clamp(-32768, 32767).to(torch.int16)
        z = torch.randn((nch, 2 * nsamp), dtype=torch.float32, device=dev, generator=gen) * (0.5 ** 0.5)
        r = R2iq(gain=1.0)
        d_open, d_count = (torch.zeros(nch, dtype=torch.int32, device=dev) for _ in range(2))
        d_level = torch.zeros(nch, dtype=torch.float32, device=dev)
        modes = np.full(nch, SQUELCH_LEVEL, np.int32)
        agc_par = np.tile(np.float32([0.25, agc_decay(4800.0), 1e-3]), (nch, 1))
        for fmt, fname, src in ((AUDIO_F32, "F32", x), (AUDIO_S16, "S16", x16)):
            d_out = torch.zeros((nch, nsamp), dtype=src.dtype, device=dev)
            r.setChannelAgc(agc_par, fmt, fmt)
            for kind, kname, sense in ((SQUELCH_SENSE_SELF, "SELF", None), (SQUELCH_SENSE_CF32, "CF32", z)):
                ms = (0.0625 * (8000.0 ** 2 if fmt == AUDIO_S16 else 1.0)) if sense is None else 1.0   # the sense stream's mean square
                floor = src.numel() * src.element_size() * 2 + (0 if sense is None else sense.numel() * 4)
                cp_a = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
                cp_b = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
                for occ in ("closed", "open", "half"):
                    thr = np.empty((nch, 2), np.float32)
                    is_open = {"closed": np.zeros(nch, bool), "open": np.ones(nch, bool), "half": np.arange(nch) % 2 == 0}[occ]
                    thr[:, 0] = np.where(is_open, ms / 100.0, ms * 100.0)
                    thr[:, 1] = thr[:, 0] / 2.0
                    r.setChannelSquelch(modes, thr, A, H, FADE, kind, fmt, fmt)

                    def leg_a():
                        r.channel_squelch_device(src, sense, nch, nsamp, nsamp, 2 * nsamp, d_out, nsamp, d_open=d_open,
                                                 d_count=d_count, d_level=d_level)

                    def leg_b():
                        cp_b.copy_(cp_a)

                    def leg_c():
                        r.channel_agc_device(src, nch, nsamp, nsamp, d_out, nsamp)

                    if args.trace_row:
                        for _ in range(args.reps):
                            leg_a()
                        torch.cuda.synchronize()
                        continue
                    leg_a()   # the check of leg (a): its first call after the set
                    torch.cuda.synchronize()
                    k = min(nsamp, 4096)
                    hs = None if sense is None else np.ascontiguousarray(sense[:2, :2 * k].cpu().numpy()).view(np.complex64)
                    want = M.definition(src[:2, :k].cpu().numpy(), hs, kind, modes[:2], thr[:2], A, H, FADE, fmt)["y"]
                    got = d_out[:2, :k].cpu().numpy()
                    word = np.uint32 if fmt == AUDIO_F32 else np.int16
                    assert np.array_equal(np.ascontiguousarray(got).view(word), np.ascontiguousarray(want).view(word))
                    leg_a(), leg_b(), leg_c()   # warm-up; the gates are in their steady state from here on
                    torch.cuda.synchronize()
                    share = float(d_count.to(torch.int64).sum().item()) / (nch * nsamp)
                    ta, tb, tc = [], [], []
                    for rnd in range(args.rounds + 1):
                        a, b, c = timed(leg_a, args.reps), timed(leg_b, args.reps), timed(leg_c, args.reps)
                        if rnd:
                            ta.append(a), tb.append(b), tc.append(c)
                    ma, mb, mc = median(ta), median(tb), median(tc)
                    cfg = {"workload": name, "channels": nch, "nsamp": nsamp, "format": fname, "sense": kname, "gates": occ,
                           "open_share": share, "floor_bytes": floor, "squelch_ms": ma, "squelch_spread_ms": max(ta) - min(ta),
                           "copy_ms": mb, "copy_spread_ms": max(tb) - min(tb), "agc_ms": mc, "agc_spread_ms": max(tc) - min(tc),
                           "squelch_over_copy": ma / mb, "squelch_over_agc": ma / mc,
                           "rounds_ms": {"squelch": ta, "copy": tb, "agc": tc}}
                    res["configs"].append(cfg)
                    say(f"{name:5s} {fname} sense {kname:4s} {nch:4d} ch x {nsamp:6d} {occ:6s} (open {100 * share:5.1f} %): "
                        f"(a) squelch {ma:8.4f} ms (+-{cfg['squelch_spread_ms']:.4f})  (b) copy of the floor {mb:8.4f} ms "
                        f"(+-{cfg['copy_spread_ms']:.4f})  (c) AGC {mc:8.4f} ms (+-{cfg['agc_spread_ms']:.4f})  "
                        f"a/b {ma / mb:5.2f}  a/c {ma / mc:5.2f}")
                del cp_a, cp_b
            del d_out
        r.close()
        del x, x16, z
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
