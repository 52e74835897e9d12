#!/usr/bin/env python3
"""Timing of the channel stereo decoder on one GPU (bench.py stays the flagship benchmark).

Workloads: a multiplex of a 1 kHz tone of amplitude 0.25 (its phase differs per channel), the 19 kHz pilot of
amplitude 0.1 and Gaussian noise of rms 0.02 at fs = 250 kS/s (S16: times 8000 as int16 codes), generated on
the device.
  c5     1024 channels x 524288 samples
  d6     128 channels x 131072 samples
  short  1024 channels x 960 samples
Input and outputs F32 and S16 alike, W = 8, A = 1, H = 0, rho = (0.004, 0.002), g = 1; the modes all AUTO (every
channel decodes in the steady state), all MONO (every channel copies) and every other one.  Four legs on the
same device buffers, timed with HIP events in interleaved rounds in ONE process:
  (a) sddc_ddc_channel_stereo_device with all four side outputs;
  (b) a torch device copy_ that moves the floor: bytes(in) + 2 bytes(out);
  (c) sddc_ddc_channel_tone_device, detect only, with the one-tone table {pilot word} and the same W on the same
      buffer: the pilot measurement alone;
  (d) (F32, all AUTO only) a composed torch path: the one-tone DFT per window as a product with a phasor table
      and a sum, the phase of the window before, sin of the carrier's phase, and the elementwise matrix.
Leg (a)'s first call after a set is checked bit for bit against the numpy model on two channels' first 8192
samples.  Prints a line per row and one JSON line: ms (median of the rounds), spread (max - min), the ratios
and the achieved bytes per second of the floor.  Nothing is gated.

  python tools/channel_stereo_bench.py [--rounds 5] [--reps 5] [--only c5,d6,short] [--out FILE] [--txt FILE]
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
    spec = importlib.util.spec_from_file_location("channel_stereo_model", os.path.join(ROOT, "tools", "channel_stereo_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--only", default="c5,d6,short")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--txt", help="also write the printed rows to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import AUDIO_F32, AUDIO_S16, STEREO_AUTO, STEREO_MONO, R2iq, stereo_pilot_word
    assert torch.cuda.is_available(), "channel_stereo_bench needs a GPU"
    M = _model()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)
    FS, W, A, H, B = 250000.0, 8, 1, 0, 256
    WB = W * B
    word = stereo_pilot_word(FS)
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
    plans = [p for p in (("c5", 1024, 524288), ("d6", 128, 131072), ("short", 1024, 960)) if p[0] in args.only.split(",")]
    for name, nch, nsamp in plans:
        t = torch.arange(nsamp, dtype=torch.float64, device=dev)
        ph = torch.arange(nch, dtype=torch.float64, device=dev)[:, None] * 0.37
        x = torch.randn((nch, nsamp), dtype=torch.float32, device=dev, generator=gen) * 0.02
        x += (0.25 * torch.sin(2 * np.pi * 1000.0 / FS * t + ph)).to(torch.float32)
        x += (0.1 * torch.sin(2 * np.pi * 19000.0 / FS * t + 0.7)).to(torch.float32)
        x16 = (x * 8000.0).round().clamp(-32768, 32767).to(torch.int16)
        del t, ph
        r = R2iq(gain=1.0)
        d_stereo, d_count, d_tone, d_open = (torch.zeros(nch, dtype=torch.int32, device=dev) for _ in range(4))
        d_level, d_phase, d_tlevel = (torch.zeros((nch, 2), dtype=torch.float32, device=dev) for _ in range(3))
        for fmt, fname, mpx, sc in ((AUDIO_F32, "F32", x, 1.0), (AUDIO_S16, "S16", x16, 8000.0)):
            params = np.tile(np.float32([0.004, 0.002, 1e-6 * sc * sc, 1.0]), (nch, 1))
            d_left, d_right = (torch.zeros((nch, nsamp), dtype=mpx.dtype, device=dev) for _ in range(2))
            size = mpx.numel() * mpx.element_size()
            floor = 3 * size
            cp_a = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
            cp_b = torch.empty(floor // 2, dtype=torch.uint8, device=dev)
            r.setChannelToneDetector([word], np.ones(nch, np.uint64), params[:, :3], W, A, H, fmt)
            for mname, modes in (("auto", np.full(nch, STEREO_AUTO, np.uint8)), ("mono", np.full(nch, STEREO_MONO, np.uint8)),
                                 ("mixed", np.where(np.arange(nch) % 2 == 0, STEREO_AUTO, STEREO_MONO).astype(np.uint8))):
                r.setChannelStereoDecoder(word, modes, params, W, A, H, fmt, fmt)

                def leg_a():
                    r.channel_stereo_device(mpx, nch, nsamp, nsamp, d_left, d_right, nsamp, d_stereo=d_stereo, d_count=d_count,
                                            d_level=d_level, d_phase=d_phase)

                def leg_b():
                    cp_b.copy_(cp_a)

                def leg_c():
                    r.channel_tone_device(mpx, nsamp, None, nch, nsamp, 0, None, 0, d_tone=d_tone, d_open=d_open, d_level=d_tlevel)

                nw = nsamp // WB
                with_d = fmt == AUDIO_F32 and mname == "auto" and nw >= 2
                if with_d:
                    tt = torch.arange(WB, dtype=torch.float64, device=dev)
                    ang = 2 * np.pi * (word / 2.0 ** 32) * tt
                    pc, ps = torch.cos(ang).to(torch.float32), torch.sin(ang).to(torch.float32)
                    tn = torch.arange(nw * WB, dtype=torch.float64, device=dev)
                    car = (2 * 2 * np.pi * (word / 2.0 ** 32) * tn).remainder(2 * np.pi).to(torch.float32).view(1, nw, WB)
                    del tt, ang, tn

                def leg_d():
                    xw = mpx[:, :nw * WB].view(nch, nw, WB)
                    zr, zi = (xw * pc).sum(-1), (xw * ps).sum(-1)
                    # a window's phasors start at its own first sample here: the rotation to the stream's phase
                    k0 = torch.arange(nw, dtype=torch.float64, device=dev) * WB
                    rot = (2 * np.pi * (word / 2.0 ** 32) * k0).remainder(2 * np.pi).to(torch.float32)
                    alpha2 = 2 * (torch.atan2(zr, zi) - rot)          # twice the pilot's phase, per window
                    prev = torch.roll(alpha2, 1, dims=1)              # the window before decides
                    d = 2 * xw * torch.sin(car + prev[:, :, None])
                    d_left[:, :nw * WB].view(nch, nw, WB).copy_(xw + d)
                    d_right[:, :nw * WB].view(nch, nw, WB).copy_(xw - d)

                leg_a()   # the check of leg (a): its first call after the set
                torch.cuda.synchronize()
                k = min(nsamp, 8192)
                want = M.definition(mpx[:2, :k].cpu().numpy(), word, modes[:2], params[:2], W, A, H, fmt)
                wd = np.uint32 if fmt == AUDIO_F32 else np.int16
                for got, nm in ((d_left, "left"), (d_right, "right")):
                    assert np.array_equal(np.ascontiguousarray(got[:2, :k].cpu().numpy()).view(wd), np.ascontiguousarray(want[nm]).view(wd))
                leg_a(), leg_b(), leg_c()   # warm-up; the gates are in their steady state from here on
                if with_d:
                    leg_d()
                torch.cuda.synchronize()
                share = float(d_count.to(torch.int64).sum().item()) / (nch * nsamp)
                ta, tb, tc, td = [], [], [], []
                for rnd in range(args.rounds + 1):
                    a, b, c = timed(leg_a, args.reps), timed(leg_b, args.reps), timed(leg_c, args.reps)
                    d = timed(leg_d, args.reps) if with_d else float("nan")
                    if rnd:
                        ta.append(a), tb.append(b), tc.append(c), td.append(d)
                ma, mb, mc, md = median(ta), median(tb), median(tc), median(td)
                cfg = {"workload": name, "channels": nch, "nsamp": nsamp, "format": fname, "modes": mname, "stereo_share": share,
                       "floor_bytes": floor, "stereo_ms": ma, "stereo_spread_ms": max(ta) - min(ta), "copy_ms": mb,
                       "copy_spread_ms": max(tb) - min(tb), "tone_ms": mc, "tone_spread_ms": max(tc) - min(tc),
                       "torch_ms": md if with_d else None, "stereo_over_copy": ma / mb, "stereo_over_tone": ma / mc,
                       "torch_over_stereo": md / ma if with_d else None, "floor_TBps": floor / ma * 1e-9,
                       "rounds_ms": {"stereo": ta, "copy": tb, "tone": tc, "torch": td if with_d else None}}
                res["configs"].append(cfg)
                say(f"{name:5s} {fname} {nch:4d} ch x {nsamp:6d} {mname:5s} (stereo {100 * share:5.1f} %): (a) stereo decoder {ma:8.4f} ms "
                    f"(+-{cfg['stereo_spread_ms']:.4f}, {cfg['floor_TBps']:.2f} TB/s of the floor)  (b) copy of the floor {mb:8.4f} ms "
                    f"(+-{cfg['copy_spread_ms']:.4f})  (c) one-tone detector {mc:8.4f} ms (+-{cfg['tone_spread_ms']:.4f})  "
                    f"a/b {ma / mb:5.2f}  a/c {ma / mc:5.2f}" + (f"  (d) torch {md:8.4f} ms  d/a {md / ma:5.2f}" if with_d else ""))
                if with_d:
                    del pc, ps, car
            del d_left, d_right, cp_a, cp_b
            torch.cuda.empty_cache()
        r.close()
        del x, x16
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
