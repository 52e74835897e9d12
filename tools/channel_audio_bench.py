#!/usr/bin/env python3
"""Timing of the channel audio filter on one GPU (bench.py stays the flagship benchmark).

Workloads, each the AM demodulator's F32 output of the library's own DDC output of uniform int16 input
(S16: the same audio scaled to +-16000):
  c5     1024 channels x 524288 samples (256 blocks at d = 4)
  d6     128 channels x 131072 samples (256 blocks at d = 6)
  batch  1024 channels x 960 samples: a 20 ms batch at 48 kS/s (the head of the c5 streams)
and on each S = 1 (a DC blocker) and S = 4 (DC blocker, 300 Hz high-pass at 48 kS/s, a 3 kHz low-pass
and a 75 us de-emphasis), F32 -> F32 and S16 -> S16.  Two legs on the same device buffers, timed with
HIP events in interleaved rounds in ONE process:
  (a) sddc_ddc_channel_audio_filter_device (the state advancing: the cost per call does not depend on
      its content; calls of a length that is no multiple of the block walk through every head / tail
      split);
  (b) a torch device copy_ of the same input to the same-sized output: the memory floor.
Leg (a)'s first call after a set is checked against the float64 recurrence and its bound on two
channels' first 2048 samples.  Prints a line per row and one JSON line: ms (median of the rounds), the bytes the stage must
move (one read and one write per sample) per second, and the ratio to the copy.  Nothing is gated.

  python tools/channel_audio_bench.py [--channels 1024] [--nblk 256] [--rounds 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model():
    spec = importlib.util.spec_from_file_location("channel_audio_model", os.path.join(ROOT, "tools", "channel_audio_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024, help="channels of the c5 workload (d = 4)")
    ap.add_argument("--channels-d6", type=int, default=128)
    ap.add_argument("--nblk", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed window")
    ap.add_argument("--heat-s", type=float, default=2.0)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, BIQUAD_DC_BLOCK, BIQUAD_HIGHPASS, BIQUAD_IDENTITY, BIQUAD_LOWPASS,
                                BIQUAD_ONE_POLE_LP, BLOCK, DEMOD_AM, HALF_FFT, R2iq, biquad, output_samples)
    assert torch.cuda.is_available(), "channel_audio_bench needs a GPU"
    M = _model()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)
    fs = 48000.0
    sets = {1: np.stack([biquad(BIQUAD_DC_BLOCK, 20.0 / fs)]),
            4: np.stack([biquad(BIQUAD_DC_BLOCK, 20.0 / fs), biquad(BIQUAD_HIGHPASS, 300.0 / fs, 0.7071),
                         biquad(BIQUAD_LOWPASS, 3000.0 / fs, 0.7071),
                         biquad(BIQUAD_ONE_POLE_LP, 1.0 / (2 * np.pi * 75e-6 * fs))])}
    assert biquad(BIQUAD_IDENTITY)[0] == 1.0

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
    for name, d, nch in (("c5", 4, args.channels), ("d6", 6, args.channels_d6)):
        nblk = args.nblk
        d_in = torch.randint(-32768, 32767, (HALF_FFT + nblk * BLOCK,), dtype=torch.int16, device=dev, generator=gen)
        nsamp0 = output_samples(d, nblk)
        r = R2iq(gain=1.0)
        r.setDecimate(d)
        tbs = [4 * c for c in range(nch)]
        iq = torch.empty((nch, 2 * nsamp0), dtype=torch.float32, device=dev)
        t_end = time.time() + args.heat_s   # heat the chip so every leg is timed at the sustained clock
        while True:
            r.process_channels_device(d_in, nblk, tbs, iq)
            torch.cuda.synchronize()
            if time.time() >= t_end:
                break
        am = torch.empty((nch, nsamp0), dtype=torch.float32, device=dev)
        r.setChannelDemodulator([DEMOD_AM] * nch)
        r.channel_demodulate_device(iq, nch, nsamp0, 2 * nsamp0, am, nsamp0)
        torch.cuda.synchronize()
        del iq, d_in
        am *= 16000.0 / float(am.max().item())
        am16 = am.round().to(torch.int16)
        workloads = [(name, nsamp0)] + ([("batch", 960)] if name == "c5" else [])
        for wname, nsamp in workloads:
            for nsec, coef1 in sets.items():
                coef = np.stack([coef1] * nch)
                for fmt, fname, src in ((AUDIO_F32, "F32", am), (AUDIO_S16, "S16", am16)):
                    d_out = torch.zeros((nch, nsamp), dtype=src.dtype, device=dev)
                    d_cp = torch.empty((nch, nsamp), dtype=src.dtype, device=dev)
                    view = src[:, :nsamp]
                    r.setChannelAudioFilter(coef, fmt, fmt)

                    def leg_a():
                        r.channel_audio_filter_device(src, nch, nsamp, nsamp0, d_out, nsamp)

                    def leg_b():
                        d_cp.copy_(view)

                    leg_a(), leg_b()   # warm-up, and the check of leg (a): its first call after the set
                    torch.cuda.synchronize()
                    k = min(nsamp, 2048)
                    x = src[:2, :k].cpu().numpy().astype(np.float32)
                    y64, bnd = M.recurrence64(x, coef[:2]), M.bounds(x, coef[:2])
                    got = d_out[:2, :k].cpu().numpy().astype(np.float64)
                    diff = float(np.abs(got - y64).max())
                    assert np.all(np.abs(got - y64) <= bnd + (0.5 if fmt == AUDIO_S16 else 0.0)), diff
                    ta, tb = [], []
                    for rnd in range(args.rounds + 1):
                        a, b = timed(leg_a, args.reps), timed(leg_b, args.reps)
                        if rnd:
                            ta.append(a), tb.append(b)
                    ma, mb = median(ta), median(tb)
                    nbytes = 2 * nch * nsamp * src.element_size()
                    cfg = {"workload": wname, "channels": nch, "nsamp": nsamp, "sections": nsec, "format": fname,
                           "kernel_ms": ma, "kernel_spread_ms": max(ta) - min(ta), "copy_ms": mb,
                           "kernel_over_copy": ma / mb, "kernel_TBps": nbytes / (ma * 1e-3) / 1e12,
                           "copy_TBps": nbytes / (mb * 1e-3) / 1e12, "maxabs_vs_float64": diff,
                           "rounds_ms": {"kernel": ta, "copy": tb}}
                    res["configs"].append(cfg)
                    print(f"{wname:5s} {fname} {nch:4d} ch x {nsamp:6d} S = {nsec}: (a) stage {ma:8.3f} ms "
                          f"(+-{cfg['kernel_spread_ms']:.3f}) {cfg['kernel_TBps']:5.2f} TB/s  (b) copy {mb:8.3f} ms "
                          f"{cfg['copy_TBps']:5.2f} TB/s  a/b {ma / mb:5.2f}  |a - y64| {diff:.2e}", flush=True)
                    del d_out, d_cp
        r.close()
        del am, am16
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
