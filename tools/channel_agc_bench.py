#!/usr/bin/env python3
"""Timing of the channel AGC on one GPU (bench.py stays the flagship benchmark).

Workloads, each the AM demodulator's F32 output of the library's own DDC output of uniform int16 input
(S16: the same audio scaled to +-16000), the audio filter's three buffers:
  c5     1024 channels x 524288 samples (256 blocks at d = 4)
  d6     128 channels x 131072 samples (256 blocks at d = 6)
  batch  1024 channels x 960 samples: a 20 ms batch at 48 kS/s (the head of the c5 streams)
F32 -> F32 and S16 -> S16.  Three legs on the same device buffers, timed with HIP events in interleaved
rounds in ONE process:
  (a) sddc_ddc_channel_agc_device with d_env (a 300 ms release at 48 kS/s; the state advancing: the cost
      per call does not depend on its content);
  (b) sddc_ddc_channel_audio_filter_device with S = 1 (a DC blocker): the stage this one is modelled on;
  (c) a torch device copy_ of the same input to the same-sized output: the memory floor.
Leg (a)'s first call after a set is checked against the float64 recurrence and its bound on two
channels' first 2048 samples.  Prints a line per row and one JSON line: ms (median of the rounds), the
bytes the stage must move (one read and one write per sample) per second, and the ratios.  Nothing is
gated.

  --sweep      also times leg (a) on the c5 F32 buffer at run lengths 128 .. 2048 blocks, interleaved
  --trace-row  runs legs (a) and (b) on the c5 buffers alone, --reps times each, F32 and S16, and
               nothing else: the run a kernel trace splits into ends / scan / outputs

  python tools/channel_agc_bench.py [--channels 1024] [--nblk 256] [--rounds 7] [--sweep] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM_CHAGC_RUN_BLOCKS = 19   # sddc_ddc_internal.h


def _model():
    spec = importlib.util.spec_from_file_location("channel_agc_model", os.path.join(ROOT, "tools", "channel_agc_model.py"))
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
    ap.add_argument("--sweep", action="store_true", help="run lengths 128 .. 2048 blocks on the c5 F32 buffer")
    ap.add_argument("--trace-row", action="store_true", help="the c5 AGC and S = 1 filter legs alone (for a kernel trace)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import (AUDIO_F32, AUDIO_S16, BIQUAD_DC_BLOCK, BLOCK, DEMOD_AM, HALF_FFT, R2iq, agc_decay, biquad,
                                output_samples)
    assert torch.cuda.is_available(), "channel_agc_bench needs a GPU"
    M = _model()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)
    fs = 48000.0
    decay = agc_decay(0.3 * fs)
    dc = np.stack([biquad(BIQUAD_DC_BLOCK, 20.0 / fs)])

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

    def set_run_blocks(r, n):
        f = r._L.sddc_ddc_internal_set_param
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
        assert f(r._h, PARAM_CHAGC_RUN_BLOCKS, n) == 0

    res = {"configs": [], "sweep": []}
    plans = (("c5", 4, args.channels),) if args.trace_row else (("c5", 4, args.channels), ("d6", 6, args.channels_d6))
    for name, d, nch in plans:
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
        d_env = torch.zeros(nch, dtype=torch.float32, device=dev)
        coef = np.stack([dc] * nch)
        if args.trace_row:
            for fmt, src, target, floor in ((AUDIO_F32, am, 0.5, 1e-4), (AUDIO_S16, am16, 16000.0, 1.0)):
                d_out = torch.zeros((nch, nsamp0), dtype=src.dtype, device=dev)
                r.setChannelAgc(np.tile(np.array([[target, decay, floor]], np.float32), (nch, 1)), fmt, fmt)
                r.setChannelAudioFilter(coef, fmt, fmt)
                for _ in range(args.reps):
                    r.channel_agc_device(src, nch, nsamp0, nsamp0, d_out, nsamp0, d_env=d_env)
                    r.channel_audio_filter_device(src, nch, nsamp0, nsamp0, d_out, nsamp0)
                torch.cuda.synchronize()
                del d_out
            r.close()
            print(json.dumps({"trace_row": {"channels": nch, "nsamp": nsamp0, "calls": args.reps}}))
            return
        workloads = [(name, nsamp0)] + ([("batch", 960)] if name == "c5" else [])
        for wname, nsamp in workloads:
            for fmt, fname, src, target, floor in ((AUDIO_F32, "F32", am, 0.5, 1e-4), (AUDIO_S16, "S16", am16, 16000.0, 1.0)):
                par = np.tile(np.array([[target, decay, floor]], np.float32), (nch, 1))
                d_out = torch.zeros((nch, nsamp), dtype=src.dtype, device=dev)
                d_aud = torch.zeros((nch, nsamp), dtype=src.dtype, device=dev)
                d_cp = torch.empty((nch, nsamp), dtype=src.dtype, device=dev)
                view = src[:, :nsamp]
                r.setChannelAgc(par, fmt, fmt)
                r.setChannelAudioFilter(coef, fmt, fmt)

                def leg_a():
                    r.channel_agc_device(src, nch, nsamp, nsamp0, d_out, nsamp, d_env=d_env)

                def leg_b():
                    r.channel_audio_filter_device(src, nch, nsamp, nsamp0, d_aud, nsamp)

                def leg_c():
                    d_cp.copy_(view)

                leg_a(), leg_b(), leg_c()   # warm-up, and the check of leg (a): its first call after the set
                torch.cuda.synchronize()
                k = min(nsamp, 2048)
                x = src[:2, :k].cpu().numpy().astype(np.float32)
                y64, bnd = M.recurrence64(x, par[:2])[0], M.bounds(x, par[:2])
                got = d_out[:2, :k].cpu().numpy().astype(np.float64)
                diff = float(np.abs(got - y64).max())
                assert np.all(np.abs(got - y64) <= bnd + (0.5 if fmt == AUDIO_S16 else 0.0)), diff
                ta, tb, tc = [], [], []
                for rnd in range(args.rounds + 1):
                    a, b, c = timed(leg_a, args.reps), timed(leg_b, args.reps), timed(leg_c, args.reps)
                    if rnd:
                        ta.append(a), tb.append(b), tc.append(c)
                ma, mb, mc = median(ta), median(tb), median(tc)
                nbytes = 2 * nch * nsamp * src.element_size()
                cfg = {"workload": wname, "channels": nch, "nsamp": nsamp, "format": fname,
                       "agc_ms": ma, "agc_spread_ms": max(ta) - min(ta), "audio_s1_ms": mb,
                       "audio_s1_spread_ms": max(tb) - min(tb), "copy_ms": mc, "agc_over_copy": ma / mc,
                       "agc_over_audio_s1": ma / mb, "agc_TBps": nbytes / (ma * 1e-3) / 1e12,
                       "copy_TBps": nbytes / (mc * 1e-3) / 1e12, "maxabs_vs_float64": diff,
                       "rounds_ms": {"agc": ta, "audio_s1": tb, "copy": tc}}
                res["configs"].append(cfg)
                print(f"{wname:5s} {fname} {nch:4d} ch x {nsamp:6d}: (a) AGC {ma:8.3f} ms (+-{cfg['agc_spread_ms']:.3f}) "
                      f"{cfg['agc_TBps']:5.2f} TB/s  (b) S = 1 filter {mb:8.3f} ms (+-{cfg['audio_s1_spread_ms']:.3f})  "
                      f"(c) copy {mc:8.3f} ms  a/b {ma / mb:5.2f}  a/c {ma / mc:5.2f}  |a - y64| {diff:.2e}", flush=True)
                if args.sweep and wname == "c5" and fmt == AUDIO_F32:
                    lengths = [128, 256, 512, 1024, 2048]
                    ts = {n: [] for n in lengths}
                    for rnd in range(args.rounds + 1):
                        for n in lengths:
                            set_run_blocks(r, n)
                            t = timed(leg_a, args.reps)
                            if rnd:
                                ts[n].append(t)
                    set_run_blocks(r, 0)
                    for n in lengths:
                        res["sweep"].append({"run_blocks": n, "agc_ms": median(ts[n]), "spread_ms": max(ts[n]) - min(ts[n])})
                        print(f"      run length {n:5d} blocks: {median(ts[n]):8.3f} ms (+-{max(ts[n]) - min(ts[n]):.3f})", flush=True)
                del d_out, d_aud, d_cp
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
