#!/usr/bin/env python3
"""Timing of the channel decimator on one GPU (bench.py stays the flagship benchmark).

Three rows, each on the DDC's own output of uniform int16 input, in CF32 and in CS16:
  c5   1024 channels x 256 blocks at d = 4 (524288 samples per channel), R = 8, 65 taps
  c5   the same buffer, R = 32, 257 taps
  d6   128 channels x 256 blocks at d = 6 (131072 samples per channel), R = 16, 129 taps
with Kaiser taps from sddc_ddc_kaiser.  Two legs on the same device buffer, timed with HIP events in
interleaved rounds in ONE process (as tools/channel_spectrum_bench.py does):
  (a) sddc_ddc_channel_decimate_device (the tails zeroed once, then advancing: the cost per call
      does not depend on their content);
  (b) the path a caller composes without it: torch conv1d with stride R over the real view of the
      buffer, every (channel, component) a batch row, zero history, including the int16 -> float
      pass under CS16 (in chunks of channels, so its buffers stay at about 1 GB).
Leg (a) (first call after a reset) is checked against leg (b).  Prints a line per row and one JSON
line: ms (median of the rounds), input samples per second, and the bytes leg (a) reads per second
against the 8 TB/s HBM roofline, counted as 8 (CF32) / 4 (CS16) bytes per input sample.

  python tools/channel_decimate_bench.py [--channels 1024] [--nblk 256] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024, help="channels of the c5 workload (d = 4)")
    ap.add_argument("--channels-d6", type=int, default=128)
    ap.add_argument("--nblk", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="launches per timed window of leg (a)")
    ap.add_argument("--chunk-bytes", type=float, default=1e9, help="leg (b): bytes of float input per chunk of channels")
    ap.add_argument("--heat-s", type=float, default=2.0)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from extio_sddc_amd import BLOCK, HALF_FFT, R2iq, kaiser, output_samples
    assert torch.cuda.is_available(), "channel_decimate_bench needs a GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0x5DDC)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    res = {"configs": []}
    # (name, d, channels, ((R, ntaps), ...)): the cut-off at 0.4 / R of the input rate, the stop band from 0.5 / R
    workloads = (("c5", 4, args.channels, ((8, 65), (32, 257))), ("d6", 6, args.channels_d6, ((16, 129),)))
    for name, d, nch, rows in workloads:
        nblk = args.nblk
        d_in = torch.randint(-32768, 32767, (HALF_FFT + nblk * BLOCK,), dtype=torch.int16, device=dev, generator=g)
        nsamp = output_samples(d, nblk)
        r = R2iq(gain=1.0)
        r.setDecimate(d)
        tbs = [4 * c for c in range(nch)]
        iq32 = torch.empty((nch, 2 * nsamp), dtype=torch.float32, device=dev)
        r.process_channels_device(d_in, nblk, tbs, iq32)
        torch.cuda.synchronize()
        cs16_scale = float(0.5 * 32767.0 / iq32.abs().max().item())
        # heat the chip so every leg is timed at the sustained clock
        t_end = time.time() + args.heat_s
        while time.time() < t_end:
            r.process_channels_device(d_in, nblk, tbs, iq32)
            torch.cuda.synchronize()
        for fmt in ("CF32", "CS16"):
            if fmt == "CS16":
                del iq32
                r.setOutputFormat("CS16", cs16_scale)
                d_iq = torch.empty((nch, 2 * nsamp), dtype=torch.int16, device=dev)
                r.process_channels_device(d_in, nblk, tbs, d_iq)
                torch.cuda.synchronize()
            else:
                d_iq = iq32
            inv_s = 1.0 / cs16_scale if fmt == "CS16" else 1.0
            for R, ntaps in rows:
                h = kaiser(ntaps, 60.0, 0.4 / R, 0.5 / R)
                assert h.size == ntaps
                nout = nsamp // R
                r.setChannelDecimator(h, R, nch)
                d_out = torch.full((nch, 2 * nout), float("nan"), dtype=torch.float32, device=dev)
                ref = torch.empty((nch, nout, 2), dtype=torch.float32, device=dev)
                w = torch.from_numpy(h[::-1].copy()).to(dev).view(1, 1, ntaps)
                cpc = max(1, min(nch, int(args.chunk_bytes // (nsamp * 8))))   # channels per chunk

                def leg_a():
                    r.channel_decimate_device(d_iq, nch, nsamp, 2 * nsamp, d_out, 2 * nout)

                def leg_b():
                    for c0 in range(0, nch, cpc):
                        c1 = min(nch, c0 + cpc)
                        x = d_iq[c0:c1].view(c1 - c0, nsamp, 2).permute(0, 2, 1)          # [ch, 2, nsamp], a view
                        x = (x.float() * inv_s if fmt == "CS16" else x).reshape((c1 - c0) * 2, 1, nsamp)
                        y = F.conv1d(x, w, stride=R, padding=ntaps - 1)[:, 0, :nout]       # zero history
                        ref[c0:c1] = y.view(c1 - c0, 2, nout).permute(0, 2, 1)

                leg_a(), leg_b()   # warm-up, and the check of leg (a): its first call after the set
                torch.cuda.synchronize()
                assert bool(torch.isfinite(d_out).all())
                diff = (d_out.view(nch, nout, 2) - ref).abs().max().item()
                vs_b = diff / ref.abs().max().item()
                ta, tb = [], []
                for rnd in range(args.rounds + 1):
                    a, b = timed(leg_a, args.reps), timed(leg_b, 1)
                    if rnd:
                        ta.append(a), tb.append(b)
                ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
                nbytes = nch * nsamp * (4 if fmt == "CS16" else 8)
                cfg = {"workload": name, "d": d, "channels": nch, "nblk": nblk, "nsamp": nsamp, "format": fmt,
                       "factor": R, "ntaps": ntaps, "kernel_ms": ma, "composed_ms": mb, "composed_over_kernel": mb / ma,
                       "kernel_faster": ma < mb, "kernel_GSps": nch * nsamp / (ma * 1e-3) / 1e9,
                       "kernel_read_TBps": nbytes / (ma * 1e-3) / 1e12,
                       "kernel_roofline_frac": nbytes / (ma * 1e-3) / HBM_BYTES_PER_S,
                       "maxrel_vs_composed": vs_b, "rounds_ms": {"kernel": ta, "composed": tb}}
                res["configs"].append(cfg)
                print(f"{name} {fmt} {nch:4d} ch x {nsamp:6d} R {R:2d} taps {ntaps:3d}: (a) kernel {ma:8.3f} ms "
                      f"{cfg['kernel_GSps']:6.1f} GS/s {cfg['kernel_read_TBps']:5.2f} TB/s "
                      f"({cfg['kernel_roofline_frac'] * 100:4.1f} % of 8 TB/s)  (b) composed {mb:8.3f} ms  "
                      f"b/a {mb / ma:5.1f}  vs composed {vs_b:.1e}", flush=True)
                del d_out, ref
            del d_iq
        r.close()
        del d_in
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
