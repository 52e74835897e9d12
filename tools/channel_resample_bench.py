#!/usr/bin/env python3
"""Timing of the channel resampler on one GPU (bench.py stays the flagship benchmark).

Four rows, each on buffers resident in device memory, in CF32 and in CS16:
  c5r8  1024 channels x 65536 samples (the decimator's R = 8 output of the c5 workload: 256 blocks
        at d = 4, 500 kS/s per channel), 12/125, 1536 taps
  d6    128 channels x 131072 samples (256 blocks at d = 6, 1 MS/s), 6/125, 1536 taps
  c5    1024 channels x 524288 samples (the c5 output itself), 3/250, 3072 taps
  d6    the d6 buffer at 1/16 with 129 taps, next to the channel decimator (R = 16, the same taps) on
        the same buffer: the ratio is recorded, not judged
with Kaiser taps from sddc_ddc_kaiser, scaled by L.  The CS16 buffers hold the same streams rounded
to int16 at a scale that puts the largest component at half of full scale.  Two legs on the same
device buffer, timed with HIP events in interleaved rounds in ONE process (as
tools/channel_decimate_bench.py does):
  (a) sddc_ddc_channel_resample_device (the tails zeroed once, then advancing: the cost per call
      does not depend on their content; the count per call moves by one with the position);
  (b) the path a caller composes without it: for each b < L one torch conv1d with stride M over the
      real view of the buffer with the reversed taps of phase (b M) mod L, offset by (b M) div L
      samples, every (channel, component) a batch row, K - 1 zeros in front, interleaved into the output,
      including the int16 -> float pass under CS16 (in chunks of channels, so its buffers stay at
      about 1 GB).
Leg (a) (first call after the set) is checked against leg (b).  Prints a line per row and one JSON
line: ms (median of the rounds), input samples per second, and the bytes leg (a) reads per second
against the 8 TB/s HBM roofline, counted as 8 (CF32) / 4 (CS16) bytes per input sample.

  python tools/channel_resample_bench.py [--channels 1024] [--nblk 256] [--rounds 5] [--out FILE]
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

    import numpy as np
    import torch
    import torch.nn.functional as F
    from extio_sddc_amd import BLOCK, HALF_FFT, R2iq, kaiser, output_samples, resample_count
    assert torch.cuda.is_available(), "channel_resample_bench needs a GPU"
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

    def median(v):
        return sorted(v)[len(v) // 2]

    def taps_for(L, M, ntaps):
        """A low-pass at the prototype rate (L x the input rate): pass to 0.4, stop from 0.5 of the
        narrower of the two Nyquist bands, DC gain L."""
        f = 1.0 / max(L, M)
        h = kaiser(ntaps, 60.0, 0.4 * f, 0.5 * f)
        assert h.size == ntaps
        return (h * np.float32(L)).astype(np.float32)

    res = {"configs": []}
    nblk = args.nblk
    # (name, d, channels, decimate the DDC's output by 8 first, ((L, M, ntaps, beside the decimator), ...))
    workloads = (("c5r8", 4, args.channels, True, ((12, 125, 1536, False),)),
                 ("d6", 6, args.channels_d6, False, ((6, 125, 1536, False), (1, 16, 129, True))),
                 ("c5", 4, args.channels, False, ((3, 250, 3072, False),)))
    for name, d, nch, pre, rows in workloads:
        d_in = torch.randint(-32768, 32767, (HALF_FFT + nblk * BLOCK,), dtype=torch.int16, device=dev, generator=g)
        nsamp = output_samples(d, nblk)
        r = R2iq(gain=1.0)
        r.setDecimate(d)
        tbs = [4 * c for c in range(nch)]
        iq32 = torch.empty((nch, 2 * nsamp), dtype=torch.float32, device=dev)
        r.process_channels_device(d_in, nblk, tbs, iq32)
        torch.cuda.synchronize()
        # heat the chip so every leg is timed at the sustained clock
        t_end = time.time() + args.heat_s
        while time.time() < t_end:
            r.process_channels_device(d_in, nblk, tbs, iq32)
            torch.cuda.synchronize()
        if pre:   # the decimator's R = 8 output is the resampler's input
            r.setChannelDecimator(kaiser(65, 60.0, 0.05, 0.0625), 8, nch)
            dec = torch.empty((nch, 2 * (nsamp // 8)), dtype=torch.float32, device=dev)
            r.channel_decimate_device(iq32, nch, nsamp, 2 * nsamp, dec, 2 * (nsamp // 8))
            torch.cuda.synchronize()
            r.setChannelDecimator(None)
            iq32, nsamp = dec, nsamp // 8
        cs16_scale = float(0.5 * 32767.0 / iq32.abs().max().item())
        for fmt in ("CF32", "CS16"):
            if fmt == "CS16":
                d_iq = (iq32 * cs16_scale).round().to(torch.int16)
                del iq32
                r.setOutputFormat("CS16", cs16_scale)
            else:
                d_iq = iq32
            inv_s = 1.0 / cs16_scale if fmt == "CS16" else 1.0
            for L, M, ntaps, beside in rows:
                h = taps_for(L, M, ntaps)
                K = -(-ntaps // L)
                nout = resample_count(L, M, 0, nsamp)
                r.setChannelResampler(h, L, M, nch)
                d_out = torch.full((nch, 2 * (nout + 1)), float("nan"), dtype=torch.float32, device=dev)
                ref = torch.empty((nch, nout, 2), dtype=torch.float32, device=dev)
                hp = np.zeros(L * K, np.float32)
                hp[:ntaps] = h
                # phase (b M) mod L reversed, as conv1d correlates
                ws = [torch.from_numpy(hp[(b * M) % L::L][::-1].copy()).to(dev).view(1, 1, K) for b in range(L)]
                cpc = max(1, min(nch, int(args.chunk_bytes // (nsamp * 8))))   # channels per chunk

                def leg_a():
                    r.channel_resample_device(d_iq, nch, nsamp, 2 * nsamp, d_out, 2 * (nout + 1))

                def leg_b():
                    for c0 in range(0, nch, cpc):
                        c1 = min(nch, c0 + cpc)
                        x = d_iq[c0:c1].view(c1 - c0, nsamp, 2).permute(0, 2, 1)          # [ch, 2, nsamp], a view
                        x = (x.float() * inv_s if fmt == "CS16" else x).reshape((c1 - c0) * 2, 1, nsamp)
                        x = F.pad(x, (K - 1, 0))   # zero history, once for the L phases
                        for b in range(L):
                            nb = -(-(nout - b) // L)   # outputs a L + b < nout
                            y = F.conv1d(x[:, :, (b * M) // L:], ws[b], stride=M)[:, 0, :nb]
                            ref[c0:c1, b::L] = y.view(c1 - c0, 2, nb).permute(0, 2, 1)

                leg_a(), leg_b()   # warm-up, and the check of leg (a): its first call after the set
                torch.cuda.synchronize()
                got = d_out.view(nch, nout + 1, 2)[:, :nout]
                assert bool(torch.isfinite(got).all()) and bool(torch.isnan(d_out.view(nch, nout + 1, 2)[:, nout]).all())
                diff = (got - ref).abs().max().item()
                vs_b = diff / ref.abs().max().item()
                if beside:
                    r.setChannelDecimator(h, M, nch)
                    d_dec = torch.empty((nch, 2 * (nsamp // M)), dtype=torch.float32, device=dev)

                    def leg_d():
                        r.channel_decimate_device(d_iq, nch, nsamp, 2 * nsamp, d_dec, 2 * (nsamp // M))
                    leg_d()
                ta, tb, td = [], [], []
                for rnd in range(args.rounds + 1):
                    a, b = timed(leg_a, args.reps), timed(leg_b, 1)
                    dd = timed(leg_d, args.reps) if beside else 0.0
                    if rnd:
                        ta.append(a), tb.append(b), td.append(dd)
                ma, mb = median(ta), median(tb)
                nbytes = nch * nsamp * (4 if fmt == "CS16" else 8)
                cfg = {"workload": name, "d": d, "channels": nch, "nblk": nblk, "nsamp": nsamp, "format": fmt,
                       "up": L, "down": M, "ntaps": ntaps, "nout": nout, "kernel_ms": ma, "composed_ms": mb,
                       "composed_over_kernel": mb / ma, "kernel_faster": ma < mb,
                       "kernel_GSps": nch * nsamp / (ma * 1e-3) / 1e9, "kernel_read_TBps": nbytes / (ma * 1e-3) / 1e12,
                       "kernel_roofline_frac": nbytes / (ma * 1e-3) / HBM_BYTES_PER_S, "maxrel_vs_composed": vs_b,
                       "rounds_ms": {"kernel": ta, "composed": tb}}
                if beside:
                    cfg["decimator_ms"] = median(td)
                    cfg["resampler_over_decimator"] = ma / median(td)
                    cfg["rounds_ms"]["decimator"] = td
                    r.setChannelDecimator(None)
                    del d_dec
                res["configs"].append(cfg)
                print(f"{name} {fmt} {nch:4d} ch x {nsamp:6d} {L:2d}/{M:3d} taps {ntaps:4d}: (a) kernel {ma:8.3f} ms "
                      f"{cfg['kernel_GSps']:6.1f} GS/s {cfg['kernel_read_TBps']:5.2f} TB/s "
                      f"({cfg['kernel_roofline_frac'] * 100:4.1f} % of 8 TB/s)  (b) composed {mb:8.3f} ms  "
                      f"b/a {mb / ma:5.1f}  vs composed {vs_b:.1e}"
                      + (f"  decimator {median(td):.3f} ms, resampler / decimator {ma / median(td):.2f}" if beside else ""),
                      flush=True)
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
