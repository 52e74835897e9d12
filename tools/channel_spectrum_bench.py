#!/usr/bin/env python3
"""Timing of the channel spectrum on one GPU (bench.py stays the flagship benchmark).

Two workloads, each produced by the DDC itself on uniform int16 input, in CF32 and in CS16:
  c5  the many-channel output of 1024 channels x 256 blocks at d = 4 (524288 samples per channel);
  d0  one d = 0 channel of 2048 blocks (67 M samples).
For n in {1024, 4096}, hop in {n/2, n}, the rectangular and the Hann window and rows of 64 frames,
two legs on the same device buffer, timed with HIP events in interleaved rounds in ONE process
(as tools/spectrum_bench.py does):
  (a) sddc_ddc_channel_spectrum_device;
  (b) the path a caller composes without it: torch frames (x window) into a complex64 buffer,
      sddc_fft_c2c, |.|^2, mean over the row's frames, roll by n/2 (in chunks of channels, so its
      buffers stay at about 1 GB).
Leg (a) is checked against leg (b).  Prints a line per configuration and one JSON line: ms (median
of the rounds), input samples per second, and the bytes leg (a) reads per second against the
8 TB/s HBM roofline, counted as (8 CF32 / 4 CS16) x n / hop bytes per input sample.

  python tools/channel_spectrum_bench.py [--channels 1024] [--nblk 256] [--nblk-d0 2048] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
FPR = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--nblk", type=int, default=256, help="blocks of the c5 workload (d = 4)")
    ap.add_argument("--nblk-d0", type=int, default=2048, help="blocks of the d0 workload")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="launches per timed window of leg (a)")
    ap.add_argument("--chunk-bytes", type=float, default=1e9, help="leg (b): bytes of frames per chunk of channels")
    ap.add_argument("--heat-s", type=float, default=2.0)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    from extio_sddc_amd import BLOCK, HALF_FFT, R2iq, _lib, output_samples, window
    assert torch.cuda.is_available(), "channel_spectrum_bench needs a GPU"
    L = _lib.load()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(0x5DDC)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    res = {"frames_per_row": FPR, "configs": []}
    workloads = (("c5", 4, args.channels, args.nblk), ("d0", 0, 1, args.nblk_d0))
    for name, d, nch, nblk in workloads:
        d_in = torch.randint(-32768, 32767, (HALF_FFT + nblk * BLOCK,), dtype=torch.int16, device=dev, generator=g)
        nsamp = output_samples(d, nblk)
        r = R2iq(gain=1.0)
        r.setDecimate(d)
        tbs = [4 * c for c in range(nch)]

        def ddc(d_out):
            if nch > 1:
                r.process_channels_device(d_in, nblk, tbs, d_out)
            else:
                r.setTuneBin(1024)
                r.process_device(d_in, nblk, d_out.view(-1))

        iq32 = torch.empty((nch, 2 * nsamp), dtype=torch.float32, device=dev)
        ddc(iq32)
        torch.cuda.synchronize()
        cs16_scale = float(0.5 * 32767.0 / iq32.abs().max().item())
        # heat the chip so every leg is timed at the sustained clock
        t_end = time.time() + args.heat_s
        while time.time() < t_end:
            ddc(iq32)
            torch.cuda.synchronize()
        for fmt in ("CF32", "CS16"):
            if fmt == "CS16":
                del iq32
                r.setOutputFormat("CS16", cs16_scale)
                d_iq = torch.empty((nch, 2 * nsamp), dtype=torch.int16, device=dev)
                ddc(d_iq)
                torch.cuda.synchronize()
            else:
                d_iq = iq32
            samp_scale = cs16_scale if fmt == "CS16" else 1.0
            for n in (1024, 4096):
                for hop in (n // 2, n):
                    nrows = ((nsamp - n) // hop + 1) // FPR
                    nfr = nrows * FPR
                    for win in ("rect", "hann"):
                        w = None if win == "rect" else window(win, n)
                        r.setChannelSpectrumWindow(w)
                        w_dev = None if w is None else torch.from_numpy(w).to(dev)
                        wsum = float(n) if w is None else float(w.astype(np.float64).sum())
                        d_psd = torch.full((nch, nrows, n), float("nan"), dtype=torch.float32, device=dev)
                        cpc = max(1, min(nch, int(args.chunk_bytes // (nfr * n * 8))))   # channels per chunk
                        fbuf = torch.empty((cpc * nfr, n), dtype=torch.complex64, device=dev)
                        obuf = torch.empty_like(fbuf)
                        ref = torch.empty((nch, nrows, n), dtype=torch.float32, device=dev)

                        def leg_a():
                            r.channel_spectrum_device(d_iq, nch, nsamp, 2 * nsamp, n, hop, FPR, nrows, d_psd)

                        def leg_b():
                            for c0 in range(0, nch, cpc):
                                c1 = min(nch, c0 + cpc)
                                x = d_iq[c0:c1].view(c1 - c0, nsamp, 2)
                                fr = x.unfold(1, n, hop)[:, :nfr]                  # [ch, nfr, 2, n], a view
                                fb = torch.view_as_real(fbuf[:(c1 - c0) * nfr]).view(c1 - c0, nfr, n, 2)
                                fb.copy_(fr.permute(0, 1, 3, 2))                   # int16 -> float here under CS16
                                if w_dev is not None:
                                    fb.mul_(w_dev[None, None, :, None])
                                rc = L.sddc_fft_c2c(fbuf.data_ptr(), obuf.data_ptr(), n, (c1 - c0) * nfr, -1, s)
                                assert rc == 0, L.sddc_ddc_last_error()
                                p = torch.view_as_real(obuf[:(c1 - c0) * nfr]).pow(2).sum(-1)
                                p = p.view(c1 - c0, nrows, FPR, n).mean(2)
                                ref[c0:c1] = torch.roll(p, n // 2, -1) / (wsum * wsum * samp_scale * samp_scale)

                        leg_a(), leg_b()   # warm-up, and the check of leg (a)
                        torch.cuda.synchronize()
                        assert bool(torch.isfinite(d_psd).all())
                        vs_b = float(((d_psd - ref).abs().amax(-1) / ref.amax(-1)).max())
                        ta, tb = [], []
                        for rnd in range(args.rounds + 1):
                            a, b = timed(leg_a, args.reps), timed(leg_b, 1)
                            if rnd:
                                ta.append(a), tb.append(b)
                        ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
                        used = nch * ((nfr - 1) * hop + n)                          # input samples the rows cover
                        nbytes = used * (4 if fmt == "CS16" else 8) * n / hop
                        cfg = {"workload": name, "d": d, "channels": nch, "nblk": nblk, "nsamp": nsamp, "format": fmt,
                               "n": n, "hop": hop, "window": win, "nrows": nrows,
                               "fused_ms": ma, "composed_ms": mb, "composed_over_fused": mb / ma,
                               "fused_faster": ma < mb, "fused_GSps": used / (ma * 1e-3) / 1e9,
                               "fused_read_TBps": nbytes / (ma * 1e-3) / 1e12,
                               "fused_roofline_frac": nbytes / (ma * 1e-3) / HBM_BYTES_PER_S,
                               "maxrel_vs_composed": vs_b, "rounds_ms": {"fused": ta, "composed": tb}}
                        res["configs"].append(cfg)
                        print(f"{name} {fmt} n {n:4d} hop {hop:4d} {win:5s} rows {nrows:5d}: (a) fused {ma:8.3f} ms "
                              f"{cfg['fused_GSps']:6.1f} GS/s {cfg['fused_read_TBps']:5.2f} TB/s "
                              f"({cfg['fused_roofline_frac'] * 100:4.1f} % of 8 TB/s)  (b) composed {mb:8.3f} ms  "
                              f"b/a {mb / ma:5.1f}  vs composed {vs_b:.1e}", flush=True)
                        del fbuf, obuf, ref, d_psd
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
