#!/usr/bin/env python3
"""Timing of the wideband spectrum on one GPU (bench.py stays the flagship benchmark).

For nblk blocks, blocks_per_row in {1, nblk} and the rectangular, Hann and Blackman-Harris windows,
three legs on the same input, timed with HIP events in interleaved rounds in ONE process (as
tools/ab_libs.py does):
  (a) sddc_ddc_spectrum_device;
  (b) sddc_ddc_process_device at d = 0 (the DDC on the same frames: forward, filter, inverse, 4 B/sample out);
  (c) the path a caller composes without (a): torch int16 -> float32 frames (x window),
      sddc_fft_r2c(8192), |.|^2, mean.
Leg (a) is also checked against leg (c) and, row 0, against the float64 model.  Prints a line per
configuration and one JSON line: ms (median of the rounds), GS/s and the fraction of the 2 B/sample
HBM roofline (8 TB/s).

  python tools/spectrum_bench.py [--nblk 2048] [--rounds 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("spectrum_model", os.path.join(ROOT, "tools", "spectrum_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblk", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed window of legs (a) and (b)")
    ap.add_argument("--reps-composed", type=int, default=2)
    ap.add_argument("--heat-s", type=float, default=2.0)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    from extio_sddc_amd import R2iq, _lib, spectrum_window
    assert torch.cuda.is_available(), "spectrum_bench needs a GPU"
    L = _lib.load()
    dev = torch.device("cuda", 0)
    nblk, nfr = args.nblk, args.nblk * M.FRAMES
    g = torch.Generator(device=dev).manual_seed(0x5DDC)
    d_in = torch.randint(-32768, 32767, (M.HALF + nblk * M.BLOCK,), dtype=torch.int16, device=dev, generator=g)
    d_iq = torch.empty(nblk * 32768 * 2, dtype=torch.float32, device=dev)
    frames_i16 = d_in.as_strided((nblk, M.FRAMES, M.FFTN), (M.BLOCK, M.HOP, 1))
    frames = torch.empty((nfr, M.FFTN), dtype=torch.float32, device=dev)
    spec = torch.empty((nfr, M.FFTN // 2 + 1, 2), dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    r = R2iq(gain=1.0)
    r.setDecimate(0)

    def leg_a(bpr, d_psd):
        r.spectrum_device(d_in, nblk, d_psd, bpr)

    def leg_b():
        r.process_device(d_in, nblk, d_iq)

    def leg_c(bpr, w_dev, wsum):
        frames.view(nblk, M.FRAMES, M.FFTN).copy_(frames_i16)
        if w_dev is not None:
            frames.mul_(w_dev)
        rc = L.sddc_fft_r2c(frames.data_ptr(), spec.data_ptr(), M.FFTN, nfr, s)
        assert rc == 0, L.sddc_ddc_last_error()
        p = spec.pow(2).sum(-1)
        return p.view(nblk // bpr, bpr * M.FRAMES, -1).mean(1)[:, :M.HALF] / (wsum * wsum)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # heat the chip so every leg is timed at the sustained clock
    t_end = time.time() + args.heat_s
    while time.time() < t_end:
        leg_b()
        torch.cuda.synchronize()

    x_host = d_in[:M.HALF + M.BLOCK].cpu().numpy()
    res = {"nblk": nblk, "samples": nblk * M.BLOCK, "configs": []}
    for bpr in (1, nblk):
        for win in ("rect", "hann", "blackman_harris"):
            w = None if win == "rect" else spectrum_window(win)
            r.setSpectrumWindow(w)
            w_dev = None if w is None else torch.from_numpy(w).to(dev)
            wsum = float(M.FFTN) if w is None else float(w.astype(np.float64).sum())
            d_psd = torch.full((nblk // bpr * M.HALF,), float("nan"), dtype=torch.float32, device=dev)
            fa, fb, fc = (lambda: leg_a(bpr, d_psd)), leg_b, (lambda: leg_c(bpr, w_dev, wsum))
            # warm-up of every leg, and the checks of leg (a)
            fa(), fb()
            ref_c = fc()
            torch.cuda.synchronize()
            psd = d_psd.view(nblk // bpr, M.HALF)
            assert bool(torch.isfinite(psd).all())
            vs_c = float(((psd - ref_c).abs().amax(1) / ref_c.amax(1)).max())
            vs_model = None
            if bpr == 1:
                ref = M.psd(x_host, 1, 1, w)
                vs_model = float(np.abs(psd[0].cpu().numpy() - ref[0]).max() / ref[0].max())
            del ref_c
            ta, tb, tc = [], [], []
            for rnd in range(args.rounds + 1):
                a, b, c = timed(fa, args.reps), timed(fb, args.reps), timed(fc, args.reps_composed)
                if rnd:
                    ta.append(a), tb.append(b), tc.append(c)
            med = [sorted(t)[len(t) // 2] for t in (ta, tb, tc)]
            gsps = [nblk * M.BLOCK / (m * 1e-3) / 1e9 for m in med]
            cfg = {"blocks_per_row": bpr, "window": win,
                   "spectrum_ms": med[0], "ddc_d0_ms": med[1], "composed_ms": med[2],
                   "spectrum_GSps": gsps[0], "ddc_d0_GSps": gsps[1], "composed_GSps": gsps[2],
                   "spectrum_roofline_frac": nblk * M.BLOCK * 2 / (med[0] * 1e-3) / HBM_BYTES_PER_S,
                   "composed_over_spectrum": med[2] / med[0], "spectrum_over_ddc_d0": med[0] / med[1],
                   "spectrum_le_ddc_d0": med[0] <= med[1],
                   "maxrel_vs_composed": vs_c, "row0_maxrel_vs_model": vs_model,
                   "rounds_ms": {"spectrum": ta, "ddc_d0": tb, "composed": tc}}
            res["configs"].append(cfg)
            print(f"bpr {bpr:5d} {win:16s} (a) spectrum {med[0]:.3f} ms {gsps[0]:6.1f} GS/s "
                  f"({cfg['spectrum_roofline_frac'] * 100:.1f} % of 2 B/sample)  (b) DDC d=0 {med[1]:.3f} ms  "
                  f"(c) composed {med[2]:.3f} ms  c/a {med[2] / med[0]:.1f}  a/b {med[0] / med[1]:.3f}  "
                  f"vs composed {vs_c:.1e}" + (f" vs model {vs_model:.1e}" if vs_model is not None else ""), flush=True)
    r.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
