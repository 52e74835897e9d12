#!/usr/bin/env python3
"""Timing of the channel noise blanker on one GPU (bench.py stays the flagship benchmark).

Workloads: complex Gaussian noise (rms 0.3) with a three-sample impulse of amplitude 30 every 997
samples, generated on the device; CS16 is the same stream times 1000 as int16 codes.
  c5     1024 channels x 524288 samples
  d6     128 channels x 131072 samples
CF32 and CS16, g = 0 and 8, M = 8, MEAN and MEDIAN, k2 = 10 dB.  Two legs on the same device buffers,
timed with HIP events in interleaved rounds in ONE process:
  (a) sddc_ddc_channel_blank_device with d_count (the state advancing: the cost per call does not
      depend on the stream position);
  (b) a torch device copy_ of the same input to the same-sized output: the memory floor.
Leg (a)'s first call after a set is checked bit for bit against the numpy model on two channels' first
4096 samples.  Prints a line per row and one JSON line: ms (median of the rounds), the bytes the stage
must move (one read and one write per sample) per second, and the ratio.  Nothing is gated.

  --sweep      also times the c5 CF32 g = 8 MEAN row at runs of 16 .. 512 blocks per wave, interleaved
  --trace-row  runs leg (a) on the c5 buffers alone, --reps times per row, and nothing else: the run a
               kernel trace splits into the outputs kernel and the state kernel

  python tools/channel_blanker_bench.py [--channels 1024] [--nsamp 524288] [--rounds 7] [--sweep] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM_CHNB_RUN_BLOCKS = 22   # sddc_ddc_internal.h


def _model():
    spec = importlib.util.spec_from_file_location("channel_blanker_model", os.path.join(ROOT, "tools", "channel_blanker_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--nsamp", type=int, default=524288)
    ap.add_argument("--channels-d6", type=int, default=128)
    ap.add_argument("--nsamp-d6", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed window")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--trace-row", action="store_true")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import BLANKER_MEAN, BLANKER_MEDIAN, R2iq, blanker_threshold
    from extio_sddc_amd.r2iq import FMT_CF32, FMT_CS16
    assert torch.cuda.is_available(), "channel_blanker_bench needs a GPU"
    M = _model()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)
    k2 = blanker_threshold(10.0)

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
        assert f(r._h, PARAM_CHNB_RUN_BLOCKS, n) == 0

    res = {"configs": [], "sweep": []}
    plans = [("c5", args.channels, args.nsamp)] + ([] if args.trace_row else [("d6", args.channels_d6, args.nsamp_d6)])
    for name, nch, nsamp in plans:
        x = torch.randn((nch, 2 * nsamp), dtype=torch.float32, device=dev, generator=gen) * (0.3 / 2 ** 0.5)
        v = x.view(nch, nsamp, 2)
        for k in range(3):
            v[:, 498 + k::997, :] = 30.0 / 2 ** 0.5
        x16 = (x * 1000.0).round().clamp(-32768, 32767).to(torch.int16)
        r = R2iq(gain=1.0)
        d_count = torch.zeros(nch, dtype=torch.int32, device=dev)
        par = np.tile(np.float32([k2, 0.0]), (nch, 1))
        for fmt, fname, src in ((FMT_CF32, "CF32", x), (FMT_CS16, "CS16", x16)):
            d_out = torch.zeros((nch, 2 * nsamp), dtype=src.dtype, device=dev)
            d_cp = torch.empty((nch, 2 * nsamp), dtype=src.dtype, device=dev)
            for g in (0, 8):
                for mode, mname in ((BLANKER_MEAN, "mean"), (BLANKER_MEDIAN, "median")):
                    m = 8
                    r.setChannelBlanker(par, g, m, mode, fmt)

                    def leg_a():
                        r.channel_blank_device(src, nch, nsamp, 2 * nsamp, d_out, 2 * nsamp, d_count=d_count)

                    def leg_b():
                        d_cp.copy_(src)

                    if args.trace_row:
                        for _ in range(args.reps):
                            leg_a()
                        torch.cuda.synchronize()
                        continue
                    leg_a(), leg_b()   # warm-up, and the check of leg (a): its first call after the set
                    torch.cuda.synchronize()
                    k = min(nsamp, 4096)
                    h = src[:2, :2 * k].cpu().numpy()
                    hx = h.reshape(2, k, 2) if fmt == FMT_CS16 else np.ascontiguousarray(h).view(np.complex64)
                    want = M.definition(hx, par[:2], g, m, mode)["y"]
                    got = d_out[:2, :2 * k].cpu().numpy()
                    want = want.reshape(2, -1) if fmt == FMT_CS16 else np.ascontiguousarray(want).view(np.float32)
                    word = np.uint32 if fmt == FMT_CF32 else np.int16
                    assert np.array_equal(np.ascontiguousarray(got).view(word), np.ascontiguousarray(want).view(word))
                    blanked = float(d_count.sum().item()) / (nch * nsamp)
                    ta, tb = [], []
                    for rnd in range(args.rounds + 1):
                        a, b = timed(leg_a, args.reps), timed(leg_b, args.reps)
                        if rnd:
                            ta.append(a), tb.append(b)
                    ma, mb = median(ta), median(tb)
                    nbytes = 2 * nch * 2 * nsamp * src.element_size()
                    cfg = {"workload": name, "channels": nch, "nsamp": nsamp, "format": fname, "guard": g, "ref_blocks": m,
                           "mode": mname, "blank_ms": ma, "blank_spread_ms": max(ta) - min(ta), "copy_ms": mb,
                           "copy_spread_ms": max(tb) - min(tb), "blank_over_copy": ma / mb,
                           "blank_TBps": nbytes / (ma * 1e-3) / 1e12, "copy_TBps": nbytes / (mb * 1e-3) / 1e12,
                           "blanked_share": blanked, "rounds_ms": {"blank": ta, "copy": tb}}
                    res["configs"].append(cfg)
                    print(f"{name} {fname} {nch:4d} ch x {nsamp:6d} g {g} M {m} {mname:6s}: (a) blanker {ma:8.3f} ms "
                          f"(+-{cfg['blank_spread_ms']:.3f}) {cfg['blank_TBps']:5.2f} TB/s  (b) copy {mb:8.3f} ms "
                          f"(+-{cfg['copy_spread_ms']:.3f})  a/b {ma / mb:5.2f}  blanked {100 * blanked:.2f} %", flush=True)
                    if args.sweep and name == "c5" and fmt == FMT_CF32 and g == 8 and mode == BLANKER_MEAN:
                        lengths = [16, 32, 64, 128, 256, 512]
                        ts = {n: [] for n in lengths}
                        for rnd in range(args.rounds + 1):
                            for n in lengths:
                                set_run_blocks(r, n)
                                t = timed(leg_a, args.reps)
                                if rnd:
                                    ts[n].append(t)
                        set_run_blocks(r, 0)
                        for n in lengths:
                            res["sweep"].append({"run_blocks": n, "blank_ms": median(ts[n]), "spread_ms": max(ts[n]) - min(ts[n])})
                            print(f"      runs of {n:4d} blocks: {median(ts[n]):8.3f} ms (+-{max(ts[n]) - min(ts[n]):.3f})", flush=True)
            del d_out, d_cp
        r.close()
        del x, x16, v
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
