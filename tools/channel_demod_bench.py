#!/usr/bin/env python3
"""Timing of the channel demodulator on one GPU (bench.py stays the flagship benchmark).

Three inputs, each the library's own output of uniform int16 input:
  c5     1024 channels x 256 blocks at d = 4 (524288 samples per channel), CF32 and CS16
  d6     128 channels x 256 blocks at d = 6 (131072 samples per channel), CF32 and CS16
  d6r8   the channel decimator's R = 8, 65-tap output of the d6 buffer (16384 samples per channel, CF32)
and on each every mode (AM, FM, BFO) in F32 and S16.  Two legs on the same device buffer, timed with
HIP events in interleaved rounds in ONE process (as tools/channel_decimate_bench.py does):
  (a) sddc_ddc_channel_demodulate_device without the power (the state advancing: the cost per call
      does not depend on its content);
  (b) the path a caller composes in torch without it: abs(x), angle(x[1:] conj(x[:-1])) or
      (x e^{j phi}).real with a phasor row that is built once outside the timed window, times the
      gain, including the int16 -> float pass under CS16 and the round / clamp / int16 pass under
      S16 (in chunks of channels, so its buffers stay at about 1 GB).
Leg (a) (first call after a set) is checked against leg (b).  Per input and format, FM / F32 is also
timed with the power computed (the fixed-order reduction and the second launch), next to the run to
run spread of leg (a).  Prints a line per row and one JSON line: ms (median of the rounds), the bytes leg (a) must move (8 or 4 in, 4 or 2
out per sample) per second against the 8 TB/s HBM roofline, and the ratio of the composed path to
the kernel.

  python tools/channel_demod_bench.py [--channels 1024] [--nblk 256] [--rounds 7] [--out FILE]
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
MODE_NAMES = ("AM", "FM", "BFO")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024, help="channels of the c5 workload (d = 4)")
    ap.add_argument("--channels-d6", type=int, default=128)
    ap.add_argument("--nblk", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window of leg (a)")
    ap.add_argument("--chunk-bytes", type=float, default=1e9, help="leg (b): bytes of float input per chunk of channels")
    ap.add_argument("--heat-s", type=float, default=2.0)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from extio_sddc_amd import AUDIO_F32, AUDIO_S16, BLOCK, HALF_FFT, R2iq, bfo_word, kaiser, output_samples
    assert torch.cuda.is_available(), "channel_demod_bench needs a GPU"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x5DDC)

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

    res = {"configs": [], "power": []}
    for name, d, nch in (("c5", 4, args.channels), ("d6", 6, args.channels_d6)):
        nblk = args.nblk
        d_in = torch.randint(-32768, 32767, (HALF_FFT + nblk * BLOCK,), dtype=torch.int16, device=dev, generator=gen)
        nsamp0 = output_samples(d, nblk)
        r = R2iq(gain=1.0)
        r.setDecimate(d)
        tbs = [4 * c for c in range(nch)]
        iq32 = torch.empty((nch, 2 * nsamp0), dtype=torch.float32, device=dev)
        r.process_channels_device(d_in, nblk, tbs, iq32)
        torch.cuda.synchronize()
        cs16_scale = float(0.5 * 32767.0 / iq32.abs().max().item())
        t_end = time.time() + args.heat_s   # heat the chip so every leg is timed at the sustained clock
        while time.time() < t_end:
            r.process_channels_device(d_in, nblk, tbs, iq32)
            torch.cuda.synchronize()
        inputs = [(name, "CF32", iq32, nsamp0)]
        if name == "d6":
            R = 8
            r.setChannelDecimator(kaiser(65, 60.0, 0.4 / R, 0.5 / R), R, nch)
            nb = torch.empty((nch, 2 * (nsamp0 // R)), dtype=torch.float32, device=dev)
            r.channel_decimate_device(iq32, nch, nsamp0, 2 * nsamp0, nb, 2 * (nsamp0 // R))
            r.setChannelDecimator(None)
            inputs.append(("d6r8", "CF32", nb, nsamp0 // R))
        r.setOutputFormat("CS16", cs16_scale)
        iq16 = torch.empty((nch, 2 * nsamp0), dtype=torch.int16, device=dev)
        r.process_channels_device(d_in, nblk, tbs, iq16)
        torch.cuda.synchronize()
        inputs.append((name, "CS16", iq16, nsamp0))
        del d_in
        for wname, fmt, d_iq, nsamp in inputs:
            r.setOutputFormat(fmt, cs16_scale if fmt == "CS16" else 1.0)
            inv_s = 1.0 / cs16_scale if fmt == "CS16" else 1.0
            amp = float(d_iq.float().abs().max().item()) * inv_s
            word = bfo_word(0.0173)
            i = torch.arange(nsamp, dtype=torch.int64, device=dev)
            phasor = torch.polar(torch.ones(nsamp, device=dev),
                                 (((i * word) & 0xffffffff).double() * (2.0 * np.pi / 2.0 ** 32)).float())
            cpc = max(1, min(nch, int(args.chunk_bytes // (nsamp * 8))))   # channels per chunk
            for mode in range(3):
                # the gain scales every mode to about +-16000, inside S16
                gain = 16000.0 / (np.pi if mode == 1 else 1.5 * amp)
                for out_fmt, oname, odt in ((AUDIO_F32, "F32", torch.float32), (AUDIO_S16, "S16", torch.int16)):
                    r.setChannelDemodulator([mode] * nch, [gain] * nch, [word] * nch, out_fmt)
                    d_out = torch.zeros((nch, nsamp), dtype=odt, device=dev)
                    ref = torch.empty((nch, nsamp), dtype=odt, device=dev)

                    def leg_a():
                        r.channel_demodulate_device(d_iq, nch, nsamp, 2 * nsamp, d_out, nsamp)

                    def leg_b():
                        for c0 in range(0, nch, cpc):
                            c1 = min(nch, c0 + cpc)
                            x = d_iq[c0:c1].view(c1 - c0, nsamp, 2)
                            x = torch.view_as_complex(x.float() * inv_s if fmt == "CS16" else x)
                            if mode == 0:
                                y = torch.abs(x) * gain
                            elif mode == 1:
                                y = torch.zeros((c1 - c0, nsamp), dtype=torch.float32, device=dev)
                                y[:, 1:] = torch.angle(x[:, 1:] * torch.conj(x[:, :-1])) * gain
                            else:
                                y = (x * phasor).real * gain
                            ref[c0:c1] = y.round().clamp(-32768, 32767).to(torch.int16) if out_fmt == AUDIO_S16 else y

                    leg_a(), leg_b()   # warm-up, and the check of leg (a): its first call after the set
                    torch.cuda.synchronize()
                    diff = (d_out.float() - ref.float()).abs().max().item()
                    ta, tb = [], []
                    for rnd in range(args.rounds + 1):
                        a, b = timed(leg_a, args.reps), timed(leg_b, 1)
                        if rnd:
                            ta.append(a), tb.append(b)
                    ma, mb = median(ta), median(tb)
                    nbytes = nch * nsamp * ((4 if fmt == "CS16" else 8) + (2 if out_fmt == AUDIO_S16 else 4))
                    cfg = {"workload": wname, "channels": nch, "nsamp": nsamp, "format": fmt, "mode": MODE_NAMES[mode],
                           "out": oname, "kernel_ms": ma, "kernel_spread_ms": max(ta) - min(ta), "composed_ms": mb,
                           "composed_over_kernel": mb / ma, "kernel_faster": ma < mb,
                           "kernel_TBps": nbytes / (ma * 1e-3) / 1e12,
                           "kernel_roofline_frac": nbytes / (ma * 1e-3) / HBM_BYTES_PER_S,
                           "maxabs_vs_composed": diff, "rounds_ms": {"kernel": ta, "composed": tb}}
                    res["configs"].append(cfg)
                    print(f"{wname:5s} {fmt} {nch:4d} ch x {nsamp:6d} {MODE_NAMES[mode]:3s} {oname}: (a) kernel {ma:8.3f} ms "
                          f"(+-{cfg['kernel_spread_ms']:.3f}) {cfg['kernel_TBps']:5.2f} TB/s "
                          f"({cfg['kernel_roofline_frac'] * 100:4.1f} % of 8 TB/s)  (b) composed {mb:8.3f} ms  b/a {mb / ma:5.1f}"
                          f"  |a - b| {diff:.2e}", flush=True)
                    if mode == 1 and out_fmt == AUDIO_F32:   # the power: FM / F32 with and without d_power
                        d_pw = torch.zeros(nch, dtype=torch.float32, device=dev)

                        def leg_p():
                            r.channel_demodulate_device(d_iq, nch, nsamp, 2 * nsamp, d_out, nsamp, d_pw)

                        leg_p()
                        torch.cuda.synchronize()
                        tn, tp = [], []
                        for rnd in range(args.rounds + 1):
                            a, p = timed(leg_a, args.reps), timed(leg_p, args.reps)
                            if rnd:
                                tn.append(a), tp.append(p)
                        pcfg = {"workload": wname, "format": fmt, "without_power_ms": median(tn), "with_power_ms": median(tp),
                                "spread_ms": max(tn) - min(tn), "rounds_ms": {"without": tn, "with": tp}}
                        res["power"].append(pcfg)
                        print(f"{wname:5s} {fmt} FM F32 power: without {median(tn):8.3f} ms (spread {pcfg['spread_ms']:.3f}), "
                              f"with {median(tp):8.3f} ms", flush=True)
                    del d_out, ref
            del phasor, i
        r.close()
        del inputs, iq32, iq16
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
