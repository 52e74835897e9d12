#!/usr/bin/env python3
"""Timing of the channel audio resampler on one GPU (bench.py stays the flagship benchmark).

Rows, each on buffers resident in device memory, F32 -> F32 and S16 -> S16:
  large  1024 channels x 524288 real samples at 1/6 with 97 taps, 1/4 with 65 taps and 24/125 with
         1536 taps (the 48 kS/s discriminator output to a 8 / 12 kS/s sense stream; 250 kS/s WFM to 48 k)
  small  128 x 131072 and 1024 x 960 at 1/4 with 65 taps
with Kaiser taps from sddc_ddc_kaiser, scaled by L.  The inputs are Gaussian noise of sigma 3000 (S16:
rounded).  Four legs on the same device buffers, timed with HIP events in interleaved rounds in ONE
process (as tools/channel_resample_bench.py does):
  (a) sddc_ddc_channel_audio_resample_device (the tails zeroed once, then advancing: the cost per call
      does not depend on their content; the count per call moves by one with the position);
  (c) a device copy_ of the input plus one of the output: what moving the stage's bytes costs;
  (i) sddc_ddc_channel_resample_device, the IQ resampler, on the widened CF32 stream (x, 0) with the
      same taps and ratio: twice the bytes, LDS traffic and fmas;
  (b) the path a caller composes without the stage: for each b < L one torch conv1d with stride M over
      the buffer with the reversed taps of phase (b M) mod L, offset by (b M) div L samples, K - 1 zeros
      in front, interleaved into the output, including the int16 -> float and the rounding passes under
      S16 (in chunks of channels, so its buffers stay at about 1 GB).
Leg (a) (first call after the set) is checked against leg (b), and bit for bit against the real part of
leg (i) under F32.  Prints a line per row and one JSON line: ms (median of the rounds), input samples
per second, the bytes leg (a) moves per second (in + out) against the 8 TB/s HBM roofline, and the
ratios (i) / (a), (b) / (a), (a) / (c).

  python tools/channel_audio_resample_bench.py [--rounds 5] [--rows large small] [--out FILE]
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
LARGE = [(1024, 524288, r) for r in ((1, 6, 97), (1, 4, 65), (24, 125, 1536))]
SMALL = [(128, 131072, (1, 4, 65)), (1024, 960, (1, 4, 65))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", choices=["large", "small"], default=["large", "small"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="launches per timed window of legs (a), (c), (i)")
    ap.add_argument("--chunk-bytes", type=float, default=1e9, help="leg (b): bytes of float input per chunk of channels")
    ap.add_argument("--heat-s", type=float, default=2.0)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    from extio_sddc_amd import AUDIO_F32, AUDIO_S16, R2iq, kaiser, resample_count
    assert torch.cuda.is_available(), "channel_audio_resample_bench needs a GPU"
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
    rows = (LARGE if "large" in args.rows else []) + (SMALL if "small" in args.rows else [])
    r = R2iq(gain=1.0)
    heated = False
    for nch, nsamp, (L, M, ntaps) in rows:
        x32 = torch.randn((nch, nsamp), dtype=torch.float32, device=dev, generator=g) * 3000.0
        iq = torch.zeros((nch, 2 * nsamp), dtype=torch.float32, device=dev)   # (x, 0)
        iq[:, 0::2] = x32
        h = taps_for(L, M, ntaps)
        K = -(-ntaps // L)
        nout = resample_count(L, M, 0, nsamp)
        r.setChannelResampler(h, L, M, nch)
        z = torch.empty((nch, 2 * (nout + 1)), dtype=torch.float32, device=dev)

        def leg_i():
            r.channel_resample_device(iq, nch, nsamp, 2 * nsamp, z, 2 * (nout + 1))

        if not heated:   # heat the chip so every leg is timed at the sustained clock
            t_end = time.time() + args.heat_s
            while time.time() < t_end:
                leg_i()
                torch.cuda.synchronize()
            heated = True
        hp = np.zeros(L * K, np.float32)
        hp[:ntaps] = h
        # phase (b M) mod L reversed, as conv1d correlates
        ws = [torch.from_numpy(hp[(b * M) % L::L][::-1].copy()).to(dev).view(1, 1, K) for b in range(L)]
        cpc = max(1, min(nch, int(args.chunk_bytes // (nsamp * 4))))   # channels per chunk
        for fmt, name in ((AUDIO_F32, "F32"), (AUDIO_S16, "S16")):
            s16 = fmt == AUDIO_S16
            dt = torch.int16 if s16 else torch.float32
            d_in = x32.round().clamp(-32768, 32767).to(torch.int16) if s16 else x32
            r.setChannelAudioResampler(h, L, M, nch, fmt, fmt)
            d_out = torch.zeros((nch, nout + 1), dtype=dt, device=dev)
            d_out[:, nout] = 12345
            ref = torch.empty((nch, nout), dtype=dt, device=dev)
            c_in, c_out = torch.empty_like(d_in), torch.empty_like(d_out)

            def leg_a():
                r.channel_audio_resample_device(d_in, nch, nsamp, nsamp, d_out, nout + 1)

            def leg_c():
                c_in.copy_(d_in)
                c_out.copy_(d_out)

            def leg_b():
                for c0 in range(0, nch, cpc):
                    c1 = min(nch, c0 + cpc)
                    xx = F.pad((d_in[c0:c1].float() if s16 else d_in[c0:c1]).view(c1 - c0, 1, nsamp), (K - 1, 0))
                    for b in range(L):
                        nb = -(-(nout - b) // L)   # outputs a L + b < nout
                        y = F.conv1d(xx[:, :, (b * M) // L:], ws[b], stride=M)[:, 0, :nb]
                        ref[c0:c1, b::L] = y.round().clamp(-32768, 32767).to(torch.int16) if s16 else y

            r.resetChannelResampler()
            leg_a(), leg_b(), leg_i()   # warm-up, and the checks of leg (a): its first call after the set
            torch.cuda.synchronize()
            got = d_out[:, :nout]
            assert bool((d_out[:, nout] == 12345).all())
            scale = ref.float().abs().max().item()
            vs_b = (got.float() - ref.float()).abs().max().item() / scale
            assert vs_b < (2.0 / scale + 1e-4 if s16 else 1e-4), vs_b
            bit_equal = None
            if not s16:
                zz = z.view(nch, nout + 1, 2)[:, :nout]
                bit_equal = bool(torch.equal(zz[:, :, 0].contiguous().view(torch.int32), got.contiguous().view(torch.int32))
                                 and bool((zz[:, :, 1] == 0).all()))
                assert bit_equal
            ta, tb, tc, ti = [], [], [], []
            for rnd in range(args.rounds + 1):
                a, c, i, b = timed(leg_a, args.reps), timed(leg_c, args.reps), timed(leg_i, args.reps), timed(leg_b, 1)
                if rnd:
                    ta.append(a), tb.append(b), tc.append(c), ti.append(i)
            ma, mb, mc, mi = median(ta), median(tb), median(tc), median(ti)
            nbytes = nch * (nsamp + nout) * (2 if s16 else 4)
            cfg = {"channels": nch, "nsamp": nsamp, "format": name, "up": L, "down": M, "ntaps": ntaps, "nout": nout,
                   "kernel_ms": ma, "copy_ms": mc, "iq_resampler_ms": mi, "composed_ms": mb,
                   "iq_over_kernel": mi / ma, "kernel_faster_than_iq": ma < mi, "composed_over_kernel": mb / ma,
                   "kernel_over_copy": ma / mc, "kernel_GSps": nch * nsamp / (ma * 1e-3) / 1e9,
                   "kernel_TBps": nbytes / (ma * 1e-3) / 1e12, "kernel_roofline_frac": nbytes / (ma * 1e-3) / HBM_BYTES_PER_S,
                   "maxrel_vs_composed": vs_b, "bit_equal_to_iq_real_part": bit_equal,
                   "rounds_ms": {"kernel": ta, "copy": tc, "iq_resampler": ti, "composed": tb}}
            res["configs"].append(cfg)
            print(f"{name} {nch:4d} ch x {nsamp:6d} {L:2d}/{M:3d} taps {ntaps:4d}: (a) kernel {ma:7.3f} ms {cfg['kernel_GSps']:6.1f} GS/s "
                  f"{cfg['kernel_TBps']:5.2f} TB/s ({cfg['kernel_roofline_frac'] * 100:4.1f} % of 8 TB/s)  (c) copy {mc:7.3f} ms  "
                  f"(i) IQ resampler on (x, 0) {mi:7.3f} ms  i/a {mi / ma:4.2f}  (b) composed {mb:8.3f} ms  b/a {mb / ma:5.1f}  "
                  f"vs composed {vs_b:.1e}", flush=True)
            del d_out, ref, c_in, c_out, d_in
        del x32, iq, z
        torch.cuda.empty_cache()
    r.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
