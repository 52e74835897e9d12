#!/usr/bin/env python3
"""Digests of the channel decimator's and the channel resampler's outputs, to hold two builds of
the library against each other bit for bit (the streaming stage the two kernels share is
channel_stage.hpp; the CPU backend's is in cpu/r2iq_cpu.cpp).

A fixed list of small cases, each in CF32 and in CS16 with 3 channels (so the channel rows start off
16-byte lines), taps and samples from a fixed seed.  A case is one stream cut into successive host
calls; the tool prints one JSON line per call with the sha256 of the output's bytes.  The cases sit
where the stage can go wrong: more than one tile, calls shorter than the kept tail, an odd sample
count per channel, no tail at all, a call without an output, M = 1, L = 1, K = 1.

Only the public Python API is used, so the file runs unchanged in any checkout that has the two
stages.  Two builds agree when their outputs for the same --device are equal line for line; a GPU
and the CPU backend add in different orders and are not expected to agree with each other.

  python tools/channel_stream_digest.py --device cpu|N [--out FILE]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCH = 3
CS16_SCALE = 8192.0
# (R, ntaps, samples per call)
DECIMATE = (
    (8, 65, (5600, 8, 24)),        # two tiles, then calls shorter than the tail
    (64, 1024, (2560, 64, 128)),   # a 45-output tile
    (3, 31, (2103, 3, 9)),         # odd nsamp: the rows of CS16 and CF32 are misaligned
    (2, 1, (1200,)),               # no tail
)
# (L, M, ntaps, samples per call)
RESAMPLE = (
    (6, 125, 259, (18757, 1, 130)),   # three tiles, a call with no output
    (3, 250, 3072, (10003, 5, 600)),  # K = 1024, two tiles, a call shorter than the tail
    (4, 1, 16, (700, 1, 33)),         # M = 1
    (1, 8, 65, (4099, 8, 3)),         # L = 1
    (2, 3, 1, (301, 2)),              # K = 1
)


def samples(rng, fmt, nsamp):
    if fmt == "CS16":
        return rng.integers(-32768, 32768, (NCH, nsamp, 2), dtype=np.int16)
    x = rng.standard_normal((NCH, nsamp, 2), dtype=np.float32)
    return np.ascontiguousarray(x).view(np.complex64)[..., 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", required=True, help="'cpu' or a GPU index")
    ap.add_argument("--out", help="also write the lines to this file")
    args = ap.parse_args()

    from extio_sddc_amd import DEVICE_CPU, R2iq
    device = DEVICE_CPU if args.device == "cpu" else int(args.device)
    lines = []

    def run(stage, params, ntaps, calls, setup, call):
        for fmt in ("CF32", "CS16"):
            rng = np.random.default_rng([0x5DDC, len(lines)])
            taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
            with R2iq(gain=1.0, device=device) as r:
                r.setOutputFormat(fmt, CS16_SCALE)
                setup(r, taps)
                for i, nsamp in enumerate(calls):
                    y = np.ascontiguousarray(call(r, samples(rng, fmt, nsamp)))
                    assert y.dtype == np.complex64 and y.shape[0] == NCH
                    lines.append(json.dumps({"stage": stage, "params": params, "ntaps": ntaps, "fmt": fmt, "call": i,
                                             "nsamp": nsamp, "nout": int(y.shape[1]),
                                             "sha256": hashlib.sha256(y.tobytes()).hexdigest()}))
                    print(lines[-1], flush=True)

    for R, ntaps, calls in DECIMATE:
        run("decimate", [R], ntaps, calls, lambda r, t, R=R: r.setChannelDecimator(t, R, NCH),
            lambda r, x: r.channel_decimate(x))
    for L, M, ntaps, calls in RESAMPLE:
        run("resample", [L, M], ntaps, calls, lambda r, t, L=L, M=M: r.setChannelResampler(t, L, M, NCH),
            lambda r, x: r.channel_resample(x))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
