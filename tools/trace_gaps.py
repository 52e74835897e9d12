#!/usr/bin/env python3
"""The d = 0 FS kernel's dispatches in a rocprofv3 kernel trace: their durations and the gaps
between consecutive ones (what the host enqueues between two launches shows up there).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python bench.py --gpus 1
  python tools/trace_gaps.py DIR [--last 100]

Prints, over the last N dispatches of r2iq_fs_kernel (the timed steps of bench.py): the median,
minimum and maximum duration, the gap from one dispatch's end to the next one's start, and the
start-to-start period.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os

import numpy as np


def fs_dispatches(trace_dir: str):
    """(path, start ns, end ns) of the FS kernel's dispatches, in start order"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {trace_dir}"
    with open(files[0]) as f:
        rows = [r for r in csv.DictReader(f) if "r2iq_fs_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    start = np.array([int(r["Start_Timestamp"]) for r in rows], dtype=np.int64)
    end = np.array([int(r["End_Timestamp"]) for r in rows], dtype=np.int64)
    return files[0], start, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--last", type=int, default=100, help="dispatches at the end of the trace to summarise")
    args = ap.parse_args()
    path, start, end = fs_dispatches(args.trace_dir)
    n = args.last
    dur = (end - start)[-n:] / 1e3
    gap = (start[1:] - end[:-1])[-n:] / 1e3
    period = np.diff(start)[-n:] / 1e3
    print(f"{os.path.basename(path)}: {start.size} FS dispatches")
    print(f"last {n} dispatches: duration median {np.median(dur):.2f} us (min {dur.min():.2f}, max {dur.max():.2f})")
    print(f"last {n} gaps end -> next start: median {np.median(gap):.2f} us (min {gap.min():.2f}, "
          f"p90 {np.percentile(gap, 90):.2f}, max {gap.max():.2f})")
    print(f"last {n} start -> start: median {np.median(period):.2f} us")


if __name__ == "__main__":
    main()
