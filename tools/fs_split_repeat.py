#!/usr/bin/env python3
"""How much of the d = 0 kernel's workgroup end-time spread repeats from launch to launch, from a
stamps build (ddc_stamps.hpp, -DSDDC_STAMPS=1): the measurement behind the adaptive frame split
(profiles/adaptive_split/).

  EXTRA=-DSDDC_STAMPS=1 tools/build_rev_lib.sh tree stamps1
  python tools/fs_split_repeat.py --lib build/ab/stamps1.so [--launches 12] [--param 10=0]

After ~2 s of back-to-back launches it runs `--launches` launches, copying the stamp buffer out
after each, and reports per launch the end-time distribution, then over the launches:
  - the deviation of each workgroup's end from its launch's mean, split into the part that repeats
    (the workgroup's mean over the launches) and the rest (noise), the repeating part further by
    slot (blockIdx quarter), XCD (blockIdx % 8), slot x XCD, place within the quarter and the
    individual workgroup;
  - whether blockIdx lands on the same CU and CU slot (HW_ID) every launch;
  - what a split fitted to the first launches would have done to the last one (each workgroup's
    measured time per frame of the last launch x the frames a model's split gives it).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEGS = 13


def capture(lib, nblk, tb, launches, params, gap_sync):
    import torch
    from extio_sddc_amd._lib import SIGNATURES
    L = ctypes.CDLL(os.path.abspath(lib))
    for name, (res, a) in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, a
    getst = L.sddc_ddc_internal_fs_stamps
    getst.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.sddc_ddc_internal_set_param.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    h = ctypes.c_void_p()
    assert L.sddc_ddc_create(1.0, 0, ctypes.byref(h)) == 0
    L.sddc_ddc_set_tunebin(h, tb)
    L.sddc_ddc_set_decimation(h, 0)
    for k, v in params:
        assert L.sddc_ddc_internal_set_param(h, k, v) == 0
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0x5DDC)
    d_in = torch.randint(-32768, 32767, (4096 + nblk * 65536,), dtype=torch.int16, device=dev, generator=g)
    out = torch.empty(nblk * 32768 * 2, dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    t_end = time.time() + 2.0
    while time.time() < t_end:
        for _ in range(10):
            assert L.sddc_ddc_process_device(h, d_in.data_ptr(), nblk, out.data_ptr(), s) == 0
        torch.cuda.synchronize()
    wpw = ctypes.c_int()
    getst(None, 0, ctypes.byref(wpw))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = 4 * cus
    caps = []
    for _ in range(launches):
        # a launch behind nine others, as in a stream of them (gap_sync: alone after a sync)
        for _ in range(1 if gap_sync else 10):
            assert L.sddc_ddc_process_device(h, d_in.data_ptr(), nblk, out.data_ptr(), s) == 0
        torch.cuda.synchronize()
        buf = np.zeros(G * 4 * wpw.value, np.uint32)
        assert getst(buf.ctypes.data, buf.size, None) == 0
        caps.append(buf.reshape(G, 4, wpw.value)[:, 0, :].copy())
    table = None
    if hasattr(L, "sddc_ddc_internal_fs_split_state"):   # the adaptive split's state after these launches
        fn = L.sddc_ddc_internal_fs_split_state
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        info, counts = (ctypes.c_long * 5)(), np.zeros(G, np.int32)
        n = fn(h, info, counts.ctypes.data, G)
        table = {"measured": info[1], "skipped": info[2], "last_launch_took_table": info[3], "frames": counts[:n].tolist()}
    L.sddc_ddc_destroy(h)
    return np.stack(caps), G, table


def pct(x):
    return (f"min {x.min():.1f} p10 {np.percentile(x, 10):.1f} p50 {np.median(x):.1f} "
            f"p90 {np.percentile(x, 90):.1f} max {x.max():.1f}")


def makespan_alloc(s, tau, ns, lo, hi):
    """integer frames per workgroup minimising max(s + n tau), lo <= n <= hi, sum n = ns"""
    a, b = 0.0, float(np.max(s + hi * tau)) + 1.0
    for _ in range(60):
        T = 0.5 * (a + b)
        n = np.clip(np.floor((T - s) / tau), lo, hi)
        if n.sum() >= ns:
            b = T
        else:
            a = T
    n = np.clip(np.floor((b - s) / tau), lo, hi).astype(np.int64)
    extra = int(n.sum() - ns)
    if extra > 0:   # drop the surplus where the end is latest
        order = np.argsort(-(s + n * tau))
        for w in order:
            if extra == 0:
                break
            if n[w] > lo[w]:
                n[w] -= 1
                extra -= 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--nblk", type=int, default=2048)
    ap.add_argument("--tunebin", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--gap-sync", action="store_true", help="each captured launch alone after a synchronise")
    ap.add_argument("--param", action="append", default=[], help="PARAM=VALUE (sddc_ddc_internal_set_param)")
    args = ap.parse_args()
    params = [tuple(int(v) for v in kv.split("=")) for kv in args.param]
    st, G, table = capture(args.lib, args.nblk, args.tunebin, args.launches, params, args.gap_sync)
    N = st.shape[0]
    fr = st[:, :, 2 * SEGS].astype(np.float64)
    rs = st[:, :, 2 * SEGS + 4].astype(np.int64)
    re = st[:, :, 2 * SEGS + 5].astype(np.int64)
    hw = st[:, :, 2 * SEGS + 6].astype(np.int64)
    t0 = rs.min(axis=1, keepdims=True)
    start = ((rs - t0) & 0xffffffff) * 0.01   # us; the 100 MHz constant-rate counter's low word
    end = ((re - t0) & 0xffffffff) * 0.01
    w = np.arange(G)
    slot, xcd, place = w * 4 // G, w % 8, w % (G // 4)
    print(f"{os.path.basename(args.lib)}: {N} launches, G = {G}, nblk = {args.nblk}, tune bin {args.tunebin}")
    for i in range(N):
        print(f"  launch {i}: end {pct(end[i])}; start max {start[i].max():.1f}; frames {fr[i].min():.0f}..{fr[i].max():.0f}")
    print("  all launches, end: " + pct(end.ravel()) + f"; mean of the launches' max {end.max(axis=1).mean():.1f}, "
          f"of their means {end.mean(axis=1).mean():.1f} us")
    for q in range(4):
        print(f"    slot {q}: end p50 {np.median(end[:, slot == q]):.1f} us, frames p50 {np.median(fr[:, slot == q]):.0f}")
    print("    end p50 by XCD: " + " ".join(f"{np.median(end[:, xcd == x]):.1f}" for x in range(8)))
    dev = end - end.mean(axis=1, keepdims=True)
    rep = dev.mean(axis=0)                 # the repeating part, per workgroup
    noise = dev - rep
    comp = {}
    r = rep.copy()
    m = np.array([r[slot == q].mean() for q in range(4)])[slot]
    comp["slot"] = m
    r = r - m
    m = np.array([r[xcd == x].mean() for x in range(8)])[xcd]
    comp["xcd"] = m
    r = r - m
    sx = slot * 8 + xcd
    m = np.array([r[sx == k].mean() for k in range(32)])[sx]
    comp["slot x xcd"] = m
    r = r - m
    m = np.array([r[place == p].mean() for p in range(G // 4)])[place]
    comp["place in quarter"] = m
    r = r - m
    comp["individual workgroup"] = r
    print(f"  deviation from the launch mean: total rms {dev.std():.2f} us = repeating {rep.std():.2f} + "
          f"noise {noise.std():.2f} (rms over launches and workgroups)")
    # the mean of N noisy launches still carries noise / sqrt(N): the repeating rms an all-noise
    # plant would show
    print(f"    (an all-noise plant would show a repeating rms of {noise.std() / np.sqrt(N):.2f} us)")
    for kname, v in comp.items():
        print(f"    repeating, {kname:22s} rms {v.std():.2f} us, range {v.min():+.1f} .. {v.max():+.1f}")
    # split-half: does the individual part of the first half of the launches predict the second's?
    h1, h2 = dev[: N // 2].mean(axis=0), dev[N // 2:].mean(axis=0)
    for kname, key in (("slot x xcd", sx), ("place", place)):
        a1 = np.array([h1[key == k].mean() for k in np.unique(key)])
        a2 = np.array([h2[key == k].mean() for k in np.unique(key)])
        print(f"    split-half correlation of the {kname} means: {np.corrcoef(a1, a2)[0, 1]:.3f}")
    i1 = h1 - np.array([h1[sx == k].mean() for k in range(32)])[sx]
    i2 = h2 - np.array([h2[sx == k].mean() for k in range(32)])[sx]
    print(f"    split-half correlation per workgroup beyond slot x xcd: {np.corrcoef(i1, i2)[0, 1]:.3f}")
    cu = (hw >> 8) & 0xfff   # HW_ID CU_ID, SH_ID, SE_ID, TG_ID
    same = (cu == cu[0]).all(axis=0)
    print(f"  blockIdx on the same CU and CU slot (HW_ID bits 8..19) in every launch: {int(same.sum())} of {G}")
    tg = (hw >> 16) & 0xf
    print("    TG_ID == blockIdx quarter: " + " ".join(f"{int((tg[i] == slot).sum())}" for i in range(N)))
    # what a fitted split would have done to the last launch
    tau = (end - start) / np.maximum(fr, 1)
    last_tau, last_s = tau[-1], start[-1]
    ns = int(fr[-1].sum())
    fit_tau, fit_s = tau[:-1].mean(axis=0), start[:-1].mean(axis=0)
    base = fr[-1]
    lo, hi = np.floor(base * 0.75), np.ceil(base * 1.25)
    res = {"measured": float(end[-1].max())}
    print(f"  the last launch: max end {end[-1].max():.1f}, mean end {end[-1].mean():.1f} us; splits fitted to the "
          f"launches before it, applied to its own times per frame:")
    for kname, key in (("slot", slot), ("slot x xcd", sx), ("workgroup", w)):
        t = np.array([fit_tau[key == k].mean() for k in np.unique(key)])[np.searchsorted(np.unique(key), key)]
        s_ = np.array([fit_s[key == k].mean() for k in np.unique(key)])[np.searchsorted(np.unique(key), key)]
        n = makespan_alloc(s_, t, ns, lo, hi)
        e = last_s + n * last_tau
        res[kname] = float(e.max())
        print(f"    {kname:12s}: max end {e.max():.1f} p90 {np.percentile(e, 90):.1f} mean {e.mean():.1f} us "
              f"(frames {n.min()}..{n.max()}); {100 * (1 - e.max() / end[-1].max()):+.1f} % of the launch")
    if table is not None:
        fr_t = np.array(table["frames"])
        print(f"  adaptive split: {table['measured']} measurements used, {table['skipped']} skipped, last launch took a "
              f"table: {table['last_launch_took_table']}")
        if fr_t.size == G:
            for q in range(4):
                v = fr_t[slot == q]
                print(f"    table, slot {q}: frames min {v.min()} mean {v.mean():.2f} max {v.max()}; even XCDs "
                      f"{fr_t[(slot == q) & (xcd % 2 == 0)].mean():.2f}, odd {fr_t[(slot == q) & (xcd % 2 == 1)].mean():.2f}")
            print("    table frames per workgroup: " + json.dumps(table["frames"]))
    print(json.dumps({"lib": os.path.basename(args.lib), "launches": N, "end_rms_us": float(dev.std()),
                      "repeating_rms_us": float(rep.std()), "noise_rms_us": float(noise.std()),
                      "components_rms_us": {k: float(v.std()) for k, v in comp.items()},
                      "same_hw_place": int(same.sum()), "last_launch_max_end_us": res}))


if __name__ == "__main__":
    main()
