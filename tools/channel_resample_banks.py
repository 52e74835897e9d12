#!/usr/bin/env python3
"""LDS bank model of the channel resampler's tile (ddc_channel_resample.hip), with the banking of
tools/channel_decimate_banks.py (MI355X_MICROARCH.md LDS table; a lane group costs one cycle per
distinct address on its busiest bank), for a decimation factor M that is no power of two: sample
position s of a tile sits at float2 slot (s mod M) pitch + s div M.

  reads   a half wave (lanes 0-31 or 32-63) holds one b and 32 consecutive a; tap j of lane a reads
          slot ((c - j) mod M) pitch + (c - j) div M + a with c = o_b + K - 1: one ds_read_b64 per
          wave, served in exactly those two 32-lane groups on 64 banks, i.e. on the slot mod 32.
          The two halves may sit on any two rows: they never meet in a group.  (The direct
          layout, slot s, puts a group's lanes M slots apart: conflict-free for an odd M alone,
          2-way at M = 250, 16-way at M = 16.)
  stores  the stage's lane l holds samples V l + e of a 16-byte vector (V = 2 CF32, 4 CS16) and
          stores e with one ds_write_b64: 16-lane groups on 32 banks, i.e. on the slot mod 16.
          A group's 16 stores are V pitch slots apart until the row wraps at M (then one column
          on), so an odd pitch spreads them (CS16: over 4 of the 16 slots at best, V pitch being
          a multiple of 4); with M no power of two the wrap falls inside a group, and the count
          below takes every group as it is.

layout() restates channel_resample_layout (K, the tile's values of a and the pitch the launch
picks: the one in [columns needed, + 15] that the LDS holds with the fewest extra store cycles);
tests/test_channel_resample_cpu.py holds the two against each other.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from channel_decimate_banks import store_conflicts  # noqa: E402,F401  the shared stage's stores (channel_stage.hpp)

LDS, MAXA, PAD = 8128, 512, 15   # ddc_kernels.h kChResLds, kChResMaxA, kChResPitchPad


def read_conflicts(M, pitch, K, transposed=True):
    """Extra cycles of one tap's read by a wave, the worst over the taps' rows and over the pairs
    of rows its two halves may sit on (transposed), or of the direct layout (slot s) for one b."""
    worst = 0
    for c in range(min(M, K + M)):
        slots = [(c % M) * pitch + c // M + a if transposed else a * M + c for a in range(32)]
        ks = [s % 32 for s in set(slots)]
        worst = max(worst, max(ks.count(k) for k in set(ks)) - 1)
    return 2 * worst   # both groups


def layout(L, M, ntaps, cs16):
    K = -(-ntaps // L)
    hcols = (K - 1 + M - 1) // M + 1
    room = LDS // M
    ta = min(room - hcols - 1, MAXA)   # one column spare: an odd pitch is always in reach
    need = ta + hcols
    V = 4 if cs16 else 2
    cost, pitch = min((store_conflicts(M, p, V), p) for p in range(need, min(need + PAD, room) + 1))
    return ta * L, pitch, cost


if __name__ == "__main__":
    for M in (125, 250, 16):
        print(f"direct layout, M = {M}: extra read cycles per instruction", read_conflicts(M, 0, 1024, False))
    for L, M, ntaps in ((12, 125, 1536), (6, 125, 1536), (3, 250, 3072), (1, 16, 129), (6, 125, 259), (32, 255, 4096),
                        (3, 2, 7), (4, 1, 16)):
        for cs16 in (0, 1):
            tile, pitch, cost = layout(L, M, ntaps, cs16)
            K = -(-ntaps // L)
            print(f"{L:2d}/{M:3d} ntaps {ntaps:4d} K {K:4d} {'CS16' if cs16 else 'CF32'}: tile {tile:4d} outputs "
                  f"({tile // L} a) pitch {pitch:4d} LDS {8 * M * pitch:5d} B reads +{read_conflicts(M, pitch, K)} "
                  f"stores +{cost} of {2 * (4 if cs16 else 2)} x 4 groups")
