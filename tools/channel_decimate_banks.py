#!/usr/bin/env python3
"""LDS bank model of the channel decimator's tile (ddc_channel_decimate.hip), with the banking of
tools/channel_banks.py (MI355X_MICROARCH.md LDS table; a lane group costs one cycle per distinct
address on its busiest bank): sample p of a tile sits at float2 slot (p mod R) pitch + p div R.

  reads   output o reads row offset k of a phase at slot r pitch + k + o: one ds_read_b64 per wave,
          32-lane groups on 64 banks, i.e. on the float2 slot mod 32
  stores  the stage's lane l holds samples V l + e of a 16-byte vector (V = 2 CF32, 4 CS16) and
          stores e with one ds_write_b64: 16-lane groups on 32 banks, i.e. on the slot mod 16

layout() restates channel_decimate_layout (the tile and the pitch the launch picks: the one in
[rows needed, + 15] with the fewest extra store cycles); tests/test_channel_decimate_cpu.py holds
the two against each other.  Extra LDS cycles per wave-instruction (two groups per read, four per
store and vector element):
  direct layout (slot p), R = 8: reads + 14 (8-way in both groups: 32 lanes on 4 of the 32 slots)
  transposed: reads + 0 for every (R, pitch); stores + 0 at R = 8 and 16, 2-way at R = 32 (a
  group's 16 lanes hold 16 phases of one row, an even number of pitches apart, on 16 slots)
"""
LDS, TILE, PAD = 4864, 512, 15   # ddc_kernels.h kChDecLds, kChDecTile, kChDecPitchPad


def store_conflicts(R, pitch, V):
    tot = 0
    for e in range(V):
        slots = [((V * l + e) % R) * pitch + (V * l + e) // R for l in range(64)]
        for g0 in range(0, 64, 16):
            ks = [s % 16 for s in slots[g0:g0 + 16]]
            tot += max(ks.count(k) for k in set(ks)) - 1
    return tot


def read_conflicts(R, pitch, transposed=True):
    """Extra cycles of one tap's read by a wave (outputs 0..63), the worst phase."""
    worst = 0
    for r in range(R):
        slots = [r * pitch + o if transposed else o * R + r for o in range(64)]
        tot = 0
        for g0 in range(0, 64, 32):
            ks = [s % 32 for s in set(slots[g0:g0 + 32])]
            tot += max(ks.count(k) for k in set(ks)) - 1
        worst = max(worst, tot)
    return worst


def layout(R, ntaps, cs16):
    hrows = (ntaps - 1 + R - 1) // R
    tile = min(LDS // R - PAD - hrows, TILE)
    if tile > 64:
        tile &= ~63
    need = tile + hrows
    V = 4 if cs16 else 2
    cost, pitch = min((store_conflicts(R, p, V), p) for p in range(need, need + PAD + 1))
    return tile, pitch, cost


if __name__ == "__main__":
    print("direct layout, R = 8: extra read cycles per instruction", read_conflicts(8, 0, False))
    for R, ntaps in ((8, 65), (16, 129), (32, 257), (5, 21), (3, 3), (64, 1024)):
        for cs16 in (0, 1):
            tile, pitch, cost = layout(R, ntaps, cs16)
            print(f"R {R:2d} ntaps {ntaps:4d} {'CS16' if cs16 else 'CF32'}: tile {tile:3d} pitch {pitch:4d} "
                  f"reads +{read_conflicts(R, pitch)} stores +{cost} of {2 * (4 if cs16 else 2)} x 4 groups")
