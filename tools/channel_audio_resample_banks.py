#!/usr/bin/env python3
"""LDS bank model of the channel audio resampler's tile (ddc_channel_audio_resample.hip): real samples,
4-byte slots, so the 4-byte instructions' banking (MI355X_MICROARCH.md LDS table: ds_read_b32 and
ds_write_b32 are served in the two 32-lane halves of a wave, each on 32 banks, the slot mod 32; a half
costs one cycle per distinct address on its busiest bank).  Sample position s of a tile sits at float
slot (s mod M) pitch + s div M.

  reads   a WAVE holds one b and 64 consecutive a; tap j of lane a reads slot ((c - j) mod M) pitch +
          (c - j) div M + a with c = o_b + K - 1: one ds_read_b32, each half on 32 consecutive slots,
          conflict-free whatever the row and the pitch.  (The IQ resampler's float2 slots took a half
          wave per b for the same reason on 64 banks; with 4-byte slots a half covers the 32 banks, and
          giving both halves one b makes every tap's row and tap set uniform over the wave.  The
          direct layout, slot s, puts a half's lanes M slots apart: conflict-free for an odd M alone.)
  stores  the stage's lane l holds samples V l + e of a 16-byte vector (V = 4 F32, 8 S16) and stores e
          with one ds_write_b32.  A half's 32 stores are V pitch slots apart until the row wraps at M,
          and V pitch is a multiple of 4 (8): within one column a half reaches 8 (4) banks at best.
          The instruction itself takes 4 cycles and the array one per half, so 2-way in both halves is
          free; the count below is the array cycles beyond 4 per instruction, summed over e.

The store count is a model at offset 0: it places lane l's samples at tile positions V l + e, while the
kernel's vector kv starts at position pg - al + kv V (the halo's length and the channel's offset to the
16-byte grid), which shifts the rows (s mod M) and with them the bank pattern.  The pitch picked is the
best for offset 0, not for every offset a call can have, and "+0 stores" is that model's figure, not a
measured one (tools/channel_resample_banks.py models the IQ kernel the same way).

layout() restates channel_audio_resample_layout (K, the tile's values of a, the LDS of the kernel
instance and the pitch the launch picks: the one in [columns needed, + 31] that the LDS holds with the
fewest extra store cycles); tests/test_channel_audio_resample_cpu.py holds the two against each other, which
pins that the C++ and this file state one rule, not that the rule is the best one.
"""
import numpy as np

LDS, LDS_SMALL, MAXA, SMALL_MIN_A, PAD = 16256, 8064, 1024, 512, 31   # ddc_kernels.h kChArs*


def store_conflicts(M, pitch, V):
    """Extra LDS cycles of the stage's V stores of one wave."""
    lanes = np.arange(64)
    cost = 0
    for e in range(V):
        p = V * lanes + e
        bank = ((p % M) * pitch + p // M) % 32
        cycles = sum(int(np.bincount(bank[g:g + 32], minlength=32).max()) for g in (0, 32))
        cost += max(0, cycles - 4)
    return cost


def best_pitch(M, need, top, V):
    """(pitch, cost): the fewest extra cycles in [need, top], the smallest pitch of equals."""
    cost, pitch = min((store_conflicts(M, p, V), p) for p in range(need, top + 1))
    return pitch, cost


def read_conflicts(M, pitch, K, transposed=True):
    """Extra cycles of one tap's read by a wave, the worst over the taps' rows (transposed), or of the
    direct layout (slot s)."""
    worst = 0
    for c in range(min(M, K + M)):
        for g in (0, 32):
            a = np.arange(g, g + 32)
            slots = (c % M) * pitch + c // M + a if transposed else a * M + c
            worst = max(worst, int(np.bincount(np.unique(slots) % 32, minlength=32).max()) - 1)
    return 2 * worst   # both halves


def layout(L, M, ntaps, in_s16):
    """(values of a per tile, LDS slots of the instance, pitch, extra store cycles)."""
    K = -(-ntaps // L)
    hcols = (K - 1 + M - 1) // M + 1

    def fit(lds):
        return min(lds // M - hcols - 1, MAXA)   # one column spare
    lds = LDS_SMALL if fit(LDS_SMALL) >= SMALL_MIN_A else LDS
    ta = fit(lds)
    need = ta + hcols
    pitch, cost = best_pitch(M, need, min(need + PAD, lds // M), 8 if in_s16 else 4)
    return ta, lds, pitch, cost


if __name__ == "__main__":
    for M in (125, 250, 16):
        print(f"direct layout, M = {M}: extra read cycles per instruction", read_conflicts(M, 0, 1024, False))
    for L, M, ntaps in ((1, 6, 97), (1, 4, 65), (24, 125, 1536), (2, 3, 40), (3, 2, 7), (32, 1, 100), (1, 256, 300),
                        (3, 250, 3072)):
        for s16 in (0, 1):
            ta, lds, pitch, cost = layout(L, M, ntaps, s16)
            K = -(-ntaps // L)
            print(f"{L:2d}/{M:3d} ntaps {ntaps:4d} K {K:4d} {'S16' if s16 else 'F32'}: tile {ta:4d} a, LDS {lds:5d} slots, "
                  f"pitch {pitch:4d} ({4 * M * pitch:5d} B) reads +{read_conflicts(M, pitch, K)} stores +{cost} "
                  f"in {8 if s16 else 4} instructions")
