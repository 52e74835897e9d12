"""The adaptive static frame split of the d = 0 kernel on the CPU: the share table's partition
(fs_shares.h) and the controller (fs_split_controller.hpp), driven through the library's
sddc_fs_split_* entry points (the same objects the runtime uses, no device).

The plant: workgroup w starts s[w] after the launch's first one and takes ct[w] per frame (slot x
XCD x place factors), its measured end carrying relative noise.  Times are ticks of the 100 MHz
counter the kernel reads (800 per frame on average, the benchmark's 8 us), wrapped to 32 bits.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

SLOTW = 31 | (26 << 8) | (18 << 16) | (13 << 24)   # kFsSlotWeights
MAX_NS = 32768 * 11                                 # SDDC_DDC_MAX_BLOCKS x frames per block
ONE = 32768
TICKS = 800.0
ETA, STEP, CLAMP = 0.25, 1.25, 0.25                 # FsSplitController kEta, kStep, kClamp


@pytest.fixture(scope="module")
def L(ddc_lib):
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    ddc_lib.sddc_fs_split_create.restype, ddc_lib.sddc_fs_split_create.argtypes = P, [I, U]
    ddc_lib.sddc_fs_split_destroy.restype, ddc_lib.sddc_fs_split_destroy.argtypes = None, [P]
    for name, args in (("load", [P, P, I]), ("table", [P, I, P, P]), ("update", [P, P, P, P]), ("model", [P, P, P])):
        fn = getattr(ddc_lib, "sddc_fs_split_" + name)
        fn.restype, fn.argtypes = I, args
    return ddc_lib


class Ctl:
    def __init__(self, L, G, slotw=SLOTW):
        self.L, self.G = L, G
        self.c = L.sddc_fs_split_create(G, slotw)
        assert self.c

    def close(self):
        self.L.sddc_fs_split_destroy(self.c)

    def load(self, shares):
        s = np.ascontiguousarray(shares, np.float32)
        return self.L.sddc_fs_split_load(self.c, s.ctypes.data, s.size)

    def table(self, ns):
        p = np.zeros(self.G + 1, np.uint32)
        first = np.zeros(self.G + 1, np.int32)
        assert self.L.sddc_fs_split_table(self.c, ns, p.ctypes.data, first.ctypes.data) == 0
        return p, first

    def counts(self, ns):
        return np.diff(self.table(ns)[1]).astype(np.int32)

    def update(self, n, start, end):
        n = np.ascontiguousarray(n, np.int32)
        s = np.ascontiguousarray(start, np.uint32)
        e = np.ascontiguousarray(end, np.uint32)
        return self.L.sddc_fs_split_update(self.c, n.ctypes.data, s.ctypes.data, e.ctypes.data)

    def model(self):
        c, o = np.zeros(self.G), np.zeros(self.G)
        assert self.L.sddc_fs_split_model(self.c, c.ctypes.data, o.ctypes.data) == self.G
        return c, o


def builtin_counts(ns, G, slotw=SLOTW):
    """ddc_queue.hpp slot_split, restated"""
    w = [(slotw >> (8 * k)) & 0xff for k in range(4)]
    Q = G // 4

    def a(v):
        if slotw == 0 or G % 4:
            return ns * v // G
        q, i = divmod(v, Q)
        sw = sum(Q * w[k] for k in range(q)) + (i * w[q] if q < 4 else 0)
        return ns * sw // (Q * sum(w))
    return np.diff([a(v) for v in range(G + 1)]).astype(np.int32)


def check_partition(p, first, ns, G):
    assert first[0] == 0 and first[G] == ns
    assert np.all(np.diff(first.astype(np.int64)) >= 0), "ranges must be monotone"
    assert np.all(np.diff(p.astype(np.int64)) >= 0) and p[G] == ONE and p.max() <= ONE
    # the kernel's arithmetic, with a 64-bit product (ns x 32768 passes 2^32 above 131072 frames)
    want = [(int(ns) * int(p[v])) >> 15 for v in range(G)] + [ns]
    assert first.tolist() == want


NS_CASES = [1, 2, 3, 375, 376, 377, 1023, 1024, 1025, 1034, 22528, 32767, 32768, 32769, 65536, 131073, MAX_NS]


@pytest.mark.parametrize("G", [4, 376, 1024])
def test_partition_covers_every_frame_once(L, G):
    rng = np.random.default_rng(7)
    tables = {
        "random": rng.random(G) + 1e-3,
        "one workgroup takes all": np.eye(G)[G // 3],
        "first and last only": np.eye(G)[0] + np.eye(G)[G - 1],
        "alternating empty": np.arange(G) % 2,
        "reversed slots": np.repeat([13.0, 18.0, 26.0, 31.0], G // 4),
        "tiny and huge": np.where(rng.random(G) < 0.5, 1e-6, 1.0),
    }
    k = Ctl(L, G)
    try:
        for ns in NS_CASES:
            p, first = k.table(ns)        # the cold controller: the built-in costs
            check_partition(p, first, ns, G)
        for name, sh in tables.items():
            assert k.load(sh) == 0, name
            for ns in NS_CASES:
                p, first = k.table(ns)
                check_partition(p, first, ns, G)
            if name == "one workgroup takes all":
                n = np.diff(k.table(1034)[1])
                assert n[G // 3] == 1034 and n.sum() == 1034   # every other range is empty
        assert k.load(np.zeros(G)) != 0 and k.load(-np.ones(G)) != 0 and k.load(np.ones(G + 1)) != 0
        assert k.load(np.zeros(0, np.float32)) == 0
        # clamped extremes: garbage measurements drive the costs to their bounds
        for it in range(60):
            n = k.counts(22528)
            st = rng.integers(0, 2 ** 32, G, dtype=np.uint64).astype(np.uint32)
            en = st + rng.integers(1, 2 ** 30, G, dtype=np.uint64).astype(np.uint32)
            k.update(n, st, en)
        for ns in NS_CASES:
            p, first = k.table(ns)
            check_partition(p, first, ns, G)
    finally:
        k.close()


def test_cold_start_is_the_builtin_split(L):
    for G, ns in ((1024, 22528), (1024, 1034), (376, 1034), (1024, 32768)):
        k = Ctl(L, G)
        try:
            n, base = k.counts(ns), builtin_counts(ns, G)
            assert n.sum() == ns
            lo, hi = np.floor(base * (1 - CLAMP)), np.ceil(base * (1 + CLAMP))
            assert np.all(n >= lo) and np.all(n <= hi)
            if (G, ns) == (1024, 22528):   # the benchmark's shape: 31 / 26 / 18 / 13 frames exactly
                assert n.tolist() == base.tolist()
        finally:
            k.close()


def plant(G, rng, slot=(1.0, 1.0, 1.0, 1.0), xcd_even=0.0, place_rms=0.0, start_max=0.0):
    w = np.arange(G)
    wk = np.array([(SLOTW >> (8 * k)) & 0xff for k in range(4)], float)
    c0 = wk.sum() / 4 / wk[w * 4 // G]
    ct = c0 * np.array(slot)[w * 4 // G] * (1 + xcd_even * (w % 2 == 0))
    ct = ct * (1 + place_rms * rng.standard_normal(G // 4))[w % (G // 4)]
    return ct, start_max * rng.random(G)


def launch(ct, s, n, rng, noise):
    """ticks: start and end per workgroup of one launch, from a random counter origin"""
    t0 = int(rng.integers(0, 2 ** 32))
    dur = n * ct * (1 + noise * rng.standard_normal(n.size))
    st = (t0 + np.rint(s * TICKS).astype(np.int64)) % 2 ** 32
    en = (st + np.maximum(np.rint(dur * TICKS).astype(np.int64), 1)) % 2 ** 32
    return st.astype(np.uint32), en.astype(np.uint32)


def ends(ct, s, n):
    return s + n * ct


def best_makespan(ct, s, ns, base):
    """the integer split with the earliest last end, for known costs, within the clamps"""
    lo, hi = np.floor(base * (1 - CLAMP)), np.ceil(base * (1 + CLAMP))
    a, b = 0.0, float(np.max(s + (hi + 1) * ct))
    for _ in range(60):
        T = 0.5 * (a + b)
        if np.clip(np.floor((T - s) / ct), lo, hi).sum() >= ns:
            b = T
        else:
            a = T
    return b


def test_converges_on_a_slot_xcd_place_plant(L):
    G, ns, noise = 1024, 22528, 0.01
    rng = np.random.default_rng(11)
    # the measured box: slot 0 ends ~8 % early, slot 3 ~4 % late, even XCDs 2 % slow, 0.5 % per place
    ct, s = plant(G, rng, slot=(0.93, 0.99, 1.01, 1.05), xcd_even=0.02, place_rms=0.005, start_max=0.7)
    base = builtin_counts(ns, G)
    k = Ctl(L, G)
    try:
        for it in range(40):
            n = k.counts(ns)
            assert n.sum() == ns
            st, en = launch(ct, s, n, rng, noise)
            assert k.update(n, st, en) == 1
        n = k.counts(ns)
    finally:
        k.close()
    e0, e1 = ends(ct, s, base), ends(ct, s, n)
    best = best_makespan(ct, s, ns, base)
    print(f"built-in: max {e0.max():.3f} mean {e0.mean():.3f}; adapted: max {e1.max():.3f} mean {e1.mean():.3f}; "
          f"best {best:.3f} (frame times)")
    # A damped average of measurements with relative noise sigma carries sigma sqrt(eta / (2 - eta))
    # (0.38 % here); the split puts a workgroup's end at the common T of its estimated cost, so
    # the last end lies above the best split's by the largest of 1024 such errors: 4 deviations
    # bound it.  And the spread above the mean end has shrunk.
    assert e1.max() <= best * (1 + 4 * noise * np.sqrt(ETA / (2 - ETA)))
    assert e1.max() < e0.max()
    assert e1.max() - e1.mean() < 0.6 * (e0.max() - e0.mean())


def test_pure_noise_plant_does_not_grow_the_spread(L):
    G, ns, noise = 1024, 22528, 0.01
    rng = np.random.default_rng(13)
    ct, s = plant(G, rng)            # exactly the built-in weights' costs: the built-in split is ideal
    base = builtin_counts(ns, G)
    k = Ctl(L, G)
    try:
        worst = 0.0
        for it in range(60):
            n = k.counts(ns)
            st, en = launch(ct, s, n, rng, noise)
            assert k.update(n, st, en) == 1
            worst = max(worst, ends(ct, s, k.counts(ns)).max())
    finally:
        k.close()
    e0 = ends(ct, s, base)
    print(f"built-in max end {e0.max():.3f}, worst adapted {worst:.3f} frame times")
    # no frame moves onto a workgroup that ends last: a moved frame would add 0.7 .. 1.7 frame times
    assert worst <= e0.max() * (1 + noise)


def test_one_garbage_launch_moves_little(L):
    G, ns = 1024, 22528
    rng = np.random.default_rng(17)
    base = builtin_counts(ns, G)
    lo, hi = np.floor(base * (1 - CLAMP)), np.ceil(base * (1 + CLAMP))
    up, dn = 1 + ETA * (STEP - 1), 1 + ETA * (1 / STEP - 1)   # one step's bounds, before the rescale
    cases = {
        "random words": (rng.integers(0, 2 ** 32, G, dtype=np.uint64), rng.integers(0, 2 ** 32, G, dtype=np.uint64)),
        "one workgroup 1000 x late": (np.zeros(G, np.uint64), np.where(np.arange(G) == 5, 10 ** 7, 10 ** 4).astype(np.uint64)),
        "all equal": (np.full(G, 123, np.uint64), np.full(G, 456, np.uint64)),
        "zero durations": (np.full(G, 99, np.uint64), np.full(G, 99, np.uint64)),
        "half the chip stalled": (np.zeros(G, np.uint64), np.where(np.arange(G) % 2 == 0, 10 ** 8, 10 ** 4).astype(np.uint64)),
    }
    for name, (st, en) in cases.items():
        k = Ctl(L, G)
        try:
            c0, _ = k.model()
            used = k.update(base, st.astype(np.uint32), en.astype(np.uint32))
            c1, _ = k.model()
            if not used:
                assert np.array_equal(c0, c1), name
            r = c1 / c0
            assert r.max() <= up / dn * (1 + 1e-9) and r.min() >= dn / up * (1 - 1e-9), (name, r.min(), r.max())
            n = k.counts(ns)
            assert n.sum() == ns and np.all(n >= lo) and np.all(n <= hi), name
            assert np.abs(n - base).max() <= np.ceil(base * (up / dn - 1)).max() + 1, name
        finally:
            k.close()
