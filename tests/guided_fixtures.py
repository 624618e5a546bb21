"""Frames and the Python-integer restatement of the guided-sampling map
(wpt_sample_map, wpt_sample_map_planes, wpt_sample_map_host; the definition:
DESIGN.md section 2, "Guided sampling").

A plain helper module (no pytest hooks): tests/test_guided_cpu.py holds
wpt_sample_map_host against `reference` below, tests/test_gpu_guided.py holds the
kernels against wpt_sample_map_host on the same frames. Everything is computed
once per process and shared; nothing returned here is modified.
"""
import numpy as np

M32 = 2 ** 32 - 1
MISS_ONCE = 1
TARGET = 8
VIEWPORTS = ((1, 1), (3, 2), (17, 16), (37, 5), (130, 70))
# one more scan chunk (kBlock * kScanPer = 1024 entries) than one pass of the
# chunk-sum scan (kBlock = 256 chunks) holds: 513 * 512 + 1 entries, 257 chunks
BIG_VIEWPORT = (513, 512)
MASKS = ("all", "rank0of2", "none")
# (target, max_per_pixel)
LIMITS = ((TARGET, 1), (TARGET, M32), (TARGET, 3), (M32, M32), (M32, 1), (1, M32))


def reference(cnt, length, kind, member, target, max_pp, budget, flags):
    """The definition in Python integers: (count list in raster order or None if
    T >= 2^32, T, the sum of the counts)."""
    need = []
    for c, l, k, m in zip(cnt.reshape(-1).tolist(), length.reshape(-1).tolist(), kind.reshape(-1).tolist(),
                          member.reshape(-1).tolist()):
        if not m:
            n = 0
        elif (flags & MISS_ONCE) and k == 0:
            n = 1 if c == 0 else 0
        else:
            e = min(c + l, M32)
            n = min(target - e if target > e else 0, max_pp)
        need.append(n)
    T = sum(need)
    if T >= 2 ** 32:
        return None, T, 0
    if budget == 0 or T <= budget:
        return need, T, T
    count, p0 = [], 0
    for n in need:
        p1 = p0 + n
        count.append(p1 * budget // T - p0 * budget // T)
        p0 = p1
    return count, T, sum(count)


def budgets(T):
    """The budgets of a frame whose needs sum to T (u32 values only)."""
    return sorted({b for b in (0, 1, T - 1, T, T + 1, M32) if 0 <= b <= M32})


_PLANES = {}


def planes(w, h):
    """(cnt, len, kind) of a w x h frame. cnt: 0, TARGET - 1, TARGET, above it,
    2^32 - 1 and small values; len: 0, small values, 2^32 - 1 and values with
    which cnt + len wraps to 0 or to a small number in u32; every kind."""
    k = (w, h)
    if k not in _PLANES:
        rng = np.random.default_rng(0x9D1DED + 131 * w + h)
        n = w * h
        cnt = rng.choice(np.array([0, 1, 3, TARGET - 1, TARGET, TARGET + 3, 1000, M32], np.uint64), n)
        ln = rng.choice(np.array([0, 0, 1, 5, TARGET, M32], np.uint64), n)
        wrap = rng.random(n) < 0.2
        ln[wrap] = (2 ** 32 - cnt[wrap] + rng.integers(0, 4, int(wrap.sum())).astype(np.uint64)) & np.uint64(M32)
        kind = rng.integers(0, 3, n).astype(np.uint8)
        if n >= 6:  # every value at least once, whatever the draw
            cnt[:5] = (0, TARGET - 1, TARGET, TARGET + 3, M32)
            ln[:5] = (0, 0, 0, 0, 1)
            cnt[5], ln[5] = 5, M32 - 3  # 5 + (2^32 - 4) wraps to 1 without the saturation
            kind[:3] = (0, 1, 2)
        out = (cnt.astype(np.uint32).reshape(h, w), ln.astype(np.uint32).reshape(h, w), kind.reshape(h, w))
        for a in out:
            a.setflags(write=False)
        _PLANES[k] = out
    return _PLANES[k]


def mask(itf, name, w, h):
    """A membership plane (u8): every pixel, those of rank 0 of 2 with tile 8
    (wpt_tile_partition), or none."""
    m = np.zeros(w * h, np.uint8)
    if name == "all":
        m[:] = 1
    elif name == "rank0of2":
        m[itf.tile_partition(w, h, 0, 2, 8)] = 1
    return m.reshape(h, w)


def same(got, want, what):
    """count and (T, dealt) of two calls, bit for bit."""
    assert got[1] == want[1], (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), (what, int((got[0] != want[0]).sum()), "counts differ")
