"""Fixtures for the adaptive round planner (wpt_adaptive.h, Renderer::
estimate_errors / plan_counts; oracle: adaptive_error / adaptive_plan):
synthetic acc / cnt frames for the error stage and (errors, stats) inputs for
the plan stage, each built to sit on one of the planner's decisions. numpy
only, deterministic. test_adaptive_cpu.py asserts on the oracle alone that
they reach what they were built for; test_gpu_adaptive.py sends them through
the device.

A frame is (acc (H, W, 3) f32 sums, cnt (H, W) u32 counts); screen half 0 is
x < W // 2, half 1 the rest (the wider one when W is odd). A plan input's view
has alpha 255 everywhere, as every sampling view has (SimpleRenderTarget
allocates it so and never writes alpha).
"""
import collections
import functools

import numpy as np

F32 = np.float32
TILE = 16          # kMseTile
SUM_CHUNK = 512    # kSumChunk
SCAN_CHUNK = 1024  # kScanChunk = kBlock * kScanPer

# (W, H): stencil larger than the viewport; one full tile + a tile of one
# column, second tile row one pixel high; the tested size; a ragged one; the
# large one (41 x 25 tiles per half, 513 scan blocks, 513 sum chunks per half)
SIZES = [(2, 1), (3, 2), (5, 3), (33, 17), (40, 24), (62, 35), (1312, 400)]
LARGE = (1312, 400)
TINY_EXPONENTS = list(range(-60, -76, -1))  # impulse amplitudes 2^-60 .. 2^-75

Frame = collections.namedtuple("Frame", "name acc cnt")
SPECIAL_KINDS = ("cnt0", "negative", "negzero", "above", "posinf", "neginf", "nan", "cnt2p24")


def half_span(W, half):
    """[x0, x1) of a screen half."""
    return (W // 2, W) if half else (0, W // 2)


def _black(W, H):
    return np.zeros((H, W, 3), F32), np.ones((H, W), np.uint32)


def grey(W, H):
    """Uniform dyadic grey: 8 samples of 0.375. Every blur is exactly 0.375
    (the products m * 0.375 and their sums are small dyadic numbers), so every
    error is exactly 0, mn == mx and the sum is 0."""
    return Frame("grey", np.full((H, W, 3), 3.0, F32), np.full((H, W), 8, np.uint32))


def impulse(W, H, x, y, amp=1.0, name=None):
    acc, cnt = _black(W, H)
    acc[y, x, :] = F32(amp)
    return Frame(name or f"impulse@{x},{y}", acc, cnt)


def impulse_positions(W, H):
    """Corners, edge midpoints, both sides of the seam, both sides of the tile
    boundaries (15, 16, 17 from the frame's and from the right half's origin),
    each clipped to the viewport; sorted, unique."""
    half = W // 2
    xs = {0, W - 1, W // 4, half - 1, half, half + 1, 15, 16, 17, half + 15, half + 16, half + 17}
    ys = {0, H - 1, H // 2, 15, 16, 17}
    xs = sorted(x for x in xs if 0 <= x < W)
    ys = sorted(y for y in ys if 0 <= y < H)
    return [(x, y) for y in ys for x in xs]


def impulses_spread(W, H):
    """The large frame's impulses in one frame, no two stencils overlapping
    (6 apart or more in x or in y): a grid of columns and rows on both sides
    of tile boundaries (x, y mod 16 in {15, 0, 1}), the corners and edges, the
    seam's right side, the last tile column and row; the seam's left side and
    the last tile's first column on rows of their own."""
    assert (W, H) == LARGE
    half = W // 2
    cols = [0, 15, 32, 49, half // 2, half - 17, half, half + 17, W - 17, W - 1]
    rows = [0, 15, 32, 49, H // 2, H - 33, H - 16, H - 1]
    at = [(x, y) for y in rows for x in cols] + [(x, y + 8) for y in (0, H // 2, H - 16) for x in (half - 1, W - 16)]
    acc, cnt = _black(W, H)
    for i, (x, y) in enumerate(at):
        assert all(abs(x - a) > 5 or abs(y - b) > 5 for a, b in at[:i]), (x, y)
        acc[y, x, :] = 1.0
    return Frame("impulses", acc, cnt), at


def noise(W, H, seed=0xADA0):
    r = np.random.default_rng([seed, W, H])
    cnt = r.integers(1, 65, (H, W)).astype(np.uint32)
    acc = (r.random((H, W, 3), dtype=F32) * cnt[..., None].astype(F32)).astype(F32)
    return Frame("noise", acc, cnt)


def special(W, H, seed=0xADA1):
    """Noise with special pixels sprinkled in (about one pixel in 12, every
    kind in turn; a frame smaller than 8 pixels holds the first kinds only).
    Returns the frame and kind -> flat pixel indices."""
    f = noise(W, H, seed)
    acc, cnt = f.acc.copy(), f.cnt.copy()
    r = np.random.default_rng([seed, W, H, 1])
    n = W * H
    k = min(n, max(len(SPECIAL_KINDS), n // 12))
    where = r.choice(n, size=k, replace=False)
    kinds = {name: where[i::len(SPECIAL_KINDS)] for i, name in enumerate(SPECIAL_KINDS)}
    a, c = acc.reshape(n, 3), cnt.reshape(n)
    c[kinds["cnt0"]] = 0
    a[kinds["cnt0"][::2]] = 0.0  # 0 / 0; the others x / 0
    a[kinds["negative"]] *= F32(-1.0)
    a[kinds["negzero"]] = F32(-0.0)
    a[kinds["above"]] = a[kinds["above"]] * F32(3.0) + c[kinds["above"], None].astype(F32)
    a[kinds["posinf"], 0] = np.inf
    a[kinds["neginf"], 1] = -np.inf
    a[kinds["nan"], 2] = np.nan
    c[kinds["cnt2p24"]] = (1 << 24) + 1  # (float)cnt rounds to 2^24
    a[kinds["cnt2p24"]] = (r.random((len(kinds["cnt2p24"]), 3), dtype=F32) * F32(1 << 24)).astype(F32)
    return Frame("special", acc, cnt), kinds


def binades(W, H, seed=0xADA2):
    """Noise whose amplitude grows by rows from 2^-12 to 1: the errors span
    more than 20 binades, small ones first, so the running sum keeps crossing
    binades as larger ones arrive."""
    f = noise(W, H, seed)
    k = 12 - (13 * np.arange(H)) // max(H, 1)
    scale = np.ldexp(F32(1.0), -k).astype(F32)
    return Frame("binades", (f.acc * scale[:, None, None]).astype(F32), f.cnt)


def last_tile(W, H, seed=0xADA6):
    """Dim noise (means below 0.25) whose smallest and largest error both lie
    in the last tile of each half alone (tile 1024 of 1025 on the large frame,
    the one entry k_mm_reduce's threads read in their second pass): there a
    flat 7 x 7 patch of dyadic grey, whose inner 3 x 3 errors are exactly 0,
    and one saturated pixel."""
    f = noise(W, H, seed)
    acc = (f.acc * F32(0.25)).astype(F32)
    cnt = f.cnt.copy()
    for half in (0, 1):
        x0, x1 = half_span(W, half)
        tx, ty = x0 + (x1 - x0 - 1) // TILE * TILE, (H - 1) // TILE * TILE
        acc[ty + 1:ty + 8, tx + 1:tx + 8] = 3.0
        cnt[ty + 1:ty + 8, tx + 1:tx + 8] = 8
        acc[ty + 12, tx + 12] = cnt[ty + 12, tx + 12]
    return Frame("last_tile", acc, cnt)


@functools.lru_cache(maxsize=None)
def frames(W, H):
    """name -> Frame for one size. Small sizes: one frame per impulse position
    and, at (33, 17) and (40, 24), the tiny amplitudes at a seam pixel and at an
    interior one; the large size: all its impulses in one frame."""
    out = collections.OrderedDict()
    for f in (grey(W, H), noise(W, H), special(W, H)[0], binades(W, H)):
        out[f.name] = f
    if (W, H) == LARGE:
        out["impulses"] = impulses_spread(W, H)[0]
        out["last_tile"] = last_tile(W, H)
        return out
    for x, y in impulse_positions(W, H):
        f = impulse(W, H, x, y)
        out[f.name] = f
    if (W, H) in ((33, 17), (40, 24)):
        for e in TINY_EXPONENTS:
            for x, y in ((W // 2 - 1, H // 2), (W // 4, H // 4)):
                f = impulse(W, H, x, y, np.ldexp(1.0, e), f"tiny2^{e}@{x},{y}")
                out[f.name] = f
    return out


# ---------------------------------------------------------------------------
# Plan stage
# ---------------------------------------------------------------------------
PlanCase = collections.namedtuple("PlanCase", "name W H half mse stats cnt samp first adaptive")
PW, PH = 129, 32  # left half 64 columns, right half 65


def _ulps(v, k):
    """v moved by k units in the last place (bit pattern arithmetic; v >= 0)."""
    b = np.asarray(v, F32).view(np.int32).astype(np.int64) + k
    return b.astype(np.int32).view(F32)


def _case(name, half, values, stats, seed, first=False, adaptive=True, fill=0.5, W=PW, H=PH):
    x0, x1 = half_span(W, half)
    n = (x1 - x0) * H
    v = np.asarray(values, F32).ravel()
    assert v.size <= n, (name, v.size, n)
    mse = np.full(n, fill, F32)
    mse[: v.size] = v
    r = np.random.default_rng([0xADA3, seed])
    cnt = r.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    samp = r.integers(0, 256, (H, W, 4), dtype=np.uint16).astype(np.uint8)
    samp[..., 3] = 255
    return PlanCase(name, W, H, half, mse.reshape(H, x1 - x0), np.asarray(stats, F32), cnt, samp, first, adaptive)


def _n(half, W=PW, H=PH):
    x0, x1 = half_span(W, half)
    return (x1 - x0) * H


def noise_errors(n, seed=0xADA4):
    """Error-like values: squares of uniform differences up to 0.1. (Spread
    over many decades instead, most of them would scale to almost 0, where
    1 + 32 scaled lies next to the integer 1 and only f32 can say which side.)"""
    r = np.random.default_rng([seed, n])
    return (r.random(n) ** 2 * 0.01).astype(F32)


def true_stats(m):
    """{sequential f32 sum, min, max} of a vector (the reference's folds)."""
    m = np.asarray(m, F32).ravel()
    return np.array([np.cumsum(m, dtype=F32)[-1], m.min(), m.max()], F32)


@functools.lru_cache(maxsize=None)
def plan_cases():
    """name -> PlanCase. With sum = n and mn = 0 the average is exactly 1 and
    the lower branch is scaled = m / 2; with mx = 2 the upper one is
    scaled = 0.5 + (m - 1) / 2."""
    C = collections.OrderedDict()

    def add(c):
        assert c.name not in C
        C[c.name] = c

    k16 = (np.arange(16) / 16.0).astype(F32)
    for half in (0, 1):
        n = float(_n(half))
        # m = k / 16: scaled = k / 32 exactly, 1 + 32 scaled = k + 1, an integer
        add(_case(f"sixteenths_h{half}", half, k16, [n, 0.0, 3.0], 1))
        # one and two ulps above and one below: the sum rounds back to the integer or not
        near = np.concatenate([_ulps(k16, 1), _ulps(k16, 2), _ulps(k16[1:], -1)])
        add(_case(f"sixteenths_near_h{half}", half, near, [n, 0.0, 3.0], 2))
        # m == avg and ulps either side (mx = 3), scaled == 0.5 and ulps either side (mx = 2)
        around = _ulps(np.full(9, 1.0, F32), np.arange(-4, 5))
        add(_case(f"around_avg_h{half}", half, around, [n, 0.0, 3.0], 3))
        add(_case(f"half_scaled_h{half}", half, around, [n, 0.0, 2.0], 4))
        # every count 1 .. 33: lower branch 1 .. 16, upper branch 17 .. 33
        every = np.concatenate([k16, (1.0 + np.arange(17) / 16.0).astype(F32)])
        add(_case(f"all_counts_h{half}", half, every, [n, 0.0, 2.0], 5))
    n0 = float(_n(0))
    probe = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0], F32)
    probe = np.concatenate([probe, _ulps(probe[1:], 1), _ulps(probe[1:], -1)])
    add(_case("avg_eq_mn", 0, probe, [n0, 1.0, 3.0], 6))        # (m - mn) / 0 below the average
    add(_case("avg_eq_mx", 0, probe, [n0, 0.0, 1.0], 7))        # (m - avg) / 0 from the average up
    add(_case("avg_below_mn", 0, probe, [0.5 * n0, 1.0, 3.0], 8))  # negative denominator below
    add(_case("avg_above_mx", 0, probe, [4.0 * n0, 0.0, 3.0], 9))  # negative denominator above
    add(_case("mn_eq_mx", 1, np.array([1.0, 0.5, 2.0, 0.0, 1.0], F32), [float(_n(1)), 1.0, 1.0], 10, fill=1.0))
    add(_case("mn_eq_mx_zero", 1, np.zeros(1, F32), [0.0, 0.0, 0.0], 11, fill=0.0))  # the uniform frame
    # errors outside [mn, mx] (statistics of another frame): scaled above 1 and below 0 before the clamp
    add(_case("beyond_max", 1, np.linspace(2.0, 50.0, 500).astype(F32), [float(_n(1)), 0.0, 2.0], 13))
    add(_case("beneath_min", 0, np.linspace(0.0, 0.5, 500, endpoint=False).astype(F32), [n0, 0.5, 2.0], 14))
    # mix_color(v) * 255 next to an integer: v = j / 510, m = 2 v = j / 255, and an ulp either side
    j = (np.arange(511) / 255.0).astype(F32)
    add(_case("mix255", 0, np.concatenate([j, _ulps(j, 1), _ulps(j[1:], -1)]), [n0, 0.0, 2.0], 12))
    # statistics that are not numbers or not finite
    inf, nan = np.inf, np.nan
    wild = np.concatenate([probe, noise_errors(200)])
    for i, st in enumerate([[inf, 0.0, 3.0], [-inf, 0.0, 3.0], [nan, 0.0, 3.0], [n0, inf, -inf], [n0, nan, 3.0],
                            [n0, 0.0, nan], [n0, 0.0, inf], [n0, -inf, 3.0], [n0, -inf, inf], [nan, nan, nan],
                            [0.0, inf, -inf]]):
        add(_case(f"wild_stats_{i}", i % 2, wild, st, 20 + i))
    # errors that are not numbers, not finite, negative, -0 or denormal
    den = np.ldexp(1.0, np.arange(-149, -125)).astype(F32)
    odd = np.concatenate([[nan, inf, -inf, -1.0, -0.0, -1e-30], den, -den[:4]]).astype(F32)
    add(_case("wild_m", 1, odd, [float(_n(1)), 0.0, 3.0], 40))
    add(_case("wild_m_true_stats", 0, np.concatenate([odd[3:], noise_errors(300)]), [0.0, -1.0, 8.0], 41))
    # denormal operands in every quotient: avg, mn, mx and m all below 2^-126
    n1 = _n(1)
    dm = (np.arange(1, 1 + 600) * np.ldexp(1.0, -149)).astype(F32)
    add(_case("denormal_quotients", 1, dm, [n1 * 301 * np.ldexp(1.0, -149), np.ldexp(1.0, -149),
                                            601 * np.ldexp(1.0, -149)], 42, fill=float(np.ldexp(301.0, -149))))
    add(_case("denormal_denominators", 0, np.concatenate([probe, _ulps(np.full(8, 1.0, F32), np.arange(-4, 4))]),
              [n0, float(_ulps(F32(1.0), -1)), float(_ulps(F32(1.0), 1))], 43, fill=1.0))
    # the round after a reset and a random half's round: the view stays
    add(_case("first", 1, wild, [n0, 0.0, 3.0], 50, first=True))
    add(_case("random_half", 0, wild, [n0, 0.0, 3.0], 51, adaptive=False))
    add(_case("random_half_first", 1, wild, [n0, 0.0, 3.0], 52, first=True, adaptive=False))
    # seeded noise with its own statistics, at a ragged size too
    for i, (W, H, half) in enumerate([(PW, PH, 0), (PW, PH, 1), (62, 35, 0), (33, 17, 1), (5, 3, 0), (2, 1, 1)]):
        m = noise_errors(_n(half, W, H), seed=0xADA5 + i)
        add(_case(f"noise_{W}x{H}_h{half}", half, m, true_stats(m), 60 + i, W=W, H=H))
    # an empty half: W == 1, left
    add(_case("empty_half", 0, np.zeros(0, F32), [0.0, inf, -inf], 70, W=1, H=4))
    return C


# the seeded-noise inputs large enough for a share of their pixels to mean something
NOISE_CASES = ("noise_129x32_h0", "noise_129x32_h1", "noise_62x35_h0", "noise_33x17_h1")
