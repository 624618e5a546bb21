"""Adaptive round planner, no GPU: the fixtures of adaptive_fixtures.py meet
the conditions the GPU suite relies on, and the oracle's two stages
(adaptive_error, adaptive_plan) agree with independent models written from
render_target.rs:74-138 and sampling_strategy.rs:132-172: an f64 one inside
derived bounds, and the f32 NaN and clamp rules case by case where f64 cannot
decide. Figures measured here: profiles/adaptive/README.md.
"""
import functools

import numpy as np
import pytest

import adaptive_fixtures as fx

F32, F64 = np.float32, np.float64
U = 2.0 ** -24     # unit roundoff of f32
DELTA = 28 * U     # absolute error of one component of v0 - blur (test_error_stage_against_f64_model)
G3 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], F64)
G5 = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]).astype(F64)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle_error(size, name, half):
    import pyoracle
    f = fx.frames(*size)[name]
    return pyoracle.adaptive_error(f.acc, f.cnt, half)


def _oracle_plan(c):
    import pyoracle
    return pyoracle.adaptive_plan(c.W, c.H, c.half, c.mse, c.stats, c.cnt, c.samp, c.first, c.adaptive)


def _half_n(c):
    x0, x1 = fx.half_span(c.W, c.half)
    return (x1 - x0) * c.H


# ---------------------------------------------------------------------------
# Models
# ---------------------------------------------------------------------------
def clamped_means(acc, cnt):
    """read_clamped (render_target.rs:75-79, :214-216) in f32: one correctly
    rounded division per channel, then max(0), min(1), which drop a NaN."""
    with np.errstate(all="ignore"):
        v = acc / cnt.astype(F32)[..., None]
    return np.fmin(np.fmax(v, F32(0.0)), F32(1.0)).astype(F32)


def model_error(acc, cnt, half):
    """The error of every pixel of a half in f64 from the f32 clamped means:
    max(|v0 - g3|^2, |v0 - g5|^2), g = the Gaussian blurs over the whole
    viewport, a tap outside it carrying no value and no weight."""
    H, W = cnt.shape
    v = clamped_means(acc, cnt).astype(F64)
    P = np.zeros((H + 4, W + 4, 3), F64)
    M = np.zeros((H + 4, W + 4), F64)
    P[2:-2, 2:-2] = v
    M[2:-2, 2:-2] = 1.0
    d = []
    for K in (G3, G5):
        r = K.shape[0] // 2
        num, den = np.zeros((H, W, 3), F64), np.zeros((H, W), F64)
        for vy in range(K.shape[0]):
            for vx in range(K.shape[1]):
                ys, xs = slice(2 + vy - r, 2 + vy - r + H), slice(2 + vx - r, 2 + vx - r + W)
                num += K[vy, vx] * P[ys, xs]
                den += K[vy, vx] * M[ys, xs]
        d.append(np.sum((v - num / den[..., None]) ** 2, axis=2))
    x0, x1 = fx.half_span(W, half)
    return np.maximum(d[0], d[1])[:, x0:x1]


def rules_f32(c):
    """sampling_strategy.rs:146-172 per pixel in f32, every rule written out:
    the average is sum / (width * height as f32); the comparison m < avg is
    false when either is a NaN; a quotient with a zero denominator is +-inf or
    (0 / 0) NaN; min(1) then max(0) drop a NaN (f32::min / max return the other
    operand), so a NaN scales to 1; ceil; the view is black iff mn == mx (false
    for NaNs), else mix_color, whose `v < 0.5` sends 0.5 to the upper mix; the
    byte is the truncation of the clamped component x 255.
    Returns the pre-clamp scaled value, the clamped one, counts and RGB."""
    m = c.mse.ravel().astype(F32)
    s, mn, mx = (F32(x) for x in c.stats)
    with np.errstate(all="ignore"):
        avg = F32(s / F32(_half_n(c)))
        below = m < avg
        lo = F32(0.5) * ((m - mn) / F32(avg - mn))
        hi = F32(0.5) + F32(0.5) * ((m - avg) / F32(mx - avg))
        raw = np.where(below, lo, hi).astype(F32)
        scaled = np.fmax(np.fmin(raw, F32(1.0)), F32(0.0)).astype(F32)
        total = (F32(1.0) + scaled * F32(32.0)).astype(F32)
        count = np.ceil(total).astype(np.uint32)
        v = scaled
        a_lo = (F32(1.0) - F32(2.0) * v).astype(F32)
        b_lo = (F32(2.0) * v).astype(F32)
        t = (v - F32(0.5)).astype(F32)
        a_hi = (F32(1.0) - F32(2.0) * t).astype(F32)
        r_hi = (F32(2.0) * t).astype(F32)
        low = v < F32(0.5)
        zero = np.zeros_like(v)
        rgb = np.stack([np.where(low, zero, r_hi), np.where(low, a_lo, zero), np.where(low, b_lo, a_hi)], 1).astype(F32)
        if mn == mx:
            rgb = np.zeros_like(rgb)
        byte = (np.fmax(np.fmin(rgb, F32(1.0)), F32(0.0)) * F32(255.0)).astype(F32).astype(np.uint8)
    return dict(avg=avg, below=below, raw=raw, scaled=scaled, total=total, count=count, rgb=byte)


def _expected_plan(c):
    """Counts, offsets, base and view of a case from rules_f32 and the round
    schedule (first: 4, random: 1, the other half: 0, the view untouched)."""
    x0, x1 = fx.half_span(c.W, c.half)
    count = np.zeros((c.H, c.W), np.uint32)
    view = c.samp.copy()
    if not c.adaptive:
        count[:, x0:x1] = 1
    elif c.first:
        count[:, x0:x1] = 4
    else:
        R = rules_f32(c)
        count[:, x0:x1] = R["count"].reshape(c.H, x1 - x0)
        view[:, x0:x1, :3] = R["rgb"].reshape(c.H, x1 - x0, 3)
    offset = np.concatenate([[0], np.cumsum(count.ravel(), dtype=np.uint64)]).astype(np.uint32)
    return count, offset, c.cnt, view


# ---------------------------------------------------------------------------
# Conditions
# ---------------------------------------------------------------------------
def test_sizes_reach_the_kernels_loops():
    """Tile, chunk and scan-block counts: the large frame sends k_mm_reduce's
    strided loop (1024 threads) and k_scan_sums' carry loop (256 blocks a pass)
    round twice and gives each half 513 sum chunks; the per-tile key buffer's
    formula (w / 16 + 2) (h / 16 + 1) covers the tiles of either half at every
    size; (33, 17) has a full tile and a one-column tile, and a tile row one
    pixel high."""
    def tiles(W, H, half):
        x0, x1 = fx.half_span(W, half)
        return -(-(x1 - x0) // fx.TILE), -(-H // fx.TILE)
    W, H = fx.LARGE
    for half in (0, 1):
        tx, ty = tiles(W, H, half)
        assert (tx, ty) == (41, 25) and tx * ty == 1025 > 1024
        assert -(-(W // 2 * H) // fx.SUM_CHUNK) == 513
    assert W * H + 1 == 524801 and -(-(W * H + 1) // fx.SCAN_CHUNK) == 513 > 2 * 256
    for (w, h) in fx.SIZES + [(1, 4), (fx.PW, fx.PH)]:
        for half in (0, 1):
            tx, ty = tiles(w, h, half)
            assert tx * ty <= (w // 16 + 2) * (h // 16 + 1), (w, h, half)
    assert tiles(33, 17, 0) == (1, 2) and tiles(33, 17, 1) == (2, 2)
    assert fx.half_span(33, 1) == (16, 33) and (33 - 16) % fx.TILE == 1 and 17 % fx.TILE == 1
    assert [fx.half_span(w, 1)[1] - fx.half_span(w, 1)[0] > w // 2 for w, _ in fx.SIZES] == \
        [False, True, True, True, False, False, False]


def test_stencil_conditions():
    """Per size and half: pixels with a tap outside the viewport and pixels
    whose taps cross the seam; below 5 x 5 every pixel has an outside tap."""
    for (W, H) in fx.SIZES:
        ys, xs = np.mgrid[0:H, 0:W]
        outside = (xs < 2) | (xs >= W - 2) | (ys < 2) | (ys >= H - 2)
        half = W // 2
        for h in (0, 1):
            x0, x1 = fx.half_span(W, h)
            mine = (xs >= x0) & (xs < x1)
            seam = mine & ((xs >= half - 2) & (xs < half) if h == 0 else (xs < half + 2))
            n_out, n_seam = int(np.sum(outside & mine)), int(np.sum(seam))
            print(f"{W}x{H} half {h}: outside-tap pixels {n_out}, seam-crossing pixels {n_seam} of {int(mine.sum())}")
            assert n_out > 0 and n_seam > 0
            if W <= 5 and H <= 3:
                assert n_out == mine.sum()
            else:
                assert n_seam == min(2, x1 - x0) * H and n_out < mine.sum()


def test_impulses_show_across_the_seam_and_the_tiles():
    """An impulse next to the seam gives the other half non-zero errors (the
    blur reads the whole viewport), and the impulse positions lie on both sides
    of every tile boundary of both halves. An impulse of 1 on black: the
    errors are those of the model within its bound and non-zero in exactly the
    5 x 5 neighbourhood."""
    W, H = 40, 24
    half = W // 2
    pos = fx.impulse_positions(W, H)
    for x in (half - 1, half, 15, 16, 17, half + 15, half + 16, half + 17, 0, W - 1):
        assert any(p[0] == x for p in pos), x
    for y in (0, 15, 16, 17, H - 1):
        assert any(p[1] == y for p in pos), y
    for x, other in ((half - 1, 1), (half, 0)):
        mse, _ = _oracle_error((W, H), f"impulse@{x},{H // 2}", other)
        assert np.count_nonzero(mse) == 2 * 5, (x, np.count_nonzero(mse))
    mse, st = _oracle_error((W, H), f"impulse@{W // 4},{H // 2}", 0)
    assert np.count_nonzero(mse) == 25 and st[1] == 0.0 and st[2] == mse.max()
    _, kept = fx.impulses_spread(*fx.LARGE)
    r0 = fx.half_span(fx.LARGE[0], 1)[0]
    assert len(kept) == 86 and r0 % 16 == 0
    assert any((x - r0) // 16 == 40 and y // 16 == 24 for x, y in kept)  # the 1025th tile of the right half
    assert {x % 16 for x, _ in kept} >= {15, 0, 1} and {y % 16 for _, y in kept} >= {15, 0, 1}
    assert any(x == r0 - 1 for x, _ in kept) and any(x == r0 for x, _ in kept)
    for half in (0, 1):
        mse, _ = _oracle_error(fx.LARGE, "impulses", half)
        x0, x1 = fx.half_span(fx.LARGE[0], half)
        lit = sum((min(x + 3, x1) - max(x - 2, x0)) * (min(y + 3, fx.LARGE[1]) - max(y - 2, 0))
                  for x, y in kept if x0 - 2 <= x < x1 + 2)
        assert np.count_nonzero(mse) == lit > 500, (half, np.count_nonzero(mse), lit)


def test_tiny_impulses_walk_through_the_denormals():
    """Amplitudes 2^-60 .. 2^-75: at first the errors next to the impulse are
    normal and those of the far taps denormal, then all are denormal, then every
    error is 0."""
    for size in ((33, 17), (40, 24)):
        W, H = size
        kinds = []
        for e in fx.TINY_EXPONENTS:
            for half in (0, 1):
                mse, st = _oracle_error(size, f"tiny2^{e}@{W // 2 - 1},{H // 2}", half)
                assert np.all(np.isfinite(mse)) and st[1] == 0.0
                nz = mse[mse > 0]
                n_den = int(np.sum(nz < np.finfo(F32).tiny))
                kinds.append("zero" if len(nz) == 0 else "denormal" if n_den == len(nz) else
                             "mixed" if n_den else "normal")
        print(size, kinds)
        assert kinds[0] == "mixed" and kinds[-1] == "zero"
        assert kinds.count("denormal") + kinds.count("mixed") >= 8 and kinds.count("zero") >= 2


def test_special_pixels_present_and_tamed():
    """Every kind of special pixel occurs (at least 4 of each from 33 x 17 up),
    reads as the clamp says, and no error of any frame is a NaN or infinite."""
    for size in fx.SIZES:
        W, H = size
        f, kinds = fx.special(W, H)
        a, c = f.acc.reshape(-1, 3), f.cnt.reshape(-1)
        v = clamped_means(f.acc, f.cnt).reshape(-1, 3)
        if W * H >= 33 * 17:
            print(size, {k: len(i) for k, i in kinds.items()})
            assert all(len(i) >= 4 for i in kinds.values())
        assert np.all(c[kinds["cnt0"]] == 0) and np.all(c[kinds["cnt2p24"]] == 2 ** 24 + 1)
        assert np.all(v[kinds["cnt0"][::2]] == 0)  # 0 / 0
        assert np.all(v[kinds["negative"]] == 0) and np.all(v[kinds["above"]] == 1)
        assert np.all(np.signbit(a[kinds["negzero"]])) and np.all(v[kinds["negzero"]] == 0)
        assert np.all(v[kinds["posinf"], 0] == 1) and np.all(v[kinds["neginf"], 1] == 0) and np.all(v[kinds["nan"], 2] == 0)
        assert np.all(np.isfinite(v))
        for half in (0, 1):
            mse, st = _oracle_error(size, "special", half)
            assert np.all(np.isfinite(mse)) and np.all(np.isfinite(st))


def test_grey_frame_is_exactly_flat():
    """The uniform frame: every error exactly 0, stats {0, 0, 0}; its plan is
    33 samples and a black view on every pixel of the half (avg = 0, m < avg
    false, 0.5 + 0.5 (0 / 0) = NaN, min(NaN, 1) = 1; mn == mx)."""
    import pyoracle
    for size in fx.SIZES:
        W, H = size
        for half in (0, 1):
            mse, st = _oracle_error(size, "grey", half)
            assert not mse.any() and not _bits(mse).any() and np.array_equal(_bits(st), np.zeros(3, np.uint32)), size
            x0, x1 = fx.half_span(W, half)
            samp = np.full((H, W, 4), 255, np.uint8)
            count, offset, base, view = pyoracle.adaptive_plan(W, H, half, mse, st, np.full((H, W), 8, np.uint32), samp)
            assert np.all(count[:, x0:x1] == 33) and offset[-1] == 33 * (x1 - x0) * H
            assert np.all(view[:, x0:x1, :3] == 0) and np.all(view[:, x0:x1, 3] == 255)
            assert np.all(np.delete(view, np.s_[x0:x1], axis=1) == 255)


def test_extremes_in_the_last_tile_alone():
    """The large frame `last_tile`: per half, the smallest error (0) and the
    largest occur in tile 1024 and in no other, so a min / max reduction that
    skips the 1025th entry returns other statistics."""
    W, H = fx.LARGE
    for half in (0, 1):
        mse, st = _oracle_error(fx.LARGE, "last_tile", half)
        ys, xs = np.mgrid[0:H, 0:mse.shape[1]]
        tile = (ys // fx.TILE) * (-(-mse.shape[1] // fx.TILE)) + xs // fx.TILE
        assert tile.max() == 1024
        rest = mse[tile != 1024]
        print(f"half {half}: min {st[1]} max {st[2]}; elsewhere min {rest.min()} max {rest.max()}")
        assert st[1] == 0.0 and np.count_nonzero(mse[tile == 1024] == 0) == 9 and rest.min() > 0
        assert st[2] > rest.max() and np.all(tile[mse == st[2]] == 1024)


def test_binades_frame_spans_twenty_binades():
    for size in fx.SIZES[3:]:
        for half in (0, 1):
            mse, st = _oracle_error(size, "binades", half)
            e = np.frexp(mse[mse > 0].astype(F64))[1]
            crossings = np.count_nonzero(np.diff(np.frexp(np.cumsum(mse.ravel(), dtype=F32).astype(F64))[1]))
            print(size, half, "error binades", e.min(), e.max(), "running-sum binade crossings", crossings)
            assert e.max() - e.min() >= 20 and crossings >= 12


def test_plan_cases_sit_on_their_decisions():
    """The plan inputs reach what they were built for, counted through the
    case rules: both branches of m < avg; scaled a NaN, below 0 and above 1
    before the clamp; 1 + 32 scaled an integer before ceil; m == avg and an
    ulp either side; scaled == 0.5 and either side of it; every count 1 .. 33;
    the black view under mn == mx; zero, negative and non-finite denominators;
    denormal operands."""
    C = fx.plan_cases()
    R = {n: rules_f32(c) for n, c in C.items() if c.adaptive and not c.first and c.mse.size}
    tot = dict(below=0, above=0, nan=0, neg=0, over=0, integer=0)
    for n, r in R.items():
        tot["below"] += int(r["below"].sum())
        tot["above"] += int((~r["below"]).sum())
        tot["nan"] += int(np.isnan(r["raw"]).sum())
        tot["neg"] += int((r["raw"] < 0).sum())
        tot["over"] += int((r["raw"] > 1).sum())
        tot["integer"] += int((r["total"] == np.floor(r["total"])).sum())
    print(tot)
    assert all(v >= 100 for v in tot.values()), tot
    for half in (0, 1):
        r = R[f"sixteenths_h{half}"]
        assert r["avg"] == 1.0
        assert np.array_equal(r["scaled"][:16], (np.arange(16) / 32).astype(F32))
        assert np.array_equal(r["total"][:16], np.arange(1, 17).astype(F32))
        assert np.array_equal(r["count"][:16], np.arange(1, 17))
        r = R[f"sixteenths_near_h{half}"]
        k = np.arange(16)
        up1, up2, dn1 = r["count"][:16], r["count"][16:32], r["count"][32:47]
        # an ulp above k / 16 the sum rounds back to k + 1 for some k and steps over it for others
        back = up1 == k + 1
        print("half", half, "one ulp above: rounds back for k =", k[back].tolist(), "steps to k + 2 for", k[~back].tolist())
        assert back.sum() >= 3 and (~back).sum() >= 3 and np.all((up1 == k + 1) | (up1 == k + 2))
        assert np.all((up2 == k + 1) | (up2 == k + 2)) and np.all(up2 >= up1)
        assert np.all((dn1 == k[1:]) | (dn1 == k[1:] + 1))
        r = R[f"around_avg_h{half}"]
        assert r["below"][:9].tolist() == [True] * 4 + [False] * 5 and r["scaled"][4] == 0.5
        r = R[f"half_scaled_h{half}"]
        s = r["scaled"][:9]
        assert s[4] == 0.5 and np.any(s[:4] < 0.5) and np.any(s[5:] > 0.5)
        assert sorted(set(R[f"all_counts_h{half}"]["count"].tolist())) == list(range(1, 34))
        oc = _oracle_plan(C[f"all_counts_h{half}"])[0]
        assert sorted(set(oc[oc > 0].tolist())) == list(range(1, 34))
    # denominators
    for n, want in (("avg_eq_mn", 0.0), ("avg_eq_mx", 0.0)):
        c, r = C[n], R[n]
        den = (r["avg"] - F32(c.stats[1])) if n == "avg_eq_mn" else (F32(c.stats[2]) - r["avg"])
        assert den == want
        assert np.isinf(r["raw"]).sum() >= 5
        # 0 / 0 needs m == avg, which only the upper branch takes
        assert np.isnan(r["raw"]).sum() >= (1 if n == "avg_eq_mx" else 0)
    # negative denominators: below the average (m - mn) / (avg - mn) is then positive and falls as m grows
    r = R["avg_below_mn"]
    assert r["avg"] < C["avg_below_mn"].stats[1] and r["below"].sum() >= 5
    assert np.all(r["raw"][r["below"]] >= 0.5) and len(set(r["count"][r["below"]].tolist())) >= 3
    r = R["avg_above_mx"]
    assert r["avg"] > C["avg_above_mx"].stats[2] and (~r["below"]).sum() >= 5 and (r["raw"][~r["below"]] < 0.5).sum() >= 3
    # mn == mx: black, whatever m is; counts still follow scaled
    for n in ("mn_eq_mx", "mn_eq_mx_zero"):
        c = C[n]
        x0, x1 = fx.half_span(c.W, c.half)
        count, _, _, view = _oracle_plan(c)
        assert np.all(view[:, x0:x1, :3] == 0) and not np.all(c.samp[:, x0:x1, :3] == 0)
    assert len(set(R["mn_eq_mx"]["count"][:5].tolist())) >= 2 and np.all(R["mn_eq_mx_zero"]["count"] == 33)
    # mix_color: both mixes, v == 0.5, and component x 255 within an ulp of an integer
    r = R["mix255"]
    x = np.fmax(np.fmin(np.stack([F32(2) * r["scaled"], F32(1) - F32(2) * r["scaled"]]), F32(1)), F32(0)) * F32(255)
    near = np.abs(x - np.rint(x)) <= np.spacing(np.maximum(x, F32(1)))
    print("mix255: scaled < 0.5:", int((r["scaled"] < 0.5).sum()), ">= 0.5:", int((r["scaled"] >= 0.5).sum()),
          "== 0.5:", int((r["scaled"] == 0.5).sum()), "component x 255 within an ulp of an integer:", int(near.sum()))
    assert (r["scaled"] < 0.5).sum() >= 700 and (r["scaled"] > 0.5).sum() >= 700 and (r["scaled"] == 0.5).sum() >= 1
    assert near.sum() >= 1000
    # denormal operands
    c, r = C["denormal_quotients"], R["denormal_quotients"]
    tiny = np.finfo(F32).tiny
    assert 0 < r["avg"] < tiny and 0 < c.stats[1] < tiny and 0 < c.stats[2] < tiny and np.all(c.mse < tiny)
    assert len(set(r["count"].tolist())) >= 30 and r["below"].sum() >= 250 and (~r["below"]).sum() >= 250
    r = R["denormal_denominators"]
    assert r["avg"] - F32(C["denormal_denominators"].stats[1]) == F32(2.0 ** -24)
    # wild statistics and errors: NaN and infinities reach the clamp
    assert sum(int(np.isnan(R[f"wild_stats_{i}"]["raw"]).sum()) for i in range(11)) >= 500
    assert np.isnan(C["wild_m"].mse).sum() == 1 and np.isinf(C["wild_m"].mse).sum() == 2
    assert (C["wild_m"].mse < 0).sum() >= 6 and np.signbit(C["wild_m"].mse).sum() >= 8


# ---------------------------------------------------------------------------
# The oracle against the models
# ---------------------------------------------------------------------------
def _error_names(size):
    return list(fx.frames(*size))


@pytest.mark.parametrize("size", fx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_error_stage_against_f64_model(wpt, size):
    """Oracle errors (f32) against model_error (f64 from the f32 clamped
    means), every frame, both halves:

        |d32 - d64| <= 2 delta sqrt(3 d64) + 3 delta^2 + 8 u d64 + 2^-146,
        u = 2^-24, delta = 28 u.

    Derivation. The clamped means are the model's inputs (one correctly
    rounded f32 division and two exact clamps, the same in any IEEE
    arithmetic), all in [0, 1]. A blur is a / S: S, a sum of integers up to
    256, is exact; a is 25 products m v, each rounded (error <= u m v; the
    powers of two exactly), summed by 24 rounded additions (the first, to 0, is
    exact) whose partial sums are at most S: |a32 - a| <= 25 u S. Dividing
    leaves 25 u, the division's own rounding adds u (the blur is <= 1), the
    subtraction v0 - g another u: each component of the difference is off by
    at most 27 u <= delta. With e the exact differences and d = sum e^2,
    perturbing each component by delta moves d by at most 2 delta sum|e| +
    3 delta^2 <= 2 delta sqrt(3 d) + 3 delta^2. The three squarings and two
    additions in f32 add a relative 5 u <= 8 u, and three products that may
    underflow add at most 3 x 2^-150 < 2^-146 in all.
    The oracle returns max(d1, d2) only; the bound is increasing in d64, so
    each of the two distances meeting it implies the maximum meets it, and that
    is what is checked here. On the tiny-amplitude impulses (d64 <= 2^-120) the
    bound is vacuous: delta^2 alone is 2^-38. Those frames are here for the bit
    comparison on the GPU.
    min and max are those of the oracle's own errors exactly, the sum is
    wpt_seq_sum of them exactly."""
    import ctypes
    L = wpt.lib()
    L.wpt_seq_sum.restype = ctypes.c_float
    worst = (0.0, None)
    for name in _error_names(size):
        f = fx.frames(*size)[name]
        for half in (0, 1):
            mse, st = _oracle_error(size, name, half)
            d64 = model_error(f.acc, f.cnt, half)
            assert mse.shape == d64.shape
            bound = 2 * DELTA * np.sqrt(3 * d64) + 3 * DELTA ** 2 + 8 * U * d64 + 2.0 ** -146
            ratio = np.abs(mse.astype(F64) - d64) / bound
            if ratio.size and ratio.max() > worst[0]:
                worst = (float(ratio.max()), (name, half))
            bad = np.argwhere(ratio > 1)
            assert len(bad) == 0, f"{size} {name} half {half}: error off its bound at {bad[0]}: {ratio[tuple(bad[0])]}"
            if mse.size:
                assert _bits(st[1:]).tolist() == _bits([mse.min(), mse.max()]).tolist(), (size, name, half)
                flat = np.ascontiguousarray(mse.ravel())
                seq = L.wpt_seq_sum(flat.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(flat.size))
                assert _bits([st[0]])[0] == _bits([seq])[0], (size, name, half, st[0], seq)
            else:
                assert st.tolist() == [0.0, np.inf, -np.inf]
    print(f"{size}: largest |d32 - d64| / bound {worst[0]:.4f} at {worst[1]}")


def _ambiguous(c):
    """Per pixel of a case's half: the f64 count, and whether f64 cannot decide
    it: 1 + 32 scaled64 within 64 u x 33 of an integer, or a denominator that
    is 0 or not finite, or an operand that is not finite."""
    m = c.mse.ravel().astype(F64)
    s, mn, mx = (F64(x) for x in c.stats)
    with np.errstate(all="ignore"):
        avg = s / F64(_half_n(c))
        d_lo, d_hi = avg - mn, mx - avg
        below = m < avg
        scaled = np.where(below, 0.5 * ((m - mn) / d_lo), 0.5 + 0.5 * ((m - avg) / d_hi))
        t = 1.0 + 32.0 * np.clip(scaled, 0.0, 1.0)
        count = np.ceil(t)
        den = np.where(below, d_lo, d_hi)
        amb = ~np.isfinite(m) | ~np.isfinite(den) | (den == 0) | ~np.isfinite(t) | (np.abs(t - np.rint(t)) <= 64 * U * 33)
    return count, amb


@pytest.mark.parametrize("name", list(fx.plan_cases()))
def test_plan_stage_against_the_models(name):
    """The oracle's plan of every input set against (a) the f64 evaluation of
    scaled and the count from the same f32 inputs, wherever f64 can decide (not
    within 64 u x 33 of an integer before the ceiling, denominators finite and
    not 0), and (b) the f32 case rules (rules_f32) on every pixel: counts,
    offsets with the sentinel, base counts and the view's bytes, the other half
    untouched. On the seeded-noise inputs f64 decides at least 99 % of the
    pixels."""
    c = fx.plan_cases()[name]
    count, offset, base, view = _oracle_plan(c)
    want = _expected_plan(c)
    for what, g, w in zip(("count", "offset", "base", "view"), (count, offset, base, view), want):
        bad = np.argwhere(np.asarray(g) != np.asarray(w))
        assert len(bad) == 0, f"{name}: {what} differs from the case rules at {bad[0]}"
    x0, x1 = fx.half_span(c.W, c.half)
    assert np.array_equal(np.delete(view, np.s_[x0:x1], axis=1), np.delete(c.samp, np.s_[x0:x1], axis=1))
    assert offset[-1] == count.sum(dtype=np.uint64) and not np.delete(count, np.s_[x0:x1], axis=1).any()
    if c.adaptive and not c.first and c.mse.size:
        c64, amb = _ambiguous(c)
        got = count[:, x0:x1].ravel()
        bad = np.nonzero(~amb & (got != c64))[0]
        assert len(bad) == 0, f"{name}: count {got[bad[0]]} != f64 {c64[bad[0]]} at {bad[0]} (m = {c.mse.ravel()[bad[0]]})"
        print(f"{name}: f64 undecided share {amb.mean():.4f}")
        if name in fx.NOISE_CASES:
            assert amb.mean() <= 0.01


def test_chained_noise_stays_inside_the_cap(wpt):
    """Both stages chained on the oracle, noise frames: the plan from the
    frame's own errors and statistics; f64 decides at least 99 % of it."""
    for size in ((40, 24), (62, 35), fx.LARGE):
        W, H = size
        f = fx.frames(W, H)["noise"]
        for half in (0, 1):
            mse, st = _oracle_error(size, "noise", half)
            samp = np.full((H, W, 4), 255, np.uint8)
            c = fx.PlanCase("chained", W, H, half, mse, st, f.cnt, samp, False, True)
            count, offset, base, view = _oracle_plan(c)
            for g, w in zip((count, offset, base, view), _expected_plan(c)):
                assert np.array_equal(g, w)
            c64, amb = _ambiguous(c)
            x0, x1 = fx.half_span(W, half)
            assert np.array_equal(count[:, x0:x1].ravel()[~amb], c64[~amb])
            print(f"{size} half {half}: f64 undecided share {amb.mean():.5f}")
            assert amb.mean() <= 0.01


# ---------------------------------------------------------------------------
# The hooks without a device
# ---------------------------------------------------------------------------
def test_hooks_without_session_fail_cleanly(wpt):
    itf = wpt.interface
    f = fx.frames(5, 3)["noise"]
    with pytest.raises(itf.WptError) as e:
        itf.adaptive_error(f.acc, f.cnt, 0)
    assert e.value.code == itf.ERR_NOT_INIT
    c = fx.plan_cases()["noise_5x3_h0"]
    with pytest.raises(itf.WptError) as e:
        itf.adaptive_plan(c.W, c.H, c.half, c.mse, c.stats, c.cnt, c.samp)
    assert e.value.code == itf.ERR_NOT_INIT
    assert wpt.lib().wpt_last_error() == b"init not called"
    # null pointers and a bad half are refused before anything is read
    L = wpt.lib()
    assert L.wpt_adaptive_error(0, 0, None, None, 2, None, None) == itf.ERR_NOT_INIT
    assert L.wpt_adaptive_plan(0, 0, 2, 0, 1, None, None, None, None, None, None, None) == itf.ERR_NOT_INIT
    for sym in ("wpt_adaptive_error", "wpt_adaptive_plan"):
        assert sym in wpt._lib.EXPORTED and sym in wpt._lib.header_symbols()
