"""The adversarial fixtures of tests/adversarial.py, on the CPU.

First the conditions: asserted on the oracle alone, so that the device tests
of tests/test_gpu_adversarial.py cannot pass vacuously (exact ties across
leaves and with the seeding plane, tie winners that no fixed rule predicts,
NaN slab products, stacks deeper than the LDS slots, mixed shadow verdicts).
Then the oracle itself against an independent f64 brute force, the torus
restatement against the independent quartic solver on the new rays, and the
host presolve against the oracle on every fixture. Measured values are kept
in profiles/adversarial/README.md.
"""
import numpy as np

import adversarial as adv
from test_presolve import camera_rays

# The oracle's largest relative deviation |t - t64| / t64 from the f64 brute
# force, plain, over meshes A, B, C, D (all sets but on_plane / on_surface) and
# the sphere and AA-rect sets, measured: 3.866e-5 (D/degenerate; D: 1.3e-6 ..
# 3.9e-5, the sphere set 3.7e-6, the dyadic sheets and the AA rects at most
# 8.3e-8). 16 x that is above the cap. Mesh F is not in this figure: see below.
ORACLE_F64_MAX_REL = 3.87e-5
F64_TOL = min(16 * ORACLE_F64_MAX_REL, 1e-4)   # 16 x covers f32 rounding at other seeds; never above the project's 1e-4
# Mesh F: see test_oracle_against_f64_brute_force_mesh_f. The largest forward
# error in units of adversarial._forward_units, measured, and the measured
# shares of each set that meet the plain bound F64_TOL (floors, rounded down).
F_FORWARD_MAX_UNITS = 1.48   # measured 1.475 (F/inside)
F_PLAIN_SHARE = {"vertices": 0.97, "edges": 0.93, "interior": 0.94, "degenerate": 0.95, "inside": 0.57}
# rays the host presolve resolves per fixture, over all its sets (test_host_presolve_agrees_with_the_oracle)
PRESOLVE_RESOLVED = {'A': 73, 'B': 112, 'Bwall': 118, 'Bulp': 102, 'C': 78, 'D': 84, 'E': 76, 'F': 79, 'G': 109, 'BA': 73}

RENDER_CAM = (1.0, 2.0, 4.5, 0.9, 0.0)   # looks down at the floor sheet and sheet A beside it (mesh BA)

_FX = {}


def fixtures(wpt, oracle):
    """Per scene-2 mesh: (mesh, oracle scene, host debug scene, sets, oracle (t, id) per set), made once."""
    if not _FX:
        for name, mesh in adv.scene2_meshes(wpt).items():
            ref = oracle.OracleScene(2, mesh)
            dbg = wpt.interface.DebugScene(2, mesh)
            sets = adv.scene2_sets(name, mesh, ref.nodes())
            hits = {k: ref.trace_rays(r)[:2] for k, r in sets.items()}
            _FX[name] = (mesh, ref, dbg, sets, hits)
    return _FX


_TIES = {}


def tie_sets(wpt, oracle):
    """(mesh, set) -> (oracle t, oracle id, brute-force t matrix) on every vertex / edge / interior ray of the tie meshes."""
    if not _TIES:
        fx = fixtures(wpt, oracle)
        for name in adv.TIE_MESHES:
            _, ref, _, sets, hits = fx[name]
            for s in ("vertices", "edges", "interior"):
                _TIES[name, s] = (*hits[s], adv.brute_hits(ref, sets[s]))
    return _TIES


def _tied(t_o, T):
    """(n, shapes) bool: shapes at exactly the oracle's winning t."""
    return np.isfinite(t_o)[:, None] & (T.view(np.uint32) == t_o.view(np.uint32)[:, None])


def test_fixture_limits(wpt, oracle):
    for name, (mesh, ref, _, sets, _) in fixtures(wpt, oracle).items():
        assert mesh.size // 9 <= adv.MAX_TRIS
        assert all(len(r) <= adv.MAX_RAYS and r.dtype == np.float32 for r in sets.values())
        assert ref.verify_bvh() == (name != "E"), name   # E: no box contains a NaN vertex
    # every triangle of a sheet has the same normal and the same n.v0
    for mesh in (adv.mesh_a(), adv.mesh_b(), adv.mesh_b_wall()):
        w = adv.world(mesh)
        n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
        assert len(np.unique(n, axis=0)) == 1 and np.count_nonzero(n[0]) == 1
        assert len(np.unique(np.einsum("ij,ij->i", n, w[:, 0]))) == 1
    # the builders are deterministic
    again = adv.scene2_meshes(wpt)
    assert all(np.array_equal(again[k], v[0], equal_nan=True) for k, v in fixtures(wpt, oracle).items())


def test_sheet_a_vertices_and_edges_tie_across_triangles(wpt, oracle):
    ties = tie_sets(wpt, oracle)
    for s in ("vertices", "edges"):
        t_o, id_o, T = ties["A", s]
        k = _tied(t_o, T).sum(axis=1)
        print(f"A {s}: {len(k)} rays, >= 2 shapes at the winning t {np.mean(k >= 2):.3f}, max {k.max()}")
        assert np.mean(k >= 2) >= 0.8
    assert _tied(*ties["A", "vertices"][::2]).sum(axis=1).max() >= 6   # six triangles meet at an inner vertex


def test_sheet_b_ties_with_the_seeding_plane(wpt, oracle):
    ties = tie_sets(wpt, oracle)
    n_inf = fixtures(wpt, oracle)["B"][1].num_inf
    both = np.concatenate([_tied(t, T)[:, :n_inf].any(axis=1) & _tied(t, T)[:, n_inf:].any(axis=1)
                           for (m, s), (t, i, T) in ties.items() if m == "B"])
    print(f"B: plane / triangle ties {both.mean():.3f} of {len(both)} rays")
    assert both.mean() >= 0.5
    for m in ("Bwall",):
        w = np.concatenate([_tied(t, T)[:, :n_inf].any(axis=1) & _tied(t, T)[:, n_inf:].any(axis=1)
                            for (mm, s), (t, i, T) in ties.items() if mm == m])
        print(f"{m}: plane / triangle ties {w.mean():.3f}")
        assert w.mean() >= 0.5


def test_no_fixed_tie_break_rule_reproduces_the_winner(wpt, oracle):
    """Over the union of the tie sets the oracle's winner is neither always the
    lowest nor always the highest tied id: the order of the visit decides."""
    not_low, not_high = [], []
    for key, (t_o, id_o, T) in tie_sets(wpt, oracle).items():
        tied = _tied(t_o, T)
        multi = tied.sum(axis=1) >= 2
        lo = np.argmax(tied, axis=1)
        hi = T.shape[1] - 1 - np.argmax(tied[:, ::-1], axis=1)
        assert np.all(tied[np.arange(len(id_o)), id_o][multi])   # the winner is one of the tied shapes
        not_low.append(multi & (id_o != lo))
        not_high.append(multi & (id_o != hi))
        print(f"{key}: ties {multi.mean():.3f}, winner not lowest {not_low[-1].mean():.3f}, "
              f"not highest {not_high[-1].mean():.3f}")
    not_low, not_high = np.concatenate(not_low), np.concatenate(not_high)
    print(f"union: not lowest {not_low.mean():.3f}, not highest {not_high.mean():.3f} of {len(not_low)}")
    assert not_low.mean() >= 0.05 and not_high.mean() >= 0.05


def test_overlap_mesh_fills_the_lds_stack(wpt, oracle):
    """kLdsSlots = 9 (wpt_render.hip): a stack depth of 11 uses the spill area
    (stack_store / stack_load, the non-uniform branch of push)."""
    _, ref, dbg, sets, _ = fixtures(wpt, oracle)["F"]
    assert adv.LDS_SLOTS == 9
    rays = sets["inside"]
    planes = ref.shapes()[: ref.num_inf]
    seed = adv.brute_hits(_Planes(planes), rays).min(axis=1)
    pend = adv.first_descent_pending(ref.nodes(), rays[:, :3], rays[:, 3:], seed)
    share = np.mean(pend >= adv.LDS_SLOTS + 2)
    print(f"F inside: first-descent pending >= {adv.LDS_SLOTS + 2}: {share:.3f}, max {pend.max()}, depth {dbg.depth}")
    assert share >= 0.25
    assert np.array_equal(ref.nodes(), dbg.nodes())


class _Planes:
    """The infinite shapes alone, for brute_hits."""

    def __init__(self, rec):
        self.rec = rec

    def shapes(self):
        return self.rec


def test_shadow_set_has_both_verdicts(wpt, oracle):
    _, ref, _, _, _ = fixtures(wpt, oracle)["G"]
    pq, li, qc, pc = adv.shadow_set(ref.shapes())
    assert len(pq) <= adv.MAX_RAYS and np.all(np.any(pq[:, :3] != pq[:, 3:], axis=1))
    occ = ref.shadow_rays(pq, li)
    print(f"G shadow: {len(pq)} segments, occluded {occ.mean():.3f}")
    assert 0.2 <= occ.mean() <= 0.8
    # single-valued by construction: a segment from the lights' plane y = 7 to a
    # light runs within that plane, parallel to every sheet and to the floor
    # (n.d == 0: no hit), and the back plane lies beyond q; never occluded
    single = {"light_plane": False}
    for names, cls in ((adv.Q_CLASSES, qc), (adv.P_CLASSES, pc)):
        for c in names:
            m = occ[cls == c]
            print(f"  {c}: {len(m)} segments, occluded {m.mean():.3f}")
            if c in single:
                assert np.all(m == single[c]), c
            else:
                assert m.any() and not m.all(), c


def test_every_set_hits(wpt, oracle):
    for name, (_, ref, _, sets, hits) in fixtures(wpt, oracle).items():
        for s, (t, ids) in hits.items():
            print(f"{name} {s}: {len(ids)} rays, hits {np.mean(ids >= 0):.3f}, mesh {np.mean(ids >= ref.num_inf):.3f}")
            assert np.mean(ids >= 0) >= 0.3, (name, s)
    for sid in (0, 100, 101):
        ref = oracle.OracleScene(sid)
        for s, (rays, _) in adv.shape_sets(sid, ref.shapes()).items():
            ids = ref.trace_rays(rays)[1]
            print(f"scene {sid} {s}: {len(ids)} rays, hits {np.mean(ids >= 0):.3f}")
            assert np.mean(ids >= 0) >= 0.3, (sid, s)


def test_on_plane_rays_make_nan_slab_products(wpt, oracle):
    """(bound - o) * (1 / d) = 0 * inf: AABB::hit's verdict on that node rests on
    f32::min / max dropping the NaN (aabb.rs:132-164)."""
    L = oracle.lib()
    for name in ("A", "F", "E"):
        nodes = fixtures(wpt, oracle)[name][1].nodes()
        rays, pick, ax = adv.on_plane_rays(nodes)
        box = nodes[:, :6].copy().view(np.float32)[pick]
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.float32(1.0) / rays[:, 3:]
            prod = (box.reshape(-1, 2, 3) - rays[:, None, :3]) * inv[:, None, :]
        nan = np.isnan(prod).any(axis=(1, 2))
        assert np.all(rays[np.arange(len(rays)), 3 + ax] == 0.0)
        assert np.signbit(rays[np.arange(len(rays)), 3 + ax]).any() and not np.signbit(rays[np.arange(len(rays)), 3 + ax]).all()
        assert nan.all()
        hit_np, h_np = adv.aabb_hit_np(box, rays[:, :3], inv)
        got = np.zeros(len(rays), bool)
        out = np.zeros(1, np.float32)
        for i in range(len(rays)):
            got[i] = bool(L.oracle_aabb_hit(np.ascontiguousarray(box[i]).ctypes.data,
                                            np.ascontiguousarray(rays[i]).ctypes.data, out.ctypes.data))
            if got[i]:
                assert out[0] == h_np[i]
        assert np.array_equal(got, hit_np)
        # NaN-driven: the same ray started one f32 step inside the slab (no NaN:
        # the axis then spans [-inf, inf]) gets another verdict on the same node
        k = np.arange(len(rays))
        o2 = rays[:, :3].copy()
        o2[k, ax] = np.nextafter(o2[k, ax], (box[k, ax] + box[k, ax + 3]) * np.float32(0.5))
        hit2, _ = adv.aabb_hit_np(box, o2, inv)
        print(f"{name} on_plane: NaN products {nan.mean():.3f}, node hit {got.mean():.3f}, "
              f"one step inside {hit2.mean():.3f}")
        assert np.sum(hit2 & ~got) >= 50


def _f64_cases(wpt, oracle, meshes, shape_scenes=()):
    out = []
    for name in meshes:
        _, ref, _, sets, hits = fixtures(wpt, oracle)[name]
        sh = ref.shapes()
        for s, rays in sets.items():
            if s not in adv.F64_EXCLUDED_SETS:
                out.append((f"{name}/{s}", sh, rays, *hits[s]))
    for sid, s in shape_scenes:
        ref = oracle.OracleScene(sid)
        rays = adv.shape_sets(sid, ref.shapes())[s][0]
        out.append((f"scene{sid}/{s}", ref.shapes(), rays, *ref.trace_rays(rays)[:2]))
    return out


def test_oracle_against_f64_brute_force(wpt, oracle):
    """The oracle's (t, id) against adversarial.f64_check (f64, from the
    geometry) on meshes A, B, C, D and the sphere and AA-rect sets, with the
    plain bound |t - t64| / t64 <= F64_TOL (mesh F: the next test). The
    on_plane and on_surface sets are left out, and only those: there the
    reference's strict culling (a box entered only at an entry < the closest
    hit, origins on a surface at t = 0) legitimately loses hits the brute force
    finds, and the device must reproduce that, which test_gpu_adversarial checks.

    Sphere grazes and surface origins are ambiguous in f32; where the oracle's
    t lies in the ambiguity window it is taken as the f64 value (`self`), so
    such a ray checks the id and the window, not t: 130 of the 672 sphere rays
    (measured; graze and surf_* classes), at most 0.2 asserted. AA-rect
    edge, corner and in-face rays never count as sure hits, but a winning
    rect's t is always compared by the slab formula."""
    assert adv.F64_EXCLUDED_SETS == ("on_plane", "on_surface")
    assert F64_TOL <= 1e-4
    worst = 0.0
    for label, sh, rays, t_o, id_o in _f64_cases(wpt, oracle, ("A", "B", "C", "D"), ((101, "sphere"), (100, "aarect"))):
        ok, rel, _, own = adv.f64_check(sh, rays, t_o, id_o, F64_TOL)
        fin = rel[np.isfinite(rel)]
        print(f"{label}: {len(rays)} rays, agree {ok.mean():.4f}, max rel {fin.max():.3e}, self {int(own.sum())}")
        worst = max(worst, float(fin.max()))
        assert ok.all(), (label, np.nonzero(~ok)[0][:10], rays[~ok][:3], t_o[~ok][:3], id_o[~ok][:3])
        assert own.mean() <= (0.2 if label.endswith("sphere") else 0.0), label
    print(f"max relative deviation of the oracle from f64: {worst:.3e}")
    assert worst <= ORACLE_F64_MAX_REL * 1.0001   # the constant is the measurement
    assert worst <= F64_TOL


def test_oracle_against_f64_brute_force_mesh_f(wpt, oracle):
    """Mesh F does NOT meet the plain relative bound, and cannot: its closest hit
    lies 1e-2 .. 1e-6 from an origin whose coordinates are about 5, so t =
    n.(v0 - o) / n.d cancels (the numerator's terms are thousands of times the
    numerator) and the reference's f32 t has a relative error far above 1e-4.
    Measured maxima of |t - t64| / t64: vertices 1.1e-3, edges 1.1e-2, interior
    7.7e-3, degenerate 1.0e-2, inside 0.374 (853 of 2000 inside rays above
    1e-4). That is the reference's arithmetic; the device reproduces it bit for
    bit. The id checks are those of the other meshes; t is bounded by its own,
    separately named criterion: the f32 forward error |t - t64| <= 16 x
    F_FORWARD_MAX_UNITS in units of U32 (sum |n_i| (|v0_i| + |o_i|) + t sum
    |n_i d_i|) / |n.d| (adversarial._forward_units), an absolute bound from
    the precision of the format. The shares of rays that do meet the plain bound
    are asserted so that a change either way is seen."""
    worst = 0.0
    for label, sh, rays, t_o, id_o in _f64_cases(wpt, oracle, ("F",)):
        ok, rel, fwd, _ = adv.f64_check(sh, rays, t_o, id_o, F64_TOL, forward=16 * F_FORWARD_MAX_UNITS)
        plain = np.mean(rel <= F64_TOL)
        print(f"{label}: {len(rays)} rays, agree {ok.mean():.4f}, max rel {rel.max():.3e}, plain bound met "
              f"{plain:.4f}, max forward error {fwd.max():.3f} units")
        worst = max(worst, float(fwd.max()))
        assert ok.all(), (label, np.nonzero(~ok)[0][:10], rays[~ok][:3], t_o[~ok][:3], id_o[~ok][:3])
        assert plain >= F_PLAIN_SHARE[label.split("/")[1]], label
    print(f"max forward error on F: {worst:.3f} units")
    assert worst <= F_FORWARD_MAX_UNITS * 1.0001


# the quartic's known-bad pairs: see test_torus_restatement_on_the_transversal_rays
TORUS_LOST = (22, 3)   # (the torus missed, a farther root returned)
TORUS_LOST_CLASSES = {"axis_tube", "equator"}


def test_torus_restatement_on_the_transversal_rays(oracle):
    """test_torus_restatement_against_independent_solver's solver (numpy's
    companion-matrix roots of the same quartic, Newton-polished) on every
    non-tangent (ray, torus) pair of the torus set (the tangent rays have an
    ill-conditioned root count).

    Known-bad, pinned by exact count (TORUS_LOST) and class: rays whose line
    meets the torus axis (axis_tube, equator) cross the tube, and the restated
    solver returns no root for 22 of them, so the oracle, and bit for bit the
    device, miss the torus; for 3 equator pairs it returns a farther root than
    the nearest (e.g. t = 20.59 where the tube is entered at 20.00). Representative: torus at (-16, -0.5, -7.5),
    ray from (-14.7, 4.5, -7.5) along (1e-7, -1, 0), the tube top at t = 4.7.
    Its depressed quartic y^4 + p y^2 + q y + r has p = 6.58, q = -1.8e-6, r =
    -0.60; the resolvent cubic's discriminant is 0 up to rounding, so
    find_roots_cubic_normalized's `d < 0.0` (ref_quartic.h: the three-real-root
    branch) is not taken and it returns the single root y = -p / 2; Ferrari's m
    = p + 2y is then 7.5e-14 and q / (2 sqrt(m)) = -3.2, and both quadratics of
    find_roots_quartic_depressed have a negative discriminant. Whether roots
    0.0.4 itself does the same cannot be established here (the crate is not in
    the reference tree; parity unpinned), so the restatement is left as it is.
    A lost pair must have q = 0 up to rounding (|q| <= 1e-9 max(1, |p|)^1.5);
    every other disagreement fails."""
    ref = oracle.OracleScene(0)
    sh = ref.shapes()
    rays, lab = adv.torus_rays(sh)
    tori = sh[sh[:, 12] == adv.KIND_TORUS]
    checked = 0
    lost = []
    for ti, tor in enumerate(tori[:: max(1, len(tori) // 6)][:6]):
        loc, A, B = tor[:3], float(tor[3]), float(tor[4])
        t_o, _, hit_o, ent_o = oracle.torus_trace(loc, A, B, rays)
        a, b = float(np.float32(A)), float(np.float32(B))
        for i, r in enumerate(rays.astype(np.float64)):
            if lab[i].startswith("tangent"):
                continue
            d = (rays[i, :3] - loc.astype(np.float32)).astype(np.float64)
            if np.abs(d).max() > 50:
                continue   # another torus's far ray: the quartic's f64 coefficients lose the roots
            e = r[3:]
            g = 4 * a * a * (e[0] ** 2 + e[2] ** 2)
            h = 8 * a * a * (d[0] * e[0] + d[2] * e[2])
            ii = 4 * a * a * (d[0] ** 2 + d[2] ** 2)
            j, k = e @ e, 2 * (d @ e)
            l_ = d @ d + a * a - b * b
            c = np.array([j * j, 2 * j * k, 2 * j * l_ + k * k - g, 2 * k * l_ - h, l_ * l_ - ii])
            z = np.roots(c)
            if np.any((np.abs(z.imag) > 1e-9) & (np.abs(z.imag) < 1e-3)):
                continue
            real = z.real[np.abs(z.imag) <= 1e-9]
            for _ in range(3):
                dp = np.polyval(np.polyder(c), real)
                real = real - np.polyval(c, real) / np.where(dp == 0, 1, dp)
            pos = real[real >= 0.0001]
            if np.any(np.abs(pos - 0.0001) < 1e-6):
                continue
            checked += 1
            if len(pos) == 0:
                assert not hit_o[i], (lab[i], i)
                continue
            t_np = pos.min()
            agree = hit_o[i] and abs(float(t_o[i]) - t_np) <= 1e-5 * max(1.0, t_np) and ent_o[i] == (len(pos) % 2 == 0)
            if not agree:
                bq, cq, dq = c[1] / c[0], c[2] / c[0], c[3] / c[0]
                p_, q_ = cq - 3 * bq * bq / 8, bq ** 3 / 8 - bq * cq / 2 + dq
                assert abs(q_) <= 1e-9 * max(1.0, abs(p_)) ** 1.5, (lab[i], i, ti, p_, q_, t_o[i], t_np)
                lost.append((ti, i, str(lab[i]), "miss" if not hit_o[i] else "other root"))
    print(f"torus: {checked} non-tangent ray / torus pairs checked, lost {len(lost)}: {lost}")
    assert checked >= 1200
    assert (sum(k == "miss" for *_, k in lost), sum(k == "other root" for *_, k in lost)) == TORUS_LOST
    assert {c for _, _, c, _ in lost} <= TORUS_LOST_CLASSES


def test_host_presolve_agrees_with_the_oracle(wpt, oracle):
    """DebugScene.presolve resolves no ray to other (t, id) bits than the
    oracle's, on every scene-2 fixture and set. It resolves rays on every
    fixture, the mesh with degenerate and NaN triangles (E) included: the
    per-mesh counts are pinned, so that a change either way is seen."""
    counts = {}
    for name, (_, ref, dbg, sets, hits) in fixtures(wpt, oracle).items():
        counts[name] = 0
        for s, rays in sets.items():
            res, t, ids = dbg.presolve(rays)
            t_r, id_r = hits[s]
            assert np.all(id_r[res] < dbg.num_inf), (name, s)
            assert np.array_equal(ids[res], id_r[res]), (name, s)
            assert np.array_equal(t[res].view(np.uint32), t_r[res].view(np.uint32)), (name, s)
            counts[name] += int(res.sum())
    print(f"presolve: resolved per mesh {counts}")
    assert counts == PRESOLVE_RESOLVED


def test_render_camera_sees_the_ties(wpt, oracle):
    """The render fixture of test_gpu_adversarial (mesh BA from RENDER_CAM): at
    least a tenth of the primary rays end in a plane / triangle tie."""
    _, ref, _, _, _ = fixtures(wpt, oracle)["BA"]
    rays = camera_rays(wpt, 2, 32, 24, RENDER_CAM)
    t_o, id_o, _ = ref.trace_rays(rays)
    T = adv.brute_hits(ref, rays)
    tied = _tied(t_o, T)
    both = tied[:, : ref.num_inf].any(axis=1) & tied[:, ref.num_inf:].any(axis=1)
    print(f"render camera: plane / triangle ties {both.mean():.3f}, sheet A {np.mean(t_o < T[:, 0]):.3f}")
    assert both.mean() >= 0.10
