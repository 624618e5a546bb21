"""The SH projection without a GPU: wpt_sh_basis (the code the kernel runs,
csrc/wpt_sh.h) against the numpy-f32 restatement of tests/probesh_fixtures.py
bit for bit, the constants from math.pi, their orthonormality under an exact
quadrature, the distance to the f64 closed form, the call without a session,
the binding, on the oracle alone that the point sets give the GPU test power,
and sh_basis under the sanitizers as a program of its own
(tests/probesh_main.cpp).
"""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import points_fixtures as px
import probesh_fixtures as ps
import rays_fixtures as rf

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def itf(wpt):
    return wpt.interface


def _same(got, want, what):
    g, w = ps.bits(got), ps.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], got[bad[:6]], want[bad[:6]])


# ---------------------------------------------------------------------------
# wpt_sh_basis == the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1, 2])
def test_basis_against_restatement(wpt, itf, order):
    fam = dict(ps.decision_dirs())
    fam["point_rays' table directions"] = ps.table_dirs(wpt)
    fam["4096 seeded unit directions"] = ps.seeded_unit_dirs()
    for name, d in fam.items():
        got = itf.sh_basis(d, order)
        assert got.shape == (len(d), (order + 1) ** 2) and got.dtype == F32
        _same(got, ps.basis(d, order), (name, order))
        # the prefix property of the basis itself
        _same(got, itf.sh_basis(d, 2)[:, :(order + 1) ** 2], (name, order, "prefix"))


def test_decision_directions_reach_their_cases(wpt, itf):
    fam = ps.decision_dirs()
    assert len(fam["axes"]) == 6 and len(fam["diagonals"]) == 8
    Y = {k: itf.sh_basis(v, 2) for k, v in fam.items()}
    # Y6 takes both signs among the neighbours of z = sqrt(1 / 3), and is tiny there
    y6 = Y["z*z about 1/3"][:, 6]
    assert (y6 < 0).any() and (y6 > 0).any() and np.abs(y6).max() < 1e-6
    # |x| = |y|: Y8 is exactly zero (of either sign)
    assert np.all((ps.bits(Y["|x| = |y|"][:, 8]) & 0x7FFFFFFF) == 0)
    # -0 components keep their sign through band 1; denormal components stay denormal (no flush)
    nz = fam["negative zeros"]
    b1 = Y["negative zeros"][:, [3, 1, 2]]  # Y3 = C1 x, Y1 = C1 y, Y2 = C1 z
    assert np.array_equal(ps.bits(b1)[ps.bits(nz) == 0x80000000], np.full((ps.bits(nz) == 0x80000000).sum(), 0x80000000))
    dn = Y["denormals"]
    tiny = (dn != 0) & (np.abs(dn) < np.finfo(F32).tiny)
    assert tiny.any()
    # the axes: band 1 is +-C1 on its own axis, Y6 is 2 C3 on z and -C3 on x, y
    ax = Y["axes"]
    assert np.array_equal(ax[:, 0], np.full(6, ps.C0))
    assert np.array_equal(np.abs(ax[:, 1:4]).max(axis=1), np.full(6, ps.C1))
    assert np.array_equal(ax[4:, 6], np.full(2, ps.C3 * F32(2.0))) and np.array_equal(ax[:4, 6], np.full(4, -ps.C3))
    # the table's directions are unit length
    t = ps.table_dirs(wpt).astype(np.float64)
    assert len(t) > 100 and np.abs((t ** 2).sum(1) - 1).max() <= 4 * 2.0 ** -23


def test_constants_from_pi(wpt, itf):
    want = [math.sqrt(1 / (4 * math.pi)), math.sqrt(3 / (4 * math.pi)), math.sqrt(15 / (4 * math.pi)),
            math.sqrt(5 / (16 * math.pi)), math.sqrt(15 / (16 * math.pi))]
    # read the library's constants out of the basis: Y0; Y1 at y = 1; Y4 at x = y = 1;
    # Y6 at z = 0 is C3 * (0 - 1); Y8 at x = 1, y = 0
    Y = itf.sh_basis(np.array([[0, 1, 0], [1, 1, 0], [1, 0, 0]], F32), 2)
    got = [Y[0, 0], Y[0, 1], Y[1, 4], -Y[0, 6], Y[2, 8]]
    for g, w, c in zip(got, want, ps.CONSTANTS):
        assert ps.bits(F32(g)) == ps.bits(F32(w)) == ps.bits(c), (g, w, c)
        # nearest: no f32 neighbour is closer to the f64 value
        f = F32(w)
        assert abs(float(f) - w) <= min(abs(float(np.nextafter(f, F32(2))) - w), abs(float(np.nextafter(f, F32(0))) - w))
    # and the literals in the source are those numbers
    src = open(os.path.join(ROOT, "wasm-pathtracer_amd", "csrc", "wpt_sh.h")).read()
    lits = re.findall(r"constexpr float kShC(\d) = ([0-9.e+-]+)f;", src)
    assert [int(i) for i, _ in lits] == [0, 1, 2, 3, 4]
    for (_, text), c in zip(lits, ps.CONSTANTS):
        assert ps.bits(F32(float(text))) == ps.bits(c), (text, c)


def test_constants_are_orthonormal():
    """<Y_i, Y_j> over the sphere with an 8-point Gauss-Legendre rule in cos(theta)
    (exact to degree 15) times 16 uniform azimuths (exact for trigonometric degree
    <= 15): the products of two basis functions have degree <= 4, so the rule is
    exact and the only error is the f32 constants' 2^-24 relative."""
    xs, ws = np.polynomial.legendre.leggauss(8)
    phi = (np.arange(16) + 0.5) * (2 * np.pi / 16)
    z = np.repeat(xs, len(phi))
    w = np.repeat(ws, len(phi)) * (2 * np.pi / len(phi))
    q = np.sqrt(1 - z * z)
    x, y = q * np.tile(np.cos(phi), len(xs)), q * np.tile(np.sin(phi), len(xs))
    c0, c1, c2, c3, c4 = (float(c) for c in ps.CONSTANTS)
    Y = np.stack([np.full_like(z, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3 * z * z - 1), c2 * x * z,
                  c4 * (x * x - y * y)], axis=1)
    G = (Y * w[:, None]).T @ Y
    err = np.abs(G - np.eye(9)).max()
    print("max |<Y_i, Y_j> - delta_ij| =", err)
    assert err <= 1e-6


def test_basis_accuracy(itf):
    """Every f32 value within 2^-20 absolute of the f64 closed form on unit
    directions: at most five roundings of quantities below 1.1."""
    d = np.concatenate([ps.seeded_unit_dirs(), ps.decision_dirs()["axes"], ps.decision_dirs()["diagonals"]])
    err = np.abs(itf.sh_basis(d, 2).astype(np.float64) - ps.basis_f64(d.astype(np.float64)))
    print("worst |f32 - f64| in units of 2^-20:", err.max() / 2.0 ** -20)
    assert err.max() <= 2.0 ** -20


# ---------------------------------------------------------------------------
# Without a session: the arguments, the binding, the header
# ---------------------------------------------------------------------------
def test_sh_basis_arguments(wpt, itf):
    L = wpt.lib()
    d = np.ascontiguousarray(ps.decision_dirs()["axes"])
    out = np.full((6, 9), 7.25, F32)
    assert L.wpt_sh_basis(6, None, 2, out.ctypes.data) == itf.ERR_INVALID_ARG
    assert L.wpt_sh_basis(6, d.ctypes.data, 2, None) == itf.ERR_INVALID_ARG
    assert L.wpt_sh_basis(6, d.ctypes.data, 3, out.ctypes.data) == itf.ERR_INVALID_ARG
    assert L.wpt_sh_basis(0, None, 3, None) == itf.ERR_INVALID_ARG
    assert np.all(out == F32(7.25))
    assert L.wpt_sh_basis(0, None, 2, None) == 0
    assert itf.sh_basis(np.zeros((0, 3), F32)).shape == (0, 9)
    with pytest.raises(itf.WptError) as e:
        itf.sh_basis(d, 3)
    assert e.value.code == itf.ERR_INVALID_ARG


def test_binding_and_header(wpt, itf):
    hdr = open(os.path.join(ROOT, "include", "wpt.h")).read()
    consts = dict(re.findall(r"^#define (WPT_SH_[A-Z_]+) (\d+)u?$", hdr, re.M))
    assert consts == {"WPT_SH_MAX_ORDER": str(itf.SH_MAX_ORDER), "WPT_SH_CHUNK": str(itf.SH_CHUNK)}
    assert itf.SH_MAX_ORDER == ps.MAX_ORDER == 2 and itf.SH_CHUNK == 1 << 18
    for name in ("wpt_probe_sh", "wpt_sh_basis"):
        assert name in wpt._lib.EXPORTED and name in wpt._lib.header_symbols()
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(wpt._lib._SIGS[name][1]), name
    with pytest.raises(itf.WptError) as e:
        itf.probe_sh(np.zeros((1, 6), F32))
    assert e.value.code == itf.ERR_NOT_INIT
    assert wpt.lib().wpt_last_error() == b"init not called"


# ---------------------------------------------------------------------------
# On the oracle alone: the GPU test has power
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rf.SCENES))
def test_point_sets_give_the_gpu_test_power(wpt, oracle, name):
    """In each scene's point set: a record whose expected order-2 vector has all
    nine coefficients non-zero in some channel (so a wrong basis function, a
    swapped coefficient or a skipped band shows), and a record whose band-1
    coefficients differ between NoNEE and NEE (so the render type reaches the
    weighted sum). The untraced samples of the far-normal records are skipped:
    every expected value is finite."""
    found_all9 = found_band1 = False
    for dist in (px.COSINE, px.SPHERE):
        sh = {}
        for rtype in (0, 1):
            sh[rtype], status, counts, traced = ps.set_expected(wpt, oracle, name, rtype, dist)
            assert np.isfinite(sh[rtype]).all()
            assert np.all(ps.bits(sh[rtype][~traced.any(axis=0)]) == 0)
            all9 = (sh[rtype] != 0).all(axis=1).any(axis=1)  # per record: some channel with nine non-zero coefficients
            found_all9 |= bool(all9.any())
            print(name, dist, rtype, "records with nine non-zero coefficients in a channel:", int(all9.sum()), "of", len(all9))
        band1 = (ps.bits(sh[0][:, 1:4]) != ps.bits(sh[1][:, 1:4])).any(axis=(1, 2))
        found_band1 |= bool(band1.any())
        print(name, dist, "records whose band 1 differs between NoNEE and NEE:", int(band1.sum()))
    assert found_all9 and found_band1, (name, found_all9, found_band1)


def test_untraced_samples_are_skipped_not_multiplied(wpt, oracle):
    """The MIXED_NORMAL records hold untraced samples whose generated direction is
    not finite: multiplying their +0 colour would give NaN, the definition skips."""
    sc, recs = px.point_set(wpt, oracle, "box")
    c, w, traced, status, _ = ps.set_samples(wpt, oracle, "box", 1, px.COSINE)
    skipped = ~traced & status.astype(bool)[None, :]
    assert skipped.any() and not np.isfinite(w[skipped]).all()
    assert np.all(ps.bits(c[~traced]) == 0)
    assert np.isfinite(ps.project(c, w, traced)).all()


# ---------------------------------------------------------------------------
# sh_basis under the sanitizers
# ---------------------------------------------------------------------------
def test_sh_basis_under_sanitizers(tmp_path):
    """tests/probesh_main.cpp, a program of its own: sh_basis and the host entry's
    body under AddressSanitizer and UBSan (linked statically). What it asserts is
    in the program."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/probesh_main.cpp"
    exe = str(tmp_path / "probesh_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "wasm-pathtracer_amd", "csrc"),
           os.path.join(ROOT, "tests", "probesh_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "probesh_main: 0 failed checks" in r.stdout, r.stdout[-2000:]
