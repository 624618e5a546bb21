"""Fixed small sessions that walk the launch layer's dispatch dimensions
(profiles/variants/README.md), for a census of what each library launches:

  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/launch_census.py fixed
  python3 tools/launch_census.py compare A_kernel_trace.csv B_kernel_trace.csv
  python3 tools/launch_census.py reached A_kernel_trace.csv [B_kernel_trace.csv ...]

`fixed` runs the sessions without async lanes (what they launch does not depend
on host timing), `stock` the adaptive sessions with the sample stock (async
lanes: their census may differ from run to run). Both at 64 x 48, on a
triangle-only scene and on one with other shapes: depth-capped and RR-only
(down to k_finish), NEE and PNEE with installed trees for the octree views 0,
1 and 2, presolve and gen-shade on and off, counting on and off, both
traversals, fused and separate launches, first_hit and photon_sample in each
view, and a session that shoots its own photons. Each prints a crc32 over all
its outputs.

`compare` holds two kernel traces against each other per kernel name: the
multiset of (grid size, workgroup size, LDS size) over its dispatches.
`reached` lists, per templated kernel family of wpt_render.hip, the
instantiations the traces show.
"""
import collections
import csv
import os
import re
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

W, H, SPP, DEPTH, SEED = 64, 48, 2, 4, 0xBABABEBE
NEE, PNEE = 1, 2
FAMILIES = ("k_extend", "k_shadow", "k_trace", "k_shade", "k_finish", "k_generate_shade", "k_first_hit",
            "k_photon_hit", "k_photon_sample")


def _trees(fx):
    """Photon lists (two lights) whose octrees k_shade reads in view 0, 1 and 2."""
    wide = fx.tree("wide").photons
    return {0: wide, 1: tuple(a[:30000] for a in wide), 2: fx.tree("octants").photons}


class Census:
    def __init__(self):
        import numpy as np
        import pnee_fixtures as fx
        import wpt_loader
        self.np, self.pkg = np, wpt_loader.load()
        self.itf = self.pkg.interface
        self.trees = _trees(fx)
        # triangle-only: scene 2 with a triangle cloud; other shapes: scene 100 (both have two lights)
        self.scenes = {"triangles": (2, self.pkg.scenes.triangle_cloud(3000, seed=0x5EED)), "shapes": (100, None)}
        self.crc, self.sessions = 0, 0
        rng = np.random.default_rng(7)
        self.points = rng.uniform(-2.0, 2.0, (257, 3)).astype(np.float32)
        self.states = rng.integers(1, 2 ** 32, 257, dtype=np.uint64).astype(np.uint32)

    def add(self, *arrays):
        for a in arrays:
            self.crc = zlib.crc32(self.np.ascontiguousarray(a).tobytes(), self.crc)

    def session(self, kind, types=(NEE, NEE), depth=DEPTH, adaptive=(0, 0), counting=0, view=None, hooks=False,
                spp=SPP, **opts):
        itf, np = self.itf, self.np
        scene_id, mesh = self.scenes[kind]
        for k, v in opts.items():
            itf.set_option(k, v)  # the defaults of the init below
        itf.init(W, H, scene_id, *self.pkg.scenes.scene_camera(scene_id))
        try:
            if mesh is not None:
                itf.store_mesh(1, mesh)
            itf.update_settings(types[0], types[1], adaptive[0], adaptive[1], 0)
            itf.set_render_options(depth, SEED, 0)
            itf.set_counting(counting)
            assert itf.get_option("scene_tri_only") == (1 if kind == "triangles" else 0)
            if view is not None:
                itf.install_photons(self.trees[view])
                assert itf.get_option("oct_view") == view
            if hooks:
                for v in (0, 1, 2):
                    self.add(*itf.photon_sample(self.points, self.states, v))
                self.add(*itf.first_hit(0).values())
            itf.compute(W * H * spp)
            itf.sync()
            self.add(*itf.read_radiance(W, H))
            st = itf.stats()
            self.add(np.array([st[k] for k in ("paths", "rays", "shadow_rays", "ext_visits", "sh_visits",
                                               "finish_paths")], np.uint64))
        finally:
            itf.shutdown()
            itf.set_option("defaults", 0)
        self.sessions += 1
        return st

    def fixed(self):
        for kind in self.scenes:
            for counting in (0, 1):
                # (the fused form runs the exact BVH2 only; a scene with other shapes takes the BVH4 by itself)
                self.session(kind, counting=counting, traversal=0, traversal_sh=0, fused=1)
                for trav, trav_sh in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    self.session(kind, counting=counting, traversal=trav, traversal_sh=trav_sh, fused=0, fused_below=0)
            self.session(kind, presolve=0)
            self.session(kind, gen_shade=0)
            self.session(kind, lanes=1, fused=0, fused_below=0)  # one lane: the full traversal grids
            st = self.session(kind, depth=0, spp=8)  # RR-only, to k_finish
            assert st["finish_paths"] > 0
            st = self.session(kind, types=(PNEE, PNEE), depth=0, spp=8, view=2)
            assert st["finish_paths"] > 0
            for view in (0, 1, 2):
                self.session(kind, types=(PNEE, PNEE), view=view, hooks=view == 2)
                self.session(kind, types=(PNEE, PNEE), view=view, presolve=0)
            st = self.session(kind, types=(NEE, PNEE))  # the session shoots its own photons
            assert st["photons"] > 0

    def stock(self):
        for kind in self.scenes:
            for types, views in (((NEE, NEE), (None,)), ((PNEE, PNEE), (0, 1, 2))):
                for view in views:
                    for opts in ({}, {"presolve": 0}):
                        st = self.session(kind, types=types, adaptive=(1, 1), view=view, spp=12, **opts)
                        assert st["stock_traced"] > 0
                st = self.session(kind, types=types, adaptive=(1, 1), depth=0, view=views[-1], spp=12)
                assert st["stock_traced"] > 0


def _rows(path):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            grid = tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ")
            wg = tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")
            yield name, (grid, wg, int(r["LDS_Block_Size"]))


def census(path):
    c = collections.defaultdict(collections.Counter)
    for name, shape in _rows(path):
        c[name][shape] += 1
    return c


def compare(a, b):
    ca, cb = census(a), census(b)
    bad = 0
    for name in sorted(set(ca) | set(cb)):
        if ca[name] != cb[name]:
            bad += 1
            only_a, only_b = ca[name] - cb[name], cb[name] - ca[name]
            print(f"DIFFERENT {name}: {sum(only_a.values())} dispatches only in the first, "
                  f"{sum(only_b.values())} only in the second; e.g. {list(only_a.items())[:2]} / {list(only_b.items())[:2]}")
    total = sum(sum(c.values()) for c in ca.values())
    print(f"kernels: first {len(ca)} names ({total} dispatches), second {len(cb)} names "
          f"({sum(sum(c.values()) for c in cb.values())}); identical {len(set(ca) | set(cb)) - bad}, different {bad}")
    return bad


def reached(paths):
    seen = collections.defaultdict(collections.Counter)
    for p in paths:
        for name, _ in _rows(p):
            # demangled, or the mangled template arguments (Lb1E: true, Li2E: 2)
            m = re.search(r"\b(k_\w+)<([^>]*)>", name) or re.search(r"(k_[a-z_]+)I((?:L[bi]\dE)+)E", name)
            if m and m.group(1) in FAMILIES:
                seen[m.group(1)][m.group(2)] += 1
    for fam in FAMILIES:
        print(f"{fam}: {len(seen[fam])} instantiations reached")
        for args in sorted(seen[fam]):
            print(f"  <{args}> {seen[fam][args]} dispatches")


def main(argv):
    if len(argv) >= 2 and argv[0] == "compare":
        return 1 if compare(argv[1], argv[2]) else 0
    if len(argv) >= 2 and argv[0] == "reached":
        reached(argv[1:])
        return 0
    if argv not in (["fixed"], ["stock"]):
        print(__doc__)
        return 2
    c = Census()
    c.itf.set_device(0)
    getattr(c, argv[0])()
    print(f"launch_census {argv[0]}: {c.sessions} sessions, outputs crc32 {c.crc:08x}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
