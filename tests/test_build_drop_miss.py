"""Register budget of the dropped misses, pinned at build level (CPU only).

WPT_OPT_DROP_MISS adds a drop test, a packed scan column and (CR) a count
store to k_shade's presolving variants, and k_generate_ps keeps kGenTile paths
per thread. As test_build_occupancy.py does, the test compiles wpt_render.hip
for gfx950 with the Makefile's own `asm` command line and reads the kernels'
resource metadata, here by full template arguments.

PARENT holds (VGPRs, scratch bytes) of every triangle-scene k_shade variant in
a build of the commit before this change, made with the same command line.
"""
import re
import subprocess

import pytest

from test_build_occupancy import CSRC, _asm_command

# k_shade<TRI_ONLY = true, PNEE, OCT, CR, PS>: (PNEE, OCT, CR, PS) -> (VGPRs, scratch bytes) of the parent commit
PARENT = {
    (0, 0, 0, 0): (72, 0), (0, 0, 0, 1): (72, 0), (0, 0, 1, 0): (74, 0), (0, 0, 1, 1): (74, 0),
    (1, 0, 0, 0): (80, 20), (1, 0, 0, 1): (80, 20), (1, 0, 1, 0): (80, 24), (1, 0, 1, 1): (80, 24),
    (1, 1, 0, 0): (80, 12), (1, 1, 0, 1): (80, 12), (1, 1, 1, 0): (80, 16), (1, 1, 1, 1): (80, 16),
    (1, 2, 0, 0): (80, 16), (1, 2, 0, 1): (80, 16), (1, 2, 1, 0): (80, 16), (1, 2, 1, 1): (80, 16),
}


def _shade(pnee, oct_, cr, ps):
    return f"k_shadeILb1ELb{pnee}ELi{oct_}ELb{cr}ELb{ps}EE"


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """Mangled kernel name -> (VGPRs, SGPRs, scratch bytes)."""
    out = str(tmp_path_factory.mktemp("asm") / "wpt_render.s")
    subprocess.run(_asm_command(out), cwd=CSRC, check=True, capture_output=True, timeout=600)
    res = {}
    for blk in open(out).read().split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return res


def _one(resources, frag):
    hits = [v for k, v in resources.items() if frag in k]
    assert len(hits) == 1, (frag, len(hits))
    return hits[0]


def test_production_shade_keeps_seven_waves(resources):
    v, s, scratch = _one(resources, _shade(0, 0, 0, 1))  # k_shade<true, false, 0, false, true>
    print("k_shade<true, false, 0, false, true>:", v, s, scratch)
    assert v <= 72 and s <= 106 and scratch == 0


@pytest.mark.parametrize("args", sorted(PARENT))
def test_triangle_shade_variants_no_larger_than_the_parents(resources, args):
    v, s, scratch = _one(resources, _shade(*args))
    print(f"k_shade<true, {args}>:", v, s, scratch)
    pv, pscratch = PARENT[args]
    assert v <= pv and scratch <= pscratch


def test_generate_ps_has_no_scratch(resources):
    v, s, scratch = _one(resources, "k_generate_psE")
    print("k_generate_ps:", v, s, scratch)
    assert scratch == 0
