"""Register budget of the shadow presolve, pinned at build level (CPU only).

WPT_OPT_PRESOLVE_SHADOW adds presolve_shadow, a read-modify-write of col and a
third scan field with its atomic lane to k_shade's presolving (PS) variants.
As test_build_drop_miss.py does, the test compiles wpt_render.hip for gfx950
with the Makefile's own `asm` command line and reads the kernels' resource
metadata. Only resource figures are asserted.

The bounds are the ones the variants had before the change: NEE 72 VGPRs and
no scratch, its CR (stock) variant 74, the PNEE variants 80 with the scratch
they had. The PNEE variant that reads the octree from global memory (OCT = 0)
is compiled without the shadow presolve, because with it its scratch grew
from 20 to 24 B; its bound holds as for the others.
"""
import pytest

from test_build_drop_miss import _one, _shade, resources  # noqa: F401  (the module-scoped fixture)

# k_shade<TRI_ONLY = true, PNEE, OCT, CR, PS = true>: (PNEE, OCT, CR) -> (VGPRs, scratch bytes) allowed
BOUNDS = {
    (0, 0, 0): (72, 0), (0, 0, 1): (74, 0),
    (1, 0, 0): (80, 20), (1, 0, 1): (80, 24),
    (1, 1, 0): (80, 12), (1, 1, 1): (80, 16),
    (1, 2, 0): (80, 16), (1, 2, 1): (80, 16),
}


@pytest.mark.parametrize("args", sorted(BOUNDS))
def test_presolving_shade_variants_stay_inside_their_bounds(resources, args):  # noqa: F811
    pnee, oct_, cr = args
    v, s, scratch = _one(resources, _shade(pnee, oct_, cr, 1))
    print(f"k_shade<true, {pnee}, {oct_}, {cr}, true>:", v, s, scratch)
    bv, bscratch = BOUNDS[args]
    assert v <= bv and scratch <= bscratch


def test_production_shade_keeps_its_scalar_registers(resources):  # noqa: F811
    v, s, scratch = _one(resources, _shade(0, 0, 0, 1))
    assert s <= 106


@pytest.mark.parametrize("frag", ["k_shadowILb1ELb0ELi0E", "k_extendILb1ELb0ELi0E", "k_traceILb1ELb0EE"])
def test_traversal_kernels_keep_eight_waves(resources, frag):  # noqa: F811
    """test_build_occupancy.py's limits: their code is untouched."""
    v, s, scratch = _one(resources, frag)
    print(frag, v, s, scratch)
    assert v <= 64 and s <= 80 and scratch == 0
