"""Register budget of k_generate_shade, pinned at build level (CPU only).

WPT_OPT_GEN_SHADE adds one kernel, k_generate_shade<TRI_ONLY>: gen_path, the
primary ray's presolve, shade_path and k_shade's presolving epilogue in one
body. As test_build_drop_miss.py does, the test compiles wpt_render.hip for
gfx950 with the Makefile's own `asm` command line and reads the kernels'
resource metadata. Only resource figures are asserted.

The kernel runs once per batch, so its occupancy is not the point; scratch
is: neither instantiation may use any. Their VGPR counts are pinned at what
the build of this change gives (triangle scenes 86, other shapes 110).
"""
import pytest

from test_build_drop_miss import _one, resources  # noqa: F401  (the module-scoped fixture)

# k_generate_shade<TRI_ONLY>: TRI_ONLY -> VGPRs of this change's build
VGPRS = {1: 86, 0: 110}


@pytest.mark.parametrize("tri_only", [1, 0])
def test_generate_shade_has_no_scratch_and_keeps_its_registers(resources, tri_only):  # noqa: F811
    v, s, scratch = _one(resources, f"k_generate_shadeILb{tri_only}EE")
    print(f"k_generate_shade<{bool(tri_only)}>:", v, s, scratch)
    assert scratch == 0
    assert v <= VGPRS[tri_only]
