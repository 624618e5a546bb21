"""The buffers a session keeps between calls, across viewport changes.

One session runs the call sequence of tests/lifecycle_fixtures.py at 24 x 16,
then after update_viewport(37, 21), where every grow-only buffer must grow and
the 777 pixels put every plane off a 256 B boundary, then after
update_viewport(8, 8), where every capacity is larger than needed. At each size
everything the calls return equals, bit for bit, the same calls in a fresh
session (shutdown, init) at that size: a stale capacity, a layout that moved or
a buffer that outlived its viewport would show here.
"""
import pytest

import lifecycle_fixtures as lf

pytestmark = pytest.mark.gpu


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def test_outputs_survive_viewport_changes(wpt, itf):
    tris = lf.mesh(wpt)
    resized = {}
    lf.start(itf, wpt, tris, lf.SIZES[0])
    for k, vp in enumerate(lf.SIZES):
        if k:
            itf.update_viewport(*vp)
        resized[vp] = lf.calls(itf, wpt, vp)
    for vp in lf.SIZES:
        itf.shutdown()
        lf.start(itf, wpt, tris, vp)
        fresh = lf.calls(itf, wpt, vp)
        assert [n for n, _ in fresh] == [n for n, _ in resized[vp]]
        for (name, want), (_, got) in zip(fresh, resized[vp]):
            assert got.dtype == want.dtype and got.shape == want.shape, (vp, name)
            assert got.tobytes() == want.tobytes(), f"{vp}: {name} differs from a fresh session's"
    # the sequence did trace: the map gave samples, the frame holds them
    cnt = dict(resized[lf.SIZES[1]])["read_radiance[1]"]
    assert cnt.min() >= 1 and cnt.max() > 1
