"""A fixed session for counting allocation calls (profiles/devmem/README.md):
the sequence of tests/lifecycle_fixtures.py at its three viewports in one
session, then adaptive sampling on both halves with the sample stock on and one
compute of 8 samples per pixel, then shutdown. Run it under a HIP API trace and
read the counts of hipMalloc, hipFree, hipHostMalloc and hipHostFree:

  rocprofv3 --hip-trace --stats -d DIR -o run -- python3 tools/alloc_calls.py

Two trees that print the same checksum and show the same four counts allocate,
free and therefore synchronise the device at the same places."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lifecycle_fixtures as lf
    import wpt_loader

    pkg = wpt_loader.load()
    itf = pkg.interface
    tris = lf.mesh(pkg)
    crc = 0
    itf.set_device(0)
    lf.start(itf, pkg, tris, lf.SIZES[0])
    try:
        for k, vp in enumerate(lf.SIZES):
            if k:
                itf.update_viewport(*vp)
            for _, a in lf.calls(itf, pkg, vp):
                crc = zlib.crc32(a.tobytes(), crc)
        vp = lf.SIZES[0]
        itf.update_viewport(*vp)
        itf.update_settings(1, 1, 1, 1, 0)  # adaptive on both halves; the stock is on by default
        assert itf.get_option("stock") > 0
        itf.compute(8 * vp[0] * vp[1])
        acc, cnt = itf.read_radiance(*vp)
        crc = zlib.crc32(cnt.tobytes(), zlib.crc32(acc.tobytes(), crc))
        st = itf.stats()
    finally:
        itf.shutdown()
    print(f"alloc_calls: outputs crc32 {crc:08x}, stock samples traced {st['stock_traced']}")


if __name__ == "__main__":
    main()
