"""csrc/wpt_devmem.h on the host: tests/devmem_main.cpp defines the four HIP
allocation calls itself (malloc-backed, counting, able to fail the k-th call),
so the owners, the hooks' scratch and Slices run without the HIP runtime, as a
program of their own under AddressSanitizer and UBSan (linked statically).
What it asserts is in the program; this test builds and runs it."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_devmem_owners_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/devmem_main.cpp"
    exe = str(tmp_path / "devmem_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
           "-I" + os.path.join(ROOT, "wasm-pathtracer_amd", "csrc"),
           os.path.join(ROOT, "tests", "devmem_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert " 0 bad frees, 0 live, 0 failed checks" in r.stdout, r.stdout
