"""The record slab's block map and the host merge under AddressSanitizer + UBSan, the way tests/c does it:
tests/c/shard_block_check.cpp, a stand-alone program with its own main, drives rt_layout.h's slab_geometry,
slab_block and slab_slot_pixel (the one map the slab kernels, rt_assemble_records_async and
rt_assemble_records_host all use) and rt_features.cpp's rt_assemble_records_host over a grid of small geometries,
compiled for the CPU with the sanitizers. Any report fails."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TC = os.path.join(ROOT, "tests", "c")
CSRC = os.path.join(ROOT, "ray-tracing_amd", "csrc")


def test_slab_block_map_is_sanitizer_clean():
    out = os.path.join(TC, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shard_block_check_asan")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(TC, "shard_block_check.cpp"), os.path.join(CSRC, "rt_features.cpp"),
                    os.path.join(CSRC, "rt_scene.cpp")], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "shard_block_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
