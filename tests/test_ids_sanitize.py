"""The host-only code of the material-ID coverage buffers under AddressSanitizer + UBSan, the way tests/c does it:
tests/c/ids_check.cpp, a stand-alone program with its own main, drives rt_ids.cpp's fold, rank resolve, matte and
preview (rt_ids.h's shared per-sample and per-pixel text) over exactly sized arrays, and rt_launch_plan.cpp's plan
as an id pass asks for it, compiled for the CPU with the sanitizers. Nothing is loaded into Python. Any report
fails."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TC = os.path.join(ROOT, "tests", "c")
CSRC = os.path.join(ROOT, "ray-tracing_amd", "csrc")


def test_id_buffers_host_code_is_sanitizer_clean():
    out = os.path.join(TC, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "ids_check_asan")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(TC, "ids_check.cpp"), os.path.join(CSRC, "rt_ids.cpp"),
                    os.path.join(CSRC, "rt_launch_plan.cpp"), os.path.join(CSRC, "rt_scene.cpp")],
                   check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ids_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
