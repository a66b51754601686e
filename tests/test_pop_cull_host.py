"""The stack cull of the 4-wide walk's packed form (rt_wkey_beyond, include/rt_wide.h): a host-and-device inline,
checked here without a GPU by a stand-alone C program (tests/c/pop_cull_check.c), built plainly and once more
with AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_pop_cull_never_drops_an_accepted_child(tmp_path, build):
    """Whenever the cull would drop a stacked word, wide_keys2's acceptance with far = min(f, tmax32) rejects that
    child; an infinite bound, an infinite slack and the -0.0 word never cull."""
    exe = str(tmp_path / f"pop_cull_check_{build}")
    flags = SAN if build == "sanitized" else ["-O2"]
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "pop_cull_check.c"), "-lm", "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pop_cull_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
