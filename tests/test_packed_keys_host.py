"""The 4-wide walk's packed sort keys (include/rt_wide.h): the pack / unpack helpers are host-and-device
inlines, checked here without a GPU by a stand-alone C program (tests/c/packed_keys_check.c) built with
AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_key_helpers(tmp_path):
    """Every admitted child reference round-trips under every key pattern; words of keys a < b never order b
    before a; a rejected word exceeds every accepted one."""
    exe = str(tmp_path / "packed_keys_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
           "-static-libasan", "-static-libubsan"]
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", *san, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "packed_keys_check.c"), "-lm", "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "packed_keys_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
