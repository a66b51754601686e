"""The lean step loop of the packed 4-wide walk reads its lane predicates off the walk's registers and ends its leaf
step with selects (rt_wlane_walking / _seeking / _holding, rt_wstep_slot, rt_wstep_postpone: host-and-device inlines
of include/rt_wide.h). Checked here without a GPU by a stand-alone C program (tests/c/walk_step_check.c), built
plainly and once more with AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_every_walking_lane_is_seeking_or_holding(tmp_path, build):
    """After any wide step or leaf step a lane that still walks is seeking or holding, so the loop that steps only
    such lanes cannot spin; the select forms of the leaf step's postpone and sweep leave the state the branch forms
    leave, and read only slots of the lane's own stack."""
    exe = str(tmp_path / f"walk_step_check_{build}")
    flags = SAN if build == "sanitized" else ["-O2"]
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "walk_step_check.c"), "-lm", "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "walk_step_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
