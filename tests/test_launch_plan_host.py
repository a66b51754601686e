"""The tier-B launch decision (rt_launch_plan.cpp plan_launch) without a GPU: for every case of the launch table
recorded on an MI355X before the plan existed (tests/golden/launch_plans.json, scripts/launch_table.py), the plan
for the same world, parameters, CU count and RTAMD_* knobs must be the recorded launch. LDS-staged launches:
every rt_launch_info field. Launches from global memory: every field but `grid`, which the launcher bounds by the
runtime's occupancy answer: the recorded grid is at most the blocks the plan asks for, and is that number or a
multiple of the CU count (whole resident blocks per CU)."""
import pytest

import rtamd
from launch_plan_cases import (CASES, CU_COUNT, IDS, SPHERES_GLOBAL, UNITS, VARIANT, params_of, plan, plan_rc,
                               scene_of)


def _setenv(monkeypatch, c):
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_plan_is_the_recorded_launch(c, monkeypatch):
    _setenv(monkeypatch, c)
    info, extra = plan(c)
    want = dict(c["launch"])
    print(c["name"], info, extra)
    if not want["lds_staged"]:
        grid = want.pop("grid")
        asked = info.pop("grid")
        assert grid <= asked and (grid == asked or grid % CU_COUNT == 0), (grid, asked)
        assert extra["grid"] == asked
    assert info == want
    assert extra["wide_packed"] == c["wide_keys"]["packed"]
    assert extra["unit"] == UNITS[c["name"]]
    assert extra["waves"] == want["waves"]
    # the kernel's trailing arguments, from the prepared world's own counts: the stack bound (+ 3 slots of the
    # 4-wide walk, + 2 of the binary one), and for LDS-staged launches the staged nodes and leaves
    w = rtamd.prepare_scene(scene_of(c))
    wide = want["loop"] == 2
    assert extra["entries"] == (w["wide_stack_need"] + 3 if wide else w["stack_need"] + 2)
    staged = want["lds_staged"]
    assert extra["n_items"] == (0 if not staged else w["n_wide_nodes"] if wide else w["n_nodes"])
    assert extra["n_leaves"] == (w["n_leaves"] if staged and want["leaf_lds"] else 0)
    assert want["wide_nodes"] == (w["n_wide_nodes"] if wide or (want["loop"] == 1 and w["mixed_wide"]) else 0)


def test_table_covers_the_decision():
    """The recorded table itself: each branch of the decision the cases were chosen for is there."""
    by = {c["name"]: c["launch"] for c in CASES}
    F_WIDE, F_COUNT, F_SKIP = 256, 128, 32768
    assert by["random_book_one"]["waves"] == 3 and by["random_book_one"]["leaf_lds"] == 1
    assert by["random_book_one at the 4th-wave threshold"]["waves"] == 4
    assert by["random_book_one below the 4th-wave threshold"]["waves"] == 3
    assert by["random_book_one frame advance"]["waves"] == 4, "the whole frame's work decides the 4th wave"
    assert by["random_book_one adaptive advance"]["variant"] & F_SKIP
    assert by["random_book_one WIDE=0"]["loop"] == 1 and by["random_book_one REPLACE=0"]["loop"] == 0
    assert by["random_book_one reference cull"]["loop"] == 1
    assert by["random_book_one LDS=0"]["lds_staged"] == 0 and by["stress_spheres"]["lds_staged"] == 0
    assert by["random_book_one LEAF_LDS=0"]["leaf_lds"] == 0
    assert by["random_book_one WAVES=2"]["waves"] == 2
    assert by["random_book_one PARTIAL_CAP=1"]["chunk_batches"] > 1
    assert by["cornell WIDE=1"]["variant"] & F_WIDE and not by["cornell"]["variant"] & F_WIDE
    assert by["next_week_final"]["wide_nodes"] > 0 and by["next_week_final"]["loop"] == 1
    for name in ("random_book_one counting build", "cornell counting build"):
        assert by[name]["variant"] & F_COUNT and by[name]["waves"] == 1 and by[name]["lds_staged"] == 0
    packed = {c["name"]: c["wide_keys"]["packed"] for c in CASES}
    assert packed["random_book_one"] == 1 and packed["random_book_one PACKED_KEYS=0"] == 0
    assert packed["random_book_one counting build"] == 1 and packed["cornell counting build"] == 0


def test_no_cold_and_qnode_leave_the_global_unit(monkeypatch):
    """The global spheres unit serves only the 128-byte tree: RTAMD_NO_COLD and a quantised upload both send the
    global-memory 4-wide launch to the spheres unit's own table."""
    c = next(c for c in CASES if c["name"] == "random_book_one")
    monkeypatch.setenv("RTAMD_LDS", "0")
    assert plan(c)[1]["unit"] == SPHERES_GLOBAL
    monkeypatch.setenv("RTAMD_NO_COLD", "1")
    assert plan(c)[1]["unit"] == VARIANT
    monkeypatch.delenv("RTAMD_NO_COLD")
    monkeypatch.setenv("RTAMD_QNODE", "1")
    assert plan(c)[1]["unit"] == VARIANT


def test_tail_and_its_knob(monkeypatch):
    c = next(c for c in CASES if c["name"] == "cornell_smoke")
    assert plan(c)[1]["tail_items"] == 768 * CU_COUNT
    assert plan(next(c for c in CASES if c["name"] == "random_book_one"))[1]["tail_items"] == 0
    monkeypatch.setenv("RTAMD_TAIL", "0")
    assert plan(c)[1]["tail_items"] == 0


def test_adaptive_counting_build_is_invalid():
    c = CASES[0]
    rc = plan_rc(scene_of(c), params_of(c), (0, -1, 1, 1))[0]
    assert rc == rtamd.RT_E_INVALID and b"counting build" in rtamd.lib().rt_last_error()


def test_bad_span_is_invalid():
    c = CASES[0]
    for span in ((-1, 1, 0, 0), (0, 0, 0, 0), (0, 10 ** 6, 0, 0)):
        assert plan_rc(scene_of(c), params_of(c), span)[0] == rtamd.RT_E_INVALID


def test_image_over_the_work_unit_bound_is_invalid():
    """More than 2^32 - 2^24 work units in one launch: 65536 x 65528 pixels pass the 32-bit pixel-id check and
    one chunk of them does not fit a launch's 32-bit unit indices."""
    c = CASES[0]
    rc = plan_rc(scene_of(c), params_of(c, width=65536, height=65528, spp=1))[0]
    assert rc == rtamd.RT_E_INVALID and b"work units" in rtamd.lib().rt_last_error()


@pytest.mark.parametrize("c", CASES[:6], ids=IDS[:6])
def test_plan_twice_is_the_same(c):
    assert plan(c) == plan(c)
