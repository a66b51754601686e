"""The recorded launch table (tests/golden/launch_plans.json, written by scripts/launch_table.py on an MI355X at
the commit before the launch plan existed) and the device-free plan (rt_internal_launch_plan) for its cases:
shared by tests/test_launch_plan_host.py and tests/test_gpu_launch_plan.py."""
import ctypes as C
import json
import os

import numpy as np

import rtamd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
with open(GOLDEN) as _f:
    TABLE = json.load(_f)
CU_COUNT = TABLE["cu_count"]
CASES = TABLE["cases"]
IDS = [c["name"].replace(" ", "_") for c in CASES]
EXTRA = ("n_items", "entries", "n_leaves", "trav_stop", "leaf_stop", "box_first", "med_batch", "batch", "batch_floor",
         "rev_tiles", "tail_items", "per_batch", "wide_packed", "unit", "grid", "waves")
# KernelForm::unit (rt_launch_plan.h) of each recorded case: the translation unit whose kernel the launch takes
VARIANT, SPHERES_PACKED, SPHERES_GLOBAL, COUNT_PACKED = 0, 1, 2, 3
UNITS = {
    "three_spheres": VARIANT, "random_book_one": SPHERES_PACKED, "stress_spheres": SPHERES_GLOBAL,
    "cornell": VARIANT, "cornell_smoke": VARIANT, "next_week_final": VARIANT,
    "random_book_one WIDE=0": VARIANT, "random_book_one LDS=0": SPHERES_GLOBAL,
    "random_book_one LEAF_LDS=0": SPHERES_PACKED, "random_book_one PACKED_KEYS=0": VARIANT,
    "random_book_one REPLACE=0": VARIANT, "random_book_one WAVES=2": SPHERES_PACKED,
    "random_book_one QNODE=1 LDS=0": VARIANT,  # (the quantised tree: the spheres unit's F_QNODE kernels)
    "random_book_one reference cull": VARIANT,
    "random_book_one at the 4th-wave threshold": SPHERES_PACKED,
    "random_book_one below the 4th-wave threshold": SPHERES_PACKED,
    "cornell WIDE=1": VARIANT,  # (Cornell's packed kernels live in its own unit)
    "cornell_smoke TAIL=0": VARIANT, "random_book_one PARTIAL_CAP=1": SPHERES_PACKED,
    "random_book_one frame advance": SPHERES_PACKED, "random_book_one adaptive advance": SPHERES_PACKED,
    "random_book_one counting build": COUNT_PACKED, "cornell counting build": VARIANT,
}
_scenes = {}


def scene_of(c):
    key = (c["world"], c["param"])
    if key not in _scenes:
        _scenes[key] = rtamd.make_scene(c["world"], rtamd.randGen(1024), param=c["param"])[0]
    return _scenes[key]


def params_of(c, **kw):
    kw = {"width": c["width"], "height": c["height"], "spp": c["spp"], "flags": c["flags"], **kw}
    return rtamd.make_params(kw["width"], kw["height"], kw["spp"], c["depth"], rtamd.RT_RNG_PHILOX, seed=c["seed"],
                             flags=kw["flags"])


def span_of(c):
    """(span_first, span_count, count_build, adaptive) of the case's recorded launch."""
    return {"render": (0, -1, 0, 0), "work": (0, -1, 1, 0), "frame": (0, 1, 0, 0), "adaptive": (1, 1, 0, 1)}[c["mode"]]


def plan_rc(scene, params, span=(0, -1, 0, 0), cu_count=None):
    """rt_internal_launch_plan under the current environment: (return code, rt_launch_info dict, extras dict)."""
    fn = rtamd.lib().rt_internal_launch_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                   C.c_void_p]
    info = rtamd.rt_launch_info()
    extra = np.zeros(len(EXTRA), dtype=np.int32)
    rc = fn(C.addressof(scene.desc), 0, CU_COUNT if cu_count is None else cu_count, C.addressof(params), *span,
            C.addressof(info), extra.ctypes.data)
    return (rc, {k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_},
            dict(zip(EXTRA, (int(x) for x in extra))))


def plan(c):
    rc, info, extra = plan_rc(scene_of(c), params_of(c), span_of(c))
    assert rc == 0, rtamd.lib().rt_last_error()
    return info, extra
