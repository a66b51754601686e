"""The launch table on the GPU: for every case of tests/golden/launch_plans.json (recorded before the launch plan
existed, scripts/launch_table.py) a render, a frame's advance or the counting build must launch exactly what was
recorded, grid included (rt_last_launch, wide_keys), and that must be the plan rt_internal_launch_plan returns
for the same inputs without a device: the plan is what launches. The cases render 64x48 to 512x512 pixels at
1 to 4 spp."""
import os
import sys

import pytest
import torch

import rtamd
from launch_plan_cases import CASES, CU_COUNT, IDS, UNITS, plan

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
import launch_table  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_launch_is_the_recorded_one_and_the_plan(gpu_ctx, c, monkeypatch):
    assert torch.cuda.get_device_properties(0).multi_processor_count == CU_COUNT, "the table's device (an MI355X)"
    got, keys = launch_table.launch(gpu_ctx, c)
    print(c["name"], got, keys)
    assert got == c["launch"]
    assert keys == c["wide_keys"]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    info, extra = plan(c)
    if not got["lds_staged"]:
        assert got["grid"] <= info["grid"]
        info["grid"] = got["grid"]
    assert info == got
    assert extra["wide_packed"] == keys["packed"]
    assert extra["unit"] == UNITS[c["name"]] and extra["waves"] == got["waves"]
