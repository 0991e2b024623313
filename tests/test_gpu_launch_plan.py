"""GPU: the public planning calls through the real C ABI against tests/golden/launch_plan_table.npz (see plan_table_grid.py
and tests/test_launch_plan_cpu.py): the default context and CUDASW4_AMD_CHAIN=4 with CUDASW4_AMD_CHAIN_ALL=1.  Host
arithmetic and one sw_set_query per query length; nothing is scanned."""
import ctypes
import os

import numpy as np
import pytest

import plan_table_grid as G
from gpu_util import gpu_modules

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", ["default", "chain4_all"])
def test_planning_calls_replay_the_recorded_table(variant, monkeypatch):
    torch, capi, _ = gpu_modules()
    table = np.load(G.DATA)
    if torch.cuda.get_device_properties(0).multi_processor_count != int(table["num_cus"]):
        pytest.skip("the table was recorded on a device with %d CUs" % int(table["num_cus"]))
    for key in list(os.environ):
        if key.startswith("CUDASW4_AMD_") and key != "CUDASW4_AMD_LIB":
            monkeypatch.delenv(key)
    for key, value in dict(G.VARIANTS)[variant].items():
        monkeypatch.setenv(key, value)
    lib = ctypes.CDLL(capi.LIB_PATH)   # (a handle of its own: record() binds argument types)
    got = G.record(lib)
    for field in G.LAUNCH_FIELDS + ("service",):
        want = table[variant + "/" + field]
        bad = np.argwhere(got[field] != want)
        assert len(bad) == 0, (field, len(bad), "first at", bad[0].tolist(), int(got[field][tuple(bad[0])]), int(want[tuple(bad[0])]))
    if variant == "default":
        assert G.plan_query_table(lib).tolist() == table["plan_query"].tolist()
