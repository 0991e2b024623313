"""The launch plan (cudasw4_amd/csrc/sw_plan.hpp: plan_launch) on the CPU, without a context or a device.

tests/golden/launch_plan_table.npz holds what the public planning calls answered, over the grid of plan_table_grid.py, at
the commit before plan_launch existed (recorded on an MI355X; the file stores its CU count).  A small stand-alone program
(tests/host/launch_plan_replay.cpp) links the library, fills PlanSettings from that CU count and the variant's environment
and calls plan_launch over the same grid: every answer must equal the recording.  The same program checks that sizing
agrees with launching:
  (a) for every scratch offered (nothing, one workgroup's need, half the reported need, the reported need) the plan's
      grid x bytes_per_workgroup stays inside it, and a multi-stripe plan that cannot fit one workgroup says so (SW_ERR_TEMP);
  (b) with gap scores (-11, -1) and exactly the scratch sw_scan_temp_bytes reports, the launch has the chain length,
      stream columns, border capacity and grid that were sized: no clamp engages;
  (c) with any other gap extension the launch never needs more than it was given."""
import os
import subprocess

import numpy as np
import pytest

import plan_table_grid as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cudasw4_amd", "lib")
CSRC = os.path.join(ROOT, "cudasw4_amd", "csrc")


@pytest.fixture(scope="module")
def table():
    return np.load(G.DATA)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_replay")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "host", "launch_plan_replay.cpp"), "-L" + LIBDIR, "-lcudasw4_amd",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    return exe


def csv(values):
    return ",".join(str(v) for v in values)


def test_plan_header_is_plain_cxx(replay):
    """sw_plan.hpp includes no HIP header (and g++ has compiled the replay program, which includes nothing else of the library)"""
    includes = [line for line in open(os.path.join(CSRC, "sw_plan.hpp")) if line.startswith("#include")]
    assert includes == ["#include <cstddef>\n", "#include <cstdint>\n"]


def test_plan_query_matches_the_recording(table):
    import ctypes
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libcudasw4_amd.so"))
    assert G.plan_query_table(lib).tolist() == table["plan_query"].tolist()


@pytest.mark.parametrize("variant", [name for name, _ in G.VARIANTS])
def test_plan_launch_replays_the_recorded_table(table, replay, variant, monkeypatch):
    for key in list(os.environ):
        if key.startswith("CUDASW4_AMD_"):
            monkeypatch.delenv(key)
    env = dict(os.environ)
    env.update(dict(G.VARIANTS)[variant])
    p = subprocess.run([replay, str(int(table["num_cus"])), csv((G.MATRIX_MAX, G.PSSM_MAX)), csv(G.QLENS), csv(G.PARTS), csv(G.NS), csv(G.MSLS),
                        ",".join("%d:%d" % g for g in G.GAPS), csv(G.SERVICE_WGS)], env=env, capture_output=True)
    # properties (a), (b), (c): the program's exit status counts the violations, stderr names the first of them
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    words = np.frombuffer(p.stdout, dtype=np.int64)
    shape = table[variant + "/rc"].shape
    n_launch = int(np.prod(shape)) * 7
    launch = words[:n_launch].reshape(shape + (7,))
    service = words[n_launch:].reshape(table[variant + "/service"].shape)
    assert (table[variant + "/rc"] == 0).all()
    for i, field in enumerate(("eff_kind", "rows", "nstripes", "lanes", "slot", "temp", "falls_back")):
        want = table[variant + "/" + field].astype(np.int64)
        bad = np.argwhere(launch[..., i] != want)
        assert len(bad) == 0, (field, len(bad), "first at [qtype, qlen, kind, part, n, max_len] =", bad[0].tolist(),
                               int(launch[..., i][tuple(bad[0])]), int(want[tuple(bad[0])]))
    assert (service == table[variant + "/service"]).all()
