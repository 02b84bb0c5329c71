"""Host side of the packed two-level CSR build: tests/native/test_graph_plan.cpp (csrc/graph_plan.h on the CPU, plain and under the
sanitizers) and fsw_graph_build_plan, the host-only export that says what fsw_graph_build_two_level does with a shape.  No GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsw_gnn_amd", "libfsw_hip.so")
WORDS = ("two_level", "packed", "tile", "stage_cap", "passes", "row_bits", "sender_bits", "buckets")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-g")], ids=["plain", "sanitized"])
def test_graph_plan_native(tmp_path, flags):
    exe = str(tmp_path / "fsw_test_graph_plan")
    src = os.path.join(ROOT, "tests", "native", "test_graph_plan.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def plan():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    L = _lib.lib()

    def f(rows, cols, edges, weighted=False):
        out = (ctypes.c_int32 * len(WORDS))()
        assert L.fsw_graph_build_plan(rows, cols, edges, int(weighted), out) == 0
        return dict(zip(WORDS, list(out)))
    return f


def test_plan_export_is_declared_bound_and_additive():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert "int fsw_graph_build_plan(int64_t num_rows, int64_t num_cols, int64_t num_edges, int weighted, int32_t* out);" in header
    assert re.search(r"#define FSW_GRAPH_PLAN_WORDS %d\b" % len(WORDS), header)
    assert "fsw_graph_build_plan" in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.FSW_ABI_VERSION


# rows, cols, edges, weighted -> two_level, packed, tile, sender bits
SHAPES = [
    (32_768, 32_768, 262_144, False, (1, 1, 8192, 15)),
    (32_767, 32_768, 262_144, False, (0, 0, 0, 0)),
    (32_768, 32_768, 262_143, False, (0, 0, 0, 0)),
    (32_768, 1 << 21, 262_144, False, (1, 1, 8192, 21)),
    (32_768, (1 << 21) + 1, 262_144, False, (1, 0, 4096, 22)),
    (32_768, 32_768, 262_144, True, (1, 0, 4096, 15)),
    (1_000_000, 1_000_000, 10_000_000, False, (1, 1, 8192, 20)),           # the benchmark's graph: 9 upper bits, one pass
    ((1 << 20) - 1, 1 << 20, 2_000_000, False, (1, 1, 8192, 20)),          # the last row count with one partition pass
    (1 << 20, 1 << 20, 2_000_000, False, (1, 0, 4096, 20)),                # 10 upper bits: two passes, bucket starts from the keys
    (40_000, 40_000, 1_400_000, False, (0, 0, 0, 0)),                      # average bucket above 65536
    (40_000, 40_000, 0, False, (0, 0, 0, 0)),
]


@pytest.mark.parametrize("rows,cols,edges,weighted,want", SHAPES)
def test_plan_boundaries(plan, rows, cols, edges, weighted, want):
    p = plan(rows, cols, edges, weighted)
    assert (p["two_level"], p["packed"], p["tile"], p["sender_bits"]) == want, p
    ref = R.bucket_plan(rows, max(edges, 1), weighted)
    assert bool(p["two_level"]) == (ref["two_level_ok"] and edges > 0)
    if p["two_level"]:
        assert (p["stage_cap"], p["passes"], p["row_bits"], p["buckets"]) == (ref["stage_cap"], ref["passes"], 11, ref["buckets"]), (p, ref)
        assert p["packed"] == int(not weighted and p["passes"] == 1 and p["row_bits"] + p["sender_bits"] <= 32)
    else:
        assert p == dict.fromkeys(WORDS, 0)


def test_plan_refuses_bad_arguments(plan):
    from fsw_gnn_amd import _lib
    out = (ctypes.c_int32 * len(WORDS))()
    L = _lib.lib()
    assert L.fsw_graph_build_plan(0, 10, 10, 0, out) != 0 and L.fsw_last_error()
    assert L.fsw_graph_build_plan(10, 10, 10, 0, None) != 0
