"""Host check of the chunk and lane plan in csrc/pbs_passes.hpp (chunk_items, lanes_wanted, lane_part: what
run_blind_rotation cuts a batch by): tests/cpp/lane_plan_check.cpp dumps them over nb = 1 ... 300, default lane counts
0 ... 6, every granted lane count and a handful of item sizes around 4 GiB, and every record is checked here against a
restatement of the rules that does not read the C++.  No GPU: hipcc builds the header's host side."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
GIB4 = 4 << 30
MAX_LANES = 4  # the caller's stream + StreamFork::MAX_SIDE

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """{"W": {(nb, dflt): wanted}, "P": {(nb, lanes): [(off, n), ...] in lane order}, "C": [(item, batch, chunk)]}"""
    d = tmp_path_factory.mktemp("lane_plan")
    exe, path = str(d / "lane_plan_check"), str(d / "plan.txt")
    subprocess.run([HIPCC, "-O2", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "lane_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    subprocess.run([exe, path], check=True, timeout=60)
    out = {"W": {}, "P": {}, "C": []}
    for line in open(path):
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "W":
            out["W"][(v[0], v[1])] = v[2]
        elif tag == "P":
            parts = out["P"].setdefault((v[0], v[1]), [])
            assert v[2] == len(parts)  # lanes in order
            parts.append((v[3], v[4]))
        else:
            out["C"].append(tuple(v))
    return out


def test_every_case_is_dumped(plan):
    assert sorted(plan["W"]) == [(nb, d) for nb in range(1, 301) for d in range(7)]
    for (nb, _), wanted in plan["W"].items():
        assert all((nb, lanes) in plan["P"] for lanes in range(1, wanted + 1))
    items = {c[0] for c in plan["C"]}
    assert {1, GIB4 - 1, GIB4 + 1} <= items and len(plan["C"]) >= 40


def test_lanes_wanted(plan):
    """One lane below 64 items; from 64 on the default clamped to 1 ... 4, with at least 16 items per lane."""
    for (nb, dflt), wanted in plan["W"].items():
        want = 1 if nb < 64 else max(1, min(dflt, MAX_LANES, nb // 16))
        assert wanted == want, (nb, dflt)
        if nb < 64:
            assert wanted == 1
        assert 1 <= wanted <= MAX_LANES
    assert plan["W"][(70, 2)] == 2 and plan["W"][(70, 4)] == 4 and plan["W"][(63, 4)] == 1 and plan["W"][(64, 4)] == 4


def test_lane_parts_cover_the_chunk_in_order(plan):
    for (nb, lanes), parts in plan["P"].items():
        assert len(parts) == lanes
        pos = 0
        for off, n in parts:  # contiguous, in order
            assert off == pos, (nb, lanes)
            pos += n
        assert pos == nb  # cover [0, nb)
        sizes = [n for _, n in parts]
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True), (nb, lanes)  # larger parts first
        assert sizes == [nb // lanes + (j < nb % lanes) for j in range(lanes)]


def test_wanted_lanes_hold_16_items_each(plan):
    for (nb, dflt), wanted in plan["W"].items():
        if wanted > 1:
            assert all(n >= 16 for _, n in plan["P"][(nb, wanted)]), (nb, dflt)


def test_seventy_items(plan):
    assert plan["W"][(70, 2)] == 2 and plan["P"][(70, 2)] == [(0, 35), (35, 35)]
    assert plan["W"][(70, 4)] == 4 and plan["P"][(70, 4)] == [(0, 18), (18, 18), (36, 17), (53, 17)]


def test_chunk_items(plan):
    for item, batch, chunk in plan["C"]:
        assert 1 <= chunk <= batch, (item, batch)
        assert chunk * item <= GIB4 or chunk == 1, (item, batch)
        assert chunk == max(1, min(batch, GIB4 // item)), (item, batch)
