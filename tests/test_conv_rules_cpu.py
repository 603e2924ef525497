"""The conv launchers' host rules answer what the recorded table says: packed sizes, *_supported / *_preferred verdicts and the
stat-slot count over the grid of tests/golden/make_conv_rules_golden.py.  Pure host arithmetic: no GPU, no environment switch."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def grid():
    spec = importlib.util.spec_from_file_location("make_conv_rules_golden", os.path.join(GOLDEN, "make_conv_rules_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tables(grid):
    from babe_amd import _lib
    with open(os.path.join(GOLDEN, "conv_rules.json")) as fh:
        want = json.load(fh)
    return want, grid.evaluate(_lib._LIB_PATH)


def test_grid_crosses_the_clauses(grid):
    """The grid is the one the table was recorded over, and it holds the cases the rules branch on."""
    cases = list(grid.verdict_cases())
    assert {1, 2, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128, 256, 2032, 2048} <= {c["Cin"] for c in cases} & {c["Cout"] for c in cases}
    assert {12, 16, 20, 30, 60, 64, 272} <= {c["T"] for c in cases}
    assert {(5, 3), (1, 1), (3, 3)} == {(c["KH"], c["KW"]) for c in cases}
    for p in ("in_", "in2", "out", "res"):
        assert {4, 8, 0} <= {c[p] % 16 for c in cases if c.get(p)}, p
    for s in ("in_bs", "in_cs", "in2_bs", "in2_cs", "out_bs", "out_cs", "res_bs", "res_cs"):
        assert {0, 1, 2, 3} <= {c[s] % 4 for c in cases if s in c}, s
    for lim in grid.LIMS:
        for s, ch in (("in_cs", "Cin"), ("out_cs", "Cout"), ("res_cs", "Cout")):
            v = [c[ch] * c[s] for c in cases if s in c]
            assert any(x < lim for x in v) and any(x >= lim for x in v), (s, lim)
    for k in ("in2", "res", "in_scale", "fbias"):
        assert any(c.get(k) for c in cases) and any(not c.get(k) for c in cases)


def test_packed_sizes_are_the_recorded_ones(tables):
    want, got = tables
    assert set(got["sizes"]) == set(want["sizes"])
    for fn, vals in want["sizes"].items():
        assert got["sizes"][fn] == vals, fn


def test_verdicts_are_the_recorded_ones(tables, grid):
    want, got = tables
    assert got["verdict_bits"] == want["verdict_bits"] and len(got["verdicts"]) == len(want["verdicts"])
    bad = [i for i, (g, w) in enumerate(zip(got["verdicts"], want["verdicts"])) if g != w]
    if bad:
        cases = list(grid.verdict_cases())
        i = bad[0]
        changed = [n for b, n in enumerate(want["verdict_bits"]) if (got["verdicts"][i] ^ want["verdicts"][i]) >> b & 1]
        pytest.fail(f"{len(bad)} of {len(cases)} verdicts changed; first: case {i} {cases[i]}: {changed}")
    # every rule says yes somewhere and no somewhere: the table is not vacuous
    for b, name in enumerate(want["verdict_bits"]):
        assert {v >> b & 1 for v in want["verdicts"]} == {0, 1}, name


def test_stat_slots_are_the_recorded_ones(tables):
    want, got = tables
    assert got["stat_slots"] == want["stat_slots"] and any(want["stat_slots"])
