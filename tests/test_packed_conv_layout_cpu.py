"""babe_packed_conv_plan - which images a Conv2d gets, how large each is, nt, raw - answers what the recorded table says over the
grid of tests/golden/make_packed_conv_layout_golden.py.  The table was recorded from the rules babe_amd/ops.py::PackedConv held
before the library owned them (csrc/model.hip's copy agreed on all 1296 shapes).  Pure host arithmetic: no GPU."""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def grid():
    spec = importlib.util.spec_from_file_location("make_packed_conv_layout_golden", os.path.join(GOLDEN, "make_packed_conv_layout_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rows(grid):
    """(cases, recorded rows, the library's rows): one (nt, raw, [bytes of the ten slots]) per case."""
    from babe_amd import _lib
    with open(os.path.join(GOLDEN, "packed_conv_layout.json")) as fh:
        want = grid.expand(json.load(fh))
    return list(grid.cases()), want, grid.evaluate(_lib._LIB_PATH)


def test_grid_crosses_the_clauses(grid):
    cases = list(grid.cases())
    want_ch = {1, 2, 4, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 128, 192, 256}
    assert {c[0] for c in cases} == want_ch and {c[1] for c in cases} == want_ch
    assert {c[2:4] for c in cases} == {(5, 3), (1, 1), (3, 3), (5, 1)}
    assert {c[4] for c in cases} == {0, 1, 2}
    assert {c[5:7] for c in cases} == {(nt, nt11) for nt in (0, 1, 2) for nt11 in (0, 2)}
    masks = {c[7] for c in cases}
    assert masks == {grid.ALL, 0} | {grid.ALL & ~(1 << b) for b in range(5)} and len(masks) == 7
    # every shape meets every setting, and every splits value every (nt, nt11) pair and every mask
    assert len(cases) == len(set(cases)) == 18 * 18 * 4 * len(grid.SETTINGS)
    for s in (0, 1, 2):
        assert {st[1:3] for st in grid.SETTINGS if st[0] == s} == {(nt, nt11) for nt in (0, 1, 2) for nt11 in (0, 2)}
        assert {st[3] for st in grid.SETTINGS if st[0] == s} == masks


def test_form_bits_are_the_headers(grid):
    """The grid's masks, ops.PackedConv's and the header's name the same bits."""
    from babe_amd import ops
    hdr = open(os.path.join(ROOT, "include", "babe_hip.h")).read()
    bits = {k: int(v) for k, v in re.findall(r"BABE_CONV_FORM_(\w+) = (\d+)", hdr)}
    assert [bits[n] for n in grid.FORM_BITS] == [1, 2, 4, 8, 16] and len(bits) == 5
    assert int(re.search(r"BABE_CONV_FORMS_ALL = (\d+)", hdr).group(1)) == grid.ALL == 31
    assert ops._FORM_BITS == ("winograd", "winograd4", "winograd45", "winograd85", "fewco")      # F23, F43, F25, F45, FEWCO


def test_layouts_are_the_recorded_ones(rows):
    cases, want, got = rows
    assert len(cases) == len(want) == len(got)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} of {len(cases)} layouts changed; first: case {cases[bad[0]]}: got {got[bad[0]]}, recorded {want[bad[0]]}"


def test_the_recorded_table_is_not_vacuous(rows, grid):
    """Every Winograd slot is present somewhere and absent somewhere, so are raw and the (1,1) rule's nt.  The two direct slots have
    no rule that omits them: they are present in every row, as fp32 and as bf16 images."""
    cases, want, _ = rows
    for i, name in enumerate(grid.SLOTS):
        present = {bool(r[2][i]) for r in want}
        assert present == ({True} if i < 2 else {True, False}), name
    assert {c[4] for c in cases} == {0, 1, 2}
    assert {r[1] for r in want} == {0, 1}
    for nt in (0, 1, 2):                                    # the caller's nt is kept; nt == 0 becomes nt11 somewhere and stays 0 somewhere
        assert {r[0] for c, r in zip(cases, want) if c[5] == nt} == ({0, 2} if nt == 0 else {nt})
    assert {r[0] for c, r in zip(cases, want) if c[6] == 0} == {0, 1, 2} and all(r[0] == c[5] for c, r in zip(cases, want) if c[6] == 0)


def test_bytes_are_the_size_functions(rows):
    """Every non-zero bytes[i] is the matching babe_conv_packed_size* value times the element size (4; 2 under splits)."""
    from babe_amd._lib import lib
    L = lib()
    cases, _, got = rows
    sizes = {}

    def size_of(shape, splits):
        if (shape, splits) not in sizes:
            co, ci, kh, kw = shape
            per_tf = []
            for tf in (0, 1):
                if splits:
                    per_tf.append([2 * L.babe_conv_packed_size_bf16(co, ci, kh, kw, tf, splits)])
                else:
                    per_tf.append([4 * L.babe_conv_packed_size(co, ci, kh, kw, tf), 4 * L.babe_conv_packed_size_wino(co, ci, kh, tf),
                                   4 * L.babe_conv_packed_size_wino4(co, ci, kh, tf), 4 * L.babe_conv_packed_size_wino45(co, ci, tf),
                                   4 * L.babe_conv_packed_size_wino85(co, ci, tf)])
            sizes[shape, splits] = per_tf
        return sizes[shape, splits]

    checked = 0
    for c, (_, _, b) in zip(cases, got):
        per_tf = size_of(c[:4], c[4])
        for i, v in enumerate(b):
            if v:
                assert i // 2 < len(per_tf[i & 1]) and v == per_tf[i & 1][i // 2], (c, i, v)
                checked += 1
    assert checked > 2 * len(cases)


def test_bad_arguments_are_refused():
    import ctypes as C
    from babe_amd._cabi import PackedConvLayout
    from babe_amd._lib import lib
    L = lib()
    lay = PackedConvLayout()
    assert L.babe_packed_conv_plan(64, 64, 5, 3, 0, 0, 2, 31, C.byref(lay)) == 0
    for bad in ((0, 64, 5, 3, 0, 0, 2, 31), (64, 0, 5, 3, 0, 0, 2, 31), (64, 64, 0, 3, 0, 0, 2, 31), (64, 64, 5, 3, 3, 0, 2, 31),
                (64, 64, 5, 3, -1, 0, 2, 31), (64, 64, 5, 3, 0, -1, 2, 31), (64, 64, 5, 3, 0, 0, -2, 31)):
        assert L.babe_packed_conv_plan(*bad, C.byref(lay)) < 0 and b"packed_conv_plan" in L.babe_last_error(), bad
    assert L.babe_packed_conv_plan(64, 64, 5, 3, 0, 0, 2, 31, None) < 0
    assert L.babe_packed_conv_pack(None, None, None) < 0 and b"packed_conv_pack" in L.babe_last_error()
