"""Record which weight images a Conv2d gets - babe_packed_conv_plan's answer: nt, raw, bytes of the ten image slots - over a grid.

    python tests/golden/make_packed_conv_layout_golden.py    # writes tests/golden/packed_conv_layout.json

The function is pure host arithmetic (no GPU, no environment switch), so the table made at one commit can be compared exactly at
another: tests/test_packed_conv_layout_cpu.py imports this module for the grid and compares what the library answers with the
table, slot by slot.  The committed table was recorded from the rules babe_amd/ops.py::PackedConv held before the library owned
them.  Regenerate it only when a rule is MEANT to change.

The table is the rows in a compact, lossless form: per case one code (bit i: slot i present; bit 10: raw; bits 11..: nt), and per
(shape, splits) the bytes of each slot where it is present - an image's size does not depend on nt or the forms, which `encode`
insists on while it builds the table.  `expand` gives the rows back.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "packed_conv_layout.json")

# both sides of every clause: <= 4 (raw image), % 16, > 32, the 32-channel tile counts of the (1,1) rule, the 64 / 96 / 128 tiles
CH = (1, 2, 4, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 128, 192, 256)
KS = ((5, 3), (1, 1), (3, 3), (5, 1))
from babe_amd._cabi import IMAGE_SLOTS as SLOTS, PackedConvLayout as Layout  # noqa: E402
# the form bits of include/babe_hip.h (BABE_CONV_FORM_*), in bit order
FORM_BITS = ("F23", "F43", "F25", "F45", "FEWCO")
ALL = (1 << len(FORM_BITS)) - 1
MASKS = (ALL, 0) + tuple(ALL & ~(1 << b) for b in range(len(FORM_BITS)))
# (splits, nt, nt11, forms): splits x nt x nt11 under the default forms, and every other mask under the loader's (nt, nt11)
SETTINGS = tuple((s, nt, nt11, ALL) for s in (0, 1, 2) for nt in (0, 1, 2) for nt11 in (0, 2)) + \
    tuple((s, 0, 2, m) for s in (0, 1, 2) for m in MASKS[1:])


def shapes():
    for co in CH:
        for ci in CH:
            for kh, kw in KS:
                yield co, ci, kh, kw


def cases():
    """(Cout, Cin, KH, KW, splits, nt, nt11, forms) of every question, in the table's order."""
    for shp in shapes():
        for st in SETTINGS:
            yield shp + st


def evaluate(path):
    """What the library at `path` answers: one row (nt, raw, [bytes of the ten slots]) per case."""
    L = C.CDLL(path)
    L.babe_packed_conv_plan.restype = C.c_int
    L.babe_packed_conv_plan.argtypes = [C.c_int] * 8 + [C.POINTER(Layout)]
    rows = []
    for case in cases():
        lay = Layout()
        if L.babe_packed_conv_plan(*case, C.byref(lay)) != 0 or lay.splits != case[4]:
            raise RuntimeError(f"babe_packed_conv_plan{case} failed")
        rows.append((lay.nt, lay.raw, list(lay.bytes)))
    return rows


def encode(rows):
    """Rows in cases() order -> the table."""
    codes, sizes = [], {}
    for case, (nt, raw, b) in zip(cases(), rows):
        assert len(b) == len(SLOTS) and raw in (0, 1) and nt >= 0 and all(v >= 0 for v in b), (case, nt, raw, b)
        codes.append(sum(1 << i for i, v in enumerate(b) if v) | raw << 10 | nt << 11)
        known = sizes.setdefault(case[:5], [0] * len(SLOTS))
        for i, v in enumerate(b):
            if v:
                assert known[i] in (0, v), (case, SLOTS[i], known[i], v)
                known[i] = v
    assert len(codes) == len(rows)
    return {"slots": list(SLOTS), "form_bits": list(FORM_BITS), "codes": codes,
            "bytes": [sizes[shp + (s,)] for shp in shapes() for s in (0, 1, 2)]}


def expand(table):
    """The table -> rows in cases() order."""
    assert table["slots"] == list(SLOTS) and table["form_bits"] == list(FORM_BITS)
    sizes = {shp + (s,): b for (shp, s), b in zip(((shp, s) for shp in shapes() for s in (0, 1, 2)), table["bytes"])}
    rows = [(code >> 11, code >> 10 & 1, [v if code >> i & 1 else 0 for i, v in enumerate(sizes[case[:5]])])
            for case, code in zip(cases(), table["codes"])]
    assert len(rows) == len(table["codes"]) == len(list(cases()))
    return rows


if __name__ == "__main__":
    from babe_amd import _lib
    table = encode(evaluate(_lib._LIB_PATH))
    with open(OUT, "w") as fh:
        json.dump(table, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{OUT}: {len(table['codes'])} cases, {os.path.getsize(OUT)} bytes")
