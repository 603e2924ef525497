"""The table of the UNet layer path's A/B switches (babe_amd/forms.py): what every environment variable parses to, that the table
is the only reader of the environment on the Python side, and that no test leaves a form behind.  No GPU."""
import ast
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, F = True, False

# variable -> {attribute or derived flag: its value with the variable unset, "0", "1", "2"}: the expressions ops.py and
# unet_engine.py applied to os.environ before the table existed, written out
TRUTH = {
    "BABE_BF16_HBM_F32": {"bf16_hbm_f32": (T, F, T, T)},
    "BABE_CONV_WINO": {"conv_wino": ("4", "0", "1", "2"), "winograd": (T, F, T, T), "winograd4": (T, F, F, F),
                       "winograd45": (T, F, F, F), "winograd85": (T, F, F, F)},
    "BABE_CONV_FEWCO": {"fewco": (T, F, T, T)},
    "BABE_CONV_WINO45": {"wino45": (T, F, T, T), "winograd": (T, T, T, T), "winograd4": (T, T, T, T),
                         "winograd45": (T, F, T, T), "winograd85": (T, F, T, T)},
    "BABE_CONV_F45": {"f45": (T, F, T, T), "winograd45": (T, T, T, T), "winograd85": (T, F, T, T)},
    "BABE_CONV11_NT": {"conv11_nt": (2, 0, 1, 2)},
    "BABE_FUSE_GN": {"fuse_gn": (F, F, T, T)},
    "BABE_FUSE_GN_FWD": {"fuse_gn_fwd": (T, F, T, T)},
    "BABE_GN_FUSED": {"gn_fused": (F, F, T, F)},
    "BABE_GELU_FIN": {"gelu_fin": (T, F, T, T)},
    "BABE_CONV_BF16U": {"units": (T, F, T, T)},
    "BABE_AXPBY2": {"axpby2": (T, F, T, T)},
    "BABE_UNET_C": {"unet_c": (F, F, T, F)},
    "BABE_MERGE_TAIL": {"merge_tail": (T, F, T, T)},
}
VALUES = (None, "0", "1", "2")


def _value(forms, environ, name):
    """A switch under `environ`: the table's rule for the two the library owns (a Forms object would ask the library), the Forms
    attribute - stored or derived - for the rest."""
    return forms.parse(environ)[name] if name in forms.LIBRARY_OWNED else getattr(forms.Forms(environ), name)


def test_every_variable_parses_as_it_did():
    from babe_amd import forms
    assert {var for _, var, _, _, _ in forms.TABLE} == set(TRUTH) and len(forms.TABLE) == 14
    for var, expected in TRUTH.items():
        for name, want in expected.items():
            for v, w in zip(VALUES, want):
                got = _value(forms, {} if v is None else {var: v}, name)
                assert got == w and type(got) is type(w), (var, v, name, got, w)
    # BABE_CONV_WINO=4, the default spelled out: every family on
    f = forms.Forms({"BABE_CONV_WINO": "4"})
    assert (f.conv_wino, f.winograd, f.winograd4, f.winograd45, f.winograd85) == ("4", T, T, T, T)
    # the derived flags follow the stored ones, they are not stored a second time
    f.conv_wino = "2"
    assert (f.winograd, f.winograd4, f.winograd45, f.winograd85) == (T, F, F, F)


def test_the_table_is_the_only_reader_of_the_environment():
    for path in ("babe_amd/ops.py", "babe_amd/networks/unet_engine.py"):
        src = open(os.path.join(ROOT, path)).read()
        assert not re.search(r"\b(environ|getenv)\b", src), path
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for var in TRUTH:
        assert re.search(r"\b%s\b" % var, doc), f"{var} is not mentioned in INTEGRATION.md"


def test_no_test_assigns_a_form_raw():
    """A form assigned with `=` stays selected for every later test of the session: monkeypatch.setattr(FORMS, ...) undoes itself."""
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "golden", "*.py"))
    assert len(files) > 50
    for path in files:
        for node in ast.walk(ast.parse(open(path).read())):
            if not isinstance(node, (ast.Assign, ast.AugAssign)):
                continue
            targets = node.targets if isinstance(node, ast.Assign) else [node.target]
            for t in (e for tgt in targets for e in ast.walk(tgt) if isinstance(e, ast.Attribute)):      # (tuple targets too)
                owner = getattr(t.value, "id", None) or getattr(t.value, "attr", None)                    # FORMS.x / forms.FORMS.x
                assert owner != "FORMS", f"{path}:{node.lineno}: FORMS.{t.attr} assigned raw"


_CHILD = """
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
print(L.babe_unet_form_get(0), L.babe_unet_form_get(1), L.babe_unet_form_get(2), L.babe_unet_form_set(2, 1))
assert L.babe_unet_form_set(0, 0) == 0 and L.babe_unet_form_set(1, 5) == 0
print(L.babe_unet_form_get(0), L.babe_unet_form_get(1))
"""


@pytest.mark.parametrize("v", VALUES)
def test_the_library_reads_its_two_forms_as_the_table_says(v):
    """babe_unet_form_get in a fresh process with BABE_FUSE_GN_FWD and BABE_FUSE_GN both unset / "0" / "1" / "2": the values of the
    truth table; a bad index is refused; a set is seen by the next get."""
    import __graft_entry__ as ge
    ge.build()
    env = {k: e for k, e in os.environ.items() if k not in ("BABE_FUSE_GN_FWD", "BABE_FUSE_GN")}
    if v is not None:
        env.update(BABE_FUSE_GN_FWD=v, BABE_FUSE_GN=v)
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "babe_amd", "libbabe_hip.so")], env=env, check=True,
                         capture_output=True, text=True).stdout.split()
    i = VALUES.index(v)
    want = [int(TRUTH["BABE_FUSE_GN_FWD"]["fuse_gn_fwd"][i]), int(TRUTH["BABE_FUSE_GN"]["fuse_gn"][i])]
    got = [int(x) for x in out]
    assert got[:3] == want + [-1] and got[3] != 0 and got[4:] == [0, 1], got
