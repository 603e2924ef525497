"""The host arithmetic behind bf16 networks on the library path (csrc/conv_auto.hip, csrc/model.hip), without a GPU: which convs a
precision turns into bf16 products (babe_conv_splits_for), which layers may take bf16 units (babe_conv2d_bf16_units_shape), what
the loader refuses before any device call, and the image sizes it carves for a (shape, splits)."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, BF16X3 = 0, 1, 2

# (Cout, Cin, KH, KW) -> splits under (precision 1, precision 2) with hbm_f32 = 1, written out from the rule's own statement: a
# conv with <= 4 channels on one side stays fp32; so does a (1,1) conv with fewer than 32 channels on its smaller side; so does
# every (1,1) conv under bf16x3.  Precision 0, and any precision with hbm_f32 = 0, return the precision itself.
TRUTH = {
    # 2 <-> N, N <-> 2 and 4-channel shapes
    (2, 64, 5, 3): (0, 0), (64, 2, 5, 3): (0, 0), (2, 64, 1, 1): (0, 0), (64, 2, 1, 1): (0, 0), (16, 2, 1, 1): (0, 0),
    (4, 64, 5, 3): (0, 0), (64, 4, 5, 3): (0, 0), (4, 4, 3, 3): (0, 0), (4, 64, 1, 1): (0, 0),
    (8, 5, 5, 3): (1, 2), (5, 8, 5, 3): (1, 2),                            # 5 channels: past the few-channel clause
    # (1,1) with 16, 31, 32 and 64 channels on the smaller side
    (16, 64, 1, 1): (0, 0), (64, 16, 1, 1): (0, 0), (31, 64, 1, 1): (0, 0), (64, 31, 1, 1): (0, 0),
    (32, 64, 1, 1): (1, 0), (64, 32, 1, 1): (1, 0), (32, 32, 1, 1): (1, 0), (64, 64, 1, 1): (1, 0), (128, 64, 1, 1): (1, 0),
    # (5,3) with 8 and 64 channels
    (8, 8, 5, 3): (1, 2), (64, 64, 5, 3): (1, 2), (8, 64, 5, 3): (1, 2), (64, 8, 5, 3): (1, 2),
    # a (3,3) kernel is no (1,1) kernel
    (16, 16, 3, 3): (1, 2),
}


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from babe_amd._lib import lib
    return lib()


def test_conv_splits_for_against_the_table():
    L = _lib()
    for shape, (s1, s2) in TRUTH.items():
        for hbm in (0, 1):
            assert L.babe_conv_splits_for(*shape, F32, hbm) == 0, (shape, hbm)
        assert L.babe_conv_splits_for(*shape, BF16, 1) == s1, shape
        assert L.babe_conv_splits_for(*shape, BF16X3, 1) == s2, shape
        assert L.babe_conv_splits_for(*shape, BF16, 0) == 1 and L.babe_conv_splits_for(*shape, BF16X3, 0) == 2, shape
    for bad in ((64, 64, 5, 3, -1, 1), (64, 64, 5, 3, 3, 1), (0, 64, 5, 3, 1, 1), (64, 64, 0, 3, 1, 1)):
        assert L.babe_conv_splits_for(*bad) == -1 and b"conv_splits_for" in L.babe_last_error(), bad


def test_python_rule_is_a_call_of_the_library(monkeypatch):
    """ops.PackedConv.splits_for gives the table's values, and follows FORMS.bf16_hbm_f32 on the Python side."""
    _lib()
    from babe_amd import ops
    from babe_amd.forms import FORMS
    for shape, (s1, s2) in TRUTH.items():
        assert ops.PackedConv.splits_for(shape, "f32") == 0
        assert (ops.PackedConv.splits_for(shape, "bf16"), ops.PackedConv.splits_for(shape, "bf16x3")) == (s1, s2), shape
    monkeypatch.setattr(FORMS, "bf16_hbm_f32", False)
    for shape in TRUTH:
        assert (ops.PackedConv.splits_for(shape, "bf16"), ops.PackedConv.splits_for(shape, "bf16x3")) == (1, 2), shape


def test_units_shape_at_each_clause_edge():
    L = _lib()
    from babe_amd._cabi import CPackedConv

    def ok(T=64, Cin=64, Cout=64, splits=1, KH=5, KW=3):
        pc = CPackedConv()
        pc.Cout, pc.Cin, pc.KH, pc.KW, pc.splits = Cout, Cin, KH, KW, splits
        return L.babe_conv2d_bf16_units_shape(C.byref(pc), T)

    assert ok() == 1
    assert ok(T=62) == 0 and ok(T=64) == 1 and ok(T=16) == 1 and ok(T=66) == 0
    assert ok(Cin=60) == 0 and ok(Cin=64) == 1 and ok(Cin=40, Cout=40) == 1
    assert ok(Cout=32) == 0 and ok(Cout=40) == 1 and ok(Cin=32, Cout=32) == 0
    assert ok(splits=0) == 0 and ok(splits=1) == 1 and ok(splits=2) == 0
    assert ok(KH=3, KW=3) == 0 and ok(KH=1, KW=1) == 0 and ok(KH=5, KW=1) == 0
    assert L.babe_conv2d_bf16_units_shape(None, 64) == 0


def test_python_units_rule_is_form_and_library(monkeypatch):
    _lib()
    from babe_amd import ops
    from babe_amd._cabi import CPackedConv
    from babe_amd.forms import FORMS

    class PC:                                            # what units_ok reads of a PackedConv
        def __init__(self, N, splits):
            self.Cout = self.Cin = N
            self.desc = CPackedConv()
            self.desc.Cout, self.desc.Cin, self.desc.KH, self.desc.KW, self.desc.splits = N, N, 5, 3, splits

    monkeypatch.setattr(FORMS, "units", True)
    assert ops.units_ok(PC(64, 1), 64, 64, 64) is True and ops.units_ok(PC(64, 1), 64, 64, 62) is False
    assert ops.units_ok(PC(32, 1), 32, 32, 64) is False and ops.units_ok(PC(64, 2), 64, 64, 64) is False
    monkeypatch.setattr(FORMS, "units", False)
    assert not ops.units_ok(PC(64, 1), 64, 64, 64)


def test_loader_refuses_a_precision_out_of_range_without_a_gpu(tmp_path):
    """babe_model_load_ex / babe_model_create_ex with precision -1 and 3: NULL and a message, whatever the path or the tables hold -
    host code before the loader's first device call (the pattern of test_loader_refuses_damaged_files_without_a_gpu).  A precision
    in range goes on to the file: the missing path is what it reports."""
    L = _lib()
    missing = str(tmp_path / "no_such_file.babe").encode()
    for p in (-1, 3):
        assert not L.babe_model_load_ex(missing, p, None)
        msg = L.babe_last_error().decode()
        assert msg.startswith("model_load") and f"precision {p}" in msg, msg
        assert not L.babe_model_create_ex(None, 0, None, 0, p, None)
        msg = L.babe_last_error().decode()
        assert msg.startswith("model_create") and f"precision {p}" in msg, msg
    for p in (F32, BF16, BF16X3):
        assert not L.babe_model_load_ex(missing, p, None) and b"cannot open" in L.babe_last_error()
        assert not L.babe_model_create_ex(None, 0, None, 0, p, None) and b"empty tables" in L.babe_last_error()
    assert L.babe_model_precision(None) == -1 and b"null model" in L.babe_last_error()


def test_a_damaged_file_is_refused_at_every_precision(tmp_path):
    """The precision changes nothing about what the parser refuses: a truncated file is refused by name at 0, 1 and 2."""
    L = _lib()
    from babe_amd import model_file
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    Ns = [8, 8, 8, 8, 16, 16, 16]
    args = default_args(sample_rate=22050, audio_len=92092, Ns=Ns, T=3, start_sigma=0.05)
    path = str(tmp_path / "good.babe")
    model_file.export(init_state_dict(Ns, args.network.num_dils, seed=0, gate_scale=1.0), args, path)
    blob = open(path, "rb").read()
    cut = str(tmp_path / "cut.babe")
    with open(cut, "wb") as fh:
        fh.write(blob[:len(blob) // 2])
    for p in (F32, BF16, BF16X3):
        assert not L.babe_model_load_ex(cut.encode(), p, None)
        assert L.babe_last_error().decode().startswith("model_load: " + cut), L.babe_last_error()


# the conv shapes of a network of widths NS_WIDE (tests/test_gpu_model_c.py) and what is particular about each
SHAPES = [(16, 2, 1, 1), (16, 16, 5, 3), (2, 16, 5, 3), (48, 16, 1, 1), (48, 48, 5, 3), (64, 48, 1, 1), (64, 64, 5, 3), (64, 128, 1, 1),
          (16, 2, 5, 3), (2, 64, 1, 1), (64, 2, 5, 3), (48, 112, 1, 1), (2, 48, 1, 1)]


@pytest.mark.parametrize("precision", [F32, BF16, BF16X3])
def test_plan_bytes_for_the_loaders_shapes_are_packed_convs_buffers(precision):
    """What Builder::conv carves for (shape, babe_conv_splits_for(shape, precision, 1)) = the buffers ops.PackedConv allocates for
    that conv: with splits, ONE int16 image per direction of babe_conv_packed_size_bf16 elements (what babe_conv_pack_weights_bf16
    writes) and nothing else - no Winograd image, no raw weights; with splits 0, the fp32 layout, untouched by the precision.
    Every byte count is a multiple of 16, so 2-byte images keep the carver's 256-byte granules aligned for 16-byte loads."""
    L = _lib()
    from babe_amd._cabi import IMAGE_SLOTS, PackedConvLayout
    seen = set()
    for shape in SHAPES:
        splits = L.babe_conv_splits_for(*shape, precision, 1)
        seen.add(splits)
        lay, ref = PackedConvLayout(), PackedConvLayout()
        assert L.babe_packed_conv_plan(*shape, splits, 0, 2, 31, C.byref(lay)) == 0
        assert lay.splits == splits
        if splits == 0:
            assert L.babe_packed_conv_plan(*shape, 0, 0, 2, 31, C.byref(ref)) == 0
            assert bytes(lay) == bytes(ref) and lay.bytes[0] == 4 * L.babe_conv_packed_size(*shape, 0)
            continue
        want = [2 * L.babe_conv_packed_size_bf16(*shape, 0, splits), 2 * L.babe_conv_packed_size_bf16(*shape, 1, splits)] + [0] * 8
        assert list(lay.bytes) == want and lay.raw == 0, (shape, dict(zip(IMAGE_SLOTS, lay.bytes)))
        assert all(b % 16 == 0 and b > 0 for b in want[:2])
        # half (bf16) or as many (bf16x3) bytes as an fp32 image of the same padded tile counts would take: 2 bytes x splits per weight
        Cout, Cin, KH, KW = shape
        pad = lambda n, m: (n + m - 1) // m * m
        assert want[0] == 2 * splits * KH * KW * pad(Cin, 16) * pad(Cout, 32)
        assert want[1] == 2 * splits * KH * KW * pad(Cout, 16) * pad(Cin, 32)
    assert seen == ({0} if precision == F32 else {0, precision})
