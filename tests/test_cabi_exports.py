"""The C-ABI library loads without a GPU and exports every symbol include/babe_hip.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_match_header():
    import __graft_entry__ as ge
    ge.build()
    hdr = open(os.path.join(ROOT, "include", "babe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(babe_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 10
    L = ctypes.CDLL(os.path.join(ROOT, "babe_amd", "libbabe_hip.so"))
    missing = [n for n in sorted(names) if not hasattr(L, n)]
    assert not missing, missing
    L.babe_version.restype = ctypes.c_char_p
    assert b"gfx950" in L.babe_version()


def _prototypes():
    """{name: (return type, [parameter declarations])} of every function include/babe_hip.h declares."""
    hdr = open(os.path.join(ROOT, "include", "babe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(babe_[a-z0-9_]+)\s*\(", hdr))
    hdr = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", hdr, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(babe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        params = params.strip()
        protos[name] = (ret.strip(), [] if params == "void" else [p.strip() for p in params.split(",")])
    assert set(protos) == names, sorted(names ^ set(protos))          # a prototype the parser cannot read: reformat it
    return protos


def _agrees(decl, ct, is_param):
    """Does the ctypes type `ct` of the binding table pass what the C declaration `decl` ('const float* x', 'long') takes?"""
    from babe_amd import _cabi
    words = [w for w in re.findall(r"\w+", decl) if w != "const"]
    if is_param:
        words = words[:-1]                                            # the parameter's name
    base = " ".join(words)
    if "*" in decl:
        if isinstance(ct, type) and issubclass(ct, ctypes._Pointer):
            return not issubclass(ct._type_, ctypes.Structure) or _cabi.STRUCTS.get(base) is ct._type_
        return ct in (ctypes.c_void_p, ctypes.c_char_p)
    if base in _cabi.STRUCTS:                                         # a struct passed by value
        return ct is _cabi.STRUCTS[base]
    if base == "void":
        return ct is None and not is_param
    if base in ("long", "size_t"):
        return ct in (ctypes.c_long, ctypes.c_ulong, ctypes.c_size_t, ctypes.c_ssize_t, ctypes.c_int64, ctypes.c_uint64) \
            and ctypes.sizeof(ct) == 8
    return {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}[base] is ct


def test_binding_table_matches_header():
    """Every entry of the binding table (babe_amd/_cabi.py::SIGS) against the prototype include/babe_hip.h declares: the function
    exists, takes as many arguments, and each argument and the return value is of the prototype's kind - a pointer where C takes a
    pointer (to the mirrored struct where the table names one), a 64-bit integer for long, c_int / c_float / c_double for int /
    float / double.  A wrong entry would truncate a pointer or shift every later argument."""
    from babe_amd import _cabi
    protos = _prototypes()
    assert len(_cabi.SIGS) >= 100
    for name, (restype, argtypes) in _cabi.SIGS.items():
        assert name in protos, f"{name}: not declared in the header"
        ret, params = protos[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        assert _agrees(ret, restype, False), (name, "returns", ret, restype)
        for i, (p, ct) in enumerate(zip(params, argtypes)):
            assert _agrees(p, ct, True), (name, i, p, ct)


def test_nothing_undeclared_is_called():
    """Every `.babe_<name>(` call in the package, the tools, the entry script and the tests names a function of the binding table,
    and the bound library has no other babe_* attribute: an undeclared function cannot be called with guessed argument types."""
    import glob
    import pytest
    from babe_amd import _cabi
    from babe_amd._lib import lib
    files = glob.glob(os.path.join(ROOT, "babe_amd", "**", "*.py"), recursive=True) + \
        glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True) + \
        glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "__graft_entry__.py")]
    assert len(files) > 50
    for f in files:
        undeclared = set(re.findall(r"\.(babe_\w+)\s*\(", open(f).read())) - set(_cabi.SIGS)
        assert not undeclared, (f, sorted(undeclared))
    L = lib()
    assert isinstance(vars(L)["babe_version"], ctypes._CFuncPtr)      # a plain attribute holding the ctypes function itself
    with pytest.raises(AttributeError, match="_cabi.py::SIGS"):
        L.babe_not_a_function


def _check_layout(tmp_path, structs):
    """sizeof and the offsetof of EVERY field of the ctypes mirrors `structs` ({header name: Structure}) against what a C compiler
    gives the header (a silent mismatch would hand the library garbage pointers).  The probe is generated from _fields_."""
    import shutil
    import subprocess
    import pytest
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname = lambda f: "in" if f == "in_" else f
    exprs, got = [], []
    for name, st in structs.items():
        exprs.append(f"sizeof({name})")
        got.append(ctypes.sizeof(st))
        for f, _ in st._fields_:
            exprs.append(f"offsetof({name}, {cname(f)})")
            got.append(getattr(st, f).offset)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){\n%sreturn 0;}\n'
                   % (os.path.join(ROOT, "include", "babe_hip.h"), "".join(f'printf("%zu\\n", {e});\n' for e in exprs)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want, [(e, g, w) for e, g, w in zip(exprs, got, want) if g != w]


_UNET_STRUCTS = ("babe_packed_conv", "babe_unet_block", "babe_unet_plan_desc")


def test_unet_plan_structs_have_the_headers_layout(tmp_path):
    """The ctypes mirrors of babe_packed_conv / babe_unet_block / babe_unet_plan_desc (babe_amd/_cabi.py)."""
    from babe_amd import _cabi
    _check_layout(tmp_path, {n: _cabi.STRUCTS[n] for n in _UNET_STRUCTS})


def test_cqt_bands_struct_has_the_headers_layout(tmp_path):
    """The ctypes mirror of babe_cqt_bands (the band kernels get it BY VALUE), the fields round 6 appended included."""
    from babe_amd import _cabi
    _check_layout(tmp_path, {"babe_cqt_bands": _cabi.STRUCTS["babe_cqt_bands"]})


def test_every_other_struct_mirror_has_the_headers_layout(tmp_path):
    """... and every remaining struct of the header that babe_amd/_cabi.py mirrors (conv / weight-gradient / denoiser-conv
    arguments, the fit configuration, the score-evaluation descriptor)."""
    from babe_amd import _cabi
    rest = {n: st for n, st in _cabi.STRUCTS.items() if n not in _UNET_STRUCTS + ("babe_cqt_bands",)}
    assert len(rest) >= 5
    _check_layout(tmp_path, rest)


def test_kaiser_poly_reproduces_the_window_table():
    """The truncated I0 series the band kernels evaluate (babe_cqt_bands::kpoly) against the float64 Kaiser window the tables
    are built from: below fp32 resolution for the betas it accepts; large betas fall back to the table."""
    import numpy as np
    from babe_amd.cqt import _kaiser, kaiser_poly
    for beta in (0.5, 1.0, 2.0, 3.0):
        deg, co = kaiser_poly(beta)
        assert 1 <= deg <= 11 and (co[deg + 1:] == 0).all()
        for M in (4, 7, 64, 1001, 4096):
            m = np.arange(-(M // 2), M - M // 2)
            a = np.maximum(1 - (2.0 * m / M) ** 2, 0)
            p = sum(co[j] * a ** j for j in range(12))
            assert np.abs(p - _kaiser(M, beta)).max() < 3e-9
    assert kaiser_poly(8.6) is None


def test_unet_plan_create_validates_every_block():
    """babe_unet_plan_create takes descriptors from any C-ABI host: a dilation-layer count outside 0..8 (it indexes saved[..][8],
    H[8], gamma[8]), a channel count that is not a positive multiple of the 8 GroupNorm groups, or a missing gamma / packed image
    in ANY block - init, main, up, out, middle - is refused with a message instead of overrunning.  Host-side
    validation only: no GPU call is made."""
    from babe_amd._lib import lib
    from babe_amd.networks import unet_c as uc
    L = lib()
    FAKE = 0x1000                                         # never dereferenced by plan_create (pointers stay the caller's)

    def good():
        d = uc.CPlanDesc()
        d.nocts, d.bpo = 2, 64
        for i in range(2):
            d.Ns[i] = 16
        def blk(b, nd):
            b.N, b.nd, b.k53 = 16, nd, 1
            for k in range(nd):
                b.H[k].Cout = b.H[k].Cin = 16
                b.H[k].KH, b.H[k].KW = 5, 3
                b.H[k].fwd = FAKE
                b.gamma[k] = FAKE
        for i in range(2):
            for arr in (d.init_blk, d.main_blk, d.up_out, d.up_blk):
                blk(arr[i], 2)
        blk(d.mid_blk, 3)
        blk(d.mid_out, 1)
        return d

    def create(d):
        p = L.babe_unet_plan_create(ctypes.byref(d))
        if p:
            L.babe_unet_plan_destroy(p)
        return bool(p), L.babe_last_error().decode()

    assert create(good())[0]
    for name, mutate in {
        "init_blk nd 9": lambda d: setattr(d.init_blk[1], "nd", 9),
        "up_out nd -1": lambda d: setattr(d.up_out[0], "nd", -1),
        "mid_blk nd 12": lambda d: setattr(d.mid_blk, "nd", 12),
        "mid_out nd 0": lambda d: setattr(d.mid_out, "nd", 0),
        "main_blk N 12": lambda d: setattr(d.main_blk[0], "N", 12),
        "up_blk gamma NULL": lambda d: d.up_blk[1].gamma.__setitem__(1, None),
        "main_blk H without image": lambda d: setattr(d.main_blk[1].H[0], "fwd", None),
        "Ns not a multiple of 8": lambda d: d.Ns.__setitem__(1, 20),
    }.items():
        d = good()
        mutate(d)
        ok, msg = create(d)
        assert not ok and "bad descriptor" in msg, (name, ok, msg)


def test_f45_dispatch_rule_is_host_logic():
    """babe_conv2d_wino85_supported / _preferred are pure host functions (no launch, no device pointer dereferenced): the dispatch
    rule of the F(4,5) x F(4,3) kernels - output channels a multiple of 128 / 96 / 64, Cin % 16 == 0, one source, T % 4 == 0 and
    >= 64, 16-byte aligned views; preferred = supported and row quads x time tiles >= 80 % full - checked without a GPU."""
    import ctypes as C
    from babe_amd._lib import ConvArgs, lib
    L = lib()

    def args(Cin=128, Cout=128, F=64, T=128, dil=4, in2=None, in_=0x10000, B=1):
        a = ConvArgs()
        a.in_, a.in_bs, a.in_cs = in_, Cin * F * T, F * T
        a.in2, a.in2_bs, a.in2_cs, a.cin_split = in2, 0, 0, Cin
        a.out, a.out_bs, a.out_cs = 0x20000, Cout * F * T, F * T
        a.res, a.res_bs, a.res_cs = None, 0, 0
        a.in_scale = a.oscale = None
        a.alpha, a.rbeta = 1.0, 0.0
        a.B, a.Cin, a.Cout, a.F, a.T, a.KH, a.KW, a.dil = B, Cin, Cout, F, T, 5, 3, dil
        return a

    sup = lambda **k: L.babe_conv2d_wino85_supported(C.byref(args(**k)))
    pre = lambda **k: L.babe_conv2d_wino85_preferred(C.byref(args(**k)))
    for co in (64, 96, 128, 192, 256, 320, 384):
        assert sup(Cout=co) == 1, co
    for co in (16, 32, 48, 80, 112, 144):
        assert sup(Cout=co) == 0, co
    assert sup(Cin=16) == 1 and sup(Cin=24) == 0 and sup(Cin=8) == 0
    assert sup(T=64) == 1 and sup(T=60) == 0 and sup(T=66) == 0 and sup(T=68) == 1
    assert sup(in2=0x30000) == 0 and sup(in_=0x10004) == 0
    a = args()
    a.KH = 3
    assert L.babe_conv2d_wino85_supported(C.byref(a)) == 0
    # fill = F / (4 * quads * dil) * T / (64 * tiles): 16 rows per class = 4 full quads; 5 rows -> 2 quads = 0.625; 6 -> 0.75; 7 -> 0.875
    assert pre(F=64, dil=4) == 1 and pre(F=40, dil=8) == 0 and pre(F=48, dil=8) == 0 and pre(F=56, dil=8) == 1
    assert pre(F=64, dil=4, T=68) == 0 and pre(F=64, dil=4, T=120) == 1          # 68 of 128 steps / 120 of 128
    # the benchmark's part-filled geometries: 320 rows at dilation 32 (0.83: taken), 384 rows at dilation 64 (0.75: left to F(2,5) x F(4,3))
    assert pre(F=320, T=256, dil=32) == 1 and pre(F=384, T=128, dil=64, Cin=256, Cout=256) == 0
    assert pre(F=448, T=64, dil=64, Cin=256, Cout=256) == 1 and pre(F=320, T=256, dil=16) == 1


def test_plan_entry_points_refuse_bad_arguments_without_a_gpu():
    """Host-side validation of the round-6 plan entry points (no GPU call is made on these paths): NULL handles, NULL buffers and
    an empty descriptor are refused with a message instead of being dereferenced."""
    from babe_amd._lib import lib
    from babe_amd.testing import eval_c
    L = lib()
    assert L.babe_cqt_workspace_bytes(None, 4) == -1
    for name in ("babe_cqt_fwd", "babe_cqt_bwd", "babe_cqt_fwd_adjoint", "babe_cqt_bwd_adjoint", "babe_cqt_hpf"):
        assert getattr(L, name)(None, None, None, None, 1, None) < 0 and b"bad arguments" in L.babe_last_error()
    d = eval_c.EvalDesc()
    assert L.babe_eval_workspace_bytes(ctypes.byref(d), 1) == -1 and b"bad descriptor" in L.babe_last_error()
    assert L.babe_score_eval(ctypes.byref(d), None, 0.1, 1.0, 1.0, 1.0, 0.0, None, None, None, None, None, None, None, 0, 1, None) < 0
    assert L.babe_filter_loss_grad(None, 0, None, None, 1, 1, 2049, 44100.0, 4096, None, None) < 0
