"""Time attention on the library path, the part that needs no GPU: the new structs' layout and the binding table, what
babe_model_load_opt refuses of an attention file before its first device call, and the host data of the bucket-table kernel
(babe_attn_bucket_thresholds) against babe_attn_buckets."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.attention_weights import LAST_TWO, SMALL_DILS, SMALL_NS, attention_dict, attention_sd
from tests.test_cabi_exports import _check_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, FS = 92092, 22050
NEW_SYMBOLS = ("babe_attn_bucket_thresholds", "babe_attn_bucket_table", "babe_model_load_opt", "babe_model_create_opt",
               "babe_model_attention")


def test_attention_structs_have_the_headers_layout(tmp_path):
    """babe_unet_attn, babe_attn_bucket_thr, babe_model_options and the block / plan structs that grew (attn, attn_core): sizeof
    and every offsetof of the ctypes mirrors against the compiler's."""
    from babe_amd import _cabi
    names = ("babe_unet_attn", "babe_attn_bucket_thr", "babe_model_options", "babe_unet_block", "babe_unet_plan_desc")
    assert [f for f, _ in _cabi.CBlock._fields_][-1] == "attn" and [f for f, _ in _cabi.CPlanDesc._fields_][-1] == "attn_core"
    _check_layout(tmp_path, {n: _cabi.STRUCTS[n] for n in names})


def test_new_entry_points_are_declared_and_exported():
    from babe_amd import _cabi
    from babe_amd._lib import lib
    hdr = open(os.path.join(ROOT, "include", "babe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    Lb = lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _cabi.SIGS and isinstance(getattr(Lb, name), C._CFuncPtr), name
    for const in ("BABE_ATTENTION_REFUSE = 0", "BABE_ATTENTION_F32 = 1", "BABE_ATTENTION_BF16 = 2"):
        assert const in hdr
    assert _cabi.ATTN_CORES == {None: 0, "f32": 1, "bf16": 2}


# ------------------------------------------------------------------------------------------------ loader refusals
def _adict(**kw):
    """One head keeps the qk weights (a [2HF, HF] matrix per block) small: nothing here reaches a device."""
    return dict(dict(attention_dict(), num_heads=1), **kw)


def _args(**network):
    from babe_amd.config import default_args
    args = default_args(sample_rate=FS, audio_len=L, Ns=SMALL_NS, T=3, start_sigma=0.05)
    args.network.update(network)
    return args


@pytest.fixture(scope="module")
def attn_sd():
    return attention_sd(SMALL_NS, SMALL_DILS, LAST_TWO, _adict())


def _load_opt(path, attention=1, precision=0):
    from babe_amd._cabi import ModelOptions
    from babe_amd._lib import lib
    opt = ModelOptions(precision=precision, attention=attention)
    h = lib().babe_model_load_opt(str(path).encode(), C.byref(opt), None)
    return h, lib().babe_last_error().decode()


def _bad_files(attn_sd, tmp):
    """{case: (path, the words the refusal must contain)} of attention files that are wrong, and the path of a sound one."""
    from babe_amd import model_file
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    args = _args(attention_layers=list(LAST_TWO), attention_dict=_adict())
    qk, table = "downs.5.2.attn_block.qk.weight", "middle.0.1.attn_block.rel_pos.relative_attention_bias.weight"
    assert qk in attn_sd and attn_sd[table].shape == (32, 1)
    plain = init_state_dict(SMALL_NS, SMALL_DILS, seed=0, gate_scale=1.0)
    cases = {
        "missing": ({k: v for k, v in attn_sd.items() if k != qk}, args, "missing tensor " + qk),
        "shape": (dict(attn_sd, **{table: torch.zeros(16, 1)}), args, "wrong shape for " + table),
        "flags off": (dict(plain, **{"downs.4.2.norm2.gamma": attn_sd["downs.4.2.norm2.gamma"]}), _args(), "does not belong"),
        "heads": (attn_sd, _args(attention_layers=list(LAST_TWO), attention_dict=_adict(num_heads=0)), "num_heads"),
        "buckets": (attn_sd, _args(attention_layers=list(LAST_TWO), attention_dict=_adict(rel_pos_num_buckets=128)), "rel_pos_num_buckets"),
    }
    out = {}
    for name, (sd, a, words) in cases.items():
        path = os.path.join(str(tmp), name.replace(" ", "_") + ".babe")
        model_file.export(sd, a, path)
        out[name] = (path, words)
    good = os.path.join(str(tmp), "good.babe")
    model_file.export(attn_sd, args, good)
    return out, good


def test_loader_refuses_attention_files_before_any_device_call(attn_sd, tmp_path):
    """babe_model_load_opt with attention = BABE_ATTENTION_F32 on attention files that are wrong: NULL and a message naming the
    fault, from host code that runs before the loader's first device call (this machine has no device to call)."""
    cases, good = _bad_files(attn_sd, tmp_path)
    for name, (path, words) in cases.items():
        h, msg = _load_opt(path)
        assert not h and words in msg and msg.startswith("model"), (name, msg)
    # an unknown attention value: the host's own mistake, asked before the file is opened
    for bad in (-1, 3):
        h, msg = _load_opt(good, attention=bad)
        assert not h and "attention %d" % bad in msg and "BABE_ATTENTION_REFUSE" in msg, msg
    h, msg = _load_opt(tmp_path / "no_such.babe", attention=3)
    assert not h and "BABE_ATTENTION_REFUSE" in msg
    # ... and REFUSE is today's refusal, in today's words
    h, msg = _load_opt(good, attention=0)
    assert not h and "attention layers are not supported by the library-side sequencers" in msg


def test_attention_parser_paths_under_the_sanitizers(attn_sd, tmp_path):
    """tools/model_file_check.cpp --attention 1 (its own main, the HIP-free parser header) built with
    -fsanitize=address,undefined and run as a program of its own over a sound attention file and the wrong ones: exit status 0, no
    sanitizer report, and per file the verdict - the very message - babe_model_load_opt gives.  Nothing sanitized is loaded into
    this process."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = str(tmp_path / "model_file_check")
    subprocess.run([cxx, *flags, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "model_file_check.cpp")], check=True)
    cases, good = _bad_files(attn_sd, tmp_path)
    paths = [good] + [p for p, _ in cases.values()]
    r = subprocess.run([exe, "--attention", "1", *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths) and lines[0].startswith(good + ": ok (")
    for line, (name, (path, words)) in zip(lines[1:], cases.items()):
        assert line.startswith(path + ": refused: "), (name, line)
        verdict = line[len(path + ": refused: "):]
        assert words in verdict and _load_opt(path)[1].endswith(verdict), (name, line)
    r = subprocess.run([exe, good], capture_output=True, text=True, timeout=300)                  # without the choice: today's refusal
    assert r.returncode == 0 and "refused: attention layers are not supported" in r.stdout


# ------------------------------------------------------------------------------------------------ the bucket kernel's host data
def _thresholds(nb, maxd):
    from babe_amd._cabi import AttnBucketThr
    from babe_amd._lib import check, lib
    thr = AttnBucketThr()
    check(lib().babe_attn_bucket_thresholds(C.byref(thr), nb, maxd), "attn_bucket_thresholds")
    return thr


def _table_from(thr, T):
    """What the kernel computes per entry (csrc/attn_buckets.hip), on the host: the count of thresholds <= |d|, plus the half."""
    rel = np.arange(2 * T - 1) - (T - 1)
    t = np.asarray(thr.thr[:thr.half - 1])
    return np.where(rel >= 0, thr.half, 0) + (t[None, :] <= np.abs(rel)[:, None]).sum(1)


def test_bucket_thresholds_reproduce_attn_buckets():
    """The thresholds of (32, 64) give babe_attn_buckets(T, 32, 64) entry for entry for every T <= 4096 (and (8, 16) at a few
    lengths); no launch is made."""
    from babe_amd import ops
    thr = _thresholds(32, 64)
    assert thr.half == 16 and thr.max_distance == 64
    t = list(thr.thr[:15])
    assert t == sorted(t) and t[:7] == [1, 2, 3, 4, 5, 6, 7] and t[-1] <= 64 and all(v == 0 for v in thr.thr[15:])
    for T in range(1, 4097):
        want = ops.attn_buckets(T, 32, 64).numpy()
        got = _table_from(thr, T)
        assert got.shape == want.shape and (got == want).all(), T
    small = _thresholds(8, 16)
    for T in (1, 2, 9, 20, 63, 64, 65, 300):
        assert (_table_from(small, T) == ops.attn_buckets(T, 8, 16).numpy()).all(), T


def test_bucket_thresholds_refuse_what_the_kernel_cannot_take():
    from babe_amd._cabi import AttnBucketThr
    from babe_amd._lib import lib
    Lb, thr = lib(), AttnBucketThr()
    for nb, maxd, words in ((66, 128, b"num_buckets"), (7, 64, b"num_buckets"), (2, 64, b"num_buckets"), (32, 8, b"max_distance"),
                            (32, 1 << 20, b"max_distance")):
        assert Lb.babe_attn_bucket_thresholds(C.byref(thr), nb, maxd) < 0 and words in Lb.babe_last_error(), (nb, maxd)
    assert Lb.babe_attn_bucket_thresholds(None, 32, 64) < 0
    assert Lb.babe_attn_bucket_table(None, 8, None, None) < 0 and b"null" in Lb.babe_last_error()


def test_plan_create_refuses_an_attention_branch_without_a_core():
    """babe_unet_plan_create on a descriptor whose middle block carries a babe_unet_attn: refused with attn_core = 0 and, with a
    core, for a field the kernels cannot take - each message names the field; a sound branch is accepted and copied.  Host
    validation only: the (fake) pointers are never dereferenced."""
    from babe_amd import _cabi
    from babe_amd._lib import lib
    Lb, FAKE = lib(), 0x1000

    def desc(core, **field):
        d = _cabi.CPlanDesc()
        d.nocts, d.bpo, d.attn_core = 2, 64, core
        blocks = [b for arr in (d.init_blk, d.main_blk, d.up_out, d.up_blk) for b in arr[:2]] + [d.mid_blk, d.mid_out]
        for b in blocks:
            b.N, b.nd, b.k53 = 16, 1, 1
            b.H[0].Cout = b.H[0].Cin = 16
            b.H[0].KH, b.H[0].KW, b.H[0].fwd, b.gamma[0] = 5, 3, FAKE, FAKE
        d.Ns[0] = d.Ns[1] = 16
        at = _cabi.CAttn()
        at.H, at.F, at.scale, at.gamma = 8, 128, 128 ** -0.5, FAKE                    # the middle block runs at 2 * 64 rows
        for pc, co, ci in ((at.proj_in, 8, 16), (at.qk, 2 * 8 * 128, 8 * 128), (at.proj_out, 16, 8)):
            pc.Cout, pc.Cin, pc.KH, pc.KW, pc.fwd, pc.bwd = co, ci, 1, 1, FAKE, FAKE
        at.emb, at.num_buckets, at.max_distance = FAKE, 32, 64
        for k, v in field.items():
            setattr(at, k, v)
        d.mid_blk.attn = C.pointer(at)
        return d, at

    def create(core, **field):
        d, keep = desc(core, **field)
        p = Lb.babe_unet_plan_create(C.byref(d))
        if p:
            Lb.babe_unet_plan_destroy(p)
        return bool(p), Lb.babe_last_error().decode()

    assert create(1)[0] and create(2)[0]
    ok, msg = create(0)
    assert not ok and "attn_core" in msg
    for field, value, words in (("F", 100, "babe_unet_attn.F"), ("F", 512, "babe_unet_attn.F"), ("H", 0, "babe_unet_attn.H"),
                                ("gamma", None, "babe_unet_attn.gamma"), ("num_buckets", 128, "num_buckets"),
                                ("max_distance", 4, "max_distance"), ("film_gate", -1, "film_gate")):
        ok, msg = create(1, **{field: value})
        assert not ok and words in msg, (field, value, msg)
    ok, msg = create(3)
    assert not ok and "attn_core" in msg
