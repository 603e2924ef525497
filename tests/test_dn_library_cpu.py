"""The host-only parts of the library's file-level flow (csrc/dn_host.h, csrc/dn_engine.hip) without a GPU: the sinc table against
babe_amd/resample.py, the two walks against the Python flows they restate, the split-K rule against networks/denoiser.py, the
denoiser weights file (round trip, every refusal by its message), and all of it as a program of its own under the address and
undefined-behaviour sanitizers (tools/dn_host_check.cpp)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(2, 1), (1, 2), (441, 320), (320, 441), (147, 160)]
CFG = dict(depth=2, num_tfc=1, num_stages=2, use_SAM=True, use_fencoding=True, f_dim=65)
DARGS = dict(CFG, sample_rate_denoiser=4000, segment_size=2, stft_win_size=128, stft_hop_size=32)


def _lib():
    from babe_amd._lib import lib
    return lib()


def _table(orig, new):
    L = _lib()
    w, o, n = C.c_int(), C.c_int(), C.c_int()
    size = L.babe_resample_sinc_table_size(orig, new, C.byref(w), C.byref(o), C.byref(n))
    assert size == n.value * (2 * w.value + o.value)
    k, kr = np.full(size, np.nan, np.float32), np.full(2 * n.value, -1, np.int32)
    assert L.babe_resample_sinc_table(orig, new, k.ctypes.data, kr.ctypes.data) == 0
    return k.reshape(n.value, -1), kr.reshape(-1, 2), w.value, o.value, n.value


# ------------------------------------------------------------------------------------------------------------ the sinc table
@pytest.mark.parametrize("orig,new", RATIOS)
def test_sinc_table_against_resample_py(orig, new):
    """babe_resample_sinc_table against resample.py::sinc_resample_kernel / _table: width, orig, new_ and krange (the support mask
    |t| < 6, all basic IEEE float32 arithmetic) exactly; taps within 1e-6 of the largest tap - four times the 2.5e-7 measured
    between two independent float32 sine / cosine implementations on the same operation sequence.  A table evaluated in double and
    rounded once misses this bar by a factor of 20 (2.1e-5 for 441:320), which is what the bar is for: the second assertion
    builds that table and shows it fail for the two ratios with a long table.
    Observed here (x86-64, glibc sinf / cosf against torch's): 0 for 2:1 and 1:2, 1.7e-7 for 441:320, 1.2e-7 for 320:441 and
    147:160.  Rates with a common factor give the table of the reduced pair."""
    from babe_amd import resample as R
    for mult in (1, 100):
        k, kr, w, o, n = _table(orig * mult, new * mult)
        kp, krp, wp, op_, np_ = R._table(orig * mult, new * mult, 6, 0.99, "cpu")
        assert (w, o, n) == (wp, op_, np_) == (wp, orig, new)
        assert kr.dtype == np.int32 and np.array_equal(kr, krp.numpy())
        kp = kp.numpy()
        err = np.abs(k - kp).max() / np.abs(kp).max()
        print(f"{orig}:{new} x{mult}: max |k_lib - k_py| / max|k| = {err:.3g}")
        assert err <= 1e-6
    if orig > 100:
        # the same formulas in float64, rounded once: not the published table
        base = min(orig, new) * 0.99
        idx = np.arange(-w, w + orig, dtype=np.float64)[None] / orig
        t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
        t = np.clip(t, -6, 6)
        win = np.cos(t * np.pi / 6 / 2) ** 2
        t = t * np.pi
        k64 = (np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * win * (base / orig)).astype(np.float32)
        assert np.abs(k64 - kp).max() / np.abs(kp).max() > 1e-6


@pytest.mark.parametrize("orig,new", RATIOS + [(44100, 16000), (16000, 22050)])
def test_resampled_length_against_resample_py(orig, new):
    """babe_resampled_length = resample.py::resampled_length around multiples of orig, for short files, and where the float32
    rounding of the quotient matters (past 2^24 samples)."""
    from babe_amd.resample import resampled_length
    import math
    o = orig // math.gcd(orig, new)
    lengths = list(range(1, 40)) + [m * o + d for m in (1, 2, 7, 1000, 33333) for d in (-2, -1, 0, 1, 2)] + \
        [479999, 480000, 480001, (1 << 24) + 1, (1 << 24) + 3, 123456789]
    L = _lib()
    for n in (v for v in lengths if v >= 0):
        assert L.babe_resampled_length(n, orig, new) == resampled_length(n, orig, new), n
    assert L.babe_resampled_length(10, 0, 1) == -1 and b"resampled_length" in L.babe_last_error()
    assert L.babe_resample_sinc_table_size(0, 1, None, None, None) == -1
    assert L.babe_resample_sinc_table(2, 1, None, None) < 0


# ------------------------------------------------------------------------------------------------------------------ the walks
def _python_walk(n, segment, overlap=1024):
    """The pointer walk of testing/denoise.py::DenoiserPrepass.apply_denoiser: starts, or None where it raises."""
    starts, pointer = [], 0
    while True:
        if pointer + segment < n:
            starts.append(pointer)
            pointer += segment - overlap
        else:
            nl = n - pointer
            if pointer != 0 and nl > segment - overlap:
                return None
            return starts + [pointer]


def _lib_walk(n, segment, overlap=1024):
    L = _lib()
    count = L.babe_denoise_signal_plan(n, segment, overlap, None, 0)
    if count < 0:
        return None
    starts = (C.c_long * count)()
    assert L.babe_denoise_signal_plan(n, segment, overlap, starts, count) == count
    return list(starts)


def test_denoise_signal_plan_is_the_walk_of_apply_denoiser():
    """n < segment and n = segment (one padded segment), n = segment + 1 (a full segment and a remainder of 1025 samples), a last
    remainder of exactly segment - 1024, one sample more (-1, where apply_denoiser raises), and a sweep over lengths."""
    seg = 8000
    hop = seg - 1024
    assert _lib_walk(5000, seg) == [0] and _lib_walk(seg, seg) == [0]
    assert _lib_walk(seg + 1, seg) == [0, hop]
    assert _lib_walk(hop + hop, seg) == [0, hop]                       # the largest legal remainder after one full segment
    assert _python_walk(hop + hop + 1, seg) is None and _lib_walk(hop + hop + 1, seg) is None
    assert b"denoise_signal_plan" in _lib().babe_last_error()
    assert _python_walk(seg + hop, seg) is None and _lib_walk(seg + hop, seg) is None      # a remainder of a whole segment
    assert _lib_walk(2 * hop + hop, seg) == [0, hop, 2 * hop]
    assert _lib_walk(2 * hop + hop + 1, seg) is None
    assert _lib_walk(20000, seg) == [0, hop, 2 * hop]
    for n in list(range(1, 60000, 997)) + [seg - 1, seg + hop + 1, 3 * hop + 1, 3 * hop]:
        assert _lib_walk(n, seg) == _python_walk(n, seg), n
    for seg2 in (2048, 2049, 110250):
        for n in (1, seg2, seg2 + 1, 2 * seg2 - 2048, 2 * seg2 - 2047, 5 * seg2):
            assert _lib_walk(n, seg2) == _python_walk(n, seg2), (n, seg2)
    starts = (C.c_long * 2)(-7, -7)                                     # max entries are filled, the count is the walk's
    assert _lib().babe_denoise_signal_plan(20000, seg, 1024, starts, 1) == 3 and list(starts) == [0, -7]
    assert _lib().babe_denoise_signal_plan(0, seg, 1024, None, 0) == -1 and _lib().babe_denoise_signal_plan(100, 2047, 1024, None, 0) == -1


@pytest.mark.parametrize("fs,dn,model", [(22050, None, 22050), (44100, None, 22050), (16000, 16000, 22050), (44100, 16000, 22050),
                                         (22050, 16000, 22050), (44100, 22050, 22050), (22050, 22050, 22050)])
def test_restore_file_plan_against_rate_plan(fs, dn, model):
    """babe_restore_file_plan against long_file.rate_plan and resample.resampled_length: equal rates, no denoiser, a file at the
    denoiser's rate (the reference's quirk: it reaches the model unconverted), all three rates distinct, a file at the model's
    rate, a denoiser at the model's rate."""
    from babe_amd.resample import resampled_length
    from babe_amd.testing.long_file import rate_plan
    for n in (2, 479999, 480000, 1234567):
        cur, mid, mask = n, None, 0
        for step in rate_plan(fs, model, dn):
            if step == "denoise":
                mid = cur
            elif step[0] != step[1]:                                    # (resample returns its input at equal rates)
                cur = resampled_length(cur, step[0], step[1])
                mask |= 1 if mid is None else 2
        want = [n, cur if mid is None else mid, cur]
        lengths = (C.c_long * 3)()
        got = _lib().babe_restore_file_plan(n, fs, dn or 0, model, lengths)
        assert (got, list(lengths)) == (mask, want), (n, got, list(lengths), mask, want)
    assert _lib().babe_restore_file_plan(0, fs, 0, model, None) == -1 and b"restore_file_plan" in _lib().babe_last_error()


# ------------------------------------------------------------------------------------------------------------------- split-K
def _launches(cfg, B, T, F):
    """(name, Cin, Cout, OH, OW, KH, KW) of every babe_dn_conv2d launch of DenoiserEngine.forward, from param_shapes: a conv
    works on the plane of its level, the strided conv writes the next level's, a transposed conv is four 2x2 launches over
    (h + 1) x (w + 1) of the level below."""
    from babe_amd.networks.denoiser import param_shapes
    import re
    sizes = [(T, F)]
    for _ in range(cfg["depth"]):
        sizes.append((sizes[-1][0] // 2 + 1, sizes[-1][1] // 2 + 1))
    out = []
    for name, shp in param_shapes(cfg).items():
        if not name.endswith(".weight"):
            continue
        m = re.search(r"\.(e|d)blocks\.(\d+)\.", name)
        lvl = int(m.group(2)) if m else (cfg["depth"] if ".i_block." in name and "blocks" not in name else 0)
        if ".tconv_1." in name:
            h, w = sizes[lvl + 1]
            out.append((name, shp[0], shp[1], h + 1, w + 1, 2, 2))
        elif ".conv2d_2." in name or ".projection." in name:
            out.append((name, shp[1], shp[0], *sizes[lvl + 1], shp[2], shp[3]))
        else:
            out.append((name, shp[1], shp[0], *sizes[lvl], shp[2], shp[3]))
    return out


def test_dn_ksplit_is_split_k_of_the_python_engine(monkeypatch):
    """babe_dn_ksplit against networks/denoiser.py::_split_k over every launch shape of the shipped network (depth 6, three TFC
    layers, two stages: 293 tensors) at T in {21, 48, 128, 431} and B in {1, 2}: the same number of splits, 1 where Python leaves
    ksplit at 0.  Both outcomes occur.  (_split_k also hands out its partial-sum buffer: here a host tensor stands in for it.)"""
    from babe_amd._cabi import DnConvArgs
    from babe_amd.networks import denoiser as D
    monkeypatch.setattr(D, "ptr", lambda t: t.data_ptr())
    monkeypatch.setattr(D, "_ws", {})
    cfg = dict(depth=6, num_tfc=3, num_stages=2, use_SAM=True, use_fencoding=True, f_dim=513)
    assert len(D.param_shapes(cfg)) == 293
    seen = set()
    for T in (21, 48, 128, 431):
        for B in (1, 2):
            shapes = _launches(cfg, B, T, 513)
            assert len(shapes) == 146
            for name, ci, co, oh, ow, kh, kw in shapes:
                a = DnConvArgs()
                a.B, a.Cin, a.Cout, a.OH, a.OW, a.KH, a.KW = B, ci, co, oh, ow, kh, kw
                got = _lib().babe_dn_ksplit(C.byref(a))
                D._split_k(a, "cpu")
                assert got == max(a.ksplit, 1), (name, T, B, got, a.ksplit)
                seen.add(got > 1)
    assert seen == {False, True}
    assert _lib().babe_dn_ksplit(None) < 0


# ---------------------------------------------------------------------------------------------------------- the weights file
def _sd(cfg=CFG, seed=3):
    from babe_amd.networks.denoiser import init_state_dict
    return init_state_dict(cfg, seed=seed)


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    from babe_amd import model_file
    path = str(tmp_path_factory.mktemp("dn") / "good.babe")
    model_file.export_denoiser(_sd(), DARGS, path)
    return path, open(path, "rb").read()


def test_export_denoiser_round_trip(good, tmp_path):
    """export_denoiser -> model_file.read: kind = "denoiser", the ten tester.denoiser leaves, the state_dict bit for bit under its
    names in its order, aux.tw4096 and aux.fade as DenoiserPrepass builds them; the command-line entry writes the same file for
    the same configuration."""
    from babe_amd import export_denoiser, model_file
    path, data = good
    assert len(data) % 64 == 0
    settings, got = model_file.read(path)
    assert settings["kind"] == "denoiser" and len(settings) == 11
    for k, v in DARGS.items():
        assert settings["tester.denoiser." + k] == int(v), k
    sd = _sd()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) and got[k].dtype == torch.float32 for k in sd)
    _, aux = model_file.read(path, aux=True)
    q = np.arange(2048)
    tw = torch.tensor(np.stack([np.cos(2 * np.pi * q / 4096), -np.sin(2 * np.pi * q / 4096)], -1), dtype=torch.float32)
    assert torch.equal(aux["aux.tw4096"], tw) and torch.equal(aux["aux.fade"], torch.hamming_window(window_length=2048))
    cli = str(tmp_path / "cli.babe")
    export_denoiser.main(["--out", cli] + [f"{k}={v}" for k, v in DARGS.items()])
    _, sd_cli = model_file.read(cli)
    want = _sd(seed=0)
    assert list(sd_cli) == list(want) and all(torch.equal(sd_cli[k], want[k]) for k in want)
    with pytest.raises(ValueError, match="lacks"):
        model_file.export_denoiser(sd, {k: v for k, v in DARGS.items() if k != "segment_size"}, str(tmp_path / "x.babe"))


def _index(buf):
    nten = struct.unpack_from("<I", buf, 28)[0]
    pos, out = struct.unpack_from("<QQQ", buf, 32)[1], {}
    for _ in range(nten):
        nlen = struct.unpack_from("<H", buf, pos)[0]
        out[buf[pos + 56:pos + 56 + nlen].decode()] = pos
        pos += 56 + nlen
    return out


def _refused(good_bytes, tmp):
    """{case: (path, the words the refusal must contain)}"""
    from babe_amd import model_file
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    out = {}

    def put(name, data, words):
        p = os.path.join(tmp, name.replace(" ", "_") + ".babe")
        open(p, "wb").write(data)
        out[name] = (p, words)

    def exported(name, sd, dargs, words):
        p = os.path.join(tmp, name.replace(" ", "_") + ".babe")
        model_file.export_denoiser(sd, dargs, p)
        out[name] = (p, words)

    ns = [8, 8, 8, 8, 16, 16, 16]
    args = default_args(sample_rate=22050, audio_len=92092, Ns=ns, T=3, start_sigma=0.05)
    p = os.path.join(tmp, "unet.babe")
    model_file.export(init_state_dict(ns, args.network.num_dils, seed=0, gate_scale=1.0), args, p)
    out["a UNet file"] = (p, "not a denoiser file")
    put("empty", b"", "empty file")
    put("cut in a tensor", good_bytes[:-4096], "truncated")
    rec = _index(good_bytes)
    a, b = rec["sam_1.conv1.bias"], rec["sam_1.conv2.bias"]
    dup = bytearray(good_bytes)
    dup[b + 56:b + 56 + 16] = good_bytes[a + 56:a + 56 + 16]
    put("duplicate name", bytes(dup), "duplicate tensor name sam_1.conv1.bias")
    sd = _sd()
    exported("missing name", {k: v for k, v in sd.items() if k != "decoder_s2.dblocks.1.projection.bias"}, DARGS,
             "missing tensor decoder_s2.dblocks.1.projection.bias")
    exported("missing encoding", {k: v for k, v in sd.items() if k != "freq_encoding.fembeddings"}, DARGS, "missing tensor freq_encoding.fembeddings")
    w = sd["decoder_s1.dblocks.0.tconv_1.0.weight"]
    exported("wrong shape", dict(sd, **{"decoder_s1.dblocks.0.tconv_1.0.weight": w.reshape(w.shape[0], w.shape[1], 2, 8)}), DARGS,
             "wrong shape for decoder_s1.dblocks.0.tconv_1.0.weight")
    exported("unexpected name", dict(sd, **{"encoder_s3.i_block.conv2d_res.bias": torch.zeros(3)}), DARGS, "does not belong")
    for flag in ("use_csff", "use_cam", "use_fam", "use_tdf", "use_alttdfs"):
        exported(flag, sd, dict(DARGS, **{flag: True}), f"option {flag} is set")
    exported("depth 0", sd, dict(DARGS, depth=0), "a depth in 1..6")
    exported("depth 7", sd, dict(DARGS, depth=7), "a depth in 1..6")
    exported("three stages", sd, dict(DARGS, num_stages=3), "1 or 2 stages")
    exported("no stage", sd, dict(DARGS, num_stages=0), "1 or 2 stages")
    exported("f_dim", sd, dict(DARGS, stft_win_size=256), "use_fencoding needs stft_win_size / 2 + 1 = 129")
    exported("one-stage file of a two-stage net", sd, dict(DARGS, num_stages=1), "does not belong")
    return out


def _load(path):
    h = _lib().babe_denoiser_load(path.encode(), None)
    return h, _lib().babe_last_error().decode()


def test_denoiser_load_refuses_without_a_gpu(good, tmp_path):
    """babe_denoiser_load on a missing path and on every file it must refuse: NULL and a message that names the fault - host code
    that runs before the loader's first device call.  babe_model_load keeps refusing a denoiser file, and f_dim is free without
    frequency encodings (checked through the stand-alone program below, which needs no device either)."""
    h, msg = _load(str(tmp_path / "no_such_file.babe"))
    assert not h and "cannot open" in msg and "no_such_file" in msg
    for name, (path, words) in _refused(good[1], str(tmp_path)).items():
        h, msg = _load(path)
        assert not h, name
        assert words in msg and msg.startswith("denoiser"), (name, msg)
    h = _lib().babe_model_load(good[0].encode(), None)
    assert not h and _lib().babe_last_error().decode().startswith("model")
    assert not _lib().babe_denoiser_create(None, 0, None, 0, None) and b"empty tables" in _lib().babe_last_error()
    assert _lib().babe_denoiser_workspace_bytes(None, 1, 21, 65) == -1 and _lib().babe_denoise_signal_workspace_bytes(None, 1, 100) == -1
    assert _lib().babe_denoiser_info(None, None) < 0 and _lib().babe_restore_file_workspace_bytes(None) == -1


# ------------------------------------------------------------------------------------------ the same, as a sanitized program
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("dn_check")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *flags, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = str(tmp / "dn_host_check")
    subprocess.run([cxx, *flags, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "dn_host_check.cpp")], check=True)

    def run(*argv):
        r = subprocess.run([exe, *map(str, argv)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r.stdout.splitlines()
    return run


def test_host_code_under_the_sanitizers(checker, good, tmp_path):
    """tools/dn_host_check.cpp (its own main over csrc/dn_host.h and csrc/model_file.h) built with -fsanitize=address,undefined and
    run as a child process: exit status 0, no report, and the library's own answers - the table bit for bit (one source, the same
    float32 operation sequence under another compiler), the lengths, both walks, and per file the very message
    babe_denoiser_load gives."""
    for orig, new in RATIOS:
        lines = checker("table", orig * 100, new * 100)
        k, kr, w, o, n = _table(orig * 100, new * 100)
        assert lines[0].split() == [str(w), str(o), str(n)] and len(lines) == 1 + n
        for j, ln in enumerate(lines[1:]):
            f = ln.split()
            assert [int(f[0]), int(f[1])] == list(kr[j])
            assert np.array([float.fromhex(v) for v in f[2:]], np.float32).tobytes() == k[j].tobytes(), (orig, new, j)
        for L in (1, 479999, (1 << 24) + 3):
            assert int(checker("length", L, orig, new)[0]) == _lib().babe_resampled_length(L, orig, new)
    for n in (5000, 8000, 8001, 13952, 13953, 20000, 1):
        got = [int(v) for v in checker("walk", n, 8000, 1024)[0].split()]
        want = _lib_walk(n, 8000)
        assert got == ([-1] if want is None else [len(want)] + want), n
    for fs, dn, model in ((22050, 0, 22050), (44100, 0, 22050), (16000, 16000, 22050), (44100, 16000, 22050)):
        lengths = (C.c_long * 3)()
        mask = _lib().babe_restore_file_plan(480000, fs, dn, model, lengths)
        assert [int(v) for v in checker("rates", 480000, fs, dn, model)[0].split()] == [mask] + list(lengths)
    from babe_amd import model_file
    free = str(tmp_path / "f_dim_free.babe")                 # without frequency encodings f_dim is not tied to the window
    nofe = dict(CFG, use_fencoding=False)
    model_file.export_denoiser(_sd(nofe), dict(DARGS, **nofe, stft_win_size=256), free)
    cases = _refused(good[1], str(tmp_path))
    lines = checker("files", good[0], free, *[p for p, _ in cases.values()])
    assert lines[0].startswith(good[0] + ": ok (") and "segment 8000" in lines[0] and lines[1].startswith(free + ": ok (")
    for line, (name, (path, words)) in zip(lines[2:], cases.items()):
        assert line.startswith(path + ": refused: "), (name, line)
        verdict = line[len(path + ": refused: "):]
        assert words in verdict and _load(path)[1].endswith(verdict), (name, line)
