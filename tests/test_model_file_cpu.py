"""The model file (babe_amd/model_file.py, csrc/model_file.h) without a GPU: the Python round trip, what babe_model_load refuses
before it touches a device, and the parser under the address and undefined-behaviour sanitizers as a program of its own
(tools/model_file_check.cpp)."""
import os
import shutil
import struct
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, L, FS = [8, 8, 8, 8, 16, 16, 16], 92092, 22050


def _args(**network):
    from babe_amd.config import default_args
    args = default_args(sample_rate=FS, audio_len=L, Ns=NS, T=3, start_sigma=0.05)
    args.network.update(network)
    return args


def _plain_sd():
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    return init_state_dict(NS, _args().network.num_dils, seed=0, gate_scale=1.0)


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """(path, bytes) of a valid model file of the small network (never modified)."""
    from babe_amd import model_file
    path = str(tmp_path_factory.mktemp("model") / "good.babe")
    model_file.export(_plain_sd(), _args(), path)
    return path, open(path, "rb").read()


def _module_of(sd):
    """A CPU module with the network's parameter tree (the network itself needs a GPU): what load_state_dict is tested on."""
    from babe_amd.networks.cqtdiff_plus import _attach, _Node
    root = _Node()
    for k, v in sd.items():
        _attach(root, k, torch.zeros_like(v), is_buffer=k.endswith(".kernel"))
    return root


@pytest.mark.parametrize("fenc", [False, True])
def test_export_read_round_trip(tmp_path, fenc):
    """export -> read: the same settings, bit-equal tensors under the same names in the same order, the two aux tables those of
    STFTOps; a network loaded from the file has the source's state_dict; unflatten gives the configuration back."""
    from babe_amd import model_file
    from babe_amd.stft import STFTOps
    from tests.fencoding_weights import fencoding_sd
    args = _args(use_fencoding=fenc)
    sd = fencoding_sd("a") if fenc else _plain_sd()
    path = str(tmp_path / "m.babe")
    size = model_file.export(sd, args, path)
    assert size == os.path.getsize(path) and size % 64 == 0
    settings, got = model_file.read(path)
    assert settings == model_file.settings_of(args)
    assert settings["exp.audio_len"] == L and settings["network.Ns.4"] == 16 and settings["network.use_fencoding"] == int(fenc)
    assert settings["tester.blind_bwe.fcmax"] == FS // 2 and settings["network.cqt.window"] == "kaiser"
    assert settings["tester.posterior_sampling.start_sigma"] == 0.05 and settings["tester.blind_bwe.initial_conditions.A.4"] == -30
    assert list(got) == list(sd)
    for k, v in sd.items():
        assert got[k].dtype == torch.float32 and got[k].shape == v.shape and torch.equal(got[k], v), k
    net = _module_of(sd)
    net.load_state_dict(got, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    _, with_aux = model_file.read(path, aux=True)
    st = STFTOps(4096, L, FS, "cpu")
    assert torch.equal(with_aux["aux.env_inv"], st.env_inv) and torch.equal(with_aux["aux.tw4096"], st.tw4096)
    back = model_file.unflatten(settings)
    assert back.network.Ns == NS and back.network.num_dils == list(args.network.num_dils) and back.network.attention_dict is None
    assert back.tester.blind_bwe.initial_conditions.fc == [280, 285, 290, 295, 300] and back.exp.sample_rate == FS
    assert model_file.settings_of(back) == settings


def test_export_command_line(tmp_path):
    """python -m babe_amd.export without --ckpt: the random weights of a fresh network, the overrides applied."""
    from babe_amd import export, model_file
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    path = str(tmp_path / "cli.babe")
    export.main(["--out", path, "--sample-rate", str(FS), "--audio-len", str(L), "--T", "3", f"network.Ns={NS}",
                 "tester.posterior_sampling.xi=0.3"])
    settings, sd = model_file.read(path)
    assert settings["tester.T"] == 3 and settings["tester.posterior_sampling.xi"] == 0.3 and settings["network.Ns.6"] == 16
    want = init_state_dict(NS, _args().network.num_dils)
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)


# ------------------------------------------------------------------------------------------------ damaged files
def _sections(buf):
    return struct.unpack_from("<QQQ", buf, 32)                    # settings, index, data offsets


def _index(buf):
    """[(name, position of its index record)]"""
    nten = struct.unpack_from("<I", buf, 28)[0]
    pos, out = _sections(buf)[1], []
    for _ in range(nten):
        nlen = struct.unpack_from("<H", buf, pos)[0]
        out.append((buf[pos + 56:pos + 56 + nlen].decode(), pos))
        pos += 56 + nlen
    return out


def _patched(buf, pos, fmt, *values):
    b = bytearray(buf)
    struct.pack_into(fmt, b, pos, *values)
    return bytes(b)


def _damaged(good_bytes, tmp):
    """{case: (path, the words the refusal must contain)} - every file is written under tmp."""
    from babe_amd import model_file
    from tests.attention_weights import LAST_TWO, attention_dict
    s_off, i_off, d_off = _sections(good_bytes)
    rec = dict(_index(good_bytes))
    first = rec["embedding.RFF_freq"]
    cases = {
        "empty": (b"", "empty file"),
        "magic": (b"BABEMODX" + good_bytes[8:], "wrong magic"),
        "version": (_patched(good_bytes, 8, "<I", 2), "unknown version 2"),
        "cut in the header": (good_bytes[:32], "truncated"),
        "cut at the settings": (good_bytes[:s_off], "truncated"),
        "cut at the index": (good_bytes[:i_off], "truncated"),
        "cut at the data": (good_bytes[:d_off], "truncated"),
        "cut in a tensor": (good_bytes[:d_off + 1000], "truncated"),
        "cut before the end": (good_bytes[:-1], "truncated"),
        "dimension overflow": (_patched(good_bytes, first + 8, "<QQ", 1 << 40, 1 << 40), "overflows"),
        "data leaves the file": (_patched(good_bytes, first + 40, "<Q", len(good_bytes) - 64), "leaves the file"),
        "overlap": (_patched(good_bytes, rec["embedding.MLP.0.bias"] + 40, "<Q", struct.unpack_from("<Q", good_bytes, first + 40)[0]),
                    "overlapping"),
    }
    a, b = rec["embedding.MLP.0.bias"], rec["embedding.MLP.1.bias"]
    dup = bytearray(good_bytes)
    dup[b + 56:b + 56 + 20] = good_bytes[a + 56:a + 56 + 20]
    cases["duplicate name"] = (bytes(dup), "duplicate tensor name embedding.MLP.0.bias")
    out = {}
    for name, (data, words) in cases.items():
        p = os.path.join(tmp, name.replace(" ", "_") + ".babe")
        open(p, "wb").write(data)
        out[name] = (p, words)

    def exported(name, sd, args, words):
        p = os.path.join(tmp, name.replace(" ", "_") + ".babe")
        model_file.export(sd, args, p)
        out[name] = (p, words)

    sd = _plain_sd()
    exported("missing name", {k: v for k, v in sd.items() if k != "downs.0.0.proj_in.weight"}, _args(),
             "missing tensor downs.0.0.proj_in.weight")
    w = sd["downs.0.2.H.0.weight"]
    exported("wrong shape", dict(sd, **{"downs.0.2.H.0.weight": w.reshape(w.shape[0], w.shape[1], 3, 5)}), _args(),
             "wrong shape for downs.0.2.H.0.weight")
    exported("unexpected name", dict(sd, **{"downs.9.1.weight": torch.zeros(3)}), _args(), "does not belong")
    exported("attention", sd, _args(attention_layers=list(LAST_TWO), attention_dict=attention_dict()), "attention")
    exported("bf16", sd, _args(precision="bf16"), "fp32 network only")
    exported("uncovered length", sd, _args_len(92093), "cqt design")
    return out


def _args_len(n):
    a = _args()
    a.exp.audio_len = n                                           # 92093 = 19 * 37 * 131: not a product of the FFT's radices
    return a


def _load(path):
    from babe_amd._lib import lib
    h = lib().babe_model_load(path.encode(), None)
    return h, lib().babe_last_error().decode()


def test_loader_refuses_damaged_files_without_a_gpu(good, tmp_path):
    """babe_model_load on a missing path and on every damaged file: NULL and a message that names the fault.  All of it is host
    code that runs before the loader's first device call (the pattern of test_plan_entry_points_refuse_bad_arguments_without_a_gpu)."""
    h, msg = _load(str(tmp_path / "no_such_file.babe"))
    assert not h and "cannot open" in msg and "no_such_file" in msg
    for name, (path, words) in _damaged(good[1], str(tmp_path)).items():
        h, msg = _load(path)
        assert not h, name
        assert words in msg and msg.startswith("model"), (name, msg)


def test_model_create_refuses_bad_tables_without_a_gpu():
    """babe_model_create validates its tables like the file parser: NULL tables, a rank outside 1..4, a duplicate name, and a
    table that is no network."""
    import ctypes as C
    from babe_amd._cabi import ModelEntry, ModelKV
    from babe_amd._lib import lib
    Lb = lib()
    assert not Lb.babe_model_create(None, 0, None, 0, None) and b"empty tables" in Lb.babe_last_error()
    data = (C.c_float * 8)()
    kv = (ModelKV * 1)(ModelKV(b"exp.sample_rate", None, 22050.0))

    def entries(*items):
        arr = (ModelEntry * len(items))()
        for e, (name, ndim, shape) in zip(arr, items):
            e.name, e.ndim, e.data = name, ndim, C.cast(data, C.c_void_p)
            e.shape[:] = shape
        return arr

    for arr, words in ((entries((b"a", 5, (1, 1, 1, 1))), b"rank 5"), (entries((b"a", 1, (8, 1, 1, 1)), (b"a", 1, (8, 1, 1, 1))), b"duplicate"),
                       (entries((b"a", 2, (1 << 40, 1 << 40, 1, 1))), b"overflows"), (entries((b"a", 1, (8, 1, 1, 1))), b"missing setting")):
        assert not Lb.babe_model_create(arr, len(arr), kv, 1, None)
        assert words in Lb.babe_last_error(), Lb.babe_last_error()


def test_parser_under_the_sanitizers(good, tmp_path):
    """tools/model_file_check.cpp (its own main, the HIP-free parser header) built with -fsanitize=address,undefined and run as a
    program of its own over the good and the damaged files: exit status 0, no sanitizer report, and per file the verdict - the
    very message - babe_model_load gives."""
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
    cases = _damaged(good[1], str(tmp_path))
    paths = [good[0]] + [p for p, _ in cases.values()]
    r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths)
    assert lines[0].startswith(good[0] + ": ok (")
    for line, (name, (path, words)) in zip(lines[1:], cases.items()):
        if name == "uncovered length":            # the CQT design is the library's (not in the header): the file itself is sound
            assert line.startswith(path + ": ok ("), line
            continue
        assert line.startswith(path + ": refused: "), (name, line)
        verdict = line[len(path + ": refused: "):]
        assert words in verdict and _load(path)[1].endswith(verdict), (name, line)


def test_integration_listing_is_the_programs_core():
    """INTEGRATION.md section 2 lists the core of examples/c_host/babe_restore.c (between its [core] marks) as it stands in the file."""
    import textwrap
    src = open(os.path.join(ROOT, "examples", "c_host", "babe_restore.c")).read()
    core = src.split("/* [core] the listing of INTEGRATION.md section 2 */\n")[1].split("    /* [/core] */")[0]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "```c\n" + textwrap.dedent(core).rstrip() + "\n```" in doc
