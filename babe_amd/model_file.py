"""The model file: one flat, versioned, little-endian, self-describing file from which the library builds a ready-to-run network
(csrc/model.hip: babe_model_load) - what a host without Python needs instead of UnetEngine, PackedConv, STFTOps and CEval.

    header, 64 bytes   magic "BABEMODL" | u32 version (1) | u32 header bytes (64) | u64 file bytes | u32 settings | u32 tensors |
                       u64 settings offset | u64 index offset | u64 data offset | u64 0
    settings           records  u16 key length | u8 kind (0 number, 1 string) | u8 0 | u32 value bytes | key | value
                       (a number is one float64, a string its ASCII characters)
    tensor index       records  u16 name length | u16 ndim (1..4) | u32 0 | u64 dims[4] (unused: 1) | u64 data offset |
                       u64 data bytes | name
    data               float32, each tensor on a 64-byte boundary

Settings are the configuration's leaves under dotted keys (`network.Ns.0`, `tester.posterior_sampling.xi`): a list becomes one key
per element, True / False are 1 / 0, None is the string "None".  Exported are `exp.sample_rate`, `exp.audio_len`, all of `network`
and all of `tester` (config.default_args), with two values resolved the way the samplers resolve them: `tester.blind_bwe.fcmax`
"nyquist" is sample_rate // 2, and `tester.diff_params` holds the training values when `same_as_training` is set.
Tensors carry the reference's state_dict keys, plus `aux.env_inv` and `aux.tw4096`: the two tables of stft.STFTOps, whose bits
this host defines (torch's float32 Hamming window, numpy's cos / sin), so that a descriptor built by the library is bit-identical
to one built here.  csrc/model_file.h is the reader the library uses; `read` below is the Python one.
The denoiser pre-pass has a file of its own in the same container (`export_denoiser`, babe_denoiser_load): the string setting
`kind` = "denoiser" tells the two apart, and each loader refuses the other's file."""
import struct

import numpy as np
import torch

from .config import to_attr

MAGIC, VERSION, HEADER, ALIGN = b"BABEMODL", 1, 64, 64
SECTIONS = ("network", "tester")


def flatten(node, prefix="", out=None):
    """{dotted key: number or string} of a nested mapping / list."""
    out = {} if out is None else out
    if isinstance(node, dict):
        for k, v in node.items():
            flatten(v, f"{prefix}{k}.", out)
    elif isinstance(node, (list, tuple)):
        for i, v in enumerate(node):
            flatten(v, f"{prefix}{i}.", out)
    elif node is None:
        out[prefix[:-1]] = "None"
    elif isinstance(node, str):
        out[prefix[:-1]] = node
    elif isinstance(node, (bool, int, float, np.integer, np.floating)):
        out[prefix[:-1]] = float(node) if not float(node).is_integer() else int(node)
    else:
        raise TypeError(f"setting {prefix[:-1]}: {type(node).__name__} is neither a number, a string, a list nor a mapping")
    return out


def unflatten(settings):
    """The nested configuration (config.AttrDict) of a flat settings mapping: keys 0..n-1 under one node make a list, "None"
    stays the string the configurations use, except for network.attention_dict, which is None."""
    root = {}
    for key, v in settings.items():
        node = root
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = v

    def lists(n):
        if not isinstance(n, dict):
            return n
        n = {k: lists(v) for k, v in n.items()}
        if n and all(k.isdigit() for k in n) and sorted(int(k) for k in n) == list(range(len(n))):
            return [n[str(i)] for i in range(len(n))]
        return n

    args = to_attr(lists(root))
    if args.get("network", {}).get("attention_dict", None) == "None":
        args.network.attention_dict = None
    return args


def settings_of(args):
    """The flat settings of a configuration (module docstring)."""
    out = {"exp.sample_rate": args.exp.sample_rate, "exp.audio_len": int(args.exp.audio_len)}
    for sec in SECTIONS:
        flatten(args[sec], sec + ".", out)
    if args.tester.blind_bwe.fcmax == "nyquist":
        out["tester.blind_bwe.fcmax"] = int(args.exp.sample_rate) // 2
    if args.tester.diff_params.get("same_as_training", False):
        for k in ("sigma_data", "sigma_min", "sigma_max", "ro", "Schurn", "Snoise", "Stmin", "Stmax"):
            out["tester.diff_params." + k] = flatten(args.diff_params[k], "v.")["v"]
    return out


def aux_tensors(args):
    """{'aux.env_inv', 'aux.tw4096'}: the tables of the STFT-domain degradation model for (NFFT, audio_len), as stft.STFTOps
    builds them."""
    from .stft import STFTOps
    st = STFTOps(args.tester.blind_bwe.NFFT, args.exp.audio_len, args.exp.sample_rate, "cpu")
    return {"aux.env_inv": st.env_inv, "aux.tw4096": st.tw4096}


def write(path, settings, tensors):
    """settings {key: number | str}, tensors {name: float32 tensor, 1..4 dimensions} -> the file."""
    srec = b""
    for key, v in settings.items():
        k = key.encode("ascii")
        val = (1, v.encode("ascii")) if isinstance(v, str) else (0, struct.pack("<d", float(v)))
        srec += struct.pack("<HBBI", len(k), val[0], 0, len(val[1])) + k + val[1]
    arrays = {}
    for name, t in tensors.items():
        a = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
        if a.dtype != np.float32 or not 1 <= a.ndim <= 4:
            raise ValueError(f"{name}: the file holds float32 tensors of 1..4 dimensions (got {a.dtype}, {a.ndim})")
        arrays[name] = a
    index_bytes = sum(56 + len(n.encode("ascii")) for n in arrays)
    s_off, i_off = HEADER, HEADER + len(srec)
    d_off = -(-(i_off + index_bytes) // ALIGN) * ALIGN
    irec, off = b"", d_off
    for name, a in arrays.items():
        n = name.encode("ascii")
        dims = list(a.shape) + [1] * (4 - a.ndim)
        irec += struct.pack("<HHI4QQQ", len(n), a.ndim, 0, *dims, off, a.nbytes) + n
        off = -(-(off + a.nbytes) // ALIGN) * ALIGN
    total = off
    with open(path, "wb") as fh:
        fh.write(MAGIC + struct.pack("<IIQIIQQQQ", VERSION, HEADER, total, len(settings), len(arrays), s_off, i_off, d_off, 0))
        fh.write(srec + irec)
        fh.write(b"\0" * (d_off - i_off - len(irec)))
        pos = d_off
        for a in arrays.values():
            fh.write(a.tobytes())
            pos += a.nbytes
            pad = -(-pos // ALIGN) * ALIGN - pos
            fh.write(b"\0" * pad)
            pos += pad
    return total


def export(net, args, path):
    """Write the model file of `net` (a network module, or its state_dict) under the configuration `args`."""
    sd = net.state_dict() if hasattr(net, "state_dict") else net
    tensors = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items()}
    tensors.update(aux_tensors(args))
    return write(path, settings_of(args), tensors)


DENOISER_LEAVES = ("depth", "num_tfc", "num_stages", "use_SAM", "use_fencoding", "f_dim", "sample_rate_denoiser", "segment_size",
                   "stft_win_size", "stft_hop_size")


def denoiser_aux_tensors():
    """{'aux.tw4096', 'aux.fade'}: the twiddle table of testing.denoise.DenoiserPrepass and the 2048-point Hamming window its
    apply_denoiser cross-fades with, as that class builds them."""
    q = np.arange(2048)
    tw = torch.tensor(np.stack([np.cos(2 * np.pi * q / 4096), -np.sin(2 * np.pi * q / 4096)], -1), dtype=torch.float32)
    return {"aux.tw4096": tw.contiguous(), "aux.fade": torch.hamming_window(window_length=2048)}


def export_denoiser(sd_or_net, dargs, path):
    """Write the denoiser's weights file (csrc/dn_engine.hip: babe_denoiser_load): the same container with the string setting
    kind = "denoiser", the leaves of `dargs` - the configuration's tester.denoiser node: DENOISER_LEAVES, and any other leaf it
    has (the use_* options the library refuses when set) - under tester.denoiser.*, the reference state_dict and the two tables
    of denoiser_aux_tensors."""
    sd = sd_or_net.state_dict() if hasattr(sd_or_net, "state_dict") else sd_or_net
    get = (lambda k: dargs[k]) if isinstance(dargs, dict) else (lambda k: getattr(dargs, k))
    missing = [k for k in DENOISER_LEAVES if (k not in dargs if isinstance(dargs, dict) else not hasattr(dargs, k))]
    if missing:
        raise ValueError(f"export_denoiser: tester.denoiser lacks {missing}")
    keys = list(dargs.keys()) if hasattr(dargs, "keys") else list(DENOISER_LEAVES)
    settings = {"kind": "denoiser"}
    flatten({k: get(k) for k in keys}, "tester.denoiser.", settings)
    tensors = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items()}
    tensors.update(denoiser_aux_tensors())
    return write(path, settings, tensors)


def read(path, aux=False):
    """-> (settings {key: number | str}, state_dict {name: float32 tensor}), ready for load_state_dict; aux=True keeps the two
    aux.* tables in the mapping as well."""
    buf = open(path, "rb").read()
    if len(buf) < HEADER or buf[:8] != MAGIC:
        raise ValueError(f"{path}: not a babe model file")
    version, hbytes, total, nset, nten, s_off, i_off, d_off, _ = struct.unpack_from("<IIQIIQQQQ", buf, 8)
    if version != VERSION:
        raise ValueError(f"{path}: version {version}, this reader knows {VERSION}")
    if total != len(buf):
        raise ValueError(f"{path}: truncated ({len(buf)} of {total} bytes)")
    settings, pos = {}, s_off
    for _ in range(nset):
        klen, kind, _, vlen = struct.unpack_from("<HBBI", buf, pos)
        key = buf[pos + 8:pos + 8 + klen].decode("ascii")
        val = buf[pos + 8 + klen:pos + 8 + klen + vlen]
        if kind:
            settings[key] = val.decode("ascii")
        else:
            v = struct.unpack("<d", val)[0]
            settings[key] = int(v) if v.is_integer() else v
        pos += 8 + klen + vlen
    sd, pos = {}, i_off
    for _ in range(nten):
        nlen, ndim, _, d0, d1, d2, d3, off, nbytes = struct.unpack_from("<HHI4QQQ", buf, pos)
        name = buf[pos + 56:pos + 56 + nlen].decode("ascii")
        shape = (d0, d1, d2, d3)[:ndim]
        if off + nbytes > len(buf) or nbytes != 4 * int(np.prod(shape)):
            raise ValueError(f"{path}: tensor {name} leaves the file")
        sd[name] = torch.from_numpy(np.frombuffer(buf, dtype="<f4", count=nbytes // 4, offset=off).reshape(shape).copy())
        pos += 56 + nlen
    return settings, (sd if aux else network_state(sd))


def network_state(sd):
    """The network's own tensors of a state_dict returned by `read` (without the aux.* tables)."""
    return {k: v for k, v in sd.items() if not k.startswith("aux.")}
