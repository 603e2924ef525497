"""Record the conv launchers' host rules - packed sizes, *_supported / *_preferred verdicts, stat slots - over a fixed grid.

    python tests/golden/make_conv_rules_golden.py            # writes tests/golden/conv_rules.json

The functions are pure host arithmetic on their arguments (no pointer is dereferenced, no GPU is needed), so the table made at
one commit can be compared exactly at another: tests/test_conv_rules_cpu.py imports this module for the grid and compares what
the library answers with the table.  Regenerate the table only when a rule is MEANT to change.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "conv_rules.json")

# both sides of every padding unit (8, 16, 32, 64) and tile width (64, 96, 128), and of the 2032-value in_scale copy
CH = (1, 2, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128, 256, 2032, 2048)
# channel counts whose weight images cross the 2 GiB descriptor limits of the nested / bf16 kernels
BIG = ((2048, 4096), (3072, 4096), (4096, 4096), (8192, 8192), (8192, 16384), (16384, 16384))
TS = (12, 16, 20, 30, 60, 64, 272)
KS = ((5, 3), (1, 1), (3, 3))
# (F, dil): full and ragged row pairs / quads per residue class
FD = ((32, 1), (33, 1), (5, 1), (7, 1), (30, 2), (17, 2), (37, 3), (9, 4), (64, 8), (128, 16), (100, 32))
PAIRS = ((64, 64), (96, 128), (128, 96), (32, 33), (16, 256), (64, 2032), (2048, 64), (5, 2), (48, 3), (256, 4), (100, 100))
VERDICTS = ("babe_conv2d_wino_supported", "babe_conv2d_wino4_supported", "babe_conv2d_wino45_supported",
            "babe_conv2d_wino45_preferred", "babe_conv2d_wino85_supported", "babe_conv2d_wino85_preferred",
            "babe_conv2d_fewco_supported", "babe_conv2d_bf16_units_supported")
P_IN, P_IN2, P_OUT, P_RES, P_AUX = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
LIMS = (0x7fffffff // 4, 0x3fffffff // 4)


def size_cases():
    """(function name, argument tuple) of every packed-size question."""
    for tf in (0, 1):
        for co in CH:
            for ci in CH:
                for kh, kw in KS:
                    yield "babe_conv_packed_size", (co, ci, kh, kw, tf)
                    for splits in (1, 2):
                        yield "babe_conv_packed_size_bf16", (co, ci, kh, kw, tf, splits)
                    yield "babe_conv_packed_size_wino", (co, ci, kh, tf)
                    yield "babe_conv_packed_size_wino4", (co, ci, kh, tf)
                yield "babe_conv_packed_size_wino45", (co, ci, tf)
                yield "babe_conv_packed_size_wino85", (co, ci, tf)
    for c in CH:
        for f, _ in FD:
            for t in TS:
                yield "babe_units_size", (c, f, t)


def _case(Cin, Cout, T=64, F=32, dil=1, k=(5, 3), in2=False, res=False, in_scale=False, fbias=False, split=None, **over):
    """Fields of one babe_conv_args: dense 16-byte aligned views unless `over` says otherwise."""
    n = F * T
    split = split if split is not None else (Cin // 2 if in2 and Cin > 1 else Cin)
    d = dict(in_=P_IN, in_bs=split * n, in_cs=n, cin_split=split, w_packed=P_AUX, out=P_OUT, out_bs=Cout * n, out_cs=n,
             B=1, Cin=Cin, Cout=Cout, F=F, T=T, KH=k[0], KW=k[1], dil=dil, alpha=1.0, rbeta=0.0)
    if in2:
        d.update(in2=P_IN2, in2_bs=(Cin - split) * n, in2_cs=n)
    if res:
        d.update(res=P_RES, res_bs=Cout * n, res_cs=n, rbeta=1.0)
    if in_scale:
        d["in_scale"] = P_AUX + 0x1000
    if fbias:
        d["fbias"] = P_AUX + 0x2000
    d.update(over)
    return d


def verdict_cases():
    """Field dicts of every babe_conv_args the verdict functions are asked about."""
    # channels x kernel shape (T = 64: every kernel's minimum), and the (5,3) kernels once more on a longer, ragged row
    for ci in CH:
        for co in CH:
            for k in KS:
                yield _case(ci, co, k=k)
            yield _case(ci, co, T=272, F=33)
    for ci, co in BIG:
        yield _case(ci, co, F=4)
        yield _case(ci, co, F=4, T=16)
    # T x (F, dil) x kernel shape: the tile fills of the *_preferred rules, T below / not a multiple of the kernels' units
    for ci, co in PAIRS:
        for t in TS:
            for f, dil in FD:
                for k in KS:
                    yield _case(ci, co, T=t, F=f, dil=dil, k=k)
    for dil in (0, -1):
        yield _case(64, 64, dil=dil)
    for ci, co in PAIRS:
        for k in KS:
            for t in (16, 64):
                # with and without a second source, a residual, an input scale, a frequency bias
                for m in range(16):
                    yield _case(ci, co, T=t, k=k, in2=bool(m & 1), res=bool(m & 2), in_scale=bool(m & 4), fbias=bool(m & 8))
                for split in (8, 16, 32, 24):
                    if split < ci:
                        yield _case(ci, co, T=t, k=k, in2=True, split=split)
                # pointers 4-, 8- and 16-byte aligned, strides odd, even and multiples of 4, one operand at a time
                base = _case(ci, co, T=t, k=k, in2=ci > 1, res=True)
                for p in ("in_", "in2", "out", "res"):
                    if p in base:
                        for off in (4, 8, 16):
                            yield dict(base, **{p: base[p] + off})
                for s in ("in_bs", "in_cs", "in2_bs", "in2_cs", "out_bs", "out_cs", "res_bs", "res_cs"):
                    if s in base:
                        for off in (1, 2, 3, 4):
                            yield dict(base, **{s: base[s] + off})
    # strides on both sides of each 32-bit limit: channels x channel stride of every view (floats below 2 GiB and below 1 GiB),
    # bytes of a unit tensor, positions of a plane
    for ci, co in ((64, 64), (128, 96), (96, 128), (16, 100), (64, 4), (2048, 64)):
        for k in ((5, 3), (1, 1)):
            for lim in LIMS:
                for res in (False, True):
                    for name, mult, in2 in (("in_cs", ci, False), ("in_cs", ci // 2, True), ("in2_cs", ci - ci // 2, True),
                                            ("out_cs", co, False), ("out_cs", (co + 31) // 32 * 32, False),
                                            ("res_cs", co, False), ("res_cs", (co + 31) // 32 * 32, True)):
                        if name == "res_cs" and not res:
                            continue
                        edge = (lim + mult - 1) // mult // 4 * 4
                        for cs in (edge - 4, edge, edge + 4):
                            yield _case(ci, co, k=k, in2=in2, res=res, **{name: cs})
        edge = 0x7fffffff // (16 * (ci >> 3)) // 4 * 4
        for cs in (edge - 4, edge, edge + 4, edge + 8):
            yield _case(ci, co, in_cs=cs)
    for f, t in ((65535, 4096), (65536, 4096), (16384, 16384), (16383, 16384), (131072, 4096), (131071, 4096)):
        yield _case(64, 64, F=f, T=t, in_cs=4096, out_cs=4096)


def stat_cases():
    for cg in (0, 2, 4, 8, 12, 16, 20, 32):
        for f, dil in FD + ((1, 1), (8, 0), (0, 1)):
            for t in TS + (0,):
                yield dict(stat_cg=cg, F=f, T=t, dil=dil)


def evaluate(path):
    """What the library at `path` answers over the grid, as JSON-ready lists in grid order.  (A handle of its own: two of the
    verdict functions are in include/babe_hip.h but not among the entry points the package declares for itself.)"""
    from babe_amd._cabi import ConvArgs
    L = C.CDLL(path)
    for fn, args in size_cases():
        getattr(L, fn).restype, getattr(L, fn).argtypes = C.c_long, [C.c_int] * len(args)
    for fn in VERDICTS + ("babe_conv2d_wino85_stat_slots",):
        getattr(L, fn).restype, getattr(L, fn).argtypes = C.c_int, [C.POINTER(ConvArgs)]
    sizes = {}
    for fn, args in size_cases():
        sizes.setdefault(fn, []).append(getattr(L, fn)(*args))
    fns = [getattr(L, v) for v in VERDICTS]
    verdicts = []
    for d in verdict_cases():
        a = C.byref(ConvArgs(**d))
        verdicts.append(sum((1 << i) for i, f in enumerate(fns) if f(a)))
    slots = [L.babe_conv2d_wino85_stat_slots(C.byref(ConvArgs(**d))) for d in stat_cases()]
    return {"verdict_bits": list(VERDICTS), "sizes": sizes, "verdicts": verdicts, "stat_slots": slots}


if __name__ == "__main__":
    from babe_amd import _lib
    table = evaluate(_lib._LIB_PATH)
    with open(OUT, "w") as fh:
        json.dump(table, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{OUT}: {sum(len(v) for v in table['sizes'].values())} sizes, {len(table['verdicts'])} verdicts, "
          f"{len(table['stat_slots'])} stat slots, {os.path.getsize(OUT)} bytes")
