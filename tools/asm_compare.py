#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees kernel by kernel.  No GPU needed.

    tools/asm_compare.py <tree_a> <tree_b> [file.hip ...]        (default: every file of babe_amd.build.SOURCES)

Each translation unit is compiled to device-only assembly with its tree's own product flags (babe_amd/build.py:
_compile_cmd, plus --cuda-device-only -S -fuse-cuid=none), local labels are renumbered per kernel, and every kernel gets
one verdict:
    identical          the same instructions in the same order
    same instructions  an equal multiset of mnemonics (s_nop / s_waitcnt aside) and equal VGPR / SGPR / LDS / scratch numbers:
                       a reordering
    differs            anything else: the resource numbers of both sides and the instruction-count deltas are printed
Exit status 1 if any kernel differs or exists on one side only.
"""
import collections
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

RESOURCES = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_asm_compare_build", os.path.join(tree, "babe_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, src, tmp):
    cmd = list(build._compile_cmd(src))
    out = os.path.join(tmp, src + ".s")
    cmd[cmd.index("-c")] = "-S"
    cmd[cmd.index("-o") + 1] = out
    r = subprocess.run(cmd + ["--cuda-device-only", "-fuse-cuid=none"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}\n{r.stdout}")
    with open(out) as fh:
        return fh.read()


def kernels(text):
    """{kernel symbol: (normalised body lines, {resource: value})} of one assembly file"""
    lines = text.splitlines()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    meta = {}
    for entry in re.split(r"^  - (?=\.)", text[text.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M).group(1)
        meta[name] = {k: int(re.search(rf"^\s*\.{k}:\s+(\d+)", entry, re.M).group(1)) for k in RESOURCES}
    out = {}
    for name in names:
        body, labels = [], {}
        for ln in lines[next(i for i, l in enumerate(lines) if l.startswith(name + ":")) + 1:]:
            ln = ln.split(";")[0].strip()
            if re.match(r"\.(section|amdhsa_kernel)\b", ln):
                break
            if not ln or (ln.startswith(".") and not re.match(r"\.L\w+:", ln)):
                continue                                   # blank, comment or directive
            body.append(re.sub(r"\.L[\w$]+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), ln))
        out[name] = (body, meta[name])
    return out


def mnemonics(body):
    # s_nop and s_waitcnt are put in after scheduling (hazard padding, counter waits): how many a kernel needs follows the
    # order of its instructions, not what they are
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":") and l.split()[0] not in ("s_nop", "s_waitcnt"))


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    res = subprocess.run([filt] + list(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return {n: d.replace("(anonymous namespace)::", "").split("(")[0] for n, d in zip(names, res)}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    tree_a, tree_b = (os.path.abspath(p) for p in sys.argv[1:3])
    build_a, build_b = load_build(tree_a), load_build(tree_b)
    files = sys.argv[3:] or [s for s in build_a.SOURCES if s in build_b.SOURCES]
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        jobs = [(f, pool.submit(assembly, build_a, f, ta), pool.submit(assembly, build_b, f, tb)) for f in files]
        for f, ja, jb in jobs:
            ka, kb = kernels(ja.result()), kernels(jb.result())
            pretty = demangle(sorted(set(ka) | set(kb)))
            verdicts = []
            for name in sorted(set(ka) | set(kb), key=lambda n: pretty[n]):
                if name not in ka or name not in kb:
                    verdicts.append((pretty[name], "only in " + ("A" if name in ka else "B"), ""))
                    continue
                (body_a, res_a), (body_b, res_b) = ka[name], kb[name]
                ma, mb = mnemonics(body_a), mnemonics(body_b)
                if body_a == body_b and res_a == res_b:
                    verdicts.append((pretty[name], "identical", ""))
                elif ma == mb and res_a == res_b:
                    verdicts.append((pretty[name], "same instructions", ""))
                else:
                    delta = ", ".join(f"{m} {mb[m] - ma[m]:+d}" for m in sorted(set(ma) | set(mb)) if ma[m] != mb[m])
                    res = ", ".join(f"{k} {res_a[k]} -> {res_b[k]}" for k in RESOURCES)
                    verdicts.append((pretty[name], "differs", f"    {res}\n    instructions {sum(ma.values())} -> {sum(mb.values())}: {delta or 'same mix'}"))
            bad += sum(v[1] not in ("identical", "same instructions") for v in verdicts)
            if all(v[1] == "identical" for v in verdicts):
                print(f"{f}: identical ({len(verdicts)} kernels)")
                continue
            print(f"{f}:")
            for name, verdict, detail in verdicts:
                print(f"  {verdict:18s}{name}")
                if detail:
                    print(detail)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
