"""Host-only owners of two facts the sequencers share: the GroupNorm split rule (babe_gn_splits, csrc/norm.hip) and the workspace
carver (csrc/workspace.h), the latter in a stand-alone C++ program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gn_split_rule_has_one_owner():
    from babe_amd import ops
    from babe_amd._lib import lib
    for n in (1, 16383, 16384, 32767, 32768, 64 * 16384 - 1, 64 * 16384, 10 ** 9):
        want = max(1, min(64, n // 16384))
        assert lib().babe_gn_splits(n) == want, n
        assert ops._splits(n) == want, n


CARVER_PROGRAM = r"""
#include "workspace.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Piece { char* p; size_t bytes; };

// a mixed list: odd byte counts, a zero-length piece, doubles after floats
static int carve(Carver& c, Piece* out) {
    int k = 0;
    out[k++] = {c.take<char>(1), 1};
    out[k++] = {c.take<char>(257), 257};
    out[k++] = {reinterpret_cast<char*>(c.take<float>(3)), 12};
    out[k++] = {reinterpret_cast<char*>(c.take<float>(0)), 0};
    out[k++] = {reinterpret_cast<char*>(c.take<float>(65)), 260};
    out[k++] = {reinterpret_cast<char*>(c.take<double>(7)), 56};
    out[k++] = {reinterpret_cast<char*>(c.take<int>(1)), 4};
    out[k++] = {reinterpret_cast<char*>(c.take<double>(33)), 264};
    out[k++] = {c.take<char>(1023), 1023};
    return k;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("line %d (granule %zu): %s\n", __LINE__, granule, #cond); return 1; } } while (0)

static int run(size_t granule) {
    Piece pc[16];
    Carver dry{nullptr, 0, granule};
    const int n = carve(dry, pc);
    CHECK(dry.ok && dry.used > 0 && dry.used % granule == 0);
    for (int k = 0; k < n; ++k) CHECK(pc[k].p == nullptr);
    const size_t total = dry.used;
    char* buf = static_cast<char*>(std::malloc(total));                  // exactly the dry total: the sanitizer guards both ends
    CHECK(buf);
    Carver c{buf, total, granule};
    CHECK(carve(c, pc) == n && c.ok && c.used == total);
    char* end = buf;
    for (int k = 0; k < n; ++k) {
        CHECK(pc[k].p != nullptr && pc[k].p >= end);                      // ascending and disjoint
        CHECK((size_t)(pc[k].p - buf) % granule == 0);
        std::memset(pc[k].p, 0x5a + k, pc[k].bytes);                      // every byte of every piece
        end = pc[k].p + (pc[k].bytes + granule - 1) / granule * granule;
        CHECK(end <= buf + total);
    }
    CHECK(end == buf + total);                                            // the last piece ends at the total
    for (int k = 0; k < n; ++k)
        for (size_t i = 0; i < pc[k].bytes; ++i) CHECK(pc[k].p[i] == (char)(0x5a + k));
    CHECK((uintptr_t)pc[5].p % alignof(double) == 0 && (uintptr_t)pc[7].p % alignof(double) == 0);
    // one byte less: the flag trips, nothing at or past the end comes back, and the total is still reported
    Carver s{buf, total - 1, granule};
    CHECK(carve(s, pc) == n && !s.ok && s.used == total);
    for (int k = 0; k < n; ++k) CHECK(pc[k].p == nullptr || pc[k].p + pc[k].bytes <= buf + total - 1);
    CHECK(pc[n - 1].p == nullptr);
    std::free(buf);
    return 0;
}

int main() {
    if (run(256) || run(4)) return 1;
    std::puts("carver ok");
    return 0;
}
"""


def test_carver_in_a_sanitized_host_program(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src, exe = tmp_path / "carver.cpp", tmp_path / "carver"
    src.write_text(CARVER_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-g", "-I",
                    os.path.join(ROOT, "babe_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "carver ok" in r.stdout, r.stdout
