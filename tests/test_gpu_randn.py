"""csrc/randn.hip: the counter-based Gaussian generator (babe_rand_bits / babe_randn) against a numpy restatement of its
definition - Philox4x32-10 words bit for bit, the normal transform against float64 Box-Muller of the same words.  Needs a MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox_words(n, seed, clip, draw):
    """The n 32-bit words of (seed, clip, draw): counter (q & 0xffffffff, q >> 32, clip, draw), q = i // 4, key (seed & 0xffffffff,
    seed >> 32), word i % 4 - ten rounds in uint64 arithmetic."""
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    c = [q & MASK, q >> np.uint64(32), np.full(nq, clip, np.uint64), np.full(nq, draw, np.uint64)]
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return np.stack(c, 1).reshape(-1)[:n].astype(np.uint32)


def test_the_numpy_restatement_reproduces_the_known_answer():
    """(0,0,0,0) / (0,0) -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8: the reference of this file is the published function."""
    assert [hex(v) for v in philox_words(4, 0, 0, 0)] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]


def _bits(B, n, seed, clip0, draw, stride=None, offset=0):
    """babe_rand_bits into a buffer filled with a canary -> (rows [B][n] uint32, everything else of the buffer)."""
    from babe_amd._lib import check, lib, stream
    stride = n if stride is None else stride
    buf = torch.full((offset + B * stride + 8,), -7, dtype=torch.int32, device="cuda")
    check(lib().babe_rand_bits(buf.data_ptr() + 4 * offset, stride, B, n, seed, clip0, draw, stream()), "rand_bits")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    body = h[offset:offset + B * stride].reshape(B, stride)
    untouched = np.concatenate([h[:offset], body[:, n:].reshape(-1), h[offset + B * stride:]])
    return body[:, :n].view(np.uint32), untouched


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 92092])
@pytest.mark.parametrize("B,stride_pad,offset,seed,clip0,draw", [
    (1, 0, 0, 1, 0, 0),
    (3, 0, 0, 1, 0, 0),                      # rows start wherever n puts them: aligned and unaligned rows in one launch
    (3, 7, 0, 0x1234567 << 12, 5, 7),        # a row stride larger than n, a seed above 2^32, clip0 = 5, draw = 7
    (1, 0, 1, 99, 5, 7),                     # the output pointer 4 bytes past a 16-byte boundary: the dword-store path
    (3, 4, 1, (1 << 40) + 3, 5, 7),
])
def test_rand_bits_equal_the_definition_word_for_word(n, B, stride_pad, offset, seed, clip0, draw):
    got, untouched = _bits(B, n, seed, clip0, draw, n + stride_pad, offset)
    for b in range(B):
        want = philox_words(n, seed, clip0 + b, draw)
        assert np.array_equal(got[b], want), (b, np.flatnonzero(got[b] != want)[:8])
    assert (untouched == -7).all(), "wrote outside the rows"


def test_rows_do_not_depend_on_the_batch_they_are_drawn_in():
    """Row b of a B = 3 call = the B = 1 call with clip0 + b (bits and normals)."""
    from babe_amd._lib import check, lib, stream
    n, seed, clip0, draw = 4099, 11, 5, 2
    got, _ = _bits(3, n, seed, clip0, draw)
    z3 = torch.empty(3, n, device="cuda")
    check(lib().babe_randn(z3.data_ptr(), n, 3, n, seed, clip0, draw, stream()), "randn")
    for b in range(3):
        one, _ = _bits(1, n, seed, clip0 + b, draw)
        assert np.array_equal(got[b], one[0])
        z1 = torch.empty(1, n, device="cuda")
        check(lib().babe_randn(z1.data_ptr(), n, 1, n, seed, clip0 + b, draw, stream()), "randn")
        assert torch.equal(z3[b], z1[0])
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(_bits(1, n, seed, clip0, draw + 1)[0], got[:1])


def _normals(n, seed, clip0=0, draw=0, B=1):
    from babe_amd._lib import check, lib, stream
    z = torch.full((B, n), float("nan"), device="cuda")
    check(lib().babe_randn(z.data_ptr(), n, B, n, seed, clip0, draw, stream()), "randn")
    torch.cuda.synchronize()
    return z.cpu().numpy()


@pytest.mark.parametrize("n,seed", [(92092, 3), (1 << 20, (1 << 33) + 1), (5, 3)])
def test_randn_is_box_muller_of_the_same_words(n, seed):
    """babe_randn against float64 Box-Muller of the definition's words: u1 = ((r >> 9) + 0.5) 2^-23, u2 = (r' >> 9) 2^-23,
    z = sqrt(-2 ln u1) (cospi(2 u2), sinpi(2 u2)) on word pairs (0,1) and (2,3).  Relative error at most 8 float32 ulp (2^-20):
    the sum of the ulp bounds of logf, sqrtf and sincospif of the HIP math tables, the logarithm's halved by the square root,
    plus the two multiplies.  At the exact zeros of a factor (u2 = 0.25, 0.75 for the cosine, 0, 0.5 for the sine) the element
    compares absolutely at 1e-7.  |z| <= 5.78 and finite everywhere."""
    z = _normals(n, seed)[0]
    w = philox_words((n + 3) // 4 * 4, seed, 0, 0).reshape(-1, 2)
    u1 = ((w[:, 0] >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    k = (w[:, 1] >> 9).astype(np.int64)                      # u2 = k 2^-23: reduce the angle exactly, in integers
    rad = np.sqrt(-2.0 * np.log(u1))
    frac = (k % (1 << 22)).astype(np.float64) * 2.0 ** -22   # 2 u2 mod 1
    sign = np.where(k >= (1 << 22), -1.0, 1.0)               # cospi(v + 1) = -cospi(v), likewise the sine
    want = np.stack([rad * sign * np.cos(np.pi * frac), rad * sign * np.sin(np.pi * frac)], 1)
    zero = np.stack([(k % (1 << 22)) == (1 << 21), (k % (1 << 22)) == 0], 1)
    want[zero] = 0.0
    want, zero = want.reshape(-1)[:n], zero.reshape(-1)[:n]
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.78
    assert np.abs(z[zero]).max(initial=0.0) <= 1e-7
    rel = np.abs(z[~zero].astype(np.float64) - want[~zero]) / np.abs(want[~zero])
    print(f"n = {n}: max relative error {rel.max() * 2 ** 23:.2f} ulp, exact zeros {int(zero.sum())}")
    assert rel.max() <= 2.0 ** -20, (rel.max() * 2 ** 23, int(rel.argmax()))


def test_moments_over_a_million_draws():
    """n = 2^20: mean, variance and lag-1 correlation each within 5 standard errors (5/sqrt(n), 5 sqrt(2/n), 5/sqrt(n))."""
    n = 1 << 20
    z = _normals(n, 20240229, clip0=1, draw=3)[0].astype(np.float64)
    mean, var = z.mean(), z.var()
    lag1 = np.mean((z[:-1] - mean) * (z[1:] - mean)) / var
    print(f"mean {mean:.3e}, variance - 1 {var - 1:.3e}, lag-1 correlation {lag1:.3e}")
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert abs(lag1) <= 5 / np.sqrt(n)
