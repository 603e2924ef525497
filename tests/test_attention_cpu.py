"""Time-attention layers, host side (no GPU): the bucket table, the state-dict layout against the imported reference (the
key list stored in tests/golden/attention_a.npz by make_attention_golden.py) and the unchanged attention-off init."""
import math
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


def reference_buckets(T, num_buckets=32, max_distance=64):
    """RelativePositionBias._relative_position_bucket of the reference, restated (float32 torch ops, .long() truncation)."""
    pos = torch.arange(T, dtype=torch.long)
    rel = pos[None, :] - pos[:, None]                 # key - query
    nb = num_buckets // 2
    ret = (rel >= 0).to(torch.long) * nb
    n = torch.abs(rel)
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).long()
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ret + torch.where(n < max_exact, n, large)


def test_bucket_table_equals_reference_formula():
    import __graft_entry__ as ge
    ge.build()
    from babe_amd import ops
    for T in (1, 2, 7, 8, 9, 64, 100, 256, 1000, 2048, 4096):
        tab = ops.attn_buckets(T).long()
        assert tab.shape == (2 * T - 1,)
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1
        assert torch.equal(tab[idx], reference_buckets(T)), T


def test_state_dict_keys_and_shapes_equal_reference():
    from babe_amd.networks.cqtdiff_plus import param_specs
    from tests.attention_weights import FIXTURES, DILS
    want = [str(s) for s in np.load(os.path.join(G, "attention_a.npz"))["keys"]]
    Ns, fs, L, layers, adict = FIXTURES["a"]
    got = {k: "x".join(str(v) for v in shape) for k, shape, _ in param_specs(Ns, DILS[id(Ns)], attention_layers=layers,
                                                                              attention_dict=adict)}
    want = dict(s.rsplit(":", 1) for s in want)
    assert got == want
    assert sum(".attn_block.qk.weight" in k for k in got) == 7        # downs 4-6, bottleneck, ups of octaves 6-4
    assert got["middle.0.1.attn_block.qk.weight"] == "7168x3584x1"


def test_state_dict_keys_options():
    from babe_amd.networks.cqtdiff_plus import param_specs
    from tests.attention_weights import FIXTURES, DILS
    Ns, fs, L, layers, adict = FIXTURES["b"]
    keys = dict((k, s) for k, s, _ in param_specs(Ns, DILS[id(Ns)], attention_layers=layers, attention_dict=adict))
    assert sum(k.endswith("attn_block.qk.bias") for k in keys) == 15 and keys["downs.0.2.attn_block.qk.bias"] == (2 * 8 * 64,)
    assert not any("rel_pos" in k for k in keys)


def test_attention_off_init_is_unchanged():
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    from tests.golden_weights import FULL_DILS
    Ns = [8, 8, 8, 8, 16, 16, 16]
    a = init_state_dict(Ns, FULL_DILS, seed=3)
    for kw in (dict(attention_layers=[0] * 8), dict(attention_layers=None, attention_dict={"num_heads": 8}),
               dict(attention_layers=[0] * 8, attention_dict={"use_rel_pos": False, "bias_qkv": True})):
        b = init_state_dict(Ns, FULL_DILS, seed=3, **kw)
        assert list(a) == list(b)
        assert all(torch.equal(a[k], b[k]) for k in a)
    # the attention net draws its extra tensors after each block's own: every shared key before the first attention block
    # is bit-identical
    c = init_state_dict(Ns, FULL_DILS, seed=3, attention_layers=[0, 0, 0, 0, 1, 1, 1, 1])
    first = list(c).index("downs.4.2.norm2.gamma")
    for k in list(c)[:first]:
        assert torch.equal(a[k], c[k]), k
