"""Seeded weights of the time-attention goldens (tests/golden/make_attention_golden.py, which imports the reference, and the
GPU tests, which must not): only outputs are stored in the fixtures, the weights are re-derived here from seeds."""
import torch

from tests.golden_weights import FULL_DILS, FULL_NS, scale_gates

SMALL_NS = [8, 8, 8, 8, 16, 16, 16]
SMALL_DILS = [2, 3, 4, 5, 6, 7, 7]
LAST_TWO = [0, 0, 0, 0, 1, 1, 1, 1]          # conf/network/cqtdiff+.yaml's commented variant: last two octaves + bottleneck


def attention_dict(use_rel_pos=True, bias_qkv=False):
    return dict(num_heads=8, attn_dropout=0.0, bias_qkv=bias_qkv, N=0, rel_pos_num_buckets=32, rel_pos_max_distance=64,
                use_rel_pos=use_rel_pos, Nproj=8)


def scale_attention(sd, seed=7):
    """gate2 is init-zero in the reference (1e-7 here): re-randomise gate2, norm2.gamma, affine2.bias, the qk bias and the
    relative-position tables to O(1) so that the attention branch is numerically visible in the block outputs."""
    g = torch.Generator().manual_seed(seed)
    for k in sorted(sd):
        if ".gate2." in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * (0.1 if k.endswith("weight") else 0.5)
        elif k.endswith(".norm2.gamma"):
            sd[k] = 1.0 + 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith(".affine2.bias"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("attn_block.qk.bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("relative_attention_bias.weight"):
            sd[k] = torch.randn(sd[k].shape, generator=g)
    return sd


def attention_sd(Ns, dils, layers, adict, seed=0):
    """babe_amd's init_state_dict(seed) with O(1) gates, then scale_gates and scale_attention."""
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    sd = init_state_dict(Ns, dils, seed=seed, gate_scale=1.0, attention_layers=layers, attention_dict=adict)
    return scale_attention(scale_gates(sd, seed=5))


# fixture name -> (Ns, sample rate, L, attention_layers, attention_dict)
FIXTURES = {
    "a": (SMALL_NS, 22050, 92092, LAST_TWO, attention_dict()),
    "b": (SMALL_NS, 22050, 92092, [1] * 8, attention_dict(use_rel_pos=False, bias_qkv=True)),
    "c": (FULL_NS, 44100, 46046, LAST_TWO, attention_dict()),
}
DILS = {id(SMALL_NS): SMALL_DILS, id(FULL_NS): FULL_DILS}


def fixture_sd(name):
    Ns, fs, L, layers, adict = FIXTURES[name]
    return attention_sd(Ns, DILS[id(Ns)], layers, adict, seed=0)
