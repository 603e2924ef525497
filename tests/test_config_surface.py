"""Config surface: every tester YAML of the reference goes through babe_amd.config.load_yaml and the
sampler class its `sampler_callable` string names (the reference resolves that string with dnnlib.call_func_by_name,
utils/setup.py:75-87, testing/blind_bwe_tester.py:214; INTEGRATION.md maps `testing.X.Y` -> `babe_amd.testing.X.Y`).
The reference's conf/ tree is stored as data in tests/golden/config_surface.yaml.gz (tests/golden/make_config_golden.py):
every conf/tester/*.yaml, the exp / network / diff_params files composed with them, and which sampler modules exist in the
reference tree.  Constructors only - no GPU work."""
import gzip
import importlib
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_surface.yaml.gz")


@pytest.fixture(scope="module")
def conf(tmp_path_factory):
    """The stored conf/ tree, read back through babe_amd.config.load_yaml (a YAML file, like the reference's own)."""
    from babe_amd.config import load_yaml
    p = tmp_path_factory.mktemp("conf") / "config_surface.yaml"
    with gzip.open(FIXTURE, "rb") as f:
        p.write_bytes(f.read())
    return load_yaml(str(p))


def compose(conf, tester, exp="maestro44k_8s"):
    """What hydra composes for test.py (conf/conf.yaml defaults + the tester/exp overrides of testing_blindbwe.sh)."""
    from babe_amd.config import to_attr
    return to_attr(dict(exp=conf.exp[exp], network=conf.network["cqtdiff+"], diff_params=conf.diff_params.edm,
                        tester=conf.tester[tester]))


class _Model:                      # the constructors never call the model
    CQTransform = None


def survey(conf):
    from babe_amd.diff_params.edm import EDM
    res = dict(ok=[], notimpl=[], error=[], no_such_class=[])
    assert len(conf.tester) == 87
    for name in sorted(conf.tester):
        args = compose(conf, name)
        mod, cls = args.tester.sampler_callable.rsplit(".", 1)
        in_reference = mod in conf.reference_modules
        # YAMLs written for the `testing.blind_bwe.` package layout the reference no longer ships: same class one level up
        mod_here = mod.replace("testing.blind_bwe.", "testing.")
        try:
            klass = getattr(importlib.import_module("babe_amd." + mod_here), cls)
        except (ImportError, AttributeError):
            res["no_such_class"].append((name, args.tester.sampler_callable, in_reference))
            continue
        try:
            klass(_Model(), EDM(args), args, True)
            res["ok"].append((name, in_reference))
        except NotImplementedError as e:
            res["notimpl"].append((name, str(e), in_reference))
        except Exception as e:                                   # noqa: BLE001 - the survey reports, the test asserts
            res["error"].append((name, f"{type(e).__name__}: {e}", in_reference))
    return res


def test_every_tester_yaml_constructs_its_sampler(conf):
    r = survey(conf)
    print({k: len(v) for k, v in r.items()})
    for k in ("notimpl", "error", "no_such_class"):
        for row in r[k]:
            print(k, row)
    # every config whose sampler module exists in the reference (63 of 87) constructs; none needs an unbuilt option
    assert not [row for row in r["error"] if row[2]], r["error"]
    resolvable_ok = [n for n, inref in r["ok"] if inref]
    assert len(resolvable_ok) == 63, len(resolvable_ok)
    assert not r["notimpl"], r["notimpl"]
    # the other 24 name a `testing.blind_bwe.*` module that is not in the reference tree (stale files: the reference's own
    # code cannot load them).  15 map onto BlindSampler and construct; 7 lack keys the reference's sampler reads
    # unconditionally (optimization.clamp_fc, blind_bwe_sampler.py:576) and fail here the way they would there; the Langevin /
    # learned-prior samplers (blind_bwe_langevin.yaml, blind_bwe_with_prior.yaml) exist nowhere
    assert sorted(n for n, _, _ in r["no_such_class"]) == ["blind_bwe_langevin.yaml", "blind_bwe_with_prior.yaml"]
    stale = sorted(n for n, _, _ in r["error"])
    assert stale == ["blind_bwe_2.yaml", "blind_bwe_backup.yaml", "blind_bwe_cocochorales.yaml", "blind_bwe_multislope.yaml",
                     "blind_bwe_noisy.yaml", "blind_bwe_vctk.yaml", "blind_bwe_vctk2.yaml"], stale
    assert all("clamp_fc" in msg for _, msg, _ in r["error"])
    assert len([n for n, inref in r["ok"] if not inref]) == 15


def test_default_args_restates_the_benchmark_yaml(conf):
    """babe_amd.config.default_args() == conf/tester/blind_bwe_formal_3000_opt_2.yaml + conf/network/cqtdiff+.yaml +
    conf/exp/maestro44k_8s.yaml + conf/diff_params/edm.yaml on every key it carries (= every key the sampler, the EDM
    wrapper and the network read)."""
    from babe_amd.config import default_args
    a = compose(conf, "blind_bwe_formal_3000_opt_2.yaml")
    d = default_args()
    skipped = {"tester.posterior_sampling.stft_distance.logmag",        # read with .get(..., False); not in this YAML
               "network.attention_dict"}                                # attention is off (attention_layers all 0)
    diffs = []

    def cmp(x, y, path):
        for k in y:
            if path + k in skipped:
                continue
            if k not in x:
                diffs.append(("missing in yaml", path + k))
            elif isinstance(y[k], dict):
                cmp(x[k], y[k], path + k + ".")
            elif x[k] != y[k]:
                diffs.append((path + k, x[k], y[k]))

    for sec in ("tester", "network", "diff_params"):
        cmp(a[sec], d[sec], sec + ".")
    assert not diffs, diffs
    assert (a.exp.sample_rate, a.exp.audio_len) == (d.exp.sample_rate, d.exp.audio_len) == (44100, 368368)


@pytest.mark.parametrize("exp,tester", [("maestro22k_8s", "edm_DC_correction_4s"), ("CocoChorales_16k_8s", "blind_bwe_denoise_brass"),
                                        ("maestro44k_8s", "blind_bwe_formal_3000_opt_2")])
def test_edm_overrides_follow_the_yaml(conf, exp, tester):
    """update_diff_params (:52-60) copies tester.diff_params over the training values: check on the three configurations
    BASELINE.json names."""
    from babe_amd.diff_params.edm import EDM
    mod = {"edm_DC_correction_4s": ("babe_amd.testing.edm_sampler", "Sampler")}.get(tester, ("babe_amd.testing.blind_bwe_sampler", "BlindSampler"))
    args = compose(conf, f"{tester}.yaml", exp)
    e = EDM(args)
    getattr(importlib.import_module(mod[0]), mod[1])(_Model(), e, args, False)
    src = args.tester.diff_params
    if not src.same_as_training:
        assert (e.sigma_min, e.sigma_max, e.ro, e.sigma_data, e.Schurn) == (src.sigma_min, src.sigma_max, src.ro, src.sigma_data, src.Schurn)
