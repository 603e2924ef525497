"""Command line: evaluate a trained prior on a folder of wav files or on a test split.

    python -m babe_amd.evaluate --config FILE [--ckpt PATH] [--precision f32|bf16x3|bf16] [--batch N] [key.sub=value ...]

Runs testing.evaluate.formal_test_bwe (the reference's BlindTester.formal_test_bwe, testing/blind_bwe_tester.py:321-577): every
item is degraded with the test filter, restored blind or with the known filter, written out and measured (log-spectral distance;
for blind runs the dB error of the estimated filter).  FILE is one YAML over config.default_args(); key.sub=value overrides are read
as YAML scalars or flow lists, as in babe_amd.train.  It reads

    exp.sample_rate, exp.audio_len, network.*, tester.*        the model and the sampler, as everywhere
    tester.formal_test.path      folder of *.wav to evaluate (sorted)
    tester.formal_test.folder    where the results go (original/ degraded/ reconstructed/ filters/ metrics.jsonl summary.json)
    tester.formal_test.blind     True: predict_blind_bwe;  False: the known test filter
    tester.formal_test.use_AR    autoregressive restoration (known filter only)
    tester.formal_test.OLA       cross-fade length between segments, samples
    tester.formal_test.typefilter   "fc_A" (default): the degradation is tester.blind_bwe.test_filter.{fc, A};
                                 anything else: the filter designed from tester.bandwidth_extension.filter
    tester.formal_test.normalize_std   optional: scale the degraded signal to this standard deviation for the sampler, and back
    dset_test                    optional section {callable, num_samples, seed, ...}: one of the test-split datasets
                                 (datasets.audiofolder_test.AudioFolderDatasetTest reads dset_test.test.path,
                                 datasets.maestro_dataset_test.MaestroDatasetTestChunks dset_test.{path, years, load_len});
                                 when present it is used instead of tester.formal_test.path

and prints the summary (summary.json) as one JSON line.  Exit status 2 when no item was found.  One process, one GPU.
Without --ckpt the network has random weights (useful only to exercise the path)."""
import argparse
import glob
import inspect
import json
import os
import sys


def default_eval_args(**kw):
    """config.default_args(**kw) plus the sections the formal test reads, with the values of the reference's
    conf/tester/blind_bwe_formal_3000_opt_2.yaml (formal_test, blind_bwe.test_filter, bandwidth_extension.filter); the two
    paths are the user's to give."""
    from .config import default_args, to_attr
    a = default_args(**kw)
    a.tester.formal_test = to_attr(dict(path="None", folder="None", blind=True, use_AR=False, OLA=256, overlap=0.25,
                                        typefilter="fc_A", normalize_std="None"))
    a.tester.blind_bwe.test_filter = to_attr(dict(fc=[1000], A=[-20]))
    a.tester.bandwidth_extension = to_attr(dict(
        decimate=dict(factor=1),
        filter=dict(type="firwin", fc=3000, order=500, fir_order=500, beta=1, ripple=0.05, resample=dict(fs=2000),
                    biquad=dict(Q=0.707))))
    return a


def load_config(path, overrides=()):
    from .config import apply_overrides, load_yaml
    from .train import merge
    args = default_eval_args()
    if path:
        merge(args, load_yaml(path))
    return apply_overrides(args, overrides)


def none_or(v):
    return None if v in (None, "None") else v


def find_items(args):
    """The dataset of the dset_test section if there is one, else the sorted *.wav of tester.formal_test.path ([] if none)."""
    dt = args.get("dset_test", None)
    if dt is not None:
        from .datasets import resolve
        cls = resolve(dt.callable)
        kw = dict(num_samples=dt.get("num_samples", 4), seed=dt.get("seed", 42))
        if "fs" in inspect.signature(cls.__init__).parameters:
            kw.update(fs=args.exp.sample_rate, seg_len=args.exp.audio_len)
        try:
            return cls(dt, **kw)
        except ValueError as e:                      # (an empty folder or split)
            print(f"dset_test: {e}", file=sys.stderr)
            return []
    path = none_or(args.tester.formal_test.path)
    return sorted(glob.glob(os.path.join(path, "*.wav"))) if path else []


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", help="YAML over config.default_args(): exp / network / tester (/ dset_test) sections")
    ap.add_argument("--ckpt", default=None, help="checkpoint of babe_amd.train or of the reference (EMA weights are loaded)")
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16x3", "bf16"], help="the network's conv arithmetic")
    ap.add_argument("--batch", type=int, default=8, help="segments restored per batch")
    ap.add_argument("overrides", nargs="*", help="key.sub=value")
    a = ap.parse_args(argv)
    args = load_config(a.config, a.overrides)
    ft = args.tester.formal_test
    out_dir = none_or(ft.folder)
    if out_dir is None:
        ap.error("tester.formal_test.folder (where the results go) is not set")
    if ft.use_AR and ft.blind:
        ap.error("tester.formal_test.use_AR needs blind=False (the reference asserts it)")
    items = find_items(args)
    if len(items) == 0:
        print("no item found: tester.formal_test.path holds no *.wav and there is no usable dset_test section", file=sys.stderr)
        return 2

    from .diff_params.edm import EDM
    from .io import load_checkpoint
    from .networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from .testing.blind_bwe_sampler import BlindSampler
    from .testing.evaluate import formal_test_bwe
    net = Unet_CQT_oct_with_attention(args, "cuda", precision=a.precision)
    if a.ckpt:
        load_checkpoint(net, a.ckpt)
    sampler = BlindSampler(net, EDM(args), args, batch_semantics="per_clip")
    summary = formal_test_bwe(sampler, items, out_dir, blind=bool(ft.blind), typefilter=ft.get("typefilter", "fc_A"),
                              use_AR=bool(ft.use_AR), batch_size=a.batch, normalize_std=none_or(ft.get("normalize_std", "None")))
    print(json.dumps(summary, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
