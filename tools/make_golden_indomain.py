#!/usr/bin/env python
"""Records tests/golden/indomain.npz from the reference's own in-domain filter arithmetic, on the CPU.

    python tools/make_golden_indomain.py /path/to/gst-visdial  [--out tests/golden/indomain.npz] [--seed 20261020]

Drives preprocessing/clip_in_domain_filtering.py's `cov_mean(feats.t(), rowvar=True)` and
`torch.distributions.MultivariateNormal(loc=mean, covariance_matrix=cov).log_prob(feats)` -- the two statements of its `-step
inference` that follow `model(image_feat)` -- on synthetic fp16 features (there is no CLIP network here: the filter starts at the
feature matrix).  The module imports clip, PIL and tqdm at its top; whichever of them is missing gets an empty stand-in in
sys.modules first (nothing of them is called by the two statements).

Two cases, fp16 features with unequal variances, a non-zero mean and a covariance of condition number 1e2 .. 1e3:
  a: N = 400, D = 32     b: N = 300, D = 64     each with 50 scored rows, part of them well outside the fit.
Stored per case: fit features, scored features, the reference's mean, cov and log-probs; and the seed."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch


def load_reference(root):
    stubbed = set()
    for name in ("clip", "PIL", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            stubbed.add(name)
    if "PIL" in stubbed:                                        # the names the module's `from PIL import ...` asks for
        pil = sys.modules["PIL"]
        pil.Image = pil.ImageFile = types.ModuleType("PIL.Image")
        pil.UnidentifiedImageError = type("UnidentifiedImageError", (Exception,), {})
    if "tqdm" in stubbed:
        sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    sys.path.insert(0, os.path.join(root, "preprocessing"))
    return importlib.import_module("clip_in_domain_filtering")


def make_case(ref, rng, n, d, m):
    scale = np.exp(rng.uniform(np.log(0.05), np.log(0.6), size=d))          # unequal variances: ratio up to 144 ...
    mix = np.eye(d) + 0.15 * rng.standard_normal((d, d)) / np.sqrt(d)       # ... mildly correlated
    loc = rng.uniform(-0.5, 0.5, size=d)
    fit = ((rng.standard_normal((n, d)) * scale) @ mix.T + loc).astype(np.float16)
    score = ((rng.standard_normal((m, d)) * scale * rng.choice([1.0, 1.0, 2.5], size=(m, 1))) @ mix.T + loc).astype(np.float16)
    feats = torch.from_numpy(fit)
    cov, mean = ref.cov_mean(feats.t(), rowvar=True)
    dist = torch.distributions.multivariate_normal.MultivariateNormal(loc=mean, covariance_matrix=cov)
    lp = dist.log_prob(torch.from_numpy(score))
    cond = float(np.linalg.cond(cov.numpy()))
    return {"fit": fit, "score": score, "mean": mean.numpy(), "cov": cov.numpy(), "log_prob": lp.numpy()}, cond


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference_root")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "indomain.npz"))
    ap.add_argument("--seed", type=int, default=20261020)
    args = ap.parse_args()
    ref = load_reference(args.reference_root)
    rng = np.random.RandomState(args.seed)
    out = {"seed": np.int64(args.seed)}
    for tag, (n, d) in (("a", (400, 32)), ("b", (300, 64))):
        case, cond = make_case(ref, rng, n, d, 50)
        print("case %s: N = %d D = %d  cond(cov) = %.1f  log_prob in [%.2f, %.2f]" % (tag, n, d, cond, case["log_prob"].min(), case["log_prob"].max()))
        assert 1e2 <= cond <= 1e3, "condition number outside 1e2 .. 1e3: change the scale range"
        for k, v in case.items():
            out["%s_%s" % (tag, k)] = v
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
