"""Timing of the in-domain image filter on the MI355X, beside the plain torch statement of the same arithmetic on the same GPU.

    python tools/bench_indomain.py --out profiles/indomain.txt [--rows 123287] [--dim 512] [--repeats 9]

Shapes: the fit on 123 287 x 512 fp16 features (the VisDial v1.0 train images, CLIP ViT-B/32 width); scoring in batches of 1440
(the reference's batch size) and of 65 536.  Features are synthetic (seeded, unequal variances, non-zero mean): there is no CLIP
network here and the arithmetic does not care.

Figures (device events around windows of `iters` calls after a warm-up, alternating the two sides; median of `repeats` windows with
min .. max; no figure is a pass / fail condition):
  fit        InDomainFilter's device part (ops.gauss_fit: two launches)      | torch: feats.double(), mean, centred matmul, 1/(N-1)
  factor     the host part of a fit (copy, Cholesky, triangular solve, pack, copy back), host clock -- paid once per fit
  log-prob   ops.gauss_logprob, one launch                                   | torch: MultivariateNormal(loc, cov).log_prob(feats.double())
The torch side is the only alternative a user has today (the reference's own statements on this GPU); its MultivariateNormal is
built once outside the timed window, as the reference builds it once per run.  Achieved FLOP/s use the operations the rule needs
(fit: N D (D + 1) for the lower triangle; log-prob: M D (D + 16), the triangle of W in 16 x 4 blocks) over the measured time.
The scores of the two sides are compared on the way (max relative difference printed)."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs):
    return "median %.4f ms (min %.4f .. max %.4f over %d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def both(ours, theirs, iters, repeats):
    for fn in (ours, theirs):
        if fn is not None:
            fn()
            fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(repeats):
        a.append(window(ours, iters))
        if theirs is not None:
            b.append(window(theirs, iters))
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=123287)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-torch", action="store_true", help="time this project's side only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_indomain.py measures on the GPU; none found")
    from gst_visdial_amd import ops
    from gst_visdial_amd.indomain import InDomainFilter, factor
    dev = torch.device("cuda:0")
    N, D = args.rows, args.dim
    g = torch.Generator(device="cpu").manual_seed(123287)
    scale = torch.exp(torch.empty(D).uniform_(math.log(0.1), math.log(0.5), generator=g))
    loc = torch.empty(D).uniform_(-0.5, 0.5, generator=g)
    feats = (torch.randn(N, D, generator=g) * scale + loc).to(torch.float16).to(dev)
    lines = ["in-domain image filter on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "fit %d x %d fp16; scoring batches of 1440 and 65536 rows" % (N, D), ""]

    # ---- fit
    mean = torch.empty(D, dtype=torch.float64, device=dev)
    cov = torch.empty(D, D, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.gauss_fit_ws_bytes(N, D), dtype=torch.uint8, device=dev)

    def fit_ours():
        ops.gauss_fit(feats, mean=mean, cov=cov, workspace=ws)

    ref = {}

    def fit_torch():
        m = feats.double().t()
        mu = m.mean(dim=1, keepdim=True)
        mc = m - mu
        ref["cov"], ref["mean"] = (1.0 / (N - 1)) * mc.matmul(mc.t()), mu.squeeze()

    a, b = both(fit_ours, None if args.no_torch else fit_torch, 5, args.repeats)
    flop = float(N) * D * (D + 1)
    lines.append("fit       device  %s   %.2f TFLOP/s of the rule's %.1f GFLOP; workspace %.1f MB"
                 % (stat(a), flop / statistics.median(a) / 1e9, flop / 1e9, ws.numel() / 1e6))
    if b:
        lines.append("fit       torch   %s   (.double(), mean, centred matmul: %.1f MB of float64 temporaries)" % (stat(b), 3 * N * D * 8 / 1e6))
        lines.append("          max |cov - torch's| %.3e   max |mean - torch's| %.3e" % ((cov - ref["cov"]).abs().max().item(), (mean - ref["mean"]).abs().max().item()))
    t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        W, hld = factor(cov)
        wp = ops.gauss_pack_w(W).to(dev)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    lines.append("factor    host    %s   once per fit: D x D to the host, Cholesky, triangular solve, pack, back" % stat(t))
    lines.append("")

    # ---- scoring
    f = InDomainFilter(dev).load_state_dict({"mean": mean, "cov": cov, "w_packed": wp, "half_log_det": torch.tensor(hld, dtype=torch.float64)})
    dist = None
    if not args.no_torch:
        try:
            dist = torch.distributions.MultivariateNormal(loc=ref["mean"], covariance_matrix=ref["cov"])
        except Exception as e:                                 # a torch build without a device solver: factor its covariance on the host
            lines.append("(torch could not factor on the device: %s; its scale_tril comes from the host)" % str(e).splitlines()[0][:120])
            dist = torch.distributions.MultivariateNormal(loc=ref["mean"], scale_tril=torch.linalg.cholesky(ref["cov"].cpu()).to(dev))
    for M, iters in ((1440, 50), (65536, 5)):
        x = (torch.randn(M, D, generator=g) * scale * 1.2 + loc).to(torch.float16).to(dev)
        out = torch.empty(M, dtype=torch.float64, device=dev)

        def score_ours():
            f.log_prob(x, out=out)

        def score_torch():
            ref["lp"] = dist.log_prob(x.double())

        a, b = both(score_ours, None if args.no_torch else score_torch, iters, args.repeats)
        flop = float(M) * D * (D + 16)
        lines.append("log-prob  M = %-6d device  %s   %.2f TFLOP/s of the rule's %.2f GFLOP; %.2f M rows/s"
                     % (M, stat(a), flop / statistics.median(a) / 1e9, flop / 1e9, M / statistics.median(a) / 1e3))
        if b:
            lines.append("log-prob  M = %-6d torch   %s   max relative difference of the scores %.3e"
                         % (M, stat(b), ((out - ref["lp"]).abs() / ref["lp"].abs()).max().item()))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
