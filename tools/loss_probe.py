#!/usr/bin/env python3
"""Per-launch device times of the loss, optimizer and cast kernels at the workload's shapes, for before / after comparisons of one
library against another: medians of `--steps` single launches between HIP events with min .. max, bf16 first.  V = 30522; the
train step's 16 x 25 = 400 logits rows (ce_fwd, ce_bwd, ce_bwd_rows, distill_fwd / _bwd at K = 8, alpha 0.5, tau 2), topk_logp on
288 rows at K = 8, the listwise step's E = 2 rounds of G = 100 candidates with U = 25 (rank_loss, answer_scores: 5000 logits rows),
the masked-region loss on 128 rows of C = 1601, AdamW and the fp32 -> bf16 cast over 64 Mi elements in 400 segments.

    python tools/loss_probe.py [--steps 40] [--warmup 5]"""
import argparse
import statistics

import torch
from ln_digest import DEV, draw                     # noqa: F401  (also puts the repository root on sys.path)
from gst_visdial_amd import ops

V, LD = 30522, 30524


def evented(name, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    print("%-44s median %9.1f us  (min %9.1f .. max %9.1f)" % (name, statistics.median(us), min(us), max(us)), flush=True)


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def logits_cases(tn, dtype, a):
    g = torch.Generator(device=DEV).manual_seed(7)
    E, G, U, M, K = 2, 100, 25, 400, 8
    n = E * G
    x = (torch.randn(n * U, LD, generator=g, device=DEV) * 2.5).to(dtype)[:, :V]
    lab = torch.randint(1, V, (M,), generator=g, device=DEV)
    lab[::9] = 0                                            # [PAD] positions
    row_loss, lse_all, stats, gs = zeros(M), zeros(n * U), zeros(3), torch.ones(1, device=DEV)
    ops.ce_fwd(x, torch.randint(1, V, (n * U,), generator=g, device=DEV), n * U, V, zeros(n * U), lse_all, zeros(3))
    lse = lse_all[:M].clone()
    dl = torch.zeros(M, LD, dtype=dtype, device=DEV)[:, :V]
    evented("ce_fwd %s %d x %d" % (tn, M, V), lambda: ops.ce_fwd(x, lab, M, V, row_loss, lse, stats), a.steps, a.warmup)
    evented("ce_bwd %s %d x %d" % (tn, M, V), lambda: ops.ce_bwd(x, lab, lse, stats, gs, True, M, V, dl), a.steps, a.warmup)
    gr = torch.rand(M, generator=g, device=DEV)
    evented("ce_bwd_rows %s %d x %d" % (tn, M, V), lambda: ops.ce_bwd_rows(x, lab, lse, gr, M, V, dl), a.steps, a.warmup)
    sid, slp = ops.topk_logp(x, lse, M, V, K)
    l, kd, lt, st = zeros(M), zeros(M), zeros(M), zeros(3)
    evented("distill_fwd %s %d x %d K=8" % (tn, M, V), lambda: ops.distill_fwd(x, lab, sid, slp, M, V, 0.5, 2.0, row_loss, l, kd, lt, st),
            a.steps, a.warmup)
    evented("distill_bwd %s %d x %d K=8" % (tn, M, V), lambda: ops.distill_bwd(x, lab, sid, slp, lse, lt, st, gs, M, V, 0.5, 2.0, dl),
            a.steps, a.warmup)
    tid, tlp = torch.zeros(288, K, dtype=torch.int64, device=DEV), zeros(288, K)
    evented("topk_logp %s 288 x %d K=8" % (tn, V), lambda: ops.topk_logp(x, lse_all, 288, V, K, tid, tlp), a.steps, a.warmup)
    ids = torch.randint(1000, 30000, (n, U), generator=g, device=DEV)
    ids[:, 18:] = 0
    rel = ((torch.rand(E, G, generator=g, device=DEV) < 0.1).float() * 0.5).reshape(-1)
    sc, p, rl, gt = zeros(n), zeros(n), zeros(E), zeros(n * U)
    evented("rank_loss %s %d x %d x %d" % (tn, E, G, U), lambda: ops.rank_loss(x, lse_all, ids, rel, E, G, U, 1.0, sc, p, rl, gt, st),
            a.steps, a.warmup)
    evented("answer_scores %s %d x %d" % (tn, n, U), lambda: ops.answer_scores(x, lse_all, ids, n, U, sc), a.steps, a.warmup)
    rows, C = 128, 1601
    s = draw(torch.Generator().manual_seed(8), rows, C, dtype=dtype, scale=2.5)
    t = torch.softmax(draw(torch.Generator().manual_seed(9), rows, C, scale=2.0), -1).contiguous()
    krl, klse, kst, kd_ = zeros(rows), zeros(rows), zeros(3), torch.zeros(rows, C, dtype=dtype, device=DEV)
    evented("kl_fwd %s %d x %d" % (tn, rows, C), lambda: ops.kl_fwd(s, t, rows, C, krl, klse, kst), a.steps, a.warmup)
    evented("kl_bwd %s %d x %d" % (tn, rows, C), lambda: ops.kl_bwd(s, t, klse, kst, gs, True, rows, C, kd_), a.steps, a.warmup)


def flat_cases(a, n=64 << 20, nseg=400):
    g = torch.Generator(device=DEV).manual_seed(11)
    p, gr, m = (torch.randn(n, generator=g, device=DEV) for _ in range(3))
    v, sh = torch.rand(n, generator=g, device=DEV) * 0.01, zeros(n, dtype=torch.bfloat16)
    seg_end = (torch.arange(1, nseg + 1, dtype=torch.int64) * (n // nseg // 64 * 64)).to(DEV)
    seg_end[-1] = n
    hp = torch.tensor([[1e-4, 0.01], [1e-4, 0.0]] * (nseg // 2), device=DEV).reshape(-1).contiguous()
    step = torch.tensor([3.0], device=DEV)
    gr_b = gr.to(torch.bfloat16)
    evented("adamw bf16 grad %d Mi elements" % (n >> 20), lambda: ops.adamw(p, gr_b, m, v, sh, seg_end, hp, step), a.steps, a.warmup)
    evented("adamw f32 grad %d Mi elements" % (n >> 20), lambda: ops.adamw(p, gr, m, v, sh, seg_end, hp, step), a.steps, a.warmup)
    evented("cast f32 -> bf16 %d Mi elements" % (n >> 20), lambda: ops.cast(p, sh), a.steps, a.warmup)
    evented("cast bf16 -> f32 %d Mi elements" % (n >> 20), lambda: ops.cast(sh, gr), a.steps, a.warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for dtype, tn in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        logits_cases(tn, dtype, a)
        torch.cuda.empty_cache()
    flat_cases(a)


if __name__ == "__main__":
    main()
