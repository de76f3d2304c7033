#!/usr/bin/env python3
"""Per-launch device times of the selection kernels at the workload's shapes (V = 30522), for before / after comparisons of one
library against another: medians of `--steps` single launches between HIP events (ops.Profiler where the wrapper records them) with
min .. max.  beam_step 16 x 5 rows; topk_logp 288 rows, K = 8; rows_argmax and the fused vocab_argmax at n = 38 (H = 768);
cos_topk on both routes (V 65 713 x D 300: 8 sources on "few", 16 384 sources on "many"); the sampler at 16 rows by setting.

    python tools/select_probe.py [--steps 40] [--warmup 5]"""
import argparse
import statistics

import torch
from ln_digest import DEV, draw                     # noqa: F401  (also puts the repository root on sys.path)
from gst_visdial_amd import ops

V = 30522


def report(name, us):
    print("%-44s median %9.1f us  (min %9.1f .. max %9.1f)" % (name, statistics.median(us), min(us), max(us)), flush=True)


def profiled(name, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    with ops.Profiler() as p:
        for _ in range(steps):
            fn()
    torch.cuda.synchronize()
    report(name, [r[3].elapsed_time(r[4]) * 1e3 for r in p.records])


def evented(name, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    report(name, [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(7)
    for dtype, tn in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        B, K = 16, 5
        x = draw(g, B * K, V + 6, dtype=dtype, scale=2.5)[:, :V]
        s_in, done = draw(g, B, K), torch.zeros(B, K, dtype=torch.int32, device=DEV)
        s_out, d_out, parent = torch.zeros_like(s_in), torch.zeros_like(done), torch.zeros_like(done)
        ids, ws = torch.zeros(1, B * K, dtype=torch.int64, device=DEV), ops.beam_workspace(B, K, DEV)
        profiled("beam_step %s 16 x 5 x %d" % (tn, V), lambda: ops.beam_step(x, s_in, done, s_out, d_out, parent, ids, 0, ws, 102, 0),
                 a.steps, a.warmup)
        M = 288
        t, lse = draw(g, M, V + 2, dtype=dtype, scale=2.5)[:, :V], draw(g, M) + 9.0
        tid, tlp = torch.zeros(M, 8, dtype=torch.int64, device=DEV), torch.zeros(M, 8, device=DEV)
        profiled("topk_logp %s 288 x %d K=8" % (tn, V), lambda: ops.topk_logp(t, lse, M, V, 8, tid, tlp), a.steps, a.warmup)
        z = draw(g, 38, V + 2, dtype=dtype, scale=2.5)[:, :V]
        profiled("rows_argmax %s 38 x %d" % (tn, V), lambda: ops.rows_argmax(z, V), a.steps, a.warmup)
        s = draw(g, 16, V + 6, dtype=dtype, scale=2.5)[:, :V]
        u, out = torch.rand(16, generator=g).clamp_min(1e-6).to(DEV), torch.zeros(16, dtype=torch.int64, device=DEV)
        lp = torch.zeros(16, device=DEV)
        for name, k, p in (("k=7", 7, 0.0), ("k=64", 64, 0.0), ("p=0.9", 0, 0.9), ("k=64 p=0.8", 64, 0.8)):
            evented("sample_topk %s 16 x %d %s" % (tn, V, name), lambda: ops.sample_topk(s, 0.7, k, u, out, top_p=p), a.steps, a.warmup)
        evented("sample_topk_scored %s 16 x %d k=7" % (tn, V), lambda: ops.sample_topk_scored(s, 0.7, 7, u, out, lp), a.steps, a.warmup)
    H, n = 768, 38
    xb, w, bias = draw(g, n, H, dtype=torch.bfloat16), draw(g, V + 2, H, dtype=torch.bfloat16, scale=0.05), draw(g, V + 2)
    wsb = torch.empty(ops.vocab_argmax_ws_bytes(n, V), dtype=torch.uint8, device=DEV)
    profiled("vocab_argmax fused n=38 H=768", lambda: ops.vocab_argmax_fused(xb, w, bias, V, n=n, ws=wsb), a.steps, a.warmup)
    Vs, D = 65713, 300
    e = torch.randn(Vs // 4 + 1, D, generator=g).repeat_interleave(4, 0)[:Vs] + 0.6 * torch.randn(Vs, D, generator=g)
    ehat = (e / e.norm(dim=1, keepdim=True)).to(DEV)
    for route, ns in (("few", 8), ("many", 16384)):
        src = torch.randint(0, Vs, (ns,), generator=g).to(torch.int32).to(DEV)
        idx, val = torch.zeros(ns, 10, dtype=torch.int32, device=DEV), torch.zeros(ns, 10, device=DEV)
        wsc = torch.empty(max(ops.cos_topk_ws_bytes(ns, Vs, 10), 8), dtype=torch.uint8, device=DEV)
        profiled("cos_topk %s %d sources V=%d D=%d" % (route, ns, Vs, D),
                 lambda: ops.cos_topk(ehat, src, K=10, threshold=0.5, route=route, idx=idx, val=val, ws=wsc), min(a.steps, 15), 2)


if __name__ == "__main__":
    main()
