"""Timing of the coreference attack's two kernels on one MI355X -> profiles/synonym.txt.  Recorded, not gated.

Synthetic vectors of the published counter-fitted shape (V 65 713, D 300, gaussian, unit rows), K 10, threshold 0.5:
  (a) the full table (every row a source): gstvd_cos_topk on its many-sources route, next to the plain torch form on the same
      device -- chunks of 4096 sources, topk(Ehat[chunk] @ Ehat.T, K + 1) in fp32 -- with the peak device memory of each;
  (b) a lookup of 8 sources: the few-sources route (split targets + merge launch), next to torch's topk(Ehat[src] @ Ehat.T, K + 1);
  (c) the full table forced through the few-sources route (for the record: the route the host does not pick at this size);
  (d) gstvd_subseq_replace on 100 context rows of T 256 with 4 substitutions each, ids only and with the three recomputed
      tensors.
Method: every shape warmed up; every figure the median of `--steps` (>= 5) individually timed iterations (HIP events around each,
the device idle before each) with min..max; the kernel and the torch form of a pair are timed ALTERNATELY.  The file also states
how far the two forms agree (torch's product is a BLAS GEMM: another summation order).

    python tools/bench_synonym.py [--steps 7] [--warmup 2] [--out profiles/synonym.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, D, K, THRESHOLD, CHUNK, N_LOOKUP = 65713, 300, 10, 0.5, 4096, 8
ROWS, T, N_SUBS = 100, 256, 4


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fns, steps, warmup):
    """The callables of `fns` timed alternately: -> one (median, min, max) in ms per callable."""
    for _ in range(warmup):
        for f in fns:
            f()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for i, f in enumerate(fns):
            ms[i].append(once(f))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def line(tag, t, extra=""):
    return "%-78s median %10.3f ms  (min %10.3f .. max %10.3f)%s" % (tag, t[0], t[1], t[2], extra)


def torch_topk(ehat, src, chunk):
    """The plain torch form: per chunk of sources the K + 1 largest of the fp32 product (rank 0 is the source itself)."""
    idx, val = [], []
    for s in range(0, src.numel(), chunk):
        v, i = torch.topk(ehat[src[s:s + chunk].long()] @ ehat.t(), K + 1, dim=1)
        idx.append(i)
        val.append(v)
    return torch.cat(idx), torch.cat(val)


def agreement(idx, val, t_idx, t_val, src):
    """Share of the kernel's used slots whose target torch also lists for that row, and the largest value difference there."""
    used = idx >= 0
    hit = (idx.long().unsqueeze(2) == t_idx.unsqueeze(1)) & used.unsqueeze(2)
    found = hit.any(2)
    dv = (val.unsqueeze(2) - t_val.unsqueeze(1)).abs()[hit]
    return int(used.sum()), int(found.sum()), (dv.max().item() if dv.numel() else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synonym.txt"))
    a = ap.parse_args()
    if a.steps < 5:
        raise SystemExit("--steps must be at least 5")
    from gst_visdial_amd import ops
    from gst_visdial_amd.synonyms import unit_rows
    dev = torch.device("cuda:0")
    out = ["coreference attack kernels, synthetic gaussian unit rows V %d x D %d, K %d, threshold %.1f (%s); %d timed iterations "
           "after %d warm-up" % (V, D, K, THRESHOLD, torch.cuda.get_device_name(0), a.steps, a.warmup)]
    rng = np.random.RandomState(0)
    centres = rng.standard_normal((V // 4 + 1, D)).astype(np.float32)
    emb = np.repeat(centres, 4, axis=0)[:V] + 0.6 * rng.standard_normal((V, D)).astype(np.float32)      # ~3 neighbours >= 0.5 per row
    ehat = unit_rows(emb).to(dev)
    all_src = torch.arange(V, dtype=torch.int32, device=dev)
    idx = torch.empty(V, K, dtype=torch.int32, device=dev)
    val = torch.empty(V, K, dtype=torch.float32, device=dev)

    many = lambda: ops.cos_topk(ehat, None, K=K, threshold=THRESHOLD, route="many", idx=idx, val=val)      # noqa: E731
    plain = lambda: torch_topk(ehat, all_src, CHUNK)                                                        # noqa: E731
    ta, tt = timed([many, plain], a.steps, a.warmup)
    pk, pt = peak_mib(many), peak_mib(plain)
    out.append(line("(a) full table, gstvd_cos_topk many-sources route", ta, "  peak %8.1f MiB" % pk))
    out.append(line("(a) full table, torch: chunks of %d, topk(Ehat[chunk] @ Ehat.T, K + 1) fp32" % CHUNK, tt, "  peak %8.1f MiB" % pt))
    many()
    t_idx, t_val = plain()
    used, found, dv = agreement(idx[:8192], val[:8192], t_idx[:8192], t_val[:8192], all_src[:8192])
    out.append("    rows 0..8191: %d used slots, %d of them in torch's K + 1 list; largest |value difference| there %.3e; "
               "%.2f neighbours per row" % (used, found, dv, used / 8192.0))
    out.append("    the %d x %d fp32 matrix the reference stores would be %.1f GiB; the table and this result are %.1f MiB"
               % (V, V, V * V * 4 / 2.0 ** 30, (V * D * 4 + V * K * 8) / 2.0 ** 20))

    src = torch.tensor(rng.randint(0, V, size=N_LOOKUP), dtype=torch.int32, device=dev)
    ws = torch.empty(ops.cos_topk_ws_bytes(N_LOOKUP, V, K), dtype=torch.uint8, device=dev)
    few = lambda: ops.cos_topk(ehat, src, K=K, threshold=THRESHOLD, route="few", ws=ws)                     # noqa: E731
    plain8 = lambda: torch_topk(ehat, src, CHUNK)                                                           # noqa: E731
    tb, tbt = timed([few, plain8], max(a.steps, 11), a.warmup)
    out.append(line("(b) lookup of %d sources, gstvd_cos_topk few-sources route (2 launches)" % N_LOOKUP, tb,
                    "  peak %8.1f MiB" % peak_mib(few)))
    out.append(line("(b) lookup of %d sources, torch: topk(Ehat[src] @ Ehat.T, K + 1) fp32" % N_LOOKUP, tbt,
                    "  peak %8.1f MiB" % peak_mib(plain8)))
    fi, fv = few()
    same = bool(torch.equal(fi, idx[src.long()])) and bool(torch.equal(fv, val[src.long()]))
    out.append("    the lookup's rows equal the full table's rows bit for bit: %s" % same)

    (tc,) = timed([lambda: ops.cos_topk(ehat, None, K=K, threshold=THRESHOLD, route="few")], 5, 1)
    out.append(line("(c) full table forced through the few-sources route", tc))

    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1000, 1040, (ROWS, T), generator=g)
    ids[:, 0] = 101
    ids[:, 12::13] = 102
    ids[:, 230:] = 0
    plans = []
    for r in range(ROWS):
        plans.append([(int(u), [int(ids[r, 13 * int(u) + 3])], [2000 + r, 2001, 2002][:1 + (r + int(u)) % 3]) for u in (0, 3, 8, 15)])
    d_ids = ids.to(dev)
    packed = ops.pack_substitutions(plans, dev)
    o, n = torch.empty_like(d_ids), torch.empty(ROWS, dtype=torch.int32, device=dev)
    seg, att = torch.empty_like(d_ids), torch.empty(ROWS, T, dtype=torch.float32, device=dev)
    sepi = torch.empty(ROWS, 25, dtype=torch.int64, device=dev)
    td, tdr = timed([lambda: ops.subseq_replace(d_ids, packed, out=o, n_replaced=n),
                     lambda: ops.subseq_replace(d_ids, packed, out=o, n_replaced=n, segments=seg, sep_indices=sepi, att_mask=att)],
                    max(a.steps, 11), a.warmup)
    out.append(line("(d) gstvd_subseq_replace, %d rows x T %d, %d substitutions each, ids only" % (ROWS, T, N_SUBS), td))
    out.append(line("(d) the same with segments, separator positions and mask recomputed", tdr))
    out.append("    matches replaced: %d in %d rows" % (int(n.sum()), ROWS))
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
