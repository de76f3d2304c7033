"""Timing of the ranking metrics on the MI355X: 20 dialogs x 10 rounds x 100 options of fp32 scores resident on the device, with
ground-truth indices, round ids and dense relevance.

    python tools/bench_rank_metrics.py --out profiles/rank_metrics.txt [--whole-loop]

Figures (no profiler; no figure is a pass / fail condition):
  (a) device    DeviceRankMetrics.observe alone, device events over windows of `iters` launches
  (b) host      the parent commit's path on the same tensors, unchanged in this tree: SparseGTMetrics.observe + NDCG.observe, whole
                calls on the host clock, synchronised at the end, alternating with (c); medians of nine with min .. max, two runs
  (c) observe   DeviceRankMetrics.observe and nothing else on the host clock, NOT synchronised: what the loop waits for
  syncs         host synchronisations per batch of each form, counted with torch.cuda.set_sync_debug_mode("warn")
  --whole-loop  one evaluate_disc over the pooled bert-base batch of tools/bench_disc_rows.py, metrics="host" against "device"
The metric dicts of the two forms are printed next to each other on the way."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs):
    return "median %.4f ms (min %.4f .. max %.4f over %d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w)


def whole_loop(lines, dialogs, repeats):
    from gst_visdial_amd import evaluate_disc as ED
    from gst_visdial_amd.config import bert_base_enc_config
    from gst_visdial_amd.modules import VisualDialogEncoder
    dev = torch.device("cuda:0")
    cfg = bert_base_enc_config()
    d = tempfile.mkdtemp(prefix="gstvd_cfg_")
    with open(os.path.join(d, "enc.json"), "w") as f:
        json.dump(cfg, f)
    D, R, O, U, Lc, T, regions = dialogs, 10, 100, 18, 38, 256, 37
    params = dict(model_enc_config=os.path.join(d, "enc.json"), gpu_ids=[0], model="enc_only_a", mode="vd_eval_val", device=dev,
                  amd_precision="bf16", max_seq_len=T, visdial_tot_rounds=11, num_options=O)
    torch.manual_seed(0)
    enc = VisualDialogEncoder(params).eval().to(dev)
    g = torch.Generator().manual_seed(1)

    def utts(*shape):
        ids = torch.randint(1000, cfg["vocab_size"], shape, generator=g)
        lens = torch.randint(1, shape[-1] + 1, shape[:-1], generator=g)
        return ids * (torch.arange(shape[-1]) < lens.unsqueeze(-1))
    gt = torch.randint(0, O, (D, R), generator=g)
    opts = utts(D, R, O, U)
    pools = dict(cap=utts(D, Lc), ques=utts(D, R, U), opts=opts, ans=torch.gather(opts, 2, gt.view(D, R, 1, 1).expand(D, R, 1, U)).squeeze(2),
                 gt_index=gt, image_feat=torch.randn(D, regions, cfg["v_feature_size"], generator=g),
                 image_loc=torch.rand(D, regions, 5, generator=g), image_mask=torch.ones(D, regions, dtype=torch.long))
    batch = {k: v.to(dev) for k, v in pools.items()}
    batch["gt_relevance"] = (torch.randint(0, 6, (D, O), generator=g) * (torch.rand(D, O, generator=g) < 0.15)).float() / 5
    batch["gt_relevance"][:, 0] += 0.2
    batch["round_id"] = torch.randint(1, R + 1, (D, 1), generator=g)

    def run(form):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = ED.evaluate_disc(enc, [batch], params, D, metrics=form)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, m
    _, mh = run("host")
    _, md = run("device")
    rows = ED.score_batch(enc, batch, params).reshape(-1, O).cpu()
    tied = sum(int(row.unique().numel() < row.numel()) for row in rows)
    h_ms, d_ms = [], []
    for _ in range(repeats):
        h_ms.append(run("host")[0])
        d_ms.append(run("device")[0])
    lines += ["evaluate_disc, one pooled batch of %d dialogs x %d x %d at the bert-base config, bf16 (host clock, synchronised, alternating):" % (D, R, O),
              "  metrics=\"host\":    %s" % stat(h_ms), "  metrics=\"device\":  %s" % stat(d_ms),
              "  device / host (medians): %.4f" % (statistics.median(d_ms) / statistics.median(h_ms)),
              "  host dict   %s" % json.dumps(mh, sort_keys=True), "  device dict %s" % json.dumps(md, sort_keys=True),
              "  lists that hold two equal scores (random weights, bf16: the two forms rank those by different rules): %d of %d" % (tied, rows.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dialogs", type=int, default=20)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--whole-loop", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_metrics needs an MI355X: no device, no number")
    from gst_visdial_amd.metrics import SparseGTMetrics, NDCG, DeviceRankMetrics
    dev = torch.device("cuda:0")
    B, R, O = a.dialogs, 10, 100
    g = torch.Generator().manual_seed(0)
    scores = (torch.randn(B, R, O, generator=g) * 3).to(dev)
    gt = torch.randint(0, O, (B, R), generator=g)
    rid = torch.randint(1, R + 1, (B, 1), generator=g)
    rel = (torch.randint(0, 6, (B, O), generator=g) * (torch.rand(B, O, generator=g) < 0.15)).float() / 5
    rel[:, 0] += 0.2
    gt_d, rid_d, rel_d = gt.to(dev), rid.to(dev), rel.to(dev)
    m = DeviceRankMetrics(dev)
    sparse, ndcg = SparseGTMetrics(), NDCG()

    def host_form():
        sparse.observe(scores, gt)
        ndcg.observe(scores[torch.arange(B), rid.squeeze(1) - 1, :], rel)

    observe = lambda: m.observe(scores, gt, rel, rid)                     # targets on the host: uploaded once per batch, as the loops do
    observe_resident = lambda: m.observe(scores, gt_d, rel_d, rid_d)
    # the library call alone: what observe() launches, on operands built once
    from gst_visdial_amd import ops
    from gst_visdial_amd.metrics import _discounts
    n = B * R
    rel_index = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rel_index[torch.arange(B, device=dev) * R + rid_d.view(-1) - 1] = torch.arange(B, dtype=torch.int32, device=dev)
    own = dict(gt_index=gt_d.view(-1), relevance=rel_d, rel_index=rel_index, discounts=_discounts(dev, O),
               gt_rank=torch.empty(n, dtype=torch.int32, device=dev), ndcg=torch.empty(n, dtype=torch.float32, device=dev),
               acc=torch.zeros(ops.RANK_ACC_SLOTS, dtype=torch.int64, device=dev))
    call_alone = lambda: ops.rank_metrics(scores.view(n, O), **own)
    host_form(); observe(); observe_resident(); call_alone()
    torch.cuda.synchronize()
    md = m.retrieve()
    mh = dict(sparse.retrieve(), **ndcg.retrieve())

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters
    lines = ["ranking metrics: %d dialogs x %d rounds x %d options = %d lists of fp32 scores resident on the device, MI355X" % (B, R, O, B * R)]
    for run in (1, 2):
        a_ms = [window(observe_resident) for _ in range(3)]
        k_ms = [window(call_alone) for _ in range(3)]
        m.reset()
        b_ms, c_ms = [], []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_form()
            torch.cuda.synchronize()
            b_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            observe()
            c_ms.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
        sparse.reset(); ndcg.reset(); m.reset()
        lines += ["run %d" % run,
                  "  (a) DeviceRankMetrics.observe, targets resident (device events, windows of %d launches): %s" % (a.iters, stat(a_ms)),
                  "      of which ops.rank_metrics alone (the list launch and the one-wave sum launch), operands built once:      %s" % stat(k_ms),
                  "  (b) SparseGTMetrics.observe + NDCG.observe, the parent commit's path (host clock, whole calls):    %s" % stat(b_ms),
                  "  (c) DeviceRankMetrics.observe with its three uploads, host clock, not synchronised:                %s" % stat(c_ms)]
    try:
        lines.append("host synchronisations per batch (torch sync debug mode): host form %d, device observe %d, device retrieve %d"
                     % (count_syncs(host_form), count_syncs(observe), count_syncs(lambda: m.retrieve())))
    except Exception as e:                                                # the counter is a torch debugging aid: say so, do not guess
        lines.append("host synchronisations per batch: not counted (%s: %s)" % (type(e).__name__, e))
    lines += ["metric dicts of one batch: host   %s" % json.dumps(mh, sort_keys=True),
              "                           device %s" % json.dumps(md, sort_keys=True)]
    if a.whole_loop:
        whole_loop(lines, a.dialogs, 3)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
