"""Timing of the pooled discriminative evaluation on the MI355X: 20 dialogs x 10 rounds x 100 options, T = 256, 37 regions at the
bert-base config (config.bert_base_enc_config), bf16, seeded synthetic weights and pools.

    python tools/bench_disc_rows.py --out profiles/disc_rows.txt [--dialogs 20 --repeats 3]

Figures (device events around the window, host clock for the whole calls, median of `repeats` with the spread; no profiler):
  rows launch   gstvd_disc_rows alone for one chunk of `rows_per_call` eval rows, and for `batch_size` sampled train rows
  pooled        evaluate_disc.score_batch on the pooled batch (pools on the device, one row launch per chunk)
  tensor        evaluate_disc.score_batch on the tensor batch of the same rows -- int64 [dialogs, 10, 100, 256] tokens / segments /
                mask on the host, shipped chunk by chunk, which is the path of the parent commit, unchanged here
  bytes         host-to-device bytes of the text tensors the pooled path does not move, and the size of the pools
The scores of the two paths are compared bit for bit on the way.  No figure is a pass / fail condition."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stat(xs):
    return "median %.4f ms (min %.4f, max %.4f over %d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dialogs", type=int, default=20)
    ap.add_argument("--rows-per-call", type=int, default=200)
    ap.add_argument("--batch-size", type=int, default=80)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_disc_rows needs an MI355X: no device, no number")
    from gst_visdial_amd import ops, disc_rows, evaluate_disc as ED
    from gst_visdial_amd.config import bert_base_enc_config
    from gst_visdial_amd.modules import VisualDialogEncoder
    dev = torch.device("cuda:0")
    cfg = bert_base_enc_config()
    d = tempfile.mkdtemp(prefix="gstvd_cfg_")
    with open(os.path.join(d, "enc.json"), "w") as f:
        json.dump(cfg, f)
    D, R, O, U, Lc, T, regions = a.dialogs, 10, 100, 18, 38, 256, 37
    params = dict(model_enc_config=os.path.join(d, "enc.json"), gpu_ids=[0], model="enc_only_a", mode="vd_eval_val", device=dev,
                  amd_precision="bf16", max_seq_len=T, visdial_tot_rounds=11, num_options=O)
    torch.manual_seed(0)
    enc = VisualDialogEncoder(params).eval().to(dev)
    g = torch.Generator().manual_seed(1)

    def utts(*shape):                                                     # 0-padded rows of 1 .. U ordinary ids
        ids = torch.randint(1000, cfg["vocab_size"], shape, generator=g)
        lens = torch.randint(1, shape[-1] + 1, shape[:-1], generator=g)
        return ids * (torch.arange(shape[-1]) < lens.unsqueeze(-1))
    gt = torch.randint(0, O, (D, R), generator=g)
    opts = utts(D, R, O, U)
    pools = dict(cap=utts(D, Lc), ques=utts(D, R, U), opts=opts, ans=torch.gather(opts, 2, gt.view(D, R, 1, 1).expand(D, R, 1, U)).squeeze(2),
                 gt_index=gt, image_feat=torch.randn(D, regions, cfg["v_feature_size"], generator=g),
                 image_loc=torch.rand(D, regions, 5, generator=g), image_mask=torch.ones(D, regions, dtype=torch.long))
    pooled = {k: v.to(dev) for k, v in pools.items()}
    n = D * R * O
    # the tensor batch of the same rows, on the host, as a loader would hand it over (built here by the kernel, copied back)
    item = ops.disc_rows(pooled["cap"], pooled["ques"], pooled["ans"], pooled["opts"], pooled["gt_index"],
                         *disc_rows._row_list(torch.arange(n, device=dev), R, O), T, 11, O, False)
    tensor_batch = {k: item[k].cpu().view((D, R, O) + tuple(item[k].shape[1:])) for k in ("tokens", "segments", "sep_indices", "mask", "hist_len")}
    tensor_batch.update({k: pools[k] for k in ("image_feat", "image_loc", "image_mask")})
    del item
    text_bytes = sum(tensor_batch[k].numel() * tensor_batch[k].element_size() for k in ("tokens", "segments", "sep_indices", "mask", "hist_len"))
    pool_bytes = sum(pools[k].numel() * pools[k].element_size() for k in disc_rows.POOL_KEYS)

    rd, rj, rs = disc_rows._row_list(torch.arange(a.rows_per_call, device=dev), R, O)
    chunk = lambda: ops.disc_rows(pooled["cap"], pooled["ques"], pooled["ans"], pooled["opts"], pooled["gt_index"], rd, rj, rs, T, 11, O, False)
    flat = torch.randperm(D * R * 3, generator=g)[:a.batch_size].to(dev)
    td, tj, ts = disc_rows._row_list(flat, R, 3)
    u_tok, u_neg = torch.rand(flat.numel(), T, device=dev), torch.rand(flat.numel(), device=dev)
    train = lambda: ops.disc_rows(pooled["cap"], pooled["ques"], pooled["ans"], pooled["opts"], pooled["gt_index"], td, tj, ts, T, 11, O, True,
                                  mask_prob=0.15, u_tok=u_tok, u_neg=u_neg)
    chunk(); train()
    torch.cuda.synchronize()
    chunk_ms = [window(chunk, a.iters) for _ in range(a.repeats)]
    train_ms = [window(train, a.iters) for _ in range(a.repeats)]

    score_p = lambda: ED.score_batch(enc, pooled, params, a.rows_per_call)
    score_t = lambda: ED.score_batch(enc, tensor_batch, params, a.rows_per_call)
    _, sp = wall(score_p)                                                 # warm-up of both: arena, every shape
    _, st = wall(score_t)
    same = torch.equal(sp.view(torch.int32), st.view(torch.int32))
    p_ms, t_ms = [], []
    for _ in range(a.repeats):                                            # alternating, so a drift of the machine meets both
        p_ms.append(wall(score_p)[0])
        t_ms.append(wall(score_t)[0])
    lines = [
        "discriminative rows from pools: %d dialogs x %d rounds x %d options = %d rows, T = %d, %d regions, bert-base config, bf16, MI355X"
        % (D, R, O, n, T, regions),
        "gstvd_disc_rows alone, %d eval rows (one chunk; device events, windows of %d):   %s" % (a.rows_per_call, a.iters, stat(chunk_ms)),
        "gstvd_disc_rows alone, %d sampled train rows, 2 negatives, mask_prob 0.15:       %s" % (flat.numel(), stat(train_ms)),
        "score_batch, pooled batch (%d chunks of %d rows; host clock, synchronised):      %s" % (-(-n // a.rows_per_call), a.rows_per_call, stat(p_ms)),
        "score_batch, tensor batch on the host (the parent commit's path, unchanged):      %s" % stat(t_ms),
        "pooled / tensor (medians): %.4f" % (statistics.median(p_ms) / statistics.median(t_ms)),
        "host-to-device text bytes per batch the pooled path does not move: %d (%.1f MB); the pools: %d bytes (%.2f MB), resident"
        % (text_bytes, text_bytes / 1e6, pool_bytes, pool_bytes / 1e6),
        "scores of the two paths bit-equal: %s" % same,
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
