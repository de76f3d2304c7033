"""Fixture of the ranking metrics: tests/golden/rank_metrics.npz.

Runs in the build container only.  It loads the reference's own utils/visdial_metrics.py (the path of oracle.ref_harness) and
copies none of its text: `scores_to_ranks`, `SparseGTMetrics` and `NDCG` run as the reference wrote them on three batches of
[4, 10, 100] fp32 scores with gt_option_inds [4, 10], round_id [4] and gt_relevance [4, 100].  Only arrays are stored:

  scores [3, 4, 10, 100] fp32, gt_option_inds [3, 4, 10] int64, round_id [3, 4] int64, gt_relevance [3, 4, 100] fp32;
  ranks [3, 4, 10, 100] int64 (scores_to_ranks), gt_ranks [3, 40] int64 (what SparseGTMetrics.observe appended),
  ndcg [3, 4] fp32 (the ratio of each dialog: NDCG.observe of that dialog alone, its numerator),
  metrics [3, 6] float64: the dict after each batch in the order r@1, r@5, r@10, mean, mrr, ndcg, and
  metrics_final [6]: the dict at the end.

Two conditions are asserted here, because without them the reference gives no rule to compare with: no list holds two equal scores
(its scores.sort(1, descending=True) is not stable, so the rank of tied options is implementation-defined), and every relevance
row has k >= 1 nonzero entries (k = 0 makes its ratio 0 / 0 and its running sum NaN).

    python tools/make_golden_rank_metrics.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                   # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, GOLDEN                # noqa: E402

NAMES = ("r@1", "r@5", "r@10", "mean", "mrr", "ndcg")
BATCHES, B, R, O = 3, 4, 10, 100


def reference_metrics():
    spec = importlib.util.spec_from_file_location("ref_visdial_metrics", os.path.join(RH.REFERENCE_ROOT, "utils", "visdial_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_metrics()
    g = torch.Generator().manual_seed(20)
    scores = torch.randn(BATCHES, B, R, O, generator=g) * 3.0
    # a few lists shaped like saturated probabilities: close values, still distinct
    scores[1, 2] = 0.5 + torch.stack([torch.randperm(O, generator=g) for _ in range(R)]).float() * 2.0 ** -20
    gt = torch.randint(0, O, (BATCHES, B, R), generator=g)
    rid = torch.randint(1, R + 1, (BATCHES, B), generator=g)
    # dense annotations: n / 5 for n of 5 annotators, most options 0; one row with every option relevant
    votes = torch.randint(0, 6, (BATCHES, B, O), generator=g) * (torch.rand(BATCHES, B, O, generator=g) < 0.15)
    rel = votes.float() / 5
    rel[2, 1] = (torch.randint(1, 6, (O,), generator=g)).float() / 5
    for l in scores.reshape(-1, O):
        assert l.unique().numel() == O, "two equal scores in a list: the reference's ranks are no rule"
    assert int((rel != 0).sum(-1).min()) >= 1, "a relevance row with k = 0: the reference's sum turns NaN"

    sparse, ndcg = ref.SparseGTMetrics(), ref.NDCG()
    out = dict(scores=scores.numpy(), gt_option_inds=gt.numpy(), round_id=rid.numpy(), gt_relevance=rel.numpy())
    ranks, gt_ranks, ratios, per_batch = [], [], [], []
    for i in range(BATCHES):
        ranks.append(ref.scores_to_ranks(scores[i]).numpy())
        seen = len(sparse._rank_list)
        sparse.observe(scores[i], gt[i])
        gt_ranks.append(np.asarray(sparse._rank_list[seen:], dtype=np.int64))
        at_round = scores[i][torch.arange(B), rid[i] - 1, :]
        ndcg.observe(at_round, rel[i])
        row = []
        for b in range(B):
            one = ref.NDCG()
            one.observe(at_round[b:b + 1], rel[i][b:b + 1])
            row.append(np.float32(one._ndcg_numerator))
        ratios.append(np.asarray(row, dtype=np.float32))
        m = dict(sparse.retrieve(reset=False))
        m.update(ndcg.retrieve(reset=False))
        per_batch.append([m[k] for k in NAMES])
    final = dict(sparse.retrieve(reset=True))
    final.update(ndcg.retrieve(reset=True))
    out.update(ranks=np.stack(ranks), gt_ranks=np.stack(gt_ranks), ndcg=np.stack(ratios),
               metrics=np.asarray(per_batch, dtype=np.float64), metrics_final=np.asarray([final[k] for k in NAMES], dtype=np.float64))
    path = os.path.join(GOLDEN, "rank_metrics.npz")
    write_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
