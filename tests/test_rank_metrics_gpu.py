"""metrics="device" end to end: evaluate.evaluate on the tiny enc_dec model, evaluate_disc.evaluate_disc on tests/golden/tiny_disc.npz
(tensor batch and pooled batch) and attack.evaluate_attack (fgsm), each against metrics="host" on the same scores.  Without two
equal scores in a list both forms rank alike, so r@k and the mean rank are EQUAL; mrr differs by the order of an fp32 sum of n
reciprocals (n 2^-24 relative) and ndcg by two fp32 sums of k terms and a division per dialog (2 (k + 1) 2^-24).  With a tie the
device form follows the stable rule."""
import numpy as np
import pytest
import torch

import exact_disc_rows as XD
import exact_rank_metrics as X
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
OPTIONS = 5


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def _no_ties(scores):
    s = scores.reshape(-1, scores.shape[-1]).cpu()
    return all(row.unique().numel() == row.numel() for row in s)


def _compare(host, dev, n, k_max):
    assert set(host) == set(dev) == {"r@1", "r@5", "r@10", "mean", "mrr", "ndcg"}, (host, dev)
    for k in ("r@1", "r@5", "r@10", "mean"):
        assert host[k] == dev[k], (k, host[k], dev[k])
    print("mrr host %.9g device %.9g; ndcg host %.9g device %.9g" % (host["mrr"], dev["mrr"], host["ndcg"], dev["ndcg"]))
    assert abs(host["mrr"] - dev["mrr"]) <= n * EPS * host["mrr"]
    assert abs(host["ndcg"] - dev["ndcg"]) <= 2 * (k_max + 1) * EPS


# ---------------------------------------------------------------------------------------------------------------- generative
@pytest.fixture(scope="module")
def gen():
    """The tiny enc_dec model and 2 dialogs x 10 rounds x 5 options as two batches of one dialog, no two equal scores in a round."""
    from gst_visdial_amd import evaluate as EV
    s = sc()
    model, params, _ = s.build_tiny_model("fp32", DEV, mode="vd_eval_val")
    model.eval()
    params = dict(params, device=torch.device(DEV), vd_version="1.0")
    batches = []
    for i, b in enumerate(s.evalset100_batches(load_npz("tiny_evalset100.npz"), dialogs_per_batch=1)[:2]):
        b = {k: (v[:, :, :OPTIONS].contiguous() if v.dim() == 4 else v) for k, v in b.items()}
        b["gt_option_inds"] = b["gt_option_inds"] % OPTIONS
        b["gt_relevance"] = b["gt_relevance"][:, :OPTIONS].clone()
        b["gt_relevance"][:, 0] += 0.2                                                       # k >= 1
        b["image_id"] = torch.tensor([100 + i])
        for _ in range(4):                                                                   # the precondition: perturb until it holds
            if _no_ties(EV.score_batch(model, b, params["device"])):
                break
            b["dec_input_ids"][:, :, 1:, 1] += torch.arange(1, OPTIONS).view(1, 1, -1)
        assert _no_ties(EV.score_batch(model, b, params["device"]))
        batches.append(b)
    return model, params, batches


def test_evaluate_device_metrics_equal_host_metrics(gen):
    from gst_visdial_amd import evaluate as EV
    model, params, batches = gen
    _, host = EV.evaluate(model, batches, params)
    json_, dev = EV.evaluate(model, batches, params, metrics="device")
    assert json_ == []
    _compare(host, dev, 20, OPTIONS)


def test_evaluate_device_ranks_json_equals_host(gen):
    from gst_visdial_amd import evaluate as EV
    model, params, batches = gen
    one_round = [{k: (v[:, 3:4].contiguous() if v.dim() >= 3 and k.startswith(("enc_input", "enc_seg", "enc_att", "dec_")) else v)
                  for k, v in b.items()} for b in batches]
    host, m_h = EV.evaluate(model, one_round, params, mode="vd_eval_test")
    dev, m_d = EV.evaluate(model, one_round, params, mode="vd_eval_test", metrics="device")
    assert m_h == m_d == {} and len(dev) == 2 and host == dev
    assert sorted(dev[0]["ranks"]) == list(range(1, OPTIONS + 1)) and dev[1]["image_id"] == 101


def test_a_deliberately_tied_round_follows_the_stable_rule(gen):
    from gst_visdial_amd import evaluate as EV
    from gst_visdial_amd.metrics import DeviceRankMetrics, scores_to_ranks_device
    model, params, batches = gen
    b = batches[0]
    scores = EV.score_batch(model, b, params["device"]).clone()
    scores[0, 3, 4] = scores[0, 3, 1]                                                        # options 1 and 4 of round 3 tie ...
    scores[0, 6, :] = scores[0, 6, 2]                                                        # ... and all of round 6
    gt = b["gt_option_inds"].clone()
    gt[0, 3], gt[0, 6] = 4, 3
    ranks = scores_to_ranks_device(scores).cpu()
    want = X.ranks_rule(scores.reshape(-1, OPTIONS).cpu().numpy())
    assert np.array_equal(ranks.reshape(-1, OPTIONS).numpy(), want)
    assert ranks[0, 3, 4] == ranks[0, 3, 1] + 1 and ranks[0, 6].tolist() == [1, 2, 3, 4, 5]
    m = DeviceRankMetrics(DEV)
    out = m.observe(scores, gt, b["gt_relevance"], b["round_id"])
    gt_rank = out["gt_rank"].cpu()
    assert gt_rank[3] == ranks[0, 3, 4] and gt_rank[6] == 4
    st = m.state()["slots"]
    assert st[X.N_SPARSE] == 10 and sum(st[X.HIST:]) == 10 and st[X.N_GT_SKIPPED] == 0 and st[X.N_NDCG] == 1 and st[X.N_CALLS] == 1
    got = m.retrieve()
    assert abs(got["mean"] - sum(int(want[l, int(gt[0, l])]) for l in range(10)) / 10.0) <= 1e-6
    assert int(m.acc.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------------ discriminative
def test_evaluate_disc_device_equals_host_on_the_tensor_batch():
    from gst_visdial_amd import evaluate_disc as ED
    enc, params, fx = sc().build_tiny_disc_encoder("fp32", DEV)
    b = sc().disc_batch(fx)
    scores = ED.score_batch(enc, b, params, rows_per_call=17)
    assert _no_ties(scores)                                                                  # the precondition
    host = ED.evaluate_disc(enc, [b, b], params, 2, rows_per_call=17)
    dev = ED.evaluate_disc(enc, [b, b], params, 2, rows_per_call=17, metrics="device")
    n = 2 * scores.shape[0] * scores.shape[1]
    _compare(host, dev, n, scores.shape[2])
    test_params = dict(params, mode="vd_eval_test")
    one = {k: (v[:, :1].contiguous() if k in ("tokens", "segments", "sep_indices", "mask", "hist_len") else v) for k, v in b.items()}
    one["image_id"] = torch.tensor([7, 8])
    assert ED.evaluate_disc(enc, [one], test_params, 2) == ED.evaluate_disc(enc, [one], test_params, 2, metrics="device")


def _pools(gen_, D, R, O, U, LC):
    row = lambda width: XD._row(width, int(gen_.integers(1, width + 1)), gen_)
    cap = np.stack([row(LC) for _ in range(D)])
    ques = np.stack([np.stack([row(U) for _ in range(R)]) for _ in range(D)])
    opts = np.stack([np.stack([np.stack([row(U) for _ in range(O)]) for _ in range(R)]) for _ in range(D)])
    gt = gen_.integers(0, O, (D, R)).astype(np.int64)
    ans = np.stack([np.stack([opts[d, j, gt[d, j]] for j in range(R)]) for d in range(D)])
    return cap, ques, ans, opts, gt


def test_evaluate_disc_device_equals_host_on_a_pooled_batch():
    from gst_visdial_amd import evaluate_disc as ED
    D, R, O, U, LC, T = 2, 3, 10, 8, 8, 40
    enc, params, fx = sc().build_tiny_disc_encoder("fp32", DEV, visdial_tot_rounds=11, num_options=O, max_seq_len=T)
    image = {k: v.to(DEV) for k, v in sc().disc_batch(fx).items() if k in ("image_feat", "image_loc", "image_mask")}
    pooled = None
    for seed in range(11, 15):                                                               # the precondition: pools without a tied round
        cap, ques, ans, opts, gt = _pools(np.random.default_rng(seed), D, R, O, U, LC)
        rel = np.random.default_rng(seed).random((D, O)).astype(np.float32)
        cand = dict({k: torch.as_tensor(v).to(DEV) for k, v in dict(cap=cap, ques=ques, ans=ans, opts=opts, gt_index=gt).items()},
                    gt_relevance=torch.as_tensor(rel), round_id=torch.tensor([[2], [3]]), **image)
        if _no_ties(ED.score_batch(enc, cand, params, rows_per_call=17)):
            pooled = cand
            break
    assert pooled is not None
    host = ED.evaluate_disc(enc, [pooled], params, 2, rows_per_call=17)
    dev = ED.evaluate_disc(enc, [pooled], params, 2, rows_per_call=17, metrics="device")
    _compare(host, dev, D * R, O)


# -------------------------------------------------------------------------------------------------------------------- attack
def test_evaluate_attack_fgsm_device_equals_host(monkeypatch):
    """Two dialogs of one round x 100 options (one chunk each); dialog 0 is at its attacked round, dialog 1 is not.  The scores
    have one round per dialog, so round_id is 1 for both (it indexes the scores on the device)."""
    from gst_visdial_amd import attack as A
    s = sc()
    model, params, _ = s.build_tiny_model("fp32", DEV, mode="vd_eval_val", state_file="tiny_state_trained.npz")
    model.eval()
    params = dict(params, device=torch.device(DEV), vd_version="1.0", attack="fgsm")
    batches = []
    for i, b in enumerate(s.evalset100_batches(load_npz("tiny_evalset100.npz"), dialogs_per_batch=1)[:2]):
        r = 2 * i                                                                            # the round whose context the chunk carries
        b = {k: (v[:, r:r + 1].contiguous() if k.startswith(("enc_input", "enc_seg", "enc_att", "dec_")) or k == "gt_option_inds" else v)
             for k, v in b.items()}
        ids = b["enc_input_ids"]
        sep = torch.zeros(ids.shape[:3] + (25,), dtype=torch.int64)
        where = (ids[0, 0, 0] == 102).nonzero().view(-1)
        sep[..., :where.numel()] = where
        b["enc_sep_indices"], b["enc_mlm_labels"] = sep, torch.full_like(ids, -1)
        assert where.numel() // 2 == r + 1
        b["round_id"] = torch.tensor([[1]])                                                  # dialog 0: the chunk's own round; 1: another
        b["gt_relevance"] = b["gt_relevance"].clone()
        b["gt_relevance"][:, 0] += 0.2
        batches.append(b)
    seen, real = [], A.score_chunk

    def recording(*a, **k):
        out = real(*a, **k)
        seen.append(out.detach().clone())
        return out

    monkeypatch.setattr(A, "score_chunk", recording)
    _, host = A.evaluate_attack(model, batches, params, epsilon=0.05)
    _, dev = A.evaluate_attack(model, batches, params, epsilon=0.05, metrics="device")
    assert len(seen) == 4 and all(_no_ties(x.view(1, -1)) for x in seen)                     # the precondition
    assert torch.equal(seen[0], seen[2]) and torch.equal(seen[1], seen[3])
    _compare(host, dev, 2, 100)
