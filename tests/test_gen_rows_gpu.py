"""The pooled path of the generative model end to end on the tiny enc_dec fixture: `evaluate` on a pooled batch against the
loader-shaped batch that the numpy rule (tests/exact_gen_rows.py) expands from the same pools, the random-token noise against the
per-row scorer, the questioner's teacher rows through the step driver, and the device-metrics loop inside one stream capture.  Both
sides run the same kernels on the same inputs, so scores, losses and metrics must be EQUAL, not close."""
import numpy as np
import pytest
import torch

import exact_gen_rows as X
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, R, O, U, LC, T, UD = 2, 3, 6, 7, 8, 40, 9


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def _pools(seed=3):
    gen = np.random.default_rng(seed)
    cap = np.stack([X._row(LC, n, gen) for n in (8, 3)])
    ques = np.stack([np.stack([X._row(U, int(gen.integers(0, 6)), gen) for _ in range(R)]) for _ in range(D)])
    opts = np.stack([np.stack([np.stack([X._row(U, int(gen.integers(0, U + 1)), gen) for _ in range(O)]) for _ in range(R)]) for _ in range(D)])
    gt = np.array([[0, 5, 3], [4, 2, 5]], np.int64)
    ans = np.stack([np.stack([opts[d, j, gt[d, j]] for j in range(R)]) for d in range(D)])
    return cap, ques, ans, opts, gt


def _dev(arrays):
    return {k: torch.as_tensor(np.asarray(v)).to(DEV) for k, v in arrays.items()}


def _image():
    ev = load_npz("tiny_evalset100.npz")
    return {k: ev["in::" + k][:D].clone() for k in ("enc_image_feat", "enc_image_loc", "enc_image_mask")}


@pytest.fixture(scope="module")
def tiny():
    model, params, _ = sc().build_tiny_model("fp32", DEV, mode="vd_eval_val")
    model.eval()
    return model, dict(params, device=torch.device(DEV), vd_version="1.0", max_seq_len=T, max_utt_len=UD)


def _batches(num_options, mask_prob=0.0, u_tok=None, seed=3):
    """(pooled batch on the device, the loader-shaped batch of the same pools on the host)."""
    cap, ques, ans, opts, gt = _pools(seed)
    image = _image()
    gen = np.random.default_rng(9)
    rel = gen.random((D, O)).astype(np.float32)
    round_id = np.array([[2], [3]], np.int64)
    order = np.array([[X.eval_option(int(gt[d, round_id[d, 0] - 1]), k) for k in range(num_options)] for d in range(D)])
    loader = dict(X.expand_eval(cap, ques, ans, opts, gt, T, UD, num_options, mask_prob, u_tok), round_id=torch.as_tensor(round_id),
                  gt_relevance=torch.as_tensor(np.take_along_axis(rel, order, 1)), **image)
    pooled = dict(_dev(dict(cap=cap, ques=ques, ans=ans, opts=opts, gt_index=gt, gt_relevance=rel, round_id=round_id)),
                  **{k: v.to(DEV) for k, v in image.items()})
    if u_tok is not None:
        pooled["u_tok"] = torch.as_tensor(u_tok).to(DEV)
    return pooled, loader


def _bits_equal(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("num_options", [6, 4])
def test_evaluate_on_pools_equals_the_loader_batch_of_the_same_pools(tiny, num_options):
    from gst_visdial_amd import evaluate as EV, gen_rows as GR
    model, params = tiny
    params = dict(params, num_options=num_options)
    pooled, loader = _batches(num_options)
    assert GR.is_pooled(pooled) and not GR.is_pooled(loader)
    seen = {}

    def scorer(tag):
        def f(m, b, d):
            seen[tag] = EV.score_batch(m, b, d, rounds_per_call=4, params=params).clone()
            return seen[tag]
        return f

    out = {(kind, m): EV.evaluate(model, [b], params, scorer=scorer((kind, m)), metrics=m)
           for kind, b in (("pooled", pooled), ("loader", loader)) for m in ("host", "device")}
    ref = seen[("loader", "host")]
    assert tuple(ref.shape) == (D, R, num_options) and len(set(ref.flatten().tolist())) > D * R * num_options // 2   # no constant score
    for key, s in seen.items():
        assert _bits_equal(s, ref), key
    for m in ("host", "device"):
        assert out[("pooled", m)] == out[("loader", m)], (m, out[("pooled", m)], out[("loader", m)])
        assert out[("pooled", m)][0] == [] and {"r@1", "mean", "mrr", "ndcg"} <= set(out[("pooled", m)][1])
    # without a scorer the loop hands `params` to score_batch itself
    assert EV.evaluate(model, [pooled], params)[1] == EV.evaluate(model, [loader], params)[1]


def test_test_split_pools_rank_like_the_loader_batch(tiny):
    """vd_eval_test: one round per dialog (n_rounds - 1), options in their original order, opts [D, 1, O, U]."""
    from gst_visdial_amd import evaluate as EV
    model, params = tiny
    cap, ques, ans, opts, gt = _pools()
    n_rounds = np.array([3, 1], np.int64)
    opts1 = np.stack([opts[d, n_rounds[d] - 1][None] for d in range(D)])
    image = _image()
    enc = np.stack([np.arange(D), n_rounds - 1]).astype(np.int32)
    dec = np.stack([np.repeat(enc[0], O), np.repeat(enc[1], O), np.tile(np.arange(O), D)]).astype(np.int32)
    w = X.rows_rule(cap, ques, ans, opts1, None, "test", enc, dec, T, UD, O)
    rep = lambda k: torch.as_tensor(w[k]).view(D, 1, 1, -1).expand(D, 1, O, -1).contiguous()
    ids = dict(image_id=torch.tensor([7, 9]), round_id=torch.as_tensor(n_rounds).view(D, 1))
    loader = dict(enc_input_ids=rep("tokens"), enc_segments=rep("segments"), enc_att_mask=rep("att"),
                  dec_input_ids=torch.as_tensor(w["dec_ids"]).view(D, 1, O, UD), dec_att_mask=torch.as_tensor(w["dec_att"]).view(D, 1, O, UD),
                  **image, **ids)
    pooled = dict(_dev(dict(cap=cap, ques=ques, ans=ans, opts=opts1, n_rounds=n_rounds)), **{k: v.to(DEV) for k, v in image.items()}, **ids)
    s_p = EV.score_batch(model, pooled, params["device"], rounds_per_call=1, params=params)
    s_l = EV.score_batch(model, loader, params["device"], rounds_per_call=1)
    assert tuple(s_p.shape) == (D, 1, O) and _bits_equal(s_p, s_l)
    for m in ("host", "device"):
        j_p, m_p = EV.evaluate(model, [pooled], params, mode="vd_eval_test", metrics=m)
        j_l, m_l = EV.evaluate(model, [loader], params, mode="vd_eval_test", metrics=m)
        assert j_p == j_l and m_p == m_l == {} and [e["image_id"] for e in j_p] == [7, 9] and [e["round_id"] for e in j_p] == [3, 1]


def test_random_token_noise_scores_equal_the_per_row_scorer(tiny):
    from gst_visdial_amd import evaluate as EV
    model, params = tiny
    params = dict(params, num_options=O, attack="random_token", mask_prob=0.15)
    u_tok = X._noise(D * R * O, T, np.random.default_rng(21))
    pooled, loader = _batches(O, 0.15, u_tok)
    ids = loader["enc_input_ids"]
    assert bool((ids == X.MASK).any()) and not bool((ids == ids[:, :, :1]).all())           # each option's copy has its own noise
    s_p = EV.score_batch(model, pooled, params["device"], rounds_per_call=2, params=params)
    s_l = EV._score_batch_per_row(model, loader, params["device"], 2)
    assert tuple(s_p.shape) == (D, R, O) and _bits_equal(s_p, s_l)
    clean = EV.score_batch(model, pooled, params["device"], rounds_per_call=2, params=dict(params, attack=None))
    assert not _bits_equal(s_p, clean)                                                       # the noise does reach the scores
    # draws of the op's own: another set of rows, same shape, finite scores
    own = EV.score_batch(model, {k: v for k, v in pooled.items() if k != "u_tok"}, params["device"], rounds_per_call=2, params=params)
    assert tuple(own.shape) == (D, R, O) and bool(torch.isfinite(own).all())


def test_questioner_train_batch_goes_through_the_step_driver():
    from gst_visdial_amd import step, gen_rows as GR
    model, params, _ = sc().build_tiny_model("fp32", DEV, mode="vd_train", seed=1)
    cap, ques, ans, opts, gt = _pools(5)
    image = _image()
    tp = dict(max_seq_len=T, max_utt_len=UD)
    pools = _dev(dict(cap=cap, ques=ques, ans=ans))
    rows = X._grid(D, R)
    dec = np.concatenate([rows, np.zeros((1, D * R), np.int32)])
    for name, mode in (("enc_dec_q", "train_q"), ("enc_dec_a", "train_a")):
        batch = GR.train_batch(pools, {k: v.to(DEV) for k, v in image.items()}, tp, model=name)
        w = X.rows_rule(cap, ques, ans, None, None, mode, rows, dec, T, UD)
        sh = lambda k: torch.as_tensor(w[k]).view(D, R, 1, -1)
        host = dict(enc_input_ids=sh("tokens"), enc_segments=sh("segments"), enc_att_mask=sh("att"), enc_mlm_labels=sh("mlm"),
                    enc_sep_indices=sh("sep_indices"), enc_hist_len=torch.as_tensor(w["hist_len"]).view(D, R, 1),
                    dec_input_ids=sh("dec_ids"), dec_att_mask=sh("dec_att"), dec_labels=sh("dec_labels"),
                    enc_next_sentence_labels=torch.full((D, R, 1), -1, dtype=torch.long), **image)
        assert set(batch) == set(host) and all(v.is_cuda for v in batch.values())
        for k, v in host.items():
            assert batch[k].dtype == v.dtype and torch.equal(batch[k].cpu(), v), (name, k)
        idx = torch.tensor([0, 2, 5, 3])
        model.eval()
        with torch.no_grad():
            l_p, s_p = step.forward(model, batch, params, sample_indices=idx)
            l_p, s_p = l_p.clone(), s_p.clone()
            l_h, s_h = step.forward(model, host, params, sample_indices=idx)
        assert bool(torch.isfinite(l_p)) and _bits_equal(l_p.reshape(1), l_h.reshape(1)) and _bits_equal(s_p, s_h), name
        model.train()
        loss, _ = step.forward(model, batch, params)                                          # train mode: rows drawn from the labelled ones
        assert bool(torch.isfinite(loss))
    q, a = GR.train_batch(pools, {k: v.to(DEV) for k, v in image.items()}, tp, model="enc_dec_q"), batch
    assert not torch.equal(q["dec_labels"], a["dec_labels"]) and int(q["enc_hist_len"][0, 0, 0]) == 0 and int(a["enc_hist_len"][0, 0, 0]) == 1


@pytest.mark.isolated
def test_device_metrics_loop_runs_inside_one_stream_capture(tiny):
    """The pooled vd_eval_val loop with the metric state on the device -- rows, scores, targets, ranks -- has no host
    synchronisation (torch's sync debug mode turns one into an error) and its launches can be captured once and replayed on other
    pool contents."""
    from gst_visdial_amd import evaluate as EV, gen_rows as GR
    from gst_visdial_amd.graph import capture
    from gst_visdial_amd.metrics import DeviceRankMetrics
    model, params = tiny
    params = dict(params, num_options=O)
    pooled, _ = _batches(O)
    other, _ = _batches(O, seed=4)
    other["gt_index"] = torch.as_tensor(np.array([[5, 0, 1], [2, 3, 0]], np.int64)).to(DEV)
    dev = DeviceRankMetrics(DEV)

    def body():
        scores = EV.score_batch(model, pooled, params["device"], rounds_per_call=4, params=params)
        gt_inds, rel = GR.eval_targets(pooled, params, scores.device)
        dev.observe(scores, gt_inds, rel, pooled["round_id"])
        return scores

    with torch.no_grad():
        want = {}
        for name, b in (("pooled", pooled), ("other", other)):                               # eager: the answers, and every lazy table built
            want[name] = EV.evaluate(model, [b], params, metrics="device")[1]
        assert want["pooled"] != want["other"]
        body()
        dev.reset()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            body()                                                                           # any synchronising torch call raises here
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert dev.retrieve() == want["pooled"]
        g = torch.cuda.CUDAGraph()
        with capture(g):
            scores = body()
        keep = {k: pooled[k].clone() for k in ("cap", "ques", "ans", "opts", "gt_index", "gt_relevance")}
        for name, src in (("other", other), ("pooled", keep)):
            for k in keep:
                pooled[k].copy_(src[k])
            dev.reset()
            scores.fill_(float("nan"))
            g.replay()
            assert dev.retrieve() == want[name], name
            assert bool(torch.isfinite(scores).all())
