"""The pooled path of the discriminative model end to end on the tiny enc_only_a fixture: `evaluate_disc` on a pooled batch against
the tensor batch that the numpy rule (tests/exact_disc_rows.py) builds from the same pools, and `forward_disc` in a train mode
with the sampled rows and every draw pinned against the tensor path.  Both sides run the same kernels on the same inputs, so the
scores, the losses and the metrics must be EQUAL, not close."""
import numpy as np
import pytest
import torch

import exact_disc_rows as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, R, O, U, LC, T = 2, 3, 10, 8, 8, 40


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def _pools(seed=3):
    gen = np.random.default_rng(seed)
    cap = np.stack([X._row(LC, n, gen) for n in (8, 3)])
    ques = np.stack([np.stack([X._row(U, int(gen.integers(0, 6)), gen) for _ in range(R)]) for _ in range(D)])
    opts = np.stack([np.stack([np.stack([X._row(U, int(gen.integers(0, U + 1)), gen) for _ in range(O)]) for _ in range(R)]) for _ in range(D)])
    gt = np.array([[0, 9, 4], [7, 2, 5]], np.int64)
    ans = np.stack([np.stack([opts[d, j, gt[d, j]] for j in range(R)]) for d in range(D)])
    return cap, ques, ans, opts, gt


def _dev(arrays):
    return {k: torch.as_tensor(np.asarray(v)).to(DEV) for k, v in arrays.items()}


@pytest.mark.parametrize("tot_rounds,num_options", [(11, 10), (2, 6)])
def test_evaluate_disc_on_pools_equals_the_tensor_batch_of_the_same_pools(tot_rounds, num_options):
    from gst_visdial_amd import evaluate_disc as ED
    enc, params, fx = sc().build_tiny_disc_encoder("fp32", DEV, visdial_tot_rounds=tot_rounds, num_options=num_options, max_seq_len=T)
    cap, ques, ans, opts, gt = _pools()
    b = sc().disc_batch(fx)
    image = {k: b[k] for k in ("image_feat", "image_loc", "image_mask")}
    rows = X._all_rows(D, R, num_options)
    w = X.rows_rule(cap, ques, ans, opts, gt, rows[0], rows[1], rows[2], T, tot_rounds, num_options, False)
    gen = np.random.default_rng(9)
    rel = gen.random((D, O)).astype(np.float32)
    round_id = np.array([[2], [3]], np.int64)
    order = np.array([[X.eval_option(int(gt[d, round_id[d, 0] - 1]), k) for k in range(num_options)] for d in range(D)])
    shape = lambda k: torch.as_tensor(w[k]).view(D, R, num_options, -1)
    tensor_batch = dict(tokens=shape("tokens"), segments=shape("segments"), sep_indices=shape("sep_indices"), mask=shape("mask"),
                        hist_len=torch.as_tensor(w["hist_len"]).view(D, R, num_options), gt_option_inds=torch.zeros(D, R, dtype=torch.long),
                        gt_relevance=torch.as_tensor(np.take_along_axis(rel, order, 1)), round_id=torch.as_tensor(round_id), **image)
    pooled = dict(_dev(dict(cap=cap, ques=ques, ans=ans, opts=opts, gt_index=gt)), gt_relevance=torch.as_tensor(rel),
                  round_id=torch.as_tensor(round_id), **{k: v.to(DEV) for k, v in image.items()})
    s_t = ED.score_batch(enc, tensor_batch, params, rows_per_call=17).cpu()
    s_p = ED.score_batch(enc, pooled, params, rows_per_call=17).cpu()
    assert tuple(s_p.shape) == (D, R, num_options) and torch.equal(s_p.view(torch.int32), s_t.view(torch.int32))
    assert len(set(s_p.flatten().tolist())) > D * R * num_options // 2                      # the rows do differ: no constant score
    m_t = ED.evaluate_disc(enc, [tensor_batch], params, 2, rows_per_call=17)
    m_p = ED.evaluate_disc(enc, [pooled], params, 2, rows_per_call=17)
    assert m_t == m_p and "ndcg" in m_p, (m_t, m_p)
    # forward_disc, eval mode: every row of the pools in one item
    item = ED.chunk_item(tensor_batch, ED.option_rows_to_dialog(D, R, num_options), 0, D * R * num_options)
    z_t = ED.forward_disc(enc, item, params)[4].cpu()
    z_p = ED.forward_disc(enc, pooled, params)[4].cpu()
    assert torch.equal(z_t.view(torch.int32), z_p.view(torch.int32))
    # the attention mask the kernel writes is evaluate_disc's own
    from gst_visdial_amd import disc_rows as DR
    it = DR.eval_item(pooled, 5, 31, params)
    att = ED.sequence_mask(ED.sequence_lengths(it["sep_indices"], it["hist_len"]), T)
    assert torch.equal(it["att"], att.float()) and it["att"].dtype == torch.float32


@pytest.mark.parametrize("dense", [False, True])
def test_forward_disc_train_on_pools_equals_the_tensor_path_with_pinned_draws(dense):
    from gst_visdial_amd import evaluate_disc as ED
    nneg, batch_size, tot_rounds, num_options, mask_prob = 2, 12, 2, 6, 0.15
    enc, params, fx = sc().build_tiny_disc_encoder("fp32", DEV, mode="vd_train", fixture="tiny_disc_train.npz", lm_loss_coeff=1.0,
                                                   nsp_loss_coeff=0.5, img_loss_coeff=2.0, batch_size=batch_size, max_seq_len=T,
                                                   visdial_tot_rounds=tot_rounds, num_options=num_options, num_negative_samples=nneg,
                                                   mask_prob=mask_prob)
    cap, ques, ans, opts, gt = _pools(4)
    b = sc().disc_batch(fx)
    gen = np.random.default_rng(17)
    n_all = D * R * (1 + nneg)
    torch.manual_seed(5)
    sample = torch.randperm(n_all)[:batch_size]
    # draws pinned per sampled row; the tensor path builds ALL rows, so row sample[i] of it receives draw i
    u_tok, u_neg = X._noise(batch_size, T, gen), gen.random(batch_size).astype(np.float32)
    u_tok_all, u_neg_all = gen.random((n_all, T)).astype(np.float32), gen.random(n_all).astype(np.float32)
    u_tok_all[sample.numpy()], u_neg_all[sample.numpy()] = u_tok, u_neg
    u_img = gen.random((D, 7))
    u_img[0, 1], u_img[1, 2] = 0.01, 0.14                                                  # zeroed / labelled only
    forced = np.array([3, 6], np.int64)
    scores = X.soft_scores((D, R, O), gen) if dense else None
    rows = X._all_rows(D, R, 1 + nneg)
    w = X.rows_rule(cap, ques, ans, opts, gt, rows[0], rows[1], rows[2], T, tot_rounds, num_options, True, mask_prob, u_tok_all, u_neg_all,
                    scores)
    feats, label = X.image_rule(b["image_feat"].numpy(), b["image_mask"].numpy(), u_img, forced, mask_prob)
    assert (w["mask"][sample.numpy()] >= 0).any() and (label == 1).any() and (feats != b["image_feat"].numpy()).any()
    shape = lambda k: torch.as_tensor(w[k]).view(D, R, 1 + nneg, -1)
    tensor_batch = dict(tokens=shape("tokens"), segments=shape("segments"), sep_indices=shape("sep_indices"), mask=shape("mask"),
                        next_sentence_labels=shape("nsp_labels"), hist_len=torch.as_tensor(w["hist_len"]).view(D, R, 1 + nneg),
                        image_feat=torch.as_tensor(feats), image_loc=b["image_loc"], image_mask=b["image_mask"],
                        image_target=b["image_target"], image_label=torch.as_tensor(label))
    pooled = dict(_dev(dict(cap=cap, ques=ques, ans=ans, opts=opts, gt_index=gt, u_tok=u_tok, u_neg=u_neg, u_img=u_img, forced_region=forced)),
                  sample_indices=sample, **{k: b[k].to(DEV) for k in ("image_feat", "image_loc", "image_mask", "image_target")})
    if dense:
        pooled["dense_scores"] = torch.as_tensor(scores).to(DEV)
    torch.manual_seed(5)                                                                   # train_rows draws the same permutation
    out_t = ED.forward_disc(enc, tensor_batch, params)
    out_p = ED.forward_disc(enc, pooled, params)
    assert len(out_t) == len(out_p) == 6 and out_t[5] is None and out_p[5] is None
    for i, (a, p) in enumerate(zip(out_t[:5], out_p[:5])):
        a, p = a.detach().float().cpu(), p.detach().float().cpu()
        assert a.shape == p.shape and torch.equal(a.view(torch.int32), p.view(torch.int32)), (i, a, p)
    assert torch.isfinite(out_p[0]).all() and tuple(out_p[4].shape) == (batch_size, 2)
    out_p[0].backward()                                                                    # the pooled path is differentiable as before
    assert any(q.grad is not None and bool(q.grad.abs().sum() > 0) for q in enc.parameters())
