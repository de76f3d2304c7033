"""Listwise candidate training (Engine.rank_step, EncoderDecoderModel.rank_loss) on a real MI355X: the tiny model of the golden
fixtures against tests/golden/tiny_rank.npz (tools/make_golden_rank.py: the reference on the 12 replicated rows, eval, fp32),
against the same loss built on the engine's own replicated path, and -- train mode, dropout on -- against the CPU oracle under the
masks the engine drew.  Gates are the project's: scores 1e-3; loss per round 2e-3, twice the score gate, the
loss being a difference of scores; every fp32 gradient 2e-4 of its tensor's maximum."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, G = 3, 4
GRAD_GATE = 2e-4


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def oracle():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import vd_oracle as O
    return O


_FX = {}


def fixture():
    if not _FX:
        _FX.update(sc().load_npz("tiny_rank.npz"))
    return _FX


def rank_kw(fx, rounds=None, feats_grad=False):
    """The keyword tensors of EncoderDecoderModel.rank_loss on the device; `rounds`: a subset of the fixture's rounds."""
    rs = list(range(E)) if rounds is None else list(rounds)
    rows = [r * G + i for r in rs for i in range(G)]
    enc = ("enc_image_features", "enc_image_spatials", "enc_image_mask", "enc_input_ids", "enc_segments", "enc_attention_mask")
    kw = {k: fx["in::" + k][rs].clone().to(DEV) for k in enc}
    kw.update({k: fx["in::" + k][rows].clone().to(DEV) for k in ("dec_input_ids", "dec_attention_mask")})
    kw["relevance"] = fx["relevance"][rs].clone().to(DEV)
    kw["num_options"] = G
    if feats_grad:
        kw["enc_image_features"].requires_grad_(True)
    return kw


def listwise(per_token, rel):
    """tools/make_golden_rank.py's restatement of the loss on per-token losses (0 at [PAD] targets)."""
    n_r, n_o = rel.shape
    scores = -per_token.view(n_r, n_o, -1).sum(-1)
    logp = torch.log_softmax(scores, 1)
    rs = rel.sum(1, keepdim=True)
    counts = rs[:, 0] > 0
    t = torch.where(counts[:, None], rel / rs.clamp_min(1e-30), torch.zeros_like(rel))
    loss_round = -torch.where(t > 0, t * logp, torch.zeros_like(logp)).sum(1) * counts
    return scores, loss_round, loss_round.sum() / counts.sum().clamp_min(1)


def grads_of(model):
    return {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


def worst(got, ref, keys):
    """Largest |got - ref| / max|ref| over the tensors `keys` (tensors whose reference is all but zero: against 1e-6)."""
    w = (-1.0, "")
    for k in keys:
        e = (got[k] - ref[k]).abs().max().item() / max(ref[k].abs().max().item(), 1e-6)
        w = max(w, (e, k))
    return w


def fixture_grads(fx, model):
    named = dict(model.named_parameters())
    ref = {k[6:]: v for k, v in fx.items() if k.startswith("grad::")}
    keys = [k for k in ref if k in named]
    assert len(keys) >= len(ref) - 2 and len(keys) > 200, (len(keys), len(ref))
    return ref, keys


def test_fp32_eval_matches_the_reference_fixture():
    fx = fixture()
    model, _, _ = sc().build_tiny_model("fp32", DEV)
    model.eval()
    kw = rank_kw(fx, feats_grad=True)
    loss, scores = model.rank_loss(**kw)
    loss.backward()
    assert scores.shape == (E, G)
    err = (scores.cpu() - fx["scores"]).abs().max().item()
    rl = model.engine.last["rank_round_loss"].cpu()
    print("scores: max error %.3e; loss per round %s vs %s; mean %.6f vs %.6f" % (err, rl.tolist(), fx["loss_round"].tolist(), loss.item(), fx["loss"].item()))
    assert err < 1e-3
    assert (rl - fx["loss_round"]).abs().max().item() < 2e-3 and abs(loss.item() - fx["loss"].item()) < 2e-3
    assert float(model.engine.last["rank_stats"][1]) == 2.0 and float(rl[1]) == 0.0
    got = grads_of(model)
    ref, keys = fixture_grads(fx, model)
    w = worst(got, ref, keys)
    fe = (kw["enc_image_features"].grad.cpu() - fx["d_feats"]).abs().max().item() / fx["d_feats"].abs().max().item()
    print("worst parameter gradient error %.3e (%s); feature gradient error %.3e" % (w[0], w[1], fe))
    assert w[0] < GRAD_GATE, w
    assert fe < GRAD_GATE
    assert bool((kw["enc_image_features"].grad[2, -2:] == 0).all())       # the padded regions
    # the round without relevance contributes nothing: the same call without it
    model2, _, _ = sc().build_tiny_model("fp32", DEV)
    model2.eval()
    kw2 = rank_kw(fx, rounds=(0, 2), feats_grad=True)
    loss2, scores2 = model2.rank_loss(**kw2)
    loss2.backward()
    assert abs(loss2.item() - loss.item()) < 1e-5 and (scores2.cpu() - scores[[0, 2]].cpu()).abs().max().item() < 1e-4
    got2 = grads_of(model2)
    w2 = worst(got2, got, keys)
    print("without the round that has no relevance: worst gradient difference %.3e (%s)" % w2)
    assert w2[0] < GRAD_GATE, w2
    assert bool((kw["enc_image_features"].grad[1] == 0).all())
    fe2 = (kw2["enc_image_features"].grad - kw["enc_image_features"].grad[[0, 2]]).abs().max().item() / fx["d_feats"].abs().max().item()
    assert fe2 < GRAD_GATE


def test_fp32_grouped_step_equals_the_same_loss_on_replicated_rows():
    """The path that works without the grouped backward: model(..., loss_reduction=False) on the 12 rows (every row its own
    encoder pass), the listwise loss in torch on the per-token losses."""
    fx = fixture()
    model, _, _ = sc().build_tiny_model("fp32", DEV)
    model.eval()
    kw = rank_kw(fx)
    loss, scores = model.rank_loss(**kw)
    loss.backward()
    got = grads_of(model)
    model2, _, _ = sc().build_tiny_model("fp32", DEV)
    model2.eval()
    rep = {k: (v.repeat_interleave(G, 0) if k.startswith("enc_") else v) for k, v in rank_kw(fx).items() if k not in ("relevance", "num_options")}
    per_token, _ = model2(dec_labels=None, loss_reduction=False, **rep)
    s2, _, l2 = listwise(per_token, kw["relevance"])
    l2.backward()
    ref = grads_of(model2)
    assert abs(l2.item() - loss.item()) < 2e-3 and (s2 - scores).abs().max().item() < 1e-3
    w = worst(got, ref, sorted(set(got) & set(ref)))
    print("grouped vs replicated: loss %.6f vs %.6f, worst gradient error %.3e (%s)" % (loss.item(), l2.item(), w[0], w[1]))
    assert set(got) == set(ref) and w[0] < GRAD_GATE, w


def test_fp32_train_mode_matches_the_oracle_under_the_masks_the_engine_drew():
    O = oracle()
    s = sc()
    fx = fixture()
    model, _, cfg = s.build_tiny_model("fp32", DEV, cfg_file="tiny_cfg_dropout.json")
    model.train()
    kw = rank_kw(fx, feats_grad=True)
    loss, scores = model.rank_loss(**kw)
    loss.backward()
    eng = model.engine
    table = s.dropout_keep_masks(eng)
    assert table and any(k.endswith(".xattn") for k in table)
    for k in list(table):                                               # encoder-side sites: one mask per round, G replicas in the oracle
        if not (k == "emb.dec" or (k[0] == "d" and k[1].isdigit())):
            table[k] = table[k].reshape(E, -1).repeat_interleave(G, 0)
    masks = O.DropMasks(table)
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    keys = [k for k in O.live_param_keys(sd)]
    for k in list(sd):                                                  # (aliasing as oracle.vd_oracle.grads restores it)
        if k.startswith(O.DEC + "embeddings."):
            sd[k] = sd[O.ENC + "embeddings." + k[len(O.DEC + "embeddings."):]]
    sd[O.LMH + "decoder.bias"] = sd[O.LMH + "bias"]
    for k in keys:
        sd[k].requires_grad_(True)
    batch = {k: (fx["in::" + k].repeat_interleave(G, 0) if k.startswith("enc_") else fx["in::" + k]).clone() for k in
             ("enc_image_features", "enc_image_spatials", "enc_image_mask", "enc_input_ids", "enc_segments", "enc_attention_mask",
              "dec_input_ids", "dec_attention_mask")}
    batch["enc_image_features"].requires_grad_(True)
    out = O.model_forward(sd, cfg["enc"], cfg["dec"], batch, train=masks, loss_reduction=False)
    s_ref, lr_ref, l_ref = listwise(out["loss"], fx["relevance"])
    l_ref.backward()
    assert set(masks.used) == set(eng.site_log), set(masks.used) ^ set(eng.site_log)
    print("train mode: loss %.6f vs oracle %.6f; scores max error %.3e" % (loss.item(), l_ref.item(), (scores.cpu() - s_ref).abs().max().item()))
    assert (scores.cpu() - s_ref).abs().max().item() < 1e-3 and abs(loss.item() - l_ref.item()) < 2e-3
    got = grads_of(model)
    ref = {k: sd[k].grad for k in keys if sd[k].grad is not None}
    common = [k for k in ref if k in got]
    assert len(common) > 200
    w = worst(got, ref, common)
    dref = batch["enc_image_features"].grad.view(E, G, *fx["in::enc_image_features"].shape[1:]).sum(1)
    fe = (kw["enc_image_features"].grad.cpu() - dref).abs().max().item() / dref.abs().max().item()
    print("train mode: worst parameter gradient error %.3e (%s); feature gradient error %.3e" % (w[0], w[1], fe))
    assert w[0] < GRAD_GATE and fe < GRAD_GATE, (w, fe)


BF16_GATE = 3e-2


def test_bf16_eval_against_the_fp32_fixture():
    """bf16 engine against the fp32 reference fixture.  The softmax over the candidates amplifies score error, so the error is
    MEASURED (printed): scores relative to the largest score, the mean loss relative, every gradient tensor's error in its norm
    (tensors whose reference norm is at least 1e-3 of the largest), the feature gradient likewise.  Measured on the MI355X
    (profiles/rank_train.txt): scores 1.1e-4, loss 2.8e-6, worst gradient tensor 7.6e-3 (the image embedding weight), feature
    gradient 9.4e-3.  The gate is twice the measurement, or 3e-2 (the step-gradient gate) where twice the measurement is below it:
    every figure is, so the gate is 3e-2."""
    fx = fixture()
    model, _, _ = sc().build_tiny_model("bf16", DEV)
    model.eval()
    kw = rank_kw(fx, feats_grad=True)
    loss, scores = model.rank_loss(**kw)
    loss.backward()
    se = (scores.cpu() - fx["scores"]).abs().max().item() / fx["scores"].abs().max().item()
    le = abs(loss.item() - fx["loss"].item()) / abs(fx["loss"].item())
    got = grads_of(model)
    ref, keys = fixture_grads(fx, model)
    big = max(ref[k].norm().item() for k in keys)
    ge = max(((got[k] - ref[k]).norm().item() / ref[k].norm().item(), k) for k in keys if ref[k].norm().item() >= 1e-3 * big)
    fe = (kw["enc_image_features"].grad.cpu() - fx["d_feats"]).norm().item() / fx["d_feats"].norm().item()
    print("bf16 vs fp32 fixture: scores %.3e, loss %.3e, worst gradient tensor %.3e (%s), feature gradient %.3e" % (se, le, ge[0], ge[1], fe))
    assert se < BF16_GATE and le < BF16_GATE and ge[0] < BF16_GATE and fe < BF16_GATE, (se, le, ge, fe)


def test_state_accumulation_optimizer_and_refusals():
    from gst_visdial_amd._lib import GstvdError
    from gst_visdial_amd.optim import FusedAdamW
    fx = fixture()
    model, _, _ = sc().build_tiny_model("fp32", DEV)
    model.eval()
    kw = rank_kw(fx)
    loss, scores = model.rank_loss(**kw)
    # score_candidates afterwards: the forward's scores, bit for bit
    again = model.score_candidates(kw["enc_image_features"], kw["enc_image_spatials"], kw["enc_image_mask"], kw["enc_input_ids"],
                                   kw["enc_segments"], kw["enc_attention_mask"], kw["dec_input_ids"], kw["dec_attention_mask"], G)
    assert torch.equal(again.view(E, G), scores)
    loss, _ = model.rank_loss(**kw)
    loss.backward()
    once = grads_of(model)
    loss, _ = model.rank_loss(**kw)
    (0.5 * loss).backward()                                            # .grad kept: accumulates, under an upstream factor
    twice = grads_of(model)
    w = worst(twice, {k: 1.5 * v for k, v in once.items()}, sorted(once))
    assert w[0] < 1e-5, w
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.01, warmup_steps=0, t_total=10)
    opt.step()
    opt.zero_grad()
    after = model.state_dict()
    assert sum(1 for k in before if not torch.equal(before[k], after[k])) > 200
    # refusals
    with pytest.raises(GstvdError, match="rank_step"):
        with model.inputs_only():
            model.rank_loss(**rank_kw(fx, feats_grad=True))
    bad = rank_kw(fx)
    bad["dec_input_ids"] = bad["dec_input_ids"][:-1]
    with pytest.raises(GstvdError, match="rank_step"):
        model.rank_loss(**bad)
    bad = rank_kw(fx)
    bad["relevance"] = bad["relevance"][:2]
    with pytest.raises(GstvdError, match="rank_step"):
        model.rank_loss(**bad)
    from gst_visdial_amd import attn_maps
    with pytest.raises(GstvdError, match="rank_step"):
        with attn_maps.capture(model.engine, attn_maps.MapRequest({}, False)):
            model.rank_loss(**kw)
    loss, _ = model.rank_loss(**kw)                                     # and the engine still works afterwards
    assert torch.isfinite(loss)
