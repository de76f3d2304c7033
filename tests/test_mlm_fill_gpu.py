"""Model layer of the random-token text attack on a real MI355X, against tests/golden/tiny_mlm_fill.npz: what transformers'
BertForMaskedLM and the reference's TextAttack.random_token_attack compute on a tiny model (tools/make_golden_mlm_fill.py).
The fixture guarantees a relative top-2 margin of 1e-3 at every masked position, ten times the fp32 logit gate, so the fp32
checks leave no position out.  Gates: fp32 logits 1e-4 of the largest magnitude, logits of the enc-dec model 1e-4, answer scores
1e-3 (the bars of tests/test_fgsm_gpu.py's second forward)."""
import numpy as np
import pytest
import torch

import exact_mlm as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# Largest |val - reference maximum| of the bf16 engine over the fixture's 12 masked positions (max|logit| 0.65), measured on an
# MI355X ("Masked-LM fill-in"); the test allows twice that.
BF16_VAL_MEASURED = 1.98e-3


@pytest.fixture(scope="module")
def fx():
    from gst_visdial_amd.selfcheck import load_npz
    return load_npz("tiny_mlm_fill.npz")


def make_filler(fx, precision):
    from gst_visdial_amd.mlm import MaskedLMFiller
    cfg = {k[len("mlm_cfg::"):]: v.item() for k, v in fx.items() if k.startswith("mlm_cfg::")}
    cfg["hidden_act"] = "gelu"
    filler = MaskedLMFiller(cfg, DEV, precision=precision, mask_token_id=int(fx["mask_token_id"]))
    ignored = filler.load_bert_mlm_state_dict({k[len("mlm_state::"):]: v for k, v in fx.items() if k.startswith("mlm_state::")})
    assert all(k.endswith("position_ids") for k in ignored)
    return filler


@pytest.fixture(scope="module")
def filler32(fx):
    return make_filler(fx, "fp32")


def test_fp32_predict_matches_at_every_masked_position(filler32, fx):
    pos, idx, val = filler32.predict(fx["ids"], fx["seg"], fx["att"])
    assert torch.equal(pos.cpu(), fx["pos_all"])
    assert torch.equal(idx.cpu(), fx["argmax_all"])                                   # none left out
    ref = fx["logits_all"]
    err = (val.cpu() - ref.max(-1).values).abs().max().item()
    print("fp32 predict: |val - max_ref| %.3e (bound %.3e)" % (err, 1e-4 * ref.abs().max().item()))
    assert err <= 1e-4 * ref.abs().max().item()
    # positions found on the host and handed in: the same answer, no device round trip for them
    pos_h = filler32.host_rows(fx["ids"])
    _, idx_h, val_h = filler32.predict(fx["ids"], fx["seg"], fx["att"], rows=pos_h)
    assert torch.equal(idx_h, idx) and torch.equal(val_h, val)


def test_fp32_fill_equals_the_reference(filler32, fx):
    ids = fx["ids"].clone()
    got = filler32.fill(ids, fx["seg"], fx["att"])
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), fx["filled"])
    assert torch.equal(ids, fx["ids"])                                                # the caller's tensor is not written
    dev_ids = fx["ids"].to(DEV)
    got = filler32.fill(dev_ids, fx["seg"].to(DEV), fx["att"].to(DEV), rows=filler32.host_rows(fx["ids"][:1]))
    assert torch.equal(got.cpu(), fx["filled"]) and torch.equal(dev_ids.cpu(), fx["ids"])
    # numpy rule of tests/exact_mlm.py on the device's arg-max: the same ids
    _, idx, _ = filler32.predict(fx["ids"][:1], fx["seg"][:1], fx["att"][:1])
    assert np.array_equal(X.fill_rule(fx["ids"].numpy(), int(fx["mask_token_id"]), argmax=idx.cpu().numpy()), fx["filled"].numpy())


def test_fp32_no_mask_and_all_real_rows(filler32, fx):
    nm = fx["nomask_ids"]
    got = filler32.fill(nm, fx["nomask_seg"], (nm != 0).float())
    assert torch.equal(got.cpu(), fx["nomask_filled"]) and torch.equal(got.cpu(), nm)
    pos, idx, val = filler32.predict(nm, fx["nomask_seg"], (nm != 0).float())
    assert pos.numel() == 0 and idx.numel() == 0 and val.numel() == 0
    got = filler32.fill(fx["full_ids"], fx["full_seg"], fx["full_att"])
    assert torch.equal(got.cpu(), fx["full_filled"])
    _, idx, val = filler32.predict(fx["full_ids"][:1], fx["full_seg"][:1], fx["full_att"][:1])
    ref = fx["full_logits"]
    assert torch.equal(idx.cpu(), fx["full_argmax"])
    assert (val.cpu() - ref.max(-1).values).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_output_does_not_depend_on_the_image(filler32, fx):
    B = fx["ids"].shape[0]
    c = filler32.enc_config
    g = torch.Generator().manual_seed(5)
    out = []
    for scale in (1.0, -3.0):
        image = ((torch.randn(B, 1, c["v_feature_size"], generator=g) * scale).to(DEV), torch.rand(B, 1, 5, generator=g).to(DEV),
                 torch.ones(B, 1, device=DEV))
        out.append(filler32.predict(fx["ids"], fx["seg"], fx["att"], image=image))
    out.append(filler32.predict(fx["ids"], fx["seg"], fx["att"]))
    for pos, idx, val in out[1:]:
        assert torch.equal(idx, out[0][1]) and torch.equal(val, out[0][2]) and torch.equal(pos, out[0][0])


def test_bf16_engine(fx):
    """No position excluded: the value within 2x the measured deviation, and the returned token's reference logit within twice
    that bound of the reference maximum (a bf16 engine may return another token than fp32 where two logits are that close)."""
    filler = make_filler(fx, "bf16")
    pos, idx, val = filler.predict(fx["ids"], fx["seg"], fx["att"])
    assert torch.equal(pos.cpu(), fx["pos_all"])
    ref = fx["logits_all"]
    top = ref.max(-1).values
    err = (val.cpu() - top).abs().max().item()
    chosen = ref.gather(1, idx.cpu().view(-1, 1)).view(-1)
    gap = (top - chosen).max().item()
    same = int((idx.cpu() == fx["argmax_all"]).sum())
    print("bf16 predict: |val - max_ref| %.3e, reference logit of the returned token below the maximum by %.3e, %d of %d tokens "
          "equal fp32's" % (err, gap, same, idx.numel()))
    bound = 2.0 * BF16_VAL_MEASURED
    assert err <= bound
    assert gap <= 2.0 * bound
    assert int(idx.max()) < ref.shape[1] and int(idx.min()) >= 0
    # the fused kernel is what ran: the head's launches of the last call carry no [n, vocab] GEMM
    from gst_visdial_amd import ops
    with ops.Profiler() as prof:
        filler.predict(fx["ids"], fx["seg"], fx["att"])
    tags = [t for t in prof.summary(scope="head.mlm")]
    assert "vocab_argmax" in tags and "rows_argmax" not in tags, tags


def test_two_stream_encoder_predict_masked(fx):
    from gst_visdial_amd.selfcheck import build_tiny_disc_encoder
    enc, params, _ = build_tiny_disc_encoder("fp32", DEV)
    args = (fx["disc::ids"].to(DEV), fx["disc::image_feat"].to(DEV), fx["disc::image_loc"].to(DEV))
    kw = dict(token_type_ids=fx["disc::seg"].to(DEV), attention_mask=fx["disc::att"].to(DEV),
              image_attention_mask=fx["disc::image_mask"].to(DEV))
    idx, val = enc.predict_masked(*args, mask_token_id=int(fx["mask_token_id"]), **kw)
    ref = fx["disc::logits"]
    assert torch.equal(idx.cpu(), fx["disc::argmax"])
    assert (val.cpu() - ref.max(-1).values).abs().max().item() <= 1e-4 * ref.abs().max().item()
    idx2, val2 = enc.predict_masked(*args, rows=fx["disc::pos"], **kw)
    assert torch.equal(idx2, idx) and torch.equal(val2, val)
    enc.train()
    with pytest.raises(NotImplementedError):
        enc.predict_masked(*args, **kw)
    enc.eval()
    # the ranking branch next to it is undisturbed
    z, p0 = enc.nsp_scores(args[0], args[1], args[2], kw["token_type_ids"], kw["attention_mask"], kw["image_attention_mask"])
    assert z.shape == (2, 2) and bool(torch.isfinite(z).all())


def chunk(fx):
    b = {k[len("atk::in::"):]: v.clone() for k, v in fx.items() if k.startswith("atk::in::")}
    b["round_id"] = torch.tensor([1])
    b["gt_relevance"] = torch.zeros(b["dec_input_ids"].shape[0])
    return b


def test_attack_forward_and_one_pass_scores(filler32, fx):
    from oracle import vd_oracle as O
    from gst_visdial_amd import attack
    from gst_visdial_amd.selfcheck import build_tiny_model
    model, params, _ = build_tiny_model("fp32", DEV, mode="vd_eval_val")
    model.eval()
    params = dict(params, attack="random_token")
    b = chunk(fx)
    ids0, dec0 = b["enc_input_ids"].clone(), b["dec_input_ids"].clone()
    with torch.no_grad():
        logits = attack.forward_attack(model, b, params, textattack=filler32).float().cpu()
    assert torch.equal(b["enc_input_ids"], ids0) and torch.equal(b["dec_input_ids"], dec0)
    err = (logits - fx["atk::logits"]).abs().max().item()
    sc = O.answer_scores(logits, dec0)
    serr = (sc - fx["atk::answer_scores"]).abs().max().item()
    print("random_token forward: logits error %.3e, score error %.3e" % (err, serr))
    assert err <= 1e-4 and serr <= 1e-3
    with torch.no_grad():
        one = attack.score_chunk(model, b, dict(params, textattack=filler32), 1.0).cpu()
    print("one-pass scores vs the fixture %.3e, vs the multi-row forward %.3e"
          % ((one - fx["atk::answer_scores"]).abs().max().item(), (one - sc).abs().max().item()))
    assert (one - sc).abs().max().item() <= 1e-3 and (one - fx["atk::answer_scores"]).abs().max().item() <= 1e-3
    # a chunk whose segments differ between rows cannot take the one-pass route: the multi-row forward, same scores for row 0
    b2 = chunk(fx)
    b2["enc_segments"][1, 2] ^= 1
    with torch.no_grad():
        many = attack.score_chunk(model, b2, params, 1.0, textattack=filler32).cpu()
    assert abs(many[0].item() - sc[0].item()) <= 1e-3
    with pytest.raises(NotImplementedError) as e:
        attack.forward_attack(model, b, params)
    assert "random_token" in str(e.value) and "BertForMaskedLM" in str(e.value)
    with pytest.raises(NotImplementedError):
        attack.score_chunk(model, b, params, 1.0)


def test_train_step_is_unchanged_by_a_fill_on_another_model(filler32, fx):
    from gst_visdial_amd.selfcheck import build_tiny_model, golden_batch, load_npz
    tr = load_npz("tiny_train.npz")
    model = build_tiny_model("fp32", DEV, seed=3)[0]
    model.eval()                                   # dropout off: the two steps differ in nothing but what ran between them

    def step():
        model.zero_grad(set_to_none=True)
        loss, _ = model(**golden_batch(tr, DEV))
        loss.backward()
        return loss.detach().clone()

    a = step()
    filler32.fill(fx["ids"], fx["seg"], fx["att"])
    b = step()
    assert torch.equal(a, b)
