"""CPU side of the FGSM attack evaluation (gst_visdial_amd/attack.py, tests/golden/tiny_fgsm.npz by tools/make_golden_fgsm.py):
the oracle reproduces what the reference recorded, the text attacks are refused by name, and the host logic of the
relevant-row subset leaves zero-relevance rows and the caller's decoder ids as the reference leaves them."""
import types

import pytest
import torch

from conftest import load_npz
from oracle import vd_oracle as O

TOL = 1e-6                  # as tests/test_oracle_golden.py compares d loss / d features and the metric values


@pytest.fixture(scope="module")
def fx():
    return load_npz("tiny_fgsm.npz")


def batch_of(fx):
    b = {k[4:]: v.clone() for k, v in fx.items() if k.startswith("in::")}
    b["dec_labels"] = None
    return b


def outside_margin(fx):
    """Elements whose sign is a statement about the attack: the golden's |g| >= margin * max|g| (max over the tensor), or g == 0."""
    g = fx["d_feats"]
    return (g.abs() >= fx["sign_margin"].item() * g.abs().max()) | (g == 0)


def test_fixture_states_its_own_conditions(fx):
    g, rel = fx["d_feats"], fx["gt_relevance"]
    assert rel.tolist() == pytest.approx([0.5, 0, 1, 0, 0, 0.2, 0, 0])
    assert fx["sign_margin"].item() == 1e-3 and fx["max_share"].item() == 0.05
    hit = fx["sign_margin_rows"].tolist()
    assert hit == [b for b in range(8) if rel[b] != 0]
    inside = ~outside_margin(fx)
    for i, b in enumerate(hit):
        share = inside[b].float().mean().item()
        assert abs(share - fx["sign_margin_share"][i].item()) < 1e-9 and share <= 0.05
    for b in range(8):
        if b not in hit:
            assert bool((g[b] == 0).all())
    assert bool((fx["in::enc_image_mask"][2, -2:] == 0).all()) and bool((g[2, -2:] == 0).all())
    ids, after = fx["in::dec_input_ids"], fx["dec_input_ids_after"]
    assert int((ids == 102).sum()) == 8 and torch.equal(after, ids.masked_fill(ids == 102, 0))
    for r in range(2):          # one context per round, ragged between the rounds
        for k in ("in::enc_input_ids", "in::enc_segments", "in::enc_attention_mask"):
            assert bool((fx[k][4 * r:4 * r + 4] == fx[k][4 * r]).all())
    assert fx["in::enc_attention_mask"].sum(1).tolist() == [17.0] * 4 + [24.0] * 4


def test_oracle_reproduces_the_attack(fx, tiny_cfg, tiny_state):
    """evaluate_gen_attack.py:101-131 on the oracle: per-token losses, d loss / d features, perturbed features."""
    enc, dec = tiny_cfg
    b = batch_of(fx)
    x = b["enc_image_features"].clone().requires_grad_(True)
    b["enc_image_features"] = x
    out = O.model_forward(tiny_state, enc, dec, b, loss_reduction=False)
    per_token = out["loss"]
    assert (per_token.detach() - fx["loss_none"]).abs().max().item() <= TOL
    n, U = b["dec_input_ids"].shape
    (per_token.view(n, U).mean(dim=1) * fx["gt_relevance"]).sum().backward()
    g, ref = x.grad, fx["d_feats"]
    assert (g - ref).abs().max().item() <= TOL
    # the same statement at the gradient's own scale (max|g| is ~2e-5 here): the project's fp32 gradient gate, 2e-4 of the maximum
    assert (g - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()
    assert torch.equal(b["dec_input_ids"], fx["dec_input_ids_after"])
    ok = outside_margin(fx)
    for tag in ("e1", "e01"):
        adv = x.detach() + fx["epsilon::" + tag].item() * torch.sign(g)
        assert ((adv - fx["adv_feats::" + tag]).abs()[ok]).max().item() <= TOL
        # and the second forward, on the golden's perturbed features and the mutated ids
        b2 = dict(batch_of(fx), enc_image_features=fx["adv_feats::" + tag].clone(), dec_input_ids=fx["dec_input_ids_after"].clone())
        with torch.no_grad():
            logits = O.model_forward(tiny_state, enc, dec, b2)["logits"]
        assert (logits - fx["logits::" + tag]).abs().max().item() <= 2e-5          # the activation tolerance of test_oracle_golden
        sc = O.answer_scores(logits, fx["in::dec_input_ids"])
        assert (sc - fx["answer_scores::" + tag]).abs().max().item() <= 1e-4


def test_text_attacks_are_refused_by_name():
    from gst_visdial_amd import attack
    for name, needs in (("coreference", "coreference dependencies"), ("random_token", "BertForMaskedLM")):
        with pytest.raises(NotImplementedError) as e:
            attack.forward_attack(None, {}, dict(attack=name, device=torch.device("cpu")))
        assert name in str(e.value) and needs in str(e.value) and "counter-fitted" in str(e.value)
    with pytest.raises(NotImplementedError):
        attack.forward_attack(None, {}, dict(attack="pgd", device=torch.device("cpu")))
    with pytest.raises(NotImplementedError):
        attack.evaluate_attack(None, [], dict(attack="coreference", device=torch.device("cpu")))


def test_relevant_row_subset_host_logic(fx):
    """A fake gradient pass: the subset it receives is the non-zero-relevance rows with their UNMUTATED decoder ids, zero-relevance
    rows come back bit for bit (negative zeros included), the caller's decoder ids are mutated on every row."""
    from gst_visdial_amd import attack
    model = types.SimpleNamespace(decoder=types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=102, pad_token_id=0)))
    kw = dict.fromkeys(attack._MODEL_KEYS)
    kw.update(batch_of(fx))
    kw["enc_image_features"][1, 0, :3] = -0.0
    feats0, ids0 = kw["enc_image_features"].clone(), kw["dec_input_ids"].clone()
    seen = {}

    def fake_grad(m, sub, weights, inputs_only):
        seen.update(sub=sub, weights=weights.clone(), inputs_only=inputs_only)
        x = sub["enc_image_features"].clone()
        g = torch.ones_like(x)
        g[:, 0] = -1.0
        g[:, 1] = 0.0
        return x, g

    adv = attack.fgsm_features(model, kw, fx["gt_relevance"], 0.25, grad_fn=fake_grad)
    rows = [0, 2, 5]
    assert attack.relevant_rows(fx["gt_relevance"]).tolist() == rows
    assert seen["inputs_only"] is True and seen["weights"].tolist() == pytest.approx([0.5, 1.0, 0.2])
    for k, v in seen["sub"].items():
        assert v is None or v.shape[0] == 3, k
    assert torch.equal(seen["sub"]["dec_input_ids"], ids0[rows]) and torch.equal(seen["sub"]["enc_input_ids"], kw["enc_input_ids"][rows])
    rest = [b for b in range(8) if b not in rows]
    assert torch.equal(adv[rest].view(torch.int32), feats0[rest].view(torch.int32))          # bit for bit
    assert torch.equal(adv[rows][:, 0], feats0[rows][:, 0] - 0.25) and torch.equal(adv[rows][:, 2:], feats0[rows][:, 2:] + 0.25)
    assert torch.equal(adv[rows][:, 1], feats0[rows][:, 1])
    assert torch.equal(kw["dec_input_ids"], fx["dec_input_ids_after"])                      # every row, not only the subset
    assert torch.equal(kw["enc_image_features"], feats0)                                    # the caller's features are not written
    # all rows relevant: no gather, same contract
    kw["dec_input_ids"] = ids0.clone()
    adv = attack.fgsm_features(model, kw, torch.ones(8), 0.25, grad_fn=fake_grad)
    assert torch.equal(seen["sub"]["dec_input_ids"], ids0) and torch.equal(kw["dec_input_ids"], fx["dec_input_ids_after"])
    assert torch.equal(adv[:, 2:], feats0[:, 2:] + 0.25)
    # no row relevant: nothing runs, everything comes back
    kw["dec_input_ids"] = ids0.clone()
    seen.clear()
    adv = attack.fgsm_features(model, kw, torch.zeros(8), 0.25, grad_fn=fake_grad)
    assert not seen and torch.equal(adv.view(torch.int32), feats0.view(torch.int32)) and torch.equal(kw["dec_input_ids"], fx["dec_input_ids_after"])
    with pytest.raises(ValueError):
        attack.fgsm_features(model, dict(kw, dec_labels=ids0), torch.zeros(8), 0.25, grad_fn=fake_grad)


def test_attacked_round_is_read_from_the_separators():
    from gst_visdial_amd import attack
    sep = torch.tensor([[4, 9, 13, 20, 0, 0], [4, 9, 13, 20, 0, 0]])
    assert attack.attacked_round(dict(enc_sep_indices=sep, round_id=torch.tensor([[2]])))
    assert not attack.attacked_round(dict(enc_sep_indices=sep, round_id=torch.tensor([[3]])))
