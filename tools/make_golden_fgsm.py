"""Fixture of the FGSM attack evaluation: tests/golden/tiny_fgsm.npz, modelled on tools/make_golden_disc_train.py.

Runs in the build container only.  It imports the reference tree through oracle.ref_harness (`build_reference_model`,
`write_tiny_configs`) and copies none of its text: it constructs the reference's EncoderDecoderModel on the tiny config with
the weights of tests/golden/tiny_state.npz, in eval() and fp32, CALLS it the way evaluate_gen_attack.forward does
(evaluate_gen_attack.py:101-148; the script itself is not imported -- its dataloader / tokenizer imports are not installed) and
records what comes back.  The five arithmetic steps between the two forwards (evaluate_gen_attack.py:124-131) are restated in
`attack_loss` / `perturb` below.

    python tools/make_golden_fgsm.py

What is recorded (in::* = the 14 keyword tensors as the first forward receives them):
  * 8 rows = 2 dialog rounds x 4 answer options, T = 24, R = 7, U = 9.  Within a round the four rows carry the same context
    (round 0: 17 tokens, round 1: all 24), the options are ragged (2-7 tokens); every row shows the same image except row 2,
    whose last two regions are padding (mask 0, zero features and boxes);
  * gt_relevance = RELEVANCE (three non-zero rows: 0, 2, 5), epsilon = 1.0 and 0.1;
  * loss_none [64]: the per-token losses of the first forward;  d_feats: d (sum_b relevance[b] * mean_u loss[b, u]) / d features;
  * per epsilon `eN`: adv_feats::eN, logits::eN (second forward, on the perturbed features and the MUTATED decoder ids, as the
    reference's second forward sees them) and answer_scores::eN (evaluate_gen_attack.py:322-333, targets from the UNMUTATED ids);
  * dec_input_ids_after: the caller's decoder ids after the first forward ([SEP] -> [PAD] in place);
  * sign_margin_share [3], sign_margin_rows [3], sign_margin: see below.

Sign margin.  adv_feats depends on the gradient only through its sign, so an element whose gradient is within rounding of zero
is not a statement about the attack but about rounding.  The project's fp32 gradient gate is 2e-4 of the tensor's largest
magnitude; SIGN_MARGIN = 1e-3 of it leaves a factor five.  `sign_margin_share[i]` is the share of row sign_margin_rows[i]'s
elements with 0 < |g| < SIGN_MARGIN * max|g| (max over the whole tensor: the scale the gradient gate is stated in); the
generator asserts it is at most MAX_SHARE on every such row, and that every element of a zero-relevance row and of a padded
region is exactly 0.  Tests compare adv_feats only outside that margin and bound the excluded share by the same MAX_SHARE.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                   # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, load_npz, GOLDEN      # noqa: E402

ROUNDS, OPTIONS, T, R, U = 2, 4, 24, 7, 9
CLS, SEP, V0, V1 = 101, 102, 104, 320
RELEVANCE = [0.5, 0.0, 1.0, 0.0, 0.0, 0.2, 0.0, 0.0]
EPSILONS = {"e1": 1.0, "e01": 0.1}
SIGN_MARGIN, MAX_SHARE = 1e-3, 0.05
SEED = 41


def make_rows():
    g = torch.Generator().manual_seed(SEED)
    B, F = ROUNDS * OPTIONS, RH.TINY_ENC_CFG["v_feature_size"]
    ids, seg = torch.zeros(B, T, dtype=torch.long), torch.zeros(B, T, dtype=torch.long)
    for r, L in enumerate([17, T][:ROUNDS]):
        row = torch.zeros(T, dtype=torch.long)
        row[:L] = torch.randint(V0, V1, (L,), generator=g)
        row[0] = CLS
        row[3:L:4] = SEP
        row[L - 1] = SEP
        s, cur = torch.zeros(T, dtype=torch.long), 0
        for t in range(L):
            s[t] = cur
            if row[t] == SEP:
                cur ^= 1
        ids[r * OPTIONS:(r + 1) * OPTIONS], seg[r * OPTIONS:(r + 1) * OPTIONS] = row, s
    feat = torch.randn(R, F, generator=g).abs()
    feat[0] = feat[1:].mean(0)
    loc = torch.rand(R, 5, generator=g)
    loc[0] = torch.tensor([0., 0., 1., 1., 1.])
    feats, locs, imask = feat.repeat(B, 1, 1), loc.repeat(B, 1, 1), torch.ones(B, R)
    imask[2, -2:] = 0
    feats[2, -2:] = 0
    locs[2, -2:] = 0
    dec_ids, dec_att = torch.zeros(B, U, dtype=torch.long), torch.zeros(B, U)
    for b, L in enumerate([5, 3, 7, 2, 4, 6, 3, 7]):
        dec_ids[b, 0] = CLS
        dec_ids[b, 1:1 + L] = torch.randint(V0, V1, (L,), generator=g)
        dec_ids[b, 1 + L] = SEP
        dec_att[b, :L + 2] = 1
    return dict(enc_image_features=feats, enc_image_spatials=locs, enc_image_mask=imask, enc_input_ids=ids, enc_segments=seg,
                enc_sep_indices=torch.zeros(B, 5, dtype=torch.long), enc_mlm_labels=torch.full((B, T), -1),
                enc_attention_mask=(ids != 0).float(), dec_input_ids=dec_ids, dec_attention_mask=dec_att)


def call(model, rows, feats, dec_ids, **kw):
    return model(enc_image_features=feats, enc_image_spatials=rows["enc_image_spatials"], enc_image_mask=rows["enc_image_mask"],
                 enc_image_target=None, enc_image_label=None, enc_next_sentence_labels=None, enc_input_ids=rows["enc_input_ids"],
                 enc_segments=rows["enc_segments"], enc_sep_indices=rows["enc_sep_indices"], enc_mlm_labels=rows["enc_mlm_labels"],
                 enc_attention_mask=rows["enc_attention_mask"], dec_input_ids=dec_ids,
                 dec_attention_mask=rows["dec_attention_mask"], dec_labels=None, **kw)


def attack_loss(per_token, relevance, rows, length):
    """evaluate_gen_attack.py:126-128: per-token losses -> per-row means -> relevance-weighted sum."""
    return (per_token.view(rows, length).mean(dim=1) * relevance).sum()


def perturb(x, grad, epsilon):
    """evaluate_gen_attack.py:131."""
    return x + epsilon * torch.sign(grad)


def answer_scores(logits, ids_unmutated):
    """evaluate_gen_attack.py:322-333: log-probabilities of the left-shifted ids, [PAD] targets excluded, summed per row."""
    lp = torch.log_softmax(logits, dim=-1)
    tgt = ids_unmutated.new_zeros(ids_unmutated.shape)
    tgt[:, :-1] = ids_unmutated[:, 1:]
    return (lp.gather(-1, tgt.unsqueeze(-1)).squeeze(-1) * (tgt != 0).float()).sum(-1)


def main():
    enc_cfg, dec_cfg = RH.write_tiny_configs(tempfile.mkdtemp(prefix="gstvd_fgsm_"))
    model, params = RH.build_reference_model(enc_cfg, dec_cfg, mode="vd_eval_val", seed=0)
    model.load_state_dict(load_npz("tiny_state.npz"), strict=True)
    model.eval()
    rows = make_rows()
    B = ROUNDS * OPTIONS
    rel = torch.tensor(RELEVANCE)
    ids_before = rows["dec_input_ids"].clone()

    x = rows["enc_image_features"].clone().requires_grad_(True)
    dec_ids = rows["dec_input_ids"].clone()
    with torch.enable_grad():
        per_token, _ = call(model, rows, x, dec_ids, loss_reduction=False)
        loss = attack_loss(per_token, rel, B, U)
    model.zero_grad()
    loss.backward()
    g = x.grad.clone()
    assert not torch.equal(dec_ids, ids_before) and int((dec_ids == SEP).sum()) == 0

    gmax = g.abs().max().item()
    hit = [b for b in range(B) if RELEVANCE[b] != 0]
    share = []
    for b in range(B):
        if b in hit:
            a = g[b].abs()
            share.append(((a > 0) & (a < SIGN_MARGIN * gmax)).float().mean().item())
        else:
            assert bool((g[b] == 0).all()), "row %d has relevance 0 and a non-zero gradient" % b
    assert bool((g[2, -2:] == 0).all()), "a padded region has a non-zero gradient"
    print("max|g| %.4e; share of elements inside the sign margin per row %s: %s" % (gmax, hit, ["%.4f" % s for s in share]))
    assert max(share) <= MAX_SHARE, "sign margin share above %.2f: change SEED or the feature scale, not the bound" % MAX_SHARE

    out = {"in::" + k: v for k, v in rows.items()}
    out.update(gt_relevance=rel, loss_none=per_token.detach(), attack_loss=loss.detach(), d_feats=g, dec_input_ids_after=dec_ids,
               sign_margin_share=torch.tensor(share, dtype=torch.float64), sign_margin_rows=torch.tensor(hit),
               sign_margin=torch.tensor(SIGN_MARGIN, dtype=torch.float64), max_share=torch.tensor(MAX_SHARE, dtype=torch.float64))
    for tag, eps in EPSILONS.items():
        adv = perturb(x.detach(), g, eps)
        with torch.no_grad():
            _, logits = call(model, rows, adv, dec_ids)              # the ids the first forward left behind
        out["epsilon::" + tag] = torch.tensor(eps, dtype=torch.float64)
        out["adv_feats::" + tag] = adv
        out["logits::" + tag] = logits
        out["answer_scores::" + tag] = answer_scores(logits, ids_before)
        print("epsilon %.1f: answer scores %s" % (eps, ["%.3f" % s for s in out["answer_scores::" + tag].tolist()]))
    with torch.no_grad():
        _, clean = call(model, rows, rows["enc_image_features"], dec_ids)
    out["answer_scores::clean"] = answer_scores(clean, ids_before)
    files = write_npz(os.path.join(GOLDEN, "tiny_fgsm.npz"), {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v))
                                                             for k, v in out.items()})
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
