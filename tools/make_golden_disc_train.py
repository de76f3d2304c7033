"""Fixture of the discriminative (enc_only_a) TRAINING step: tests/golden/tiny_disc_train.npz, the counterpart of
tools/make_golden_disc.py.

Runs in the build container only.  It imports the reference tree through oracle.ref_harness (`_install_shims`,
`write_tiny_configs`) and copies none of its text: it constructs the reference's VisualDialogEncoder (model = 'enc_only_a',
mode = 'vd_train') on the tiny config, puts it in eval() (no dropout draws: the result is deterministic), CALLS it with the
arguments and in the order train_disc.forward does (train_disc.py:27-124: randperm row sampling, sequence lengths from
sep_indices / hist_len, the reference's sequence_mask, .mean() and the three coefficients) and records what comes back.

    python tools/make_golden_disc_train.py

What is recorded (state::* = the encoder's state dict, in::* = the batch in the disc train dataloader's layout with the image
tensors once per dialog, row::* = the sampled rows as the encoder received them):
  * 2 dialogs x 2 rounds x 3 samples (1 positive + 2 negatives), T = 40, R = 7; ragged text; dialog 1 has padded regions;
    3-6 masked tokens per row ([MASK] = 103 in the inputs, the original id in `mask`, -1 elsewhere), one row with none;
    1-2 masked regions per dialog; soft NSP labels [1, 0] / [0, 1] and one dense-style [0.3, 0.7]; image_target rows that sum
    to 1 with exact zeros;
  * the three losses, seq_relationship_score, the weighted totals for the coefficient triples (1, 1, 1) and COEFFS2;
  * after loss.backward() (coefficients (1, 1, 1)) the gradients named in GRADS and d loss / d image_feat;
  * the three losses before and after each of three plain-SGD steps (lr 0.1) on the same rows.

As in make_golden_disc.py the Linear weights of the encoder, the poolers and the heads are re-drawn at larger standard deviations
(with N(0, 0.02) everywhere the gradients would be a statement about rounding); the word table, which is also the MLM decoder,
is re-drawn at WORD_STD for the same reason.  One value differs from make_golden_disc.py: the pooler weights are drawn at 0.05, not
0.25.  At 0.25 the fused value pt * pv reaches ~10 and plain SGD at lr 0.1 is unstable IN THE REFERENCE (its NSP loss went
3.7 -> 4.8 -> 18.1 -> 13.9 over the three steps, and as wildly for five other seeds): a trajectory that amplifies rounding
differences cannot be compared at 2e-4, and "the loss went down" would be false of the reference itself.  At 0.05 the recorded
total goes 9.04 -> 7.26 -> 8.70 -> 8.56.

ReLU ties.  The two poolers are Linear + ReLU on ONE row per batch row, and the gradient of a pooler weight is a DISCONTINUOUS
function of the encoder's output where a pre-activation crosses zero: an element decided the other way adds or removes its
whole term dpt[b, n] * x0[b, :].  As drawn, 1 % of the 2 x 12 x 128 pre-activations lay within 5e-3 of zero, so the comparison
of a reduced-precision run would be a statement about which side of zero rounding puts them on (the analogue of the
near-equal probabilities make_golden_disc.separate_ties removes from the ranking fixture).  `separate_relu_ties` therefore
moves each pooler bias to the value nearest the drawn one for which no pre-activation of its column lies within MIN_PRE of
zero.  MIN_PRE = 2^-5: four bf16 ulps at the pre-activations' own scale (|a| up to ~1, ulp 2^-7), i.e. the size of a few
rounding steps of the inputs, taken from the number format and not from any run; the fixture stores it and
tests/test_disc_train_cpu.py re-checks it on the restatement.
"""
import os
import sys
import tempfile
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                      # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, GOLDEN   # noqa: E402

ENC_STD, POOLER_STD, HEAD_STD, WORD_STD = 0.15, 0.05, 0.12, 0.1
B, ROUNDS, SAMPLES, T, R, MAX_SEP = 2, 2, 3, 40, 7, 6
CLS, SEP, MASK, V0, V1 = 101, 102, 103, 110, 320
COEFFS2 = (0.7, 2.0, 1.3)                                 # (lm, nsp, img)
SAMPLE_SEED, LR, STEPS = 21, 0.1, 3
MIN_PRE = 2.0 ** -5                                       # no pooler pre-activation closer to zero than this (see above)
P = "bert_pretrained."
GRADS = [P + "bert.embeddings.word_embeddings.weight", P + "cls.predictions.transform.dense.weight", P + "cls.predictions.bias",
         P + "cls.imagePredictions.decoder.weight", P + "bert.t_pooler.dense.weight", P + "bert.v_pooler.dense.weight",
         P + "cls.bi_seq_relationship.weight", P + "cls.bi_seq_relationship.bias",
         P + "bert.encoder.layer.1.attention.self.query.weight", P + "bert.encoder.v_layer.0.output.dense.weight",
         P + "bert.encoder.c_layer.1.biattention.key2.weight"]


def words(g, lo=2, hi=6):
    return torch.randint(V0, V1, (int(torch.randint(lo, hi, (1,), generator=g)),), generator=g).tolist()


def encode_row(utterances):
    ids, seg, seps, cur = [CLS], [0], [], 0
    for u in utterances:
        ids += u + [SEP]
        seg += [cur] * (len(u) + 1)
        seps.append(len(ids) - 1)
        cur ^= 1
    assert len(ids) <= T and len(seps) <= MAX_SEP
    n = len(ids)
    return (ids + [0] * (T - n), seg + [0] * (T - n), seps + [0] * (MAX_SEP - len(seps)), len(seps) - 1)


def separate_relu_ties(lin, pre):
    """`pre` [rows, Hb]: the pre-activations lin produced for the fixture's rows.  Shift each bias by the smallest amount after
    which every pre-activation of its column is at least MIN_PRE away from zero; -> number of biases moved."""
    moved = 0
    with torch.no_grad():
        for n in range(pre.shape[1]):
            a = pre[:, n].double()
            if a.abs().min() >= MIN_PRE:
                continue
            v = torch.sort(-a)[0]                                  # shift d is admissible iff |d - v_i| >= MIN_PRE for every i
            cand = torch.cat([v - MIN_PRE, v + MIN_PRE]) * (1.0 + 1e-6)
            ok = [(abs(d.item()), d.item()) for d in cand if bool(((d - v).abs() >= MIN_PRE).all())]
            lin.bias[n] += min(ok)[1]
            moved += 1
    return moved


def main():
    mods = RH._install_shims()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda x, *a, **k: x)
    from utils.data_utils import sequence_mask as ref_sequence_mask
    enc_cfg, dec_cfg = RH.write_tiny_configs(tempfile.mkdtemp(prefix="gstvd_disc_train_"))
    n = B * ROUNDS * SAMPLES
    params = dict(model_enc_config=enc_cfg, model_dec_config=dec_cfg, gpu_ids=[0], model="enc_only_a", mode="vd_train",
                  batch_size=n, device=torch.device("cpu"), lm_loss_coeff=1.0, nsp_loss_coeff=1.0, img_loss_coeff=1.0)
    torch.manual_seed(31)
    enc = mods["E"].VisualDialogEncoder(params)
    enc.eval()
    g = torch.Generator().manual_seed(32)
    bert, cls = enc.bert_pretrained.bert, enc.bert_pretrained.cls
    C = cls.imagePredictions.decoder.weight.shape[0]
    with torch.no_grad():
        for m in bert.encoder.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * ENC_STD)
        for lin in (bert.t_pooler.dense, bert.v_pooler.dense):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * POOLER_STD)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * HEAD_STD)
        cls.bi_seq_relationship.weight.copy_(torch.randn(cls.bi_seq_relationship.weight.shape, generator=g) * HEAD_STD)
        cls.bi_seq_relationship.bias.copy_(torch.randn(2, generator=g) * HEAD_STD)
        bert.embeddings.word_embeddings.weight.copy_(torch.randn(bert.embeddings.word_embeddings.weight.shape, generator=g) * WORD_STD)
        for lin in (cls.predictions.transform.dense, cls.imagePredictions.transform.dense, cls.imagePredictions.decoder):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * ENC_STD)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * HEAD_STD)
        cls.predictions.bias.copy_(torch.randn(cls.predictions.bias.shape, generator=g) * HEAD_STD)
    assert cls.predictions.decoder.weight is bert.embeddings.word_embeddings.weight

    # ---- the batch, in the loader's layout (image tensors once per dialog) -----------------------------------------------------
    feat = torch.randn(B, R, RH.TINY_ENC_CFG["v_feature_size"], generator=g)
    loc = torch.rand(B, R, 5, generator=g)
    imask = torch.ones(B, R, dtype=torch.long)
    imask[1, R - 2:] = 0
    feat, loc = feat * imask[..., None].float(), loc * imask[..., None].float()
    image_label = torch.full((B, R), -1, dtype=torch.long)
    image_label[0, [1, 4]] = 1
    image_label[1, [2]] = 1
    image_target = torch.rand(B, R, C, generator=g) * (torch.rand(B, R, C, generator=g) < 0.6).float()
    image_target[..., 0] += 0.05
    image_target = image_target / image_target.sum(-1, keepdim=True)
    assert int((image_target == 0).sum()) > 10

    tok = torch.zeros(B, ROUNDS, SAMPLES, T, dtype=torch.long)
    seg, sep = torch.zeros_like(tok), torch.zeros(B, ROUNDS, SAMPLES, MAX_SEP, dtype=torch.long)
    hl = torch.zeros(B, ROUNDS, SAMPLES, dtype=torch.long)
    mask = torch.full((B, ROUNDS, SAMPLES, T), -1, dtype=torch.long)
    nsl = torch.zeros(B, ROUNDS, SAMPLES, 2)
    for b in range(B):
        for r in range(ROUNDS):
            ctx = [words(g) for _ in range(2 + r + b)]
            for s in range(SAMPLES):
                i, sg, p_, h = encode_row(ctx + [words(g)])
                tok[b, r, s], seg[b, r, s], sep[b, r, s], hl[b, r, s] = torch.tensor(i), torch.tensor(sg), torch.tensor(p_), h
                nsl[b, r, s] = torch.tensor([1.0, 0.0] if s == 0 else [0.0, 1.0])
                if (b, r, s) == (1, 0, 2):
                    continue                                   # the row without a masked token
                cand = [t for t in range(1, T) if int(tok[b, r, s, t]) >= V0]
                k = int(torch.randint(3, 7, (1,), generator=g))
                for t in [cand[j] for j in torch.randperm(len(cand), generator=g)[:k].tolist()]:
                    mask[b, r, s, t] = tok[b, r, s, t]
                    tok[b, r, s, t] = MASK
    nsl[0, 1, 0] = torch.tensor([0.3, 0.7])                      # -train_dense style soft label

    # ---- train_disc.forward's call sequence ---------------------------------------------------------------------------------
    def sampled_rows():
        torch.manual_seed(SAMPLE_SEED)
        idx = torch.randperm(n)[:params["batch_size"]]
        ex = lambda x: x.unsqueeze(1).unsqueeze(1).expand(B, ROUNDS, SAMPLES, *x.shape[1:]).contiguous().view(n, *x.shape[1:])
        rows = dict(tokens=tok.view(n, T)[idx], segments=seg.view(n, T)[idx], sep_indices=sep.view(n, MAX_SEP)[idx],
                    mask=mask.view(n, T)[idx], hist_len=hl.view(n)[idx], next_sentence_labels=nsl.view(n, 2)[idx],
                    image_feat=ex(feat)[idx], image_loc=ex(loc)[idx], image_mask=ex(imask)[idx],
                    image_target=ex(image_target)[idx], image_label=ex(image_label)[idx])
        lengths = (torch.gather(rows["sep_indices"], 1, rows["hist_len"].view(-1, 1)) + 1).squeeze(1)
        rows["attention_mask"] = ref_sequence_mask(lengths, params, max_len=T)
        return idx, rows

    def call(rows, feat_rows):
        out = enc(rows["tokens"], feat_rows, rows["image_loc"], sep_indices=rows["sep_indices"], token_type_ids=rows["segments"],
                  masked_lm_labels=rows["mask"], attention_mask=rows["attention_mask"],
                  next_sentence_label=rows["next_sentence_labels"], image_attention_mask=rows["image_mask"],
                  image_label=rows["image_label"], image_target=rows["image_target"])
        lm, img, nsp, z = out[0], out[1], out[2], out[3]
        assert tuple(lm.shape) == tuple(img.shape) == tuple(nsp.shape) == (1,)
        return lm.mean(), img.mean(), nsp.mean(), z

    idx, rows = sampled_rows()
    pre, hooks = {}, []
    for name, lin in (("t", bert.t_pooler.dense), ("v", bert.v_pooler.dense)):
        hooks.append(lin.register_forward_hook(lambda m, i, o, name=name: pre.__setitem__(name, o.detach().clone())))
    with torch.no_grad():
        call(rows, rows["image_feat"])
        print("pooler biases moved off ReLU ties:", separate_relu_ties(bert.t_pooler.dense, pre["t"]),
              separate_relu_ties(bert.v_pooler.dense, pre["v"]))
        call(rows, rows["image_feat"])
    for h in hooks:
        h.remove()
    min_pre = min(pre["t"].abs().min().item(), pre["v"].abs().min().item())
    print("smallest |pooler pre-activation| %.4f (MIN_PRE %.4f)" % (min_pre, MIN_PRE))
    assert min_pre >= MIN_PRE
    fr = rows["image_feat"].clone().requires_grad_(True)
    lm, img, nsp, z = call(rows, fr)
    total = 1.0 * lm + 1.0 * nsp + 1.0 * img
    total2 = COEFFS2[0] * lm + COEFFS2[1] * nsp + COEFFS2[2] * img
    enc.zero_grad()
    total.backward()
    named = dict(enc.named_parameters())
    no_grad = sorted(k for k, p_ in named.items() if p_.grad is None)
    print("losses lm %.6f img %.6f nsp %.6f | total %.6f total2 %.6f" % (lm.item(), img.item(), nsp.item(), total.item(), total2.item()))
    print("parameters without a gradient:", no_grad)
    out = {"state::" + k: v.detach().clone().numpy() for k, v in enc.state_dict().items()}
    out.update({"in::tokens": tok.numpy(), "in::segments": seg.numpy(), "in::sep_indices": sep.numpy(), "in::mask": mask.numpy(),
                "in::hist_len": hl.numpy(), "in::next_sentence_labels": nsl.numpy(), "in::image_feat": feat.numpy(),
                "in::image_loc": loc.numpy(), "in::image_mask": imask.numpy(), "in::image_target": image_target.numpy(),
                "in::image_label": image_label.numpy()})
    out.update({"row::" + k: v.numpy() for k, v in rows.items()})
    out.update({"sample_indices": idx.numpy(), "sample_seed": torch.tensor(SAMPLE_SEED).numpy(),
                "lm_loss": lm.detach().numpy(), "img_loss": img.detach().numpy(), "nsp_loss": nsp.detach().numpy(),
                "seq_relationship_score": z.detach().numpy(), "total": total.detach().numpy(), "total2": total2.detach().numpy(),
                "coeffs2": torch.tensor(COEFFS2, dtype=torch.float64).numpy(),
                "grad::image_feat": fr.grad.numpy()})
    for k in GRADS:
        out["grad::" + k] = named[k].grad.detach().clone().numpy()
        print("grad %-70s max %.3e" % (k, named[k].grad.abs().max().item()))
    out["no_grad_names"] = "\n".join(no_grad).encode()
    import numpy as np
    out["no_grad_names"] = np.frombuffer(out["no_grad_names"], dtype=np.uint8)

    # ---- three plain-SGD steps on the same rows -------------------------------------------------------------------------------
    traj = []
    for step in range(STEPS + 1):
        enc.zero_grad()
        lm, img, nsp, _ = call(rows, rows["image_feat"])
        traj.append([lm.item(), img.item(), nsp.item()])
        if step == STEPS:
            break
        (lm + nsp + img).backward()
        with torch.no_grad():
            for p_ in enc.parameters():
                if p_.grad is not None:
                    p_.add_(p_.grad, alpha=-LR)
    print("trajectory (lm, img, nsp):", traj)
    out["sgd_losses"] = torch.tensor(traj, dtype=torch.float64).numpy()
    out["sgd_lr"] = torch.tensor(LR, dtype=torch.float64).numpy()
    out["min_pre"] = torch.tensor(MIN_PRE, dtype=torch.float64).numpy()
    files = write_npz(os.path.join(GOLDEN, "tiny_disc_train.npz"), out)
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
