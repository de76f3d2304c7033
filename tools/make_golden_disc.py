"""Fixture of the discriminative (enc_only_a) evaluation: tests/golden/tiny_disc.npz.

Runs in the build container only: it is the one file of this feature that imports the reference tree, through
oracle.ref_harness (`_install_shims`, `write_tiny_configs`), and it copies none of its text -- it CALLS the reference's
VisualDialogEncoder (model = 'enc_only_a', mode = 'vd_eval_val'), its utils.data_utils.sequence_mask and its
utils.visdial_metrics classes, in the order evaluate_disc.py:27-118 / train_disc.py:27-124 call them, and records what they return.

    python tools/make_golden_disc.py

What is recorded (state::* = the encoder's state dict, in::* = the batch in the disc eval dataloader's layout):
  * 2 dialogs x 3 rounds x 10 options, ragged rows (3 .. 5 utterances, zero padded to T = 40), 7 image regions per dialog of
    which the last 1 .. 3 are padding (image_mask 0); sep_indices, hist_len, gt_option_inds, gt_relevance, round_id;
  * seq_relationship_score [60, 2], prob0 [2, 3, 10], the reference's ranks and its metric values.

BERT's N(0, 0.02) initialisation makes every NSP logit nearly equal (the ranking would be a statement about rounding), so the
two pooler weights are re-drawn at N(0, POOLER_STD), their biases and bi_seq_relationship at N(0, HEAD_STD).  That alone does
not separate the options of a ROUND: with 0.02-scale attention and FFN weights the first token's final state moves by ~1e-3
between two answers (all 54 neighbouring pairs stayed within 0.02 of each other through 200 re-draws), so the Linear weights of
the encoder's text / vision / connection layers are re-drawn at N(0, ENC_STD) as well -- attention that is not uniform, the state
of a trained checkpoint in that respect (round 4's fixture used a trained one for the same reason).  Options whose
prob0 lies closer than MIN_GAP to a neighbour of the same round get a fresh random answer until no such pair is left (the
precedent: oracle/make_golden_r4.separate_ties); the fixture stores MIN_GAP and tests/test_disc_cpu.py re-checks it.
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

ENC_STD, POOLER_STD, HEAD_STD, MIN_GAP = 0.15, 0.25, 0.12, 0.01
B, ROUNDS, OPTIONS, T, R, MAX_SEP = 2, 3, 10, 40, 7, 6
CLS, SEP, V0, V1 = 101, 102, 110, 320
ROWS_PER_CALL = 20                                        # the reference's 200-row chunks, scaled to 60 rows


def words(g, lo=1, hi=5):
    return torch.randint(V0, V1, (int(torch.randint(lo, hi, (1,), generator=g)),), generator=g).tolist()


def encode_row(utterances):
    """[CLS] u0 [SEP] u1 [SEP] ... zero padded; segments alternate per utterance; sep_indices / hist_len as the disc loader
    stores them (positions of the [SEP]s, zero padded; index of the last one)."""
    ids, seg, seps, cur = [CLS], [0], [], 0
    for u in utterances:
        ids += u + [SEP]
        seg += [cur] * (len(u) + 1)
        seps.append(len(ids) - 1)
        cur ^= 1
    assert len(ids) <= T and len(seps) <= MAX_SEP
    n = len(ids)
    return (ids + [0] * (T - n), seg + [0] * (T - n), seps + [0] * (MAX_SEP - len(seps)), len(seps) - 1)


def materialize(ctx, answers):
    tok = torch.zeros(B, ROUNDS, OPTIONS, T, dtype=torch.long)
    seg, sep = torch.zeros_like(tok), torch.zeros(B, ROUNDS, OPTIONS, MAX_SEP, dtype=torch.long)
    hl = torch.zeros(B, ROUNDS, OPTIONS, dtype=torch.long)
    for b in range(B):
        for r in range(ROUNDS):
            for o in range(OPTIONS):
                i, s, p, h = encode_row(ctx[b][r] + [answers[b][r][o]])
                tok[b, r, o], seg[b, r, o], sep[b, r, o], hl[b, r, o] = torch.tensor(i), torch.tensor(s), torch.tensor(p), h
    return tok, seg, sep, hl


def main():
    mods = RH._install_shims()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda x, *a, **k: x)
    from utils.data_utils import sequence_mask as ref_sequence_mask
    _, vm, _ = RH.reference_utils()
    enc_cfg, dec_cfg = RH.write_tiny_configs(tempfile.mkdtemp(prefix="gstvd_disc_"))
    params = dict(model_enc_config=enc_cfg, model_dec_config=dec_cfg, gpu_ids=[0], model="enc_only_a", mode="vd_eval_val",
                  batch_size=1, device=torch.device("cpu"))
    torch.manual_seed(11)
    enc = mods["E"].VisualDialogEncoder(params)
    enc.eval()
    g = torch.Generator().manual_seed(12)
    bert, cls = enc.bert_pretrained.bert, enc.bert_pretrained.cls
    with torch.no_grad():
        for m in bert.encoder.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * ENC_STD)
        for lin in (bert.t_pooler.dense, bert.v_pooler.dense):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * POOLER_STD)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * HEAD_STD)
        cls.bi_seq_relationship.weight.copy_(torch.randn(cls.bi_seq_relationship.weight.shape, generator=g) * HEAD_STD)
        cls.bi_seq_relationship.bias.copy_(torch.randn(2, generator=g) * HEAD_STD)

    feat = torch.randn(B, R, RH.TINY_ENC_CFG["v_feature_size"], generator=g)
    loc = torch.rand(B, R, 5, generator=g)
    imask = torch.ones(B, R, dtype=torch.long)
    imask[0, R - 1:] = 0
    imask[1, R - 3:] = 0
    feat, loc = feat * imask[..., None].float(), loc * imask[..., None].float()
    ctx = [[[words(g) for _ in range(2 + r)] for r in range(ROUNDS)] for _ in range(B)]
    answers = [[[words(g) for _ in range(OPTIONS)] for _ in range(ROUNDS)] for _ in range(B)]
    gt_inds = torch.randint(0, OPTIONS, (B, ROUNDS), generator=g)
    round_id = torch.tensor([[2], [3]])
    rel = torch.zeros(B, OPTIONS)
    for b in range(B):
        rel[b, gt_inds[b, round_id[b, 0] - 1]] = 1.0
        for o in torch.randperm(OPTIONS, generator=g)[:3].tolist():
            rel[b, o] = max(float(rel[b, o]), float(torch.randint(1, 5, (1,), generator=g)) / 4.0 * 0.8)

    def reference_scores():
        """evaluate_disc.py:31-87 on this batch: flatten, expand the image tensors per option, chunks through the eval branch of
        train_disc.forward (sequence lengths from sep_indices / hist_len, the reference's sequence_mask), softmax column 0."""
        tok, seg, sep, hl = materialize(ctx, answers)
        n = B * ROUNDS * OPTIONS
        ftok, fseg, fsep, fhl = tok.view(n, T), seg.view(n, T), sep.view(n, MAX_SEP), hl.view(n)
        ex = lambda x: x.unsqueeze(1).unsqueeze(1).expand(B, ROUNDS, OPTIONS, *x.shape[1:]).contiguous().view(n, *x.shape[1:])
        ff, fl, fm = ex(feat), ex(loc), ex(imask)
        zs, ps, masks = [], [], []
        with torch.no_grad():
            for s in range(0, n, ROWS_PER_CALL):
                e = slice(s, s + ROWS_PER_CALL)
                lengths = (torch.gather(fsep[e], 1, fhl[e].view(-1, 1)) + 1).squeeze(1)
                att = ref_sequence_mask(lengths, params, max_len=T)
                out = enc(ftok[e], ff[e], fl[e], sep_indices=fsep[e], token_type_ids=fseg[e], masked_lm_labels=torch.zeros_like(ftok[e]),
                          attention_mask=att, image_attention_mask=fm[e])
                z = out[3]
                zs.append(z)
                ps.append(torch.softmax(z, dim=1)[:, 0])
                masks.append(att)
        return (tok, seg, sep, hl), torch.cat(zs), torch.cat(ps).view(B, ROUNDS, OPTIONS), torch.cat(masks)

    for it in range(400):
        batch, z, prob0, att = reference_scores()
        srt, idx = prob0.sort(-1)
        close = (srt[..., 1:] - srt[..., :-1]) < MIN_GAP
        print("pass %d: %d neighbouring pairs closer than %g; prob0 range %.3f .. %.3f" %
              (it, int(close.sum()), MIN_GAP, prob0.min().item(), prob0.max().item()), flush=True)
        if not close.any():
            break
        for b, r, j in close.nonzero().tolist():
            o = int(idx[b, r, j + 1])
            if o == int(gt_inds[b, r]):
                o = int(idx[b, r, j])
            answers[b][r][o] = words(g)
    else:
        raise RuntimeError("ties not separated")

    tok, seg, sep, hl = batch
    sparse, ndcg = vm.SparseGTMetrics(), vm.NDCG()
    sparse.observe(prob0, gt_inds)
    ndcg.observe(prob0[torch.arange(B), round_id.squeeze(1) - 1, :], rel)
    metrics = {}
    metrics.update(sparse.retrieve(reset=True))
    metrics.update(ndcg.retrieve(reset=True))
    ranks = vm.scores_to_ranks(prob0)
    print("metrics", metrics)
    print("z range", z.min().item(), z.max().item(), "smallest gap", (srt[..., 1:] - srt[..., :-1]).min().item())

    out = {"state::" + k: v.detach().clone().numpy() for k, v in enc.state_dict().items()}
    out.update({"in::tokens": tok.numpy(), "in::segments": seg.numpy(), "in::sep_indices": sep.numpy(),
                "in::mask": torch.zeros_like(tok).numpy(), "in::hist_len": hl.numpy(), "in::image_feat": feat.numpy(),
                "in::image_loc": loc.numpy(), "in::image_mask": imask.numpy(), "in::gt_option_inds": gt_inds.numpy(),
                "in::gt_relevance": rel.numpy(), "in::round_id": round_id.numpy(),
                "seq_relationship_score": z.numpy(), "prob0": prob0.numpy(), "attention_mask": att.numpy(),
                "ranks": ranks.numpy(),
                "sparse": torch.tensor([metrics[k] for k in ("r@1", "r@5", "r@10", "mean", "mrr")], dtype=torch.float64).numpy(),
                "ndcg": torch.tensor(metrics["ndcg"], dtype=torch.float64).numpy(),
                "min_gap": torch.tensor(MIN_GAP, dtype=torch.float64).numpy(),
                "enc_std": torch.tensor(ENC_STD, dtype=torch.float64).numpy(),
                "pooler_std": torch.tensor(POOLER_STD, dtype=torch.float64).numpy(),
                "head_std": torch.tensor(HEAD_STD, dtype=torch.float64).numpy(),
                "rows_per_call": torch.tensor(ROWS_PER_CALL).numpy()})
    files = write_npz(os.path.join(GOLDEN, "tiny_disc.npz"), out)
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
