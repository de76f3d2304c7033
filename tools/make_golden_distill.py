"""Fixture of the soft pseudo-label (distillation) step: tests/golden/tiny_distill.npz, modelled on tools/make_golden_rank.py.

Runs in the build container only.  It imports the reference tree through oracle.ref_harness and copies none of its text: it
constructs the reference's EncoderDecoderModel on the tiny config twice -- the student with the weights of
tests/golden/tiny_state.npz, the teacher with the reference's own initialisation under another seed -- in eval() and fp32, CALLS
both on the rows of tests/golden/tiny_train.npz and records what comes back.  The reference has no distillation loss; the rule
("Soft pseudo-labels") is restated in `distill_loss` below, in float64 on the reference's logits.

    python tools/make_golden_distill.py

What is recorded (the inputs are tiny_train.npz's in::*):
  * soft_ids int64 / soft_logp fp32 [3, 9, 4]: the top-4 of the teacher's log_softmax at every position; row 1 carries no soft
    label (ids -1, logp 0);
  * alpha = 0.5, tau = 2; loss (mean over the kept tokens), row_loss [3, 9], row_kd [3, 9];
  * grad::<key> for the parameters tiny_train.npz names (oracle.make_golden.GRAD_KEYS) and d_feats [3, 7, F].
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                   # noqa: E402
from oracle.make_golden import GRAD_KEYS, call_model                   # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, load_npz, GOLDEN      # noqa: E402

ALPHA, TAU, TOP_K, TEACHER_SEED, NO_SOFT_ROW = 0.5, 2.0, 4, 5, 1


def distill_loss(logits, labels, soft_ids, soft_logp, alpha, tau, pad=0):
    """float64: l = (1 - a) * ce + a * tau^2 * KL(q || softmax(x / tau)) per kept token (label != pad), a = alpha where
    soft_ids[..., 0] >= 0 and 0 elsewhere, q = softmax(soft_logp / tau) over the K entries -> (mean over the kept tokens, l, kd)."""
    x = logits.double()
    keep = labels != pad
    soft = keep & (soft_ids[..., 0] >= 0)
    lp = torch.log_softmax(x, -1)
    ce = -torch.gather(lp, -1, labels.unsqueeze(-1)).squeeze(-1) * keep
    lpt = torch.log_softmax(x / tau, -1)
    lq = torch.log_softmax(soft_logp.double() / tau, -1)
    q = lq.exp()
    kd = (q * (lq - torch.gather(lpt, -1, soft_ids.clamp_min(0)))).sum(-1) * soft
    a = alpha * soft.double()
    l = (1 - a) * ce + a * tau * tau * kd
    return l.sum() / keep.sum(), l, kd


def main():
    enc_cfg, dec_cfg = RH.write_tiny_configs(tempfile.mkdtemp(prefix="gstvd_distill_"))
    student, _ = RH.build_reference_model(enc_cfg, dec_cfg, mode="vd_train", seed=0)
    student.load_state_dict(load_npz("tiny_state.npz"), strict=True)
    student.eval()
    teacher, _ = RH.build_reference_model(enc_cfg, dec_cfg, mode="vd_train", seed=TEACHER_SEED)
    teacher.eval()
    g = load_npz("tiny_train.npz")
    inp = {k[4:]: v.clone() for k, v in g.items() if k.startswith("in::")}
    with torch.no_grad():
        _, t_logits = call_model(teacher, inp, inp["dec_input_ids"].clone(), inp["dec_labels"])
    t_logp, t_ids = torch.topk(torch.log_softmax(t_logits.double(), -1), TOP_K, dim=-1)
    soft_ids, soft_logp = t_ids.clone(), t_logp.float()
    soft_ids[NO_SOFT_ROW], soft_logp[NO_SOFT_ROW] = -1, 0.0
    feats = inp["enc_image_features"].clone().requires_grad_(True)
    student.zero_grad()
    _, logits = call_model(student, dict(inp, enc_image_features=feats), inp["dec_input_ids"].clone(), inp["dec_labels"])
    assert (logits.detach() - g["logits"]).abs().max().item() < 1e-5          # the student IS tiny_train.npz's model
    loss, row_loss, row_kd = distill_loss(logits, inp["dec_labels"], soft_ids, soft_logp, ALPHA, TAU)
    loss.backward()
    named = dict(student.named_parameters())
    out = dict(soft_ids=soft_ids, soft_logp=soft_logp, alpha=np.float64(ALPHA), tau=np.float64(TAU), loss=loss.detach(),
               row_loss=row_loss.detach(), row_kd=row_kd.detach(), d_feats=feats.grad)
    for k in GRAD_KEYS:
        out["grad::" + k] = named[k].grad.clone()
    print("loss %.8f (plain cross entropy %.8f); kd per token %.4f .. %.4f" % (float(loss.detach()), float(g["loss"]), float(row_kd.min()), float(row_kd.max())))
    files = write_npz(os.path.join(GOLDEN, "tiny_distill.npz"), {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
