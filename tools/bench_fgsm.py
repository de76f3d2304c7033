"""Timing of the FGSM attack's gradient pass on one MI355X -> profiles/fgsm.txt.  Recorded, not gated.

Full config (bench.build_model), eval mode, 100 rows (one dialog round's answer options), T = 256, R = 37, U = 25, bf16 and fp32:
  (a) forward (loss_reduction=False) + the full per-token backward, parameter gradients included, as the reference runs it;
  (b) the same forward + the inputs-only backward (Engine.inputs_only);
  (c) as (b) on 30 rows -- the share of a round's options that typically carry a non-zero relevance;
  (d) the mean-loss forward + backward at the same 100 rows (the path that existed before; the yardstick);
  (e) attack.fgsm_features as a whole with 30 relevant rows of 100 (row gather, (c), the sign step, the scatter).
Every figure is the median of `--steps` individually timed iterations (HIP events around each, the device idle before each)
after `--warmup` untimed ones, with the min-max spread.  The file ends with the figures of the tiny fixture's second forward on
the engine's own perturbed features (tests/test_fgsm_gpu.py::test_second_forward measures the same).

    python tools/bench_fgsm.py [--rows 100] [--relevant 30] [--steps 10] [--warmup 3] [--out profiles/fgsm.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                             # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def measure(precision, a, dev):
    from gst_visdial_amd import attack
    model, _ = bench.build_model(dev, precision, 0)
    model.eval()
    c = model.encoder.config
    T, R, U, F = 256, 37, 25, c.v_feature_size
    full = bench.synthetic_rows(a.rows, T, R, U, F, c.vocab_size, 77, dev)
    # decoder ids as the eval loader has them: [CLS] answer [SEP]; labels come from them (dec_labels None)
    ids = full["dec_input_ids"].clone()
    ids[:, 1:] = torch.where(full["dec_labels"][:, :-1] == 102, torch.full_like(ids[:, 1:], 102), ids[:, 1:])
    kw = dict.fromkeys(attack._MODEL_KEYS)
    kw.update({k: v for k, v in full.items() if k != "dec_labels"})
    kw["dec_input_ids"] = ids
    part = {k: (v[:a.relevant] if v is not None else None) for k, v in kw.items()}
    rel = torch.zeros(a.rows)
    rel[torch.randperm(a.rows, generator=torch.Generator().manual_seed(5))[:a.relevant]] = 0.5
    w_full, w_part = torch.full((a.rows,), 0.5, device=dev), torch.full((a.relevant,), 0.5, device=dev)

    def grad_pass(k, w, inputs_only):
        attack._feature_grad(model, dict(k, dec_input_ids=k["dec_input_ids"].clone()), w, inputs_only)

    def mean_step():
        x = kw["enc_image_features"].detach().clone().requires_grad_(True)
        with torch.enable_grad():
            loss, _ = model(**dict(kw, enc_image_features=x, dec_input_ids=ids.clone()))
            loss.backward()

    runs = [("(a) forward + full per-token backward, %d rows" % a.rows, lambda: grad_pass(kw, w_full, False)),
            ("(b) forward + inputs-only backward, %d rows" % a.rows, lambda: grad_pass(kw, w_full, True)),
            ("(c) forward + inputs-only backward, %d rows" % a.relevant, lambda: grad_pass(part, w_part, True)),
            ("(d) mean-loss forward + backward, %d rows" % a.rows, mean_step),
            ("(e) attack.fgsm_features, %d relevant rows of %d" % (a.relevant, a.rows),
             lambda: attack.fgsm_features(model, dict(kw, dec_input_ids=ids.clone()), rel, 1.0))]
    lines = []
    for name, fn in runs:
        med, lo, hi = timed(fn, a.steps, a.warmup)
        lines.append("%-5s %-58s median %8.3f ms  (min %8.3f, max %8.3f, spread %4.1f %% of the median)"
                     % (precision, name, med, lo, hi, 100.0 * (hi - lo) / med))
        print(lines[-1], flush=True)
    del model
    torch.cuda.empty_cache()
    return lines


def tiny_second_forward(dev):
    """The tiny fixture's second forward on the engine's OWN perturbed features against the golden (fp32)."""
    from gst_visdial_amd import attack
    from gst_visdial_amd.selfcheck import build_tiny_model, load_npz
    fx = load_npz("tiny_fgsm.npz")
    model = build_tiny_model("fp32", str(dev), mode="vd_eval_val")[0]
    model.eval()
    ids0 = fx["in::dec_input_ids"]
    tgt = torch.zeros_like(ids0)
    tgt[:, :-1] = ids0[:, 1:]
    lines = []
    for tag in ("e1", "e01"):
        kw = dict.fromkeys(attack._MODEL_KEYS)
        kw.update({k[4:]: v.clone().to(dev) for k, v in fx.items() if k.startswith("in::")})
        adv = attack.fgsm_features(model, kw, fx["gt_relevance"], fx["epsilon::" + tag].item())
        flips = int((adv.cpu() != fx["adv_feats::" + tag]).sum())
        with torch.no_grad():
            _, logits = model(**dict(kw, enc_image_features=adv))
        lp = torch.log_softmax(logits.cpu(), -1)
        sc = (lp.gather(-1, tgt.unsqueeze(-1)).squeeze(-1) * (tgt != 0).float()).sum(-1)
        lines.append("tiny fixture, epsilon %.1f, fp32: %d of %d perturbed elements differ from the golden's; scores of the second forward "
                     "on the engine's own features deviate from the golden's by at most %.3e (logits %.3e)"
                     % (fx["epsilon::" + tag].item(), flips, adv.numel(), (sc - fx["answer_scores::" + tag]).abs().max().item(),
                        (logits.cpu() - fx["logits::" + tag]).abs().max().item()))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--relevant", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fgsm.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["FGSM gradient pass, full config, eval mode, T 256, R 37, U 25 (%s); %d timed iterations after %d warm-up"
             % (torch.cuda.get_device_name(0), a.steps, a.warmup)]
    for precision in a.precisions.split(","):
        lines += measure(precision, a, dev)
    lines += tiny_second_forward(dev)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
