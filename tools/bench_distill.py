#!/usr/bin/env python3
"""Soft pseudo-labels at the full model size (bf16, 1 GPU, random weights, synthetic rows): 16 rows, T = 256, U = 25, K = 8.
Three alternating runs in one session, medians of 9 replay-free eager calls each ([median, min, max] ms):
  (a) the train step as it is without soft labels: forward, backward, FusedAdamW;
  (b) the same step with K = 8 soft labels (alpha 0.5, tau 2);
  (c) a sampling decode of 16 answers followed by `rescore_sampled`, without and with `soft_top_k = 8` (the decode is part of
      both: the rescoring pass needs the decode state it reuses);
and the device time of the three new launches from ops.Profiler's events in a run of its own (per launch, and as a share of (b)
and of (c, with)).  (a) and (c, without) are the parent code path: nothing new is launched in them.
Writes profiles/distill.txt (or the path given as the first argument) and prints one JSON line."""
import json, os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import bench
from gst_visdial_amd import ops
from gst_visdial_amd.optim import FusedAdamW

dev = torch.device("cuda", 0)
ROWS, T, REGIONS, U, K, ALPHA, TAU = 16, 256, 37, 25, 8, 0.5, 2.0
teacher, t_params = bench.build_model(dev, "bf16", seed=1)
teacher.eval()
student, s_params = bench.build_model(dev, "bf16", seed=2)
student.train()
opt = FusedAdamW(student, lr=2e-5, warmup_steps=1500, t_total=100000)
V = student.decoder.config.vocab_size
rows = bench.synthetic_rows(ROWS, T, REGIONS, U, 2048, V, 7, dev)

t_params["mode"] = "vd_eval_val"
_, _, (soft_ids, soft_logp, _) = teacher.soft_labels(**rows, top_k=K)
soft = dict(dec_soft_ids=soft_ids, dec_soft_logp=soft_logp, distill_alpha=ALPHA, distill_temperature=TAU)
t_params["mode"] = "cc12m_gen"
enc = {k: v for k, v in rows.items() if k.startswith("enc_")}
start = dict(dec_input_ids=torch.full((ROWS, 1), 101, dtype=torch.long, device=dev), dec_attention_mask=torch.ones(ROWS, 1, device=dev))


def train_step(extra):
    loss, _ = student(**rows, **extra)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss


def decode_rescore(top_k):
    with torch.no_grad():
        ans = teacher(temperature=0.7, top_k=7, **start, **enc)
        return teacher.engine.rescore_sampled(ans, (ans != 0).float(), soft_top_k=top_k)


def median_ms(fn, n=9, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]


out = dict(rows=ROWS, T=T, U=U, K=K, alpha=ALPHA, tau=TAU, runs=[])
for r in range(3):
    out["runs"].append(dict(a=median_ms(lambda: train_step({})), b=median_ms(lambda: train_step(soft)),
                            c0=median_ms(lambda: decode_rescore(None)), c1=median_ms(lambda: decode_rescore(K))))
loss = float(train_step(soft).detach())
out["loss_finite"] = loss == loss and abs(loss) != float("inf")
with ops.Profiler() as prof:                                # event-timed: a run of its own, not one of the timed windows
    for _ in range(5):
        train_step(soft)
        decode_rescore(K)
summ = prof.summary()
new = {}
for tag in ("topk_logp", "distill_fwd", "distill_bwd", "ce_fwd", "ce_bwd"):
    rec = summ.get(tag)
    if rec:
        new[tag] = dict(launches=rec["launches"], ms_per_launch=round(rec["ms"] / rec["launches"], 4))
out["launches"] = new
med = lambda k: statistics.median(run[k][0] for run in out["runs"])
out["share_of_b"] = round((new["distill_fwd"]["ms_per_launch"] + new["distill_bwd"]["ms_per_launch"]) / med("b"), 4)
out["share_of_c1"] = round(new["topk_logp"]["ms_per_launch"] / med("c1"), 4)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "distill.txt")
with open(path, "w") as f:
    f.write("tools/bench_distill.py: soft pseudo-labels, full-size bf16 models, random weights (MI355X)\n")
    f.write("%d rows, T = %d, U = %d, K = %d, alpha %g, tau %g; eager calls, no graph replay, no backward pipeline\n" % (ROWS, T, U, K, ALPHA, TAU))
    f.write("three alternating runs of one session, medians of 9 calls after 2 warm-up calls: [median, min, max] ms\n\n")
    names = (("a", "train step without soft labels (the parent code path)"), ("b", "train step with K = 8 soft labels"),
             ("c0", "sample + rescore_sampled (the parent code path)"), ("c1", "sample + rescore_sampled(soft_top_k=8)"))
    for r, run in enumerate(out["runs"]):
        for k, name in names:
            f.write("  run %d (%-2s) %-56s %s\n" % (r + 1, k, name, run[k]))
    f.write("\n  device time per launch (ops.Profiler events, 5 iterations in a run of their own):\n")
    for tag, rec in new.items():
        f.write("    %-12s %3d launches, %.4f ms each\n" % (tag, rec["launches"], rec["ms_per_launch"]))
    f.write("  distill_fwd + distill_bwd = %.2f %% of (b); topk_logp = %.2f %% of (c1); loss finite: %s\n"
            % (100 * out["share_of_b"], 100 * out["share_of_c1"], out["loss_finite"]))
print(json.dumps(out))
