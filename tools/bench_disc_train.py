"""Timing of the discriminative (enc_only_a) training step on one MI355X -> profiles/disc_train.txt.  Recorded, not gated.

Full config (gst_visdial_amd.config.bert_base_enc_config), bf16, T = 256, R = 37, train mode (dropout on): `--rows` rows (the
reference samples `batch_size` rows out of a batch of dialogs x 10 rounds x samples; train_disc.py:54-55), ~15 % of the tokens of
every row masked, 2 masked regions per row.  Reports forward + backward ms (HIP events around whole steps), the heads' share
from ops.Profiler (records made inside the head scopes, forward and backward), the compacted row counts, and the same step
with compaction off (the MLM head over all B * T rows) when the memory fits.

    python tools/bench_disc_train.py [--rows 64] [--steps 10] [--warmup 3] [--out profiles/disc_train.txt]
"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_train.txt"))
    a = ap.parse_args()
    from gst_visdial_amd import ops
    from gst_visdial_amd.config import bert_base_enc_config
    from gst_visdial_amd.modules import VisualDialogEncoder
    dev = torch.device("cuda:0")
    cfg = bert_base_enc_config()
    d = tempfile.mkdtemp(prefix="gstvd_bench_")
    with open(os.path.join(d, "enc.json"), "w") as f:
        json.dump(cfg, f)
    params = dict(model_enc_config=os.path.join(d, "enc.json"), gpu_ids=[0], model="enc_only_a", mode="vd_train", batch_size=a.rows,
                  device=dev, amd_precision="bf16")
    torch.manual_seed(0)
    enc = VisualDialogEncoder(params).to(dev)
    enc.train()
    c = enc.config
    B, T, R = a.rows, 256, 37
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, c.vocab_size, (B, T), generator=g)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    att = torch.arange(T)[None] < lens[:, None]
    mask = torch.full((B, T), -1, dtype=torch.long)
    pick = (torch.rand(B, T, generator=g) < 0.15) & att
    pick[:, 0] = False
    mask[pick] = ids[pick]
    ids = torch.where(pick, torch.full_like(ids, 103), ids) * att
    label = torch.full((B, R), -1, dtype=torch.long)
    label[:, 3] = 1
    label[:, 17] = 1
    target = torch.rand(B, R, c.v_target_size, generator=g)
    target = target / target.sum(-1, keepdim=True)
    nsl = torch.tensor([[1.0, 0.0], [0.0, 1.0]])[torch.randint(0, 2, (B,), generator=g)]
    t = dict(ids=ids, feat=torch.randn(B, R, c.v_feature_size, generator=g), loc=torch.rand(B, R, 5, generator=g),
             seg=torch.zeros_like(ids), att=att, mask=mask, nsl=nsl, imask=torch.ones(B, R, dtype=torch.long), label=label, target=target)
    tok_rows = (mask.view(-1) != -1).nonzero().view(-1).to(dev)
    reg_rows = (label.view(-1) == 1).nonzero().view(-1).to(dev)
    t = {k: v.to(dev) for k, v in t.items()}
    eng = enc.engine

    def step(compact):
        lm, img, nsp, z = eng.disc_step(t["feat"], t["loc"], t["imask"], t["ids"], t["seg"], t["att"], t["mask"], t["nsl"], t["label"],
                                        t["target"], token_rows=tok_rows, region_rows=reg_rows, compact=compact)
        (lm + img + nsp).sum().backward()

    def timed(compact):
        for _ in range(a.warmup):
            step(compact)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step(compact)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        with ops.Profiler() as prof:
            step(compact)
            torch.cuda.synchronize()
        heads, total = {}, 0.0
        for tag, flops, nbytes, s0, s1, detail, sc in prof.records:
            dt_ = s0.elapsed_time(s1)
            total += dt_
            if sc is not None and sc.startswith("head."):
                heads[sc] = heads.get(sc, 0.0) + dt_
        return ms, heads, total

    lines = ["discriminative training step, full config, bf16, train mode: rows %d, T %d, R %d (%s)" % (B, T, R, torch.cuda.get_device_name(0)),
             "compacted rows: %d of %d tokens (%.1f %%), %d of %d regions" % (tok_rows.numel(), B * T, 100.0 * tok_rows.numel() / (B * T),
                                                                          reg_rows.numel(), B * R)]
    for compact in (True, False):
        try:
            ms, heads, total = timed(compact)
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
            lines.append("compaction %s: did not run (%s)" % ("on" if compact else "off", str(e).splitlines()[0][:120]))
            continue
        hs = sum(heads.values())
        lines.append("compaction %-3s: forward + backward %.3f ms per step (%d steps after %d warm-up); kernels of one instrumented step "
                     "%.3f ms, of which the heads %.3f ms (%.1f %%): %s" % ("on" if compact else "off", ms, a.steps, a.warmup, total, hs,
                                                                        100.0 * hs / max(total, 1e-9),
                                                                        ", ".join("%s %.3f" % kv for kv in sorted(heads.items()))))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
