"""Timing of the listwise candidate step on one MI355X -> profiles/rank_train.txt.  Recorded, not gated.

Full-size bf16 model in TRAIN mode (dropout on), random weights, T 256, R 37, U 25, G = 100 candidates per round:
  (a) grouped:    EncoderDecoderModel.rank_loss on E rounds -- one encoder pass and one cross-attention K/V projection per round,
                  the decoder on E * G rows, backward through gstvd_attn_group_bwd -- forward + loss.backward();
  (b) replicated: the same loss on the path that needs no grouped backward -- model(..., loss_reduction=False) on the E * G
                  replicated rows (every row its own encoder pass), the listwise loss in torch on the per-token losses, backward.
E = 2 both ways (timed alternately inside one session); E = 8 grouped only.  Every figure is the median of `--steps` (>= 20)
individually timed steps after `--warmup` (HIP events around each step, the device idle before each), with min..max.  The
launches of gstvd_attn_group_bwd are timed one by one in a further step under ops.Profiler (events around every launch).

    python tools/bench_rank_train.py [--steps 20] [--warmup 3] [--out profiles/rank_train.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                             # noqa: E402

T, R, U, G = 256, 37, 25, 100
ENC = ("enc_image_features", "enc_image_spatials", "enc_image_mask", "enc_input_ids", "enc_segments", "enc_attention_mask")


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fns, steps, warmup):
    for _ in range(warmup):
        for f in fns:
            f()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for i, f in enumerate(fns):
            ms[i].append(once(f))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def line(tag, t, extra=""):
    return "%-64s median %9.3f ms  (min %9.3f .. max %9.3f)%s" % (tag, t[0], t[1], t[2], extra)


class Lines(list):
    """The lines of the report, shown as they are measured."""

    def append(self, x):
        print(x, flush=True)
        list.append(self, x)


def listwise(per_token, rel):
    n_r, n_o = rel.shape
    logp = torch.log_softmax(-per_token.view(n_r, n_o, -1).sum(-1), 1)
    t = rel / rel.sum(1, keepdim=True)
    return -(t * logp).sum(1).mean()


def batch(model, E, dev, seed):
    c = model.encoder.config
    enc = bench.synthetic_rows(E, T, R, U, c.v_feature_size, c.vocab_size, seed, torch.device("cpu"))
    dec = bench.synthetic_rows(E * G, T, R, U, c.v_feature_size, c.vocab_size, seed + 1, torch.device("cpu"))
    b = {k: enc[k].to(dev) for k in ENC}
    b.update(dec_input_ids=dec["dec_input_ids"].to(dev), dec_attention_mask=dec["dec_attention_mask"].to(dev))
    g = torch.Generator().manual_seed(seed)
    rel = (torch.rand(E, G, generator=g) < 0.1).float() * torch.randint(1, 5, (E, G), generator=g).float() * 0.25
    rel[:, 0] = 1.0
    return b, rel.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_train.txt"))
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps must be at least 20")
    from gst_visdial_amd import ops
    dev = torch.device("cuda:0")
    model, _ = bench.build_model(dev, "bf16", 0)
    model.train()
    out = Lines()
    out.append("listwise candidate step, full-size bf16 model in train mode (dropout on), T %d, R %d, U %d, G %d, random weights (%s); "
           "%d timed steps after %d warm-up" % (T, R, U, G, torch.cuda.get_device_name(0), a.steps, a.warmup))

    def zero():
        for p in model.engine.flat.live:
            p.grad = None

    def grouped(b, rel):
        def f():
            loss, _ = model.rank_loss(relevance=rel, num_options=G, **b)
            loss.backward()
            zero()
        return f

    def replicated(b, rel):
        rep = {k: (v.repeat_interleave(G, 0) if k in ENC else v) for k, v in b.items()}

        def f():
            per_token, _ = model(dec_labels=None, loss_reduction=False, **dict(rep, dec_input_ids=rep["dec_input_ids"].clone()))
            listwise(per_token, rel).backward()
            zero()
        return f

    b2, rel2 = batch(model, 2, dev, 11)
    tg, tr = timed([grouped(b2, rel2), replicated(b2, rel2)], a.steps, a.warmup)
    out.append(line("(a) E = 2, grouped (rank_loss + backward)", tg))
    out.append(line("(b) E = 2, replicated rows (%d encoder passes) + backward" % (2 * G), tr, "  grouped is x%.2f %s" % (
        tr[0] / tg[0], "faster" if tg[0] < tr[0] else "SLOWER")))
    torch.cuda.empty_cache()
    b8, rel8 = batch(model, 8, dev, 13)
    (t8,) = timed([grouped(b8, rel8)], a.steps, a.warmup)
    out.append(line("(a) E = 8, grouped (rank_loss + backward)", t8))
    for tag, (b, rel) in (("E = 2", (b2, rel2)), ("E = 8", (b8, rel8))):
        f = grouped(b, rel)
        with ops.Profiler() as prof:
            f()
        recs = [(e0.elapsed_time(e1), d) for t, _, _, e0, e1, d, _ in (torch.cuda.synchronize() or prof.records) if t.startswith("attn_group_bwd")]
        ms = [r[0] for r in recs]
        out.append("    %s: %d launches of attn_group_bwd %s, per launch median %.3f ms (min %.3f .. max %.3f), %.3f ms of the step in all"
                   % (tag, len(ms), "x".join(str(x) for x in recs[0][1]), statistics.median(ms), min(ms), max(ms), sum(ms)))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
