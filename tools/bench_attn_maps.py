"""Timing of the attention maps on one MI355X -> profiles/attn_maps.txt.  Recorded, not gated.

Full-size bf16 model in eval mode, 16 rows, T 256, R 37, U 25, random weights:
  (a) the teacher-forced forward alone;
  (b) the same with every map per head (EncoderDecoderModel.attention_maps);
  (c) the same with heads="mean";
  (d) select={"c": "all", "decoder_cross": "all"} with the head mean;
  (e) per site kind, on fused Q|K buffers of the site's shape and layout: the kernel (ops.attn_probs, per head and head mean)
      and, as the yardstick, the torch formulation softmax(q @ k^T * scale + mask) reading the same buffers -- for one text layer,
      one connection layer (both directions) and one decoder cross site; the vision and decoder self sites kernel only.
For every kernel line of (e): the event time and the bytes written over that time, against the 6.3 TB/s the hardware guide gives
as achievable.
Method: every variant warmed up; every figure the median of `--steps` (>= 9) individually timed iterations (HIP events around
each, the device idle before each) with min..max; the variants of a group are timed ALTERNATELY inside one session.

    python tools/bench_attn_maps.py [--steps 11] [--warmup 3] [--out profiles/attn_maps.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                             # noqa: E402

ROWS, T, R, U = 16, 256, 37, 25
ACHIEVABLE_TBS = 6.3


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fns, steps, warmup):
    """The callables of `fns` timed alternately: -> one (median, min, max) in ms per callable."""
    for _ in range(warmup):
        for f in fns:
            f()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for i, f in enumerate(fns):
            ms[i].append(once(f))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def line(tag, t, extra=""):
    return "%-78s median %8.3f ms  (min %8.3f .. max %8.3f)%s" % (tag, t[0], t[1], t[2], extra)


def site(ops, dev, g, name, nh, d, Lq, Lk, causal=False, neg=-10000.0, self_attn=False):
    """Fused buffers of one site kind: Q a column slice of a [rows, 3 H] projection (decoder cross: [rows, H]), K a column slice of a
    [rows, 3 H] projection (decoder cross: of the [rows, 2 * 12 * H] K/V projection of all layers); ragged key mask."""
    H = nh * d
    qw = H if name.startswith("decoder cross") else 3 * H
    kw = 24 * H if name.startswith("decoder cross") else 3 * H
    qbuf = (torch.randn(ROWS * Lq, qw, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    kbuf = qbuf if self_attn else (torch.randn(ROWS * Lk, kw, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    Q, K = qbuf[:, :H], kbuf[:, H:2 * H]
    lens = torch.randint(int(0.6 * Lk), Lk + 1, (ROWS,), generator=g)
    km = (torch.arange(Lk)[None] < lens[:, None]).float().to(dev)
    a = ops.attn_desc(Q, K, None, None, None, km, ROWS, nh, Lq, Lk, d, causal=causal, mask_neg=neg, ldv=0, ldo=0)
    per_head = torch.empty(ROWS, nh, Lq, Lk, dtype=torch.float32, device=dev)
    mean = torch.empty(ROWS, Lq, Lk, dtype=torch.float32, device=dev)
    scale = 1.0 / d ** 0.5
    add = ((1.0 - km) * neg)[:, None, None, :]
    if causal:
        add = add.expand(-1, -1, Lq, -1).clone()
        add.masked_fill_(torch.ones(Lq, Lk, device=dev, dtype=torch.bool).triu(1)[None, None], neg)

    def torch_form():
        q = Q.unflatten(0, (ROWS, Lq)).unflatten(-1, (nh, d)).permute(0, 2, 1, 3)
        k = K.unflatten(0, (ROWS, Lk)).unflatten(-1, (nh, d)).permute(0, 2, 3, 1)
        return torch.softmax((q @ k).float() * scale + add, -1)
    return dict(name=name, a=a, per_head=per_head, mean=mean, torch_form=torch_form, nh=nh, Lq=Lq, Lk=Lk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_maps.txt"))
    a = ap.parse_args()
    if a.steps < 9:
        raise SystemExit("--steps must be at least 9")
    from gst_visdial_amd import ops
    dev = torch.device("cuda:0")
    out = ["attention maps, full-size bf16 model in eval mode, %d rows, T %d, R %d, U %d, random weights (%s); %d timed iterations "
           "after %d warm-up" % (ROWS, T, R, U, torch.cuda.get_device_name(0), a.steps, a.warmup)]

    model, params = bench.build_model(dev, "bf16", 0)
    model.eval()
    model.params["mode"] = "vd_eval_val"
    c = model.encoder.config
    rows = bench.synthetic_rows(ROWS, T, R, U, c.v_feature_size, c.vocab_size, 77, torch.device("cpu"))
    keys = ("enc_image_features", "enc_image_spatials", "enc_image_mask", "enc_input_ids", "enc_segments", "enc_attention_mask",
            "dec_input_ids", "dec_attention_mask", "dec_labels")
    b = {k: rows[k].to(dev) for k in keys}

    def fwd():
        with torch.no_grad():
            return model(**b)

    def maps(**kw):
        def f():
            with torch.no_grad():
                return model.attention_maps(**dict(b, **kw))
        return f
    variants = [("(a) teacher-forced forward alone", fwd),
                ("(b) forward + every map, per head", maps()),
                ("(c) forward + every map, heads=\"mean\"", maps(heads="mean")),
                ("(d) forward + select c, decoder_cross, heads=\"mean\"", maps(select={"c": "all", "decoder_cross": "all"}, heads="mean"))]
    ts = timed([f for _, f in variants], a.steps, a.warmup)
    for (tag, _), t in zip(variants, ts):
        out.append(line(tag, t, "" if t is ts[0] else "  +%.3f ms over (a)" % (t[0] - ts[0][0])))
    _, m = maps()()
    nbytes = sum(x.numel() * 4 for x in m.encoder.t + m.encoder.v + [p for pair in m.encoder.c for p in pair] + m.decoder_self + m.decoder_cross)
    out.append("    (b) returns %d maps, %.1f MB of fp32" % (len(m.encoder.t) + len(m.encoder.v) + 2 * len(m.encoder.c) + len(m.decoder_self)
                                                              + len(m.decoder_cross), nbytes / 1e6))
    del m
    torch.cuda.empty_cache()

    g = torch.Generator().manual_seed(5)
    nhb, db = c.bi_num_attention_heads, c.bi_hidden_size // c.bi_num_attention_heads
    nht, dt_ = c.num_attention_heads, c.hidden_size // c.num_attention_heads
    nhv, dv = c.v_num_attention_heads, c.v_hidden_size // c.v_num_attention_heads
    sites = [site(ops, dev, g, "text self-attention %d x %d" % (T, T), nht, dt_, T, T, self_attn=True),
             site(ops, dev, g, "connection, text over regions %d x %d" % (T, R), nhb, db, T, R),
             site(ops, dev, g, "connection, regions over text %d x %d" % (R, T), nhb, db, R, T),
             site(ops, dev, g, "decoder cross-attention %d x %d" % (U, R + T), nht, dt_, U, R + T, neg=-1e9),
             site(ops, dev, g, "vision self-attention %d x %d" % (R, R), nhv, dv, R, R, self_attn=True),
             site(ops, dev, g, "decoder self-attention %d x %d" % (U, U), nht, dt_, U, U, causal=True, self_attn=True)]
    out.append("(e) per site kind, %d rows: the kernel on fused Q|K buffers against the torch formulation on the same buffers" % ROWS)
    for s in sites:
        yard = not s["name"].startswith(("vision", "decoder self"))
        fns = [lambda s=s: ops.attn_probs(s["a"], s["per_head"]), lambda s=s: ops.attn_probs(s["a"], s["mean"], head_mean=True)]
        if yard:
            fns.append(s["torch_form"])
        t = timed(fns, a.steps, a.warmup)
        n1, n2 = s["per_head"].numel() * 4, s["mean"].numel() * 4
        out.append(line("    %s, %d heads: kernel, per head" % (s["name"], s["nh"]), t[0],
                        "  %.1f MB written, %.2f TB/s (%.0f %% of %.1f)" % (n1 / 1e6, n1 / t[0][0] / 1e9, 100 * n1 / t[0][0] / 1e9 / ACHIEVABLE_TBS, ACHIEVABLE_TBS)))
        out.append(line("    %s, %d heads: kernel, head mean" % (s["name"], s["nh"]), t[1],
                        "  %.1f MB written, %.2f TB/s" % (n2 / 1e6, n2 / t[1][0] / 1e9)))
        if yard:
            err = (s["torch_form"]() - s["per_head"]).abs().max().item()
            out.append(line("    %s, %d heads: torch softmax(q @ k^T * scale + mask)" % (s["name"], s["nh"]), t[2],
                            "  kernel %s (x%.2f); largest |difference| %.2e" % ("faster" if t[0][0] < t[2][0] else "SLOWER", t[2][0] / t[0][0], err)))
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
