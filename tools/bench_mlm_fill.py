"""Timing of the masked-LM fill-in of the random-token text attack on one MI355X -> profiles/mlm_fill.txt.  Recorded, not gated.

bert-base shape (12 layers, H 768, 12 heads, V 30522), T 256, random weights, bf16:
  (a) MaskedLMFiller.fill on a row with 38 [MASK] tokens (15 %): the text-only encoder on one row, the head on 38 rows;
  (b) the head's arg-max alone, fused (gstvd_vocab_argmax), at n = 1 / 38 / 256 rows of transformed hidden states;
  (c) the same n through the existing GEMM into an [n, Vp] fp32 buffer + gstvd_rows_argmax;
  (d) an attacked chunk of 100 answer options of the full enc-dec model: scored in one pass (attack.score_chunk: the fill-in and
      ONE encoder pass, score_candidates) and as the reference does it (attack.forward_attack: the fill-in and a 100-row forward,
      then the answer scores).
Method: every shape warmed up; every figure the median of `--steps` (>= 9) individually timed iterations (HIP events around
each, the device idle before each) with min..max; (b) and (c) are timed ALTERNATELY inside one call, in three runs.  The file also
states whether (b) and (c) return identical token ids at the timed sizes.

    python tools/bench_mlm_fill.py [--steps 11] [--warmup 3] [--out profiles/mlm_fill.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                             # noqa: E402

T, N_MASK, ROWS, R, U = 256, 38, 100, 37, 25
BERT_BASE = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 hidden_act="gelu", max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)


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


def line(tag, t):
    return "%-72s median %9.3f ms  (min %9.3f .. max %9.3f)" % (tag, t[0], t[1], t[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlm_fill.txt"))
    a = ap.parse_args()
    if a.steps < 9:
        raise SystemExit("--steps must be at least 9")
    from gst_visdial_amd import attack, ops
    from gst_visdial_amd.mlm import MaskedLMFiller
    dev = torch.device("cuda:0")
    out = ["masked-LM fill-in, bert-base shape (12 layers, H 768, V 30522), T %d, random weights, bf16 (%s); %d timed iterations "
           "after %d warm-up" % (T, torch.cuda.get_device_name(0), a.steps, a.warmup)]

    torch.manual_seed(0)
    filler = MaskedLMFiller(BERT_BASE, dev, precision="bf16")
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30000, (ROWS, T), generator=g)
    ids[:, 0] = 101
    ids[:, 20::21] = 102
    seg = ((ids == 102).long().cumsum(1) - (ids == 102).long()) % 2
    mask_pos = torch.randperm(T - 2, generator=g)[:N_MASK] + 1
    ids[:, mask_pos] = 103
    ids[:] = ids[:1]
    seg[:] = seg[:1]
    att = torch.ones(ROWS, T)
    rows0 = filler.host_rows(ids[:1])
    assert rows0.numel() == N_MASK
    d_ids, d_seg, d_att = ids.to(dev), seg.to(dev), att.to(dev)
    (ta,) = timed([lambda: filler.fill(d_ids, d_seg, d_att, rows=rows0)], a.steps, a.warmup)
    out.append(line("(a) fill: 1 row x %d tokens, %d [MASK] positions (encoder + head)" % (T, N_MASK), ta))

    eng = filler.model.engine
    w, b, V, H = eng.W["mlm.dec.w"], eng.Pv["mlm.b"], BERT_BASE["vocab_size"], BERT_BASE["hidden_size"]
    same = {}
    for run in range(3):
        for n in (1, N_MASK, 256):
            x = (torch.randn(n, H, generator=g) * 1.0).to(dev).to(torch.bfloat16)
            ws = torch.empty(ops.vocab_argmax_ws_bytes(n, V), dtype=torch.uint8, device=dev)
            logits = torch.empty(n, w.shape[0], dtype=torch.float32, device=dev)
            fused = lambda: ops.vocab_argmax_fused(x, w, b, V, n=n, ws=ws)                       # noqa: E731
            gemm = lambda: ops.vocab_argmax(x, w, b, V, n=n, logits=logits, fused=False)         # noqa: E731
            tb, tc = timed([fused, gemm], a.steps, a.warmup)
            fi, fv = fused()
            gi, gv = gemm()
            eq = bool(torch.equal(fi, gi))
            same[n] = same.get(n, True) and eq
            out.append(line("(b) run %d, head alone, fused gstvd_vocab_argmax, n = %d" % (run + 1, n), tb))
            out.append(line("(c) run %d, head alone, gstvd_gemm [n, Vp] fp32 + gstvd_rows_argmax, n = %d" % (run + 1, n), tc))
            out.append("    n = %d: token ids of (b) and (c) %s; largest |val_b - val_c| %.3e"
                       % (n, "identical" if eq else "DIFFER in %d rows" % int((fi != gi).sum()), (fv - gv).abs().max().item()))
    out.append("(b) vs (c) token ids identical at every timed size in all three runs: %s" % all(same.values()))

    model, params = bench.build_model(dev, "bf16", 0)
    model.eval()
    c = model.encoder.config
    full = bench.synthetic_rows(ROWS, T, R, U, c.v_feature_size, c.vocab_size, 77, torch.device("cpu"))
    dec_ids = full["dec_input_ids"].clone()
    dec_ids[:, 1:] = torch.where(full["dec_labels"][:, :-1] == 102, torch.full_like(dec_ids[:, 1:], 102), dec_ids[:, 1:])
    item = dict(enc_input_ids=ids, enc_segments=seg, enc_att_mask=att, enc_sep_indices=torch.zeros(ROWS, 5, dtype=torch.long),
                enc_mlm_labels=torch.full((ROWS, T), -1), dec_input_ids=dec_ids, dec_att_mask=full["dec_attention_mask"],
                enc_image_feat=full["enc_image_features"][:1].expand(ROWS, -1, -1), enc_image_loc=full["enc_image_spatials"][:1].expand(ROWS, -1, -1),
                enc_image_mask=full["enc_image_mask"][:1].expand(ROWS, -1), round_id=torch.tensor([1]), gt_relevance=torch.zeros(ROWS))
    p = dict(params, attack="random_token", textattack=filler, mode="vd_eval_val")
    model.params["mode"] = "vd_eval_val"

    def one_pass():
        with torch.no_grad():
            return attack.score_chunk(model, item, p, 1.0)

    def many_rows():
        with torch.no_grad():
            attack.forward_attack(model, item, p)
            last = model.engine.last
            scores = torch.empty(ROWS, dtype=torch.float32, device=dev)
            ops.answer_scores(last["logits"].t, last["lse"], dec_ids.to(dev).contiguous(), ROWS, U, scores)
            return scores

    td1, td2 = timed([one_pass, many_rows], a.steps, a.warmup)
    dev_sc = (one_pass() - many_rows()).abs().max().item()
    out.append(line("(d) attacked chunk, %d options: fill + ONE encoder pass (score_chunk)" % ROWS, td1))
    out.append(line("(d) attacked chunk, %d options: fill + %d-row forward + answer scores" % (ROWS, ROWS), td2))
    out.append("    largest |score difference| between the two forms (bf16): %.3e" % dev_sc)
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
