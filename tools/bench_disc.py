"""Timing of one discriminative scoring chunk on the MI355X: 200 rows x 256 tokens x 37 regions at the bert-base config
(config.bert_base_enc_config), bf16, seeded synthetic weights -- what evaluate_disc issues per call at the reference's chunk size.

    python tools/bench_disc.py --out profiles/disc_head.txt [--rows 200 --tokens 256 --iters 50]

Three figures, each from device events around a window of `iters` back-to-back issues after a warm-up of every shape (no
profiler attached), median of `repeats` windows with the spread next to it:
  encoder   the two-stream encoder alone (Engine.encoder: the schedule the generative path runs)
  head      gstvd_nsp_head alone, on the activations the encoder left
  pieces    the same head assembled from what the library had before: row-0 copy of both streams, two ops.gemm (bias),
            torch ReLU / mul, one ops.gemm (classifier rows padded 2 -> 4: the GEMM ABI wants N % 4 == 0), torch softmax
`head` and `pieces` windows alternate within a repeat.  No figure is a pass / fail condition.  Outputs of the two heads are
compared on the way (bf16 pieces round pt / pv to bf16 only if asked to; here both keep fp32 poolers)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--regions", type=int, default=37)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--enc-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_disc needs an MI355X: no device, no number")
    from gst_visdial_amd import ops
    from gst_visdial_amd.config import bert_base_enc_config
    from gst_visdial_amd.modules import VisualDialogEncoder
    dev = torch.device("cuda:0")
    cfg = bert_base_enc_config()
    d = tempfile.mkdtemp(prefix="gstvd_cfg_")
    with open(os.path.join(d, "enc.json"), "w") as f:
        json.dump(cfg, f)
    params = dict(model_enc_config=os.path.join(d, "enc.json"), gpu_ids=[0], model="enc_only_a", mode="vd_eval_val", device=dev,
                  amd_precision="bf16")
    torch.manual_seed(0)
    enc = VisualDialogEncoder(params).eval().to(dev)
    B, T, R = a.rows, a.tokens, a.regions
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, cfg["vocab_size"], (B, T), generator=g)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    att = torch.arange(T)[None] < lens[:, None]
    ids = (ids * att).to(dev)
    segs = ((torch.arange(T)[None] // 16) % 2 * att).to(dev)
    feats = torch.randn(B, R, cfg["v_feature_size"], generator=g).to(dev)
    loc = torch.rand(B, R, 5, generator=g).to(dev)
    imask = torch.ones(B, R, dtype=torch.long, device=dev)
    att = att.to(dev)
    eng = enc.engine

    with torch.no_grad():
        z, p = eng.nsp_scores(feats, loc, imask, ids, segs, att)                      # warm-up: flat buffers, arena, every shape
        z, p = eng.nsp_scores(feats, loc, imask, ids, segs, att)
        torch.cuda.synchronize()
        arena_gb = sum(c.numel() for c in eng.arena.chunks) / 2.0 ** 30

        def encoder_only():
            eng._begin(dev, False, inference=True)
            I = eng._inputs(feats, loc, imask, ids, segs, att, ids.new_zeros(B, 1), None)
            return eng.encoder(I)

        encoder_only()
        enc_ms = [window(encoder_only, a.enc_iters) for _ in range(a.repeats)]
        xt, xv = encoder_only()
        torch.cuda.synchronize()
        W, Pv = eng.W, eng.Pv
        H, Hv, Hb = cfg["hidden_size"], cfg["v_hidden_size"], cfg["bi_hidden_size"]
        z1, p1 = torch.empty(B, 2, device=dev), torch.empty(B, device=dev)

        def head():
            ops.nsp_head(xt.t, T, xv.t, R, W["pool.t.w"], Pv["pool.t.b"], W["pool.v.w"], Pv["pool.v.b"], Pv["nsp.w"], Pv["nsp.b"],
                         B, "mul", z1, p1)

        wn4 = torch.zeros(4, Hb, device=dev)
        wn4[:2] = Pv["nsp.w"]
        bn4 = torch.zeros(4, device=dev)
        bn4[:2] = Pv["nsp.b"]
        pt, pv, z4 = torch.empty(B, Hb, device=dev), torch.empty(B, Hb, device=dev), torch.empty(B, 4, device=dev)
        keep = {}

        def pieces():
            t0 = xt.t.view(B, T, H)[:, 0].contiguous()
            v0 = xv.t.view(B, R, Hv)[:, 0].contiguous()
            ops.gemm(t0, W["pool.t.w"], pt, B, Hb, H, bias=Pv["pool.t.b"])
            ops.gemm(v0, W["pool.v.w"], pv, B, Hb, Hv, bias=Pv["pool.v.b"])
            f = torch.relu(pt) * torch.relu(pv)
            ops.gemm(f, wn4, z4, B, 4, Hb, bias=bn4)
            keep["z"] = z4[:, :2]
            keep["p"] = torch.softmax(z4[:, :2], 1)[:, 0]

        head(); pieces()
        torch.cuda.synchronize()
        dz = (z1 - keep["z"]).abs().max().item()
        dp = (p1 - keep["p"]).abs().max().item()
        head_ms, pieces_ms = [], []
        for _ in range(a.repeats):
            head_ms.append(window(head, a.iters))
            pieces_ms.append(window(pieces, a.iters))
        full_ms = [window(lambda: eng.nsp_scores(feats, loc, imask, ids, segs, att), a.enc_iters) for _ in range(a.repeats)]

    med = statistics.median
    sp = lambda v: "median %.4f ms (min %.4f, max %.4f over %d windows)" % (med(v), min(v), max(v), len(v))
    lines = [
        "discriminative scoring chunk: %d rows x %d tokens x %d regions, bert-base config (H %d / Hv %d / Hb %d), bf16, MI355X"
        % (B, T, R, H, Hv, Hb),
        "device events around windows of back-to-back issues after warm-up, no profiler; arena after warm-up: %.1f GiB" % arena_gb,
        "encoder alone (Engine.encoder, windows of %d):        %s" % (a.enc_iters, sp(enc_ms)),
        "gstvd_nsp_head alone (windows of %d):                 %s" % (a.iters, sp(head_ms)),
        "head from existing pieces (2 copies, 3 ops.gemm, 4 torch ops; windows of %d): %s" % (a.iters, sp(pieces_ms)),
        "Engine.nsp_scores, whole call (windows of %d):         %s" % (a.enc_iters, sp(full_ms)),
        "options ranked per second (rows / whole call):        %.0f" % (B / (med(full_ms) * 1e-3)),
        "head kernel vs pieces on the same activations: max |dz| %.3e, max |dprob0| %.3e" % (dz, dp),
    ]
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
