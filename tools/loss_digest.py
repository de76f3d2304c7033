#!/usr/bin/env python3
"""SHA-256 of what the loss, optimizer and elementwise kernels write (csrc/ce_row.h's and csrc/loss_reduce.h's callers, csrc/optim.hip,
csrc/elementwise.hip), from fixed seeds on NON-integer inputs, where a reordered sum would show: run it against two builds of the
library and diff the outputs.  None of these kernels uses atomics, so two runs of one build agree line for line.  The logits entries
run at V = 1, 3, 4, 1025 and 30522 on 5 to 7 rows whose stride is the next multiple of 4 above V, fp32 and bf16:
  ce_fwd, ce_bwd (mean and sum), ce_bwd_rows (rows with g == 0), answer_scores, rank_loss (one round whose relevance is all zero)
  distill_fwd / _bwd            tau 0.5, 1, 2 and alpha 0, 0.3, 1; a row without a soft label, an ignored row, duplicate ids
  topk_logp                     K = 1, 8, 16
  kl_fwd / kl_bwd               C = 1601, with and without labels and target_row
  nsp_train_fwd / _bwd          both fusions, dropout 0.1
  adamw                         fp32 and bf16 gradient, a block list with a skipped segment, a segment boundary inside a 4-vector
  cast (four pairs), cast_ranges, scale_, fgsm_step, vl_split (p = 0 and 0.5), dropout_mask"""
import torch
from ln_digest import DEV, draw, sha, show          # noqa: F401  (also puts the repository root on sys.path)
from gst_visdial_amd import ops

DTYPES = ((torch.float32, "f32"), (torch.bfloat16, "bf16"))
VS = (1, 3, 4, 1025, 30522)
IGNORE = -100


def rows(g, n, V, dtype, scale=2.5):
    """[n, V] logits inside a buffer whose row stride is the next multiple of 4 above V (never a dense tail)."""
    return draw(g, n, (V + 4) // 4 * 4, dtype=dtype, scale=scale)[:, :V]


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def ce_case(tn, dtype, V, M=7):
    g = torch.Generator().manual_seed(100 + V)
    x = rows(g, M, V, dtype)
    lab = torch.randint(0, V, (M,), generator=g).to(DEV)
    lab[2] = IGNORE
    lab[4] = V + 3                                          # out of range: does not count, is not read
    row_loss, lse, stats = zeros(M), zeros(M), zeros(3)
    ops.ce_fwd(x, lab, M, V, row_loss, lse, stats, ignore_index=IGNORE)
    name = "ce %s V=%d" % (tn, V)
    show(name + " fwd", [("row_loss", row_loss), ("lse", lse), ("stats", stats)])
    gs = torch.tensor([0.37], device=DEV)
    for mean in (True, False):
        dl = rows(g, M, V + 4, dtype)                       # (stale values: every column of the stride is written)
        ops.ce_bwd(x, lab, lse, stats, gs, mean, M, V, dl, ignore_index=IGNORE)
        show(name + " bwd %s" % ("mean" if mean else "sum"), [("dlogits", dl.as_strided((M, dl.stride(0)), (dl.stride(0), 1)))])
    gr = draw(g, M)
    gr[1] = 0.0
    gr[5] = -0.0
    dl = rows(g, M, V + 4, dtype)
    ops.ce_bwd_rows(x, lab, lse, gr, M, V, dl, ignore_index=IGNORE)
    show(name + " bwd_rows", [("dlogits", dl.as_strided((M, dl.stride(0)), (dl.stride(0), 1)))])
    for K in (1, 8, 16):
        if K <= V:
            ids, logp = ops.topk_logp(x, lse, M, V, K)
            show("topk_logp %s V=%d K=%d" % (tn, V, K), [("ids", ids), ("logp", logp)])
    return x, lab, row_loss, lse, stats, gs


def distill_case(tn, dtype, V, x, lab, ce_loss, lse, gs, K=4):
    M = x.shape[0]
    g = torch.Generator().manual_seed(200 + V)
    sid = torch.randint(0, V, (M, K), generator=g).to(DEV)
    sid[1, 0] = -1                                          # no soft label
    sid[3, 1] = sid[3, 0]                                   # duplicate ids (row 2 is ignored, row 4's label is out of range)
    slp = torch.log_softmax(draw(g, M, K, scale=1.5), -1).contiguous()
    for tau in (0.5, 1.0, 2.0):
        for alpha in (0.0, 0.3, 1.0):
            l, kd, lt, st = zeros(M), zeros(M), zeros(M), zeros(3)
            ops.distill_fwd(x, lab, sid, slp, M, V, alpha, tau, ce_loss, l, kd, lt, st, ignore_index=IGNORE)
            dl = rows(g, M, V + 4, dtype)
            ops.distill_bwd(x, lab, sid, slp, lse, lt, st, gs, M, V, alpha, tau, dl, ignore_index=IGNORE)
            show("distill %s V=%d tau=%g alpha=%g" % (tn, V, tau, alpha),
                 [("row_loss", l), ("row_kd", kd), ("lse_tau", lt), ("stats", st), ("dlogits", dl.as_strided((M, dl.stride(0)), (dl.stride(0), 1)))])


def rank_case(tn, dtype, V, E=3, G=2, U=5):
    """E * G candidate rows of U positions (M = 30 logits rows); round 1's relevance is all zero."""
    g = torch.Generator().manual_seed(300 + V)
    n = E * G
    x, lse = rows(g, n * U, V, dtype), (draw(g, n * U) + 9.0)
    ids = torch.randint(0, V, (n, U), generator=g).to(DEV)
    if V > 1:
        ids[1, 3:] = 0                                      # [PAD] tail
    scores = zeros(n)
    ops.answer_scores(x, lse, ids, n, U, scores)
    show("answer_scores %s V=%d" % (tn, V), [("scores", scores)])
    rel = torch.rand(E, G, generator=g).to(DEV)
    rel[1] = 0.0
    sc, p, rl, gt, st = zeros(n), zeros(n), zeros(E), zeros(n * U), zeros(3)
    ops.rank_loss(x, lse, ids, rel.reshape(-1), E, G, U, 1.0 / 0.7, sc, p, rl, gt, st)
    show("rank_loss %s V=%d" % (tn, V), [("scores", sc), ("p", p), ("round", rl), ("g_tok", gt), ("stats", st)])


def kl_case(tn, dtype, C=1601, M=7):
    g = torch.Generator().manual_seed(400)
    x = draw(g, M, C, dtype=dtype, scale=2.5)
    t = torch.softmax(draw(g, 5, C, scale=2.0), -1).contiguous()
    t[0, :100] = 0.0                                        # exact zeros in the target
    trow = torch.randint(0, 5, (M,), generator=g).to(DEV)
    lab = torch.tensor([1, 0, 1, 1, -1, 1, 1], device=DEV)
    gs = torch.tensor([1.7], device=DEV)
    for who, tr, lb in (("labels, target_row", trow, lab), ("neither", None, None)):
        tt = t if tr is not None else torch.softmax(draw(g, M, C, scale=2.0), -1).contiguous()
        rl, lse, st = zeros(M), zeros(M), zeros(3)
        ops.kl_fwd(x, tt, M, C, rl, lse, st, target_row=tr, labels=lb)
        outs = [("row_loss", rl), ("lse", lse), ("stats", st)]
        for mean in (True, False):
            d = draw(g, M, C + 7, dtype=dtype)
            ops.kl_bwd(x, tt, lse, st, gs, mean, M, C, d[:, :C + 3], target_row=tr, labels=lb)
            outs.append(("d " + ("mean" if mean else "sum"), d))
        show("kl %s C=%d %s" % (tn, C, who), outs)


def nsp_case(tn, dtype, fusion, rng, B=6, H=768, Hv=1024, Hb=1024):
    g = torch.Generator().manual_seed(500)
    xt, xv = draw(g, B * 3, H, dtype=dtype), draw(g, B * 2, Hv, dtype=dtype)
    wt, wv = draw(g, Hb, H, dtype=dtype, scale=0.05), draw(g, Hb, Hv, dtype=dtype, scale=0.05)
    bt, bv, wn, bn = draw(g, Hb, scale=0.1), draw(g, Hb, scale=0.1), draw(g, 2, Hb, scale=0.1), draw(g, 2)
    labels = torch.softmax(draw(g, B, 2), -1).contiguous()
    z, pt, pv, keep = zeros(B, 2), zeros(B, Hb), zeros(B, Hb), zeros(B, Hb, dtype=torch.uint8)
    row_loss, stats = zeros(B), zeros(3)
    d = ops.nsp_train_desc(xt, 3, xv, 2, wt, bt, wv, bv, wn, bn, labels, B, fusion, z, pt, pv, keep, row_loss, stats, p=0.1, site=5, rng=rng)
    ops.nsp_train_fwd(d)
    dwn, dbn, dpt, dpv = zeros(2, Hb), zeros(2), zeros(B, Hb, dtype=dtype), zeros(B, Hb, dtype=dtype)
    ops.nsp_train_bwd(d, torch.tensor([0.6], device=DEV), dwn, dbn, dpt, dpv)
    show("nsp_train %s %s" % (tn, fusion), [("z", z), ("pt", pt), ("pv", pv), ("keep", keep), ("row_loss", row_loss), ("stats", stats),
                                            ("dwn", dwn), ("dbn", dbn), ("dpt", dpt), ("dpv", dpv)])


def adamw_case(n=6002):
    """Segment ends 1000 | 2050 (inside a 4-vector) | 3072 (lr == 0) | 5001 (inside a 4-vector) | n, which is no multiple of 4."""
    seg_end = torch.tensor([1000, 2050, 3072, 5001, n], dtype=torch.int64, device=DEV)
    hp = torch.tensor([[1e-3, 0.01], [2e-3, 0.0], [0.0, 0.0], [5e-4, 0.05], [1e-3, 0.0]], device=DEV).reshape(-1).contiguous()
    step = torch.tensor([3.0], device=DEV)

    def state(seed):
        g = torch.Generator().manual_seed(seed)
        return [draw(g, n) for _ in range(3)] + [draw(g, n).abs() * 0.01, zeros(n, dtype=torch.bfloat16)]

    for name, kw in (("f32 grad", {}), ("f32 grad from 2048", dict(begin=2048)), ("bf16 grad", dict(bf16=True)),
                     ("bf16 grad origin 1024", dict(bf16=True, begin=2048, origin=1024))):
        p, gr, m, v, sh = state(600)
        if kw.get("bf16"):
            gr = gr[kw.get("origin", 0):].to(torch.bfloat16).contiguous()
        ops.adamw(p, gr, m, v, sh, seg_end, hp, step, grad_scale=0.5, begin=kw.get("begin", 0), grad_origin=kw.get("origin", 0))
        show("adamw " + name, [("param", p), ("m", m), ("v", v), ("shadow", sh)])
    p, gr, m, v, sh = state(601)
    blocks = torch.tensor([0, 1, 2, 4, 5], dtype=torch.int32, device=DEV)
    skip = torch.tensor([0, 1, 0, 0, 0], dtype=torch.uint8, device=DEV)
    ops.adamw_blocks(p, gr, m, v, sh, seg_end, hp, step, blocks, skip, grad_scale=0.5, begin=1024)
    show("adamw blocks 0 1 2 4 5 from 1024, segment 1 skipped", [("param", p), ("m", m), ("v", v), ("shadow", sh)])


def elementwise_case(rng, n=4099):
    g = torch.Generator().manual_seed(700)
    for sd, sn in DTYPES:
        for dd, dn in DTYPES:
            src, dst = draw(g, n, dtype=sd), draw(g, n + 5, dtype=dd)
            ops.cast(src, dst, n)
            show("cast %s -> %s n=%d" % (sn, dn, n), [("dst", dst)])
    src, dst = draw(g, 6000), draw(g, 6000, dtype=torch.bfloat16)
    ops.CastRanges([(0, 1500), (2048, 1030), (4096, 3), (5000, 1000)], DEV).run(src, dst)
    show("cast_ranges", [("dst", dst)])
    x = draw(g, n)
    ops.scale_(x, torch.tensor([0.377], device=DEV))
    show("scale_ n=%d" % n, [("x", x)])
    x, gr = draw(g, n), draw(g, n)
    gr[::7] = 0.0
    gr[3::7] = -0.0
    gr[5] = float("nan")
    show("fgsm_step n=%d" % n, [("out", ops.fgsm_step(x, gr, 0.0123))])
    B, R, T, H = 2, 3, 5, 768
    for dtype, tn in DTYPES:
        d = draw(g, B * (R + T), H, dtype=dtype)
        for p in (0.0, 0.5):
            dv, dt_ = zeros(B * R, H, dtype=dtype), zeros(B * T, H, dtype=dtype)
            ops.vl_split(d, B, R, T, H, dv, dt_, p, 11, 12, rng)
            show("vl_split %s p=%g" % (tn, p), [("d_v", dv), ("d_t", dt_)])
    show("dropout_mask n=%d p=0.1" % n, [("mask", ops.dropout_mask(n, 0.1, 7, rng, DEV))])


def main():
    rng = ops.Rng(torch.device(DEV), seed=1)
    for V in VS:
        for dtype, tn in DTYPES:
            x, lab, row_loss, lse, stats, gs = ce_case(tn, dtype, V)
            distill_case(tn, dtype, V, x, lab, row_loss, lse, gs)
            rank_case(tn, dtype, V)
    for dtype, tn in DTYPES:
        kl_case(tn, dtype)
        for fusion in ("mul", "sum"):
            nsp_case(tn, dtype, fusion, rng)
    adamw_case()
    elementwise_case(rng)


if __name__ == "__main__":
    main()
