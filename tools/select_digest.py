#!/usr/bin/env python3
"""SHA-256 of what the selection kernels write (csrc/select.h's callers), from fixed seeds on NON-integer inputs, where a reordered
sum or comparison would show: run it against two builds of the library and diff the outputs.  These kernels use no atomics, so two
runs of one build agree line for line.  V = 1025 and 30522, fp32 and bf16 where the entry takes both:
  beam_step                     K = 1, 5, 8 (3 dialog rows; a done beam, a beam without a finite score)
  topk_logp                     K = 1, 8, 16
  rows_argmax, vocab_argmax     fused (n = 5, 20, 38, 60: all four tile heights) and through the GEMM + rows_argmax
  cos_topk                      the full table on the many-sources route, 37 sources on both routes, K = 10 with the 0.5 cut and
                                K = 16 without a cut
  sample_topk / _scored         top-k 7 and 64, top-p alone, top-k with top-p, and bans with one row banned entirely"""
import torch
from ln_digest import DEV, draw, sha, show          # noqa: F401  (also puts the repository root on sys.path)
from gst_visdial_amd import ops

DTYPES = ((torch.float32, "f32"), (torch.bfloat16, "bf16"))
VS = (1025, 30522)


def rows(g, n, V, dtype, scale=2.5):
    """[n, V] logits inside a buffer whose row stride is the next multiple of 4 above V (never a dense tail)."""
    return draw(g, n, (V + 4) // 4 * 4, dtype=dtype, scale=scale)[:, :V]


def beam_case(tn, dtype, V, K, B=3):
    g = torch.Generator().manual_seed(1000 + V + K)
    x, s_in = rows(g, B * K, V, dtype), draw(g, B, K)
    done = torch.zeros(B, K, dtype=torch.int32, device=DEV)
    done[1, 0] = 1
    if K > 1:
        s_in[2, K - 1] = float("-inf")
    s_out, d_out, parent = torch.zeros_like(s_in), torch.zeros_like(done), torch.zeros_like(done)
    ids = torch.zeros(2, B * K, dtype=torch.int64, device=DEV)
    ops.beam_step(x, s_in, done, s_out, d_out, parent, ids, 1, ops.beam_workspace(B, K, DEV), eos=102, pad=0)
    show("beam_step %s V=%d K=%d" % (tn, V, K), [("ids", ids), ("parent", parent), ("score", s_out), ("done", d_out)])


def topk_case(tn, dtype, V, K, M=5):
    g = torch.Generator().manual_seed(2000 + V + K)
    x, lse = rows(g, M, V, dtype), draw(g, M) + 9.0
    ids, logp = ops.topk_logp(x, lse, M, V, K)
    show("topk_logp %s V=%d K=%d" % (tn, V, K), [("ids", ids), ("logp", logp)])


def argmax_case(V, H=128):
    g = torch.Generator().manual_seed(3000 + V)
    for dtype, tn in DTYPES:
        idx, val = ops.rows_argmax(rows(g, 7, V, dtype), V)
        show("rows_argmax %s V=%d" % (tn, V), [("idx", idx), ("val", val)])
    Vp = (V + 3) // 4 * 4
    w, bias = draw(g, Vp, H, dtype=torch.bfloat16, scale=0.3), draw(g, Vp)
    for n in (5, 20, 38, 60):
        x = draw(g, n, H, dtype=torch.bfloat16)
        for fused in (True, False):
            idx, val = ops.vocab_argmax(x, w, bias, V, fused=fused)
            show("vocab_argmax %s V=%d n=%d" % ("fused" if fused else "gemm", V, n), [("idx", idx), ("val", val)])


def cos_case(V, D=100):
    g = torch.Generator().manual_seed(4000 + V)
    e = torch.randn(V // 4 + 1, D, generator=g).repeat_interleave(4, 0)[:V] + 0.6 * torch.randn(V, D, generator=g)
    ehat = (e / e.norm(dim=1, keepdim=True)).to(DEV)
    src = torch.randint(0, V, (37,), generator=g).to(torch.int32).to(DEV)
    for K, thr in ((10, 0.5), (16, None)):
        idx, val = ops.cos_topk(ehat, None, K=K, threshold=thr, route="many")
        show("cos_topk many V=%d full table K=%d thr=%s" % (V, K, thr), [("idx", idx), ("val", val)])
        for route in ("many", "few"):
            idx, val = ops.cos_topk(ehat, src, K=K, threshold=thr, route=route)
            show("cos_topk %s V=%d 37 sources K=%d thr=%s" % (route, V, K, thr), [("idx", idx), ("val", val)])


def sample_case(tn, dtype, V, B=6):
    g = torch.Generator().manual_seed(5000 + V)
    x, u = rows(g, B, V, dtype), torch.rand(B, generator=g).clamp_min(1e-6).to(DEV)
    banned = (torch.rand(B, V, generator=g) < 0.3).to(DEV)
    banned[2] = True
    for name, kw in (("k=7", dict(top_k=7)), ("k=64", dict(top_k=64)), ("p=0.9", dict(top_k=0, top_p=0.9)),
                     ("k=64 p=0.8", dict(top_k=64, top_p=0.8)), ("k=7 banned", dict(top_k=7, banned=banned)),
                     ("k=64 p=0.8 banned", dict(top_k=64, top_p=0.8, banned=banned))):
        out, out_s = torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
        logp = torch.zeros(B, device=DEV)
        ops.sample_topk(x, 0.7, kw["top_k"], u, out, banned=kw.get("banned"), top_p=kw.get("top_p", 0.0))
        ops.sample_topk_scored(x, 0.7, kw["top_k"], u, out_s, logp, banned=kw.get("banned"), top_p=kw.get("top_p", 0.0))
        show("sample_topk %s V=%d %s" % (tn, V, name), [("ids", out), ("ids scored", out_s), ("logp", logp)])


def main():
    for V in VS:
        for dtype, tn in DTYPES:
            for K in (1, 5, 8):
                beam_case(tn, dtype, V, K)
            for K in (1, 8, 16):
                topk_case(tn, dtype, V, K)
            sample_case(tn, dtype, V)
        argmax_case(V)
        cos_case(V)


if __name__ == "__main__":
    main()
