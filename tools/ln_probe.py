#!/usr/bin/env python3
"""Back-to-back timing of the fused dropout+residual+LayerNorm kernels (bf16) at the step's shapes.
usage: ln_probe.py            ln_fwd / ln_bwd at the step's shapes
       ln_probe.py mscale     ... at the decoder's row counts
       ln_probe.py fold       the LayerNorm-folded GEMMs (gemm_ln_fwd / gemm_ln_bwd) at the decoder's and the vision stream's shapes
       ln_probe.py gemv       the decode step's skinny GEMM with and without the folded LayerNorm (M = 16)"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from gst_visdial_amd import ops
from gst_visdial_amd._lib import LN_RESID
dev = "cuda"
rng = ops.Rng(torch.device(dev), seed=1)
def run(M, H, p, reps=40):
    bf = torch.bfloat16
    x, res, y, dy = [torch.randn(M, H, device=dev).to(bf) for _ in range(4)]
    dres, dx = torch.empty_like(x), torch.empty_like(x)
    g, b = torch.ones(H, device=dev), torch.zeros(H, device=dev)
    kw = dict(mode=LN_RESID, dtype=ops.BF16, M=M, H=H, gamma=g, beta=b, mean=torch.empty(M, device=dev), rstd=torch.empty(M, device=dev),
              eps=1e-12, x=x, res=res, y=y, p_pre=p, site_pre=3, rng=rng)
    nblk = ops.ln_bwd_blocks(M)
    partial = torch.empty(nblk * 3 * H, device=dev)
    def t(fn):
        for _ in range(3): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    tf = t(lambda: ops.ln_fwd(**kw))
    tb = t(lambda: ops.ln_bwd(kw, dy, partial, dres=dres, dx=dx))
    byt_f, byt_b = 3 * M * H * 2, (5 * M * H * 2 + nblk * 3 * H * 4)
    print("M=%5d H=%4d p=%.1f  fwd %6.1f us (%5.0f GB/s)   bwd %6.1f us (%5.0f GB/s)" % (M, H, p, tf, byt_f / tf / 1e3, tb, byt_b / tb / 1e3))
def timed(fn, reps=40):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps
def run_fold(M, H, N, p):
    bf = torch.bfloat16
    x, res, y, dy = [torch.randn(M, H, device=dev).to(bf) for _ in range(4)]
    dres, dx = torch.empty_like(x), torch.empty_like(x)
    kw = dict(mode=LN_RESID, dtype=ops.BF16, M=M, H=H, gamma=torch.ones(H, device=dev), beta=torch.zeros(H, device=dev),
              mean=torch.empty(M, device=dev), rstd=torch.empty(M, device=dev), eps=1e-12, x=x, res=res, y=y, p_pre=p, site_pre=3, rng=rng)
    Wf, Wb = (torch.randn(N, H, device=dev) * 0.05).to(bf), (torch.randn(H, N, device=dev) * 0.05).to(bf)
    Cf, Cb = torch.empty(M, N, device=dev, dtype=bf), torch.empty(M, N, device=dev, dtype=bf)
    rpb = ops.gemm_ln_rows()
    nblk = (M + rpb - 1) // rpb
    partial = torch.empty(nblk * 3 * H, device=dev)
    tf = timed(lambda: ops.gemm_ln_fwd(kw, Wf, Cf, N))
    tb = timed(lambda: ops.gemm_ln_bwd(kw, dy, partial, nblk, Wb, Cb, N, dres=dres, dx=dx))
    print("fold M=%5d H=%4d N=%4d p=%.1f  fwd %6.1f us   bwd %6.1f us" % (M, H, N, p, tf, tb))
def run_gemv(M, K, N):
    bf = torch.bfloat16
    A, B = torch.randn(M, K, device=dev).to(bf), (torch.randn(N, K, device=dev) * 0.05).to(bf)
    C_, y = torch.empty(M, N, device=dev, dtype=bf), torch.empty(M, K, device=dev, dtype=bf)
    g, b, bias = torch.ones(K, device=dev), torch.zeros(K, device=dev), torch.zeros(N, device=dev)
    t0 = timed(lambda: ops.gemm(A, B, C_, M, N, K, bias=bias), reps=200)
    t1 = timed(lambda: ops.gemv_ln(A, B, C_, M, N, K, g, b, 1e-12, y_out=y, bias=bias), reps=200)
    print("gemv M=%3d K=%4d N=%4d  gemv16 %6.2f us   gemv16_ln %6.2f us" % (M, K, N, t0, t1))
if len(sys.argv) > 1 and sys.argv[1] == "fold":
    for M, H, N in ((400, 768, 768), (400, 768, 2304), (400, 768, 3072), (592, 1024, 1024)):
        for p in (0.0, 0.3):
            run_fold(M, H, N, p)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "gemv":
    for N in (768, 3072):
        run_gemv(16, 768, N)
    sys.exit(0)
shapes = ((4096, 768), (592, 1024), (400, 768), (16384, 768))
if len(sys.argv) > 1 and sys.argv[1] == "mscale":      # row scaling of the decoder's LayerNorms (see tools/row_split_probe.sh)
    shapes = ((400, 768), (200, 768), (100, 768))
for M, H in shapes:
    for p in (0.0, 0.3):
        run(M, H, p)
