#!/usr/bin/env python3
"""SHA-256 of what the LayerNorm family writes, from fixed seeds: run it against two builds of the library and diff the outputs.
  ln_fwd / ln_bwd        three modes, both dtypes, H = 256, 768, 1024, 2048, M = 13, 2049, 8193 (dropout 0.1 before and behind);
                         backward at the geometry the step passes (ln_bwd_blocks(M, H, mode)) and, where that differs, at nblk = 0
  gemm_ln_fwd / _bwd     M = 77 and 400, H = 768 and 1024, N = 768
  gemv_ln                M = 5, K = 768
  ColsumBatch            one flush: nblk 1, 4, 28, 29, 32, 33, 61 and a slab entry
Left out, because they add in arrival order (atomics) on inputs that are not exactly summable: the embedding mode's table gradients
dword / dpos / dtt / dtt_ext (its column partials ARE digested) and locgrad.  colsum_partials and colsum are left out because their
summation order is allowed to follow the batched kernel's (LayerNorm section)."""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from gst_visdial_amd import ops
from gst_visdial_amd._lib import LN_RESID, LN_EMBED, LN_IMAGE

DEV = "cuda"
MODES = (("resid", LN_RESID), ("embed", LN_EMBED), ("image", LN_IMAGE))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def show(name, outs):
    torch.cuda.synchronize()
    print(name)
    for label, t in outs:
        print("  %-9s %s" % (label, sha(t)))


def route(kw, bwd=None):
    """The launched kernel's name and template arguments (the mangled symbol without its parameter list)."""
    return ops.ln_kernel_symbol(kw, bwd=bwd).rsplit("Ev", 1)[0]


def draw(g, *shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def ln_case(mname, mode, dtype, tn, M, H, rng):
    g = torch.Generator().manual_seed(20241021 + 7 * M + H)
    od = ops.BF16 if dtype == torch.bfloat16 else ops.F32
    y, dy = torch.zeros(M, H, dtype=dtype, device=DEV), draw(g, M, H, dtype=dtype)
    mean, rstd = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    kw = dict(mode=mode, dtype=od, M=M, H=H, gamma=draw(g, H) + 1.0, beta=draw(g, H), mean=mean, rstd=rstd, eps=1e-12, y=y,
              p_post=0.1, site_post=4, rng=rng)
    bw = {}
    if mode == LN_RESID:
        kw.update(x=draw(g, M, H, dtype=dtype), res=draw(g, M, H, dtype=dtype), p_pre=0.1, site_pre=3)
        bw.update(dres=torch.zeros_like(y), dx=torch.zeros_like(y))
    elif mode == LN_IMAGE:
        kw.update(x=draw(g, M, H, dtype=dtype), loc=torch.rand(M, 5, generator=g).to(DEV), w_loc=draw(g, H, 5), b_loc=draw(g, H))
        bw.update(dres=torch.zeros_like(y))
    else:
        V, T = 50, 64
        kw.update(ids=torch.randint(0, V, (M,), generator=g).to(DEV), segs=torch.randint(0, 4, (M,), generator=g).to(DEV), T=T,
                  type_vocab=2, word=draw(g, V, H), pos=draw(g, T + 2, H), tt=draw(g, 2, H), tt_ext=draw(g, 2, H), pos_offset=2)
        bw.update(dword=torch.zeros(V, H, device=DEV), dpos=torch.zeros(T + 2, H, device=DEV), dtt=torch.zeros(2, H, device=DEV),
                  dtt_ext=torch.zeros(2, H, device=DEV))
    name = "ln %s %s M=%d H=%d" % (mname, tn, M, H)
    ops.ln_fwd(**kw)
    show(name + " fwd " + route(kw), [("y", y), ("mean", mean), ("rstd", rstd)])
    nvp = 4 if mode == LN_EMBED else 3
    wide = ops.ln_bwd_blocks(M, H, mode)
    for nblk in sorted(set((wide, 0)), reverse=True):
        n = nblk or ops.ln_bwd_blocks(M)
        partial = torch.zeros(n * nvp * H, device=DEV)
        for t in bw.values():
            t.zero_()
        args = dict(dy=dy, partial=partial, nblk=nblk, **bw)
        ops.ln_bwd(kw, **args)
        outs = [("partial", partial)] + [(k, bw[k]) for k in ("dres", "dx") if k in bw]
        show(name + " bwd nblk=%d " % nblk + route(kw, args), outs)


def fold_case(M, H, N, rng):
    g = torch.Generator().manual_seed(99 + M + H)
    bf = torch.bfloat16
    x, res, dy = draw(g, M, H, dtype=bf), draw(g, M, H, dtype=bf), draw(g, M, H, dtype=bf)
    y, dres, dx = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    mean, rstd = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    kw = dict(mode=LN_RESID, dtype=ops.BF16, M=M, H=H, gamma=draw(g, H) + 1.0, beta=draw(g, H), mean=mean, rstd=rstd, eps=1e-12,
              x=x, res=res, y=y, p_pre=0.1, site_pre=3, rng=rng)
    W = draw(g, N, H, dtype=bf, scale=0.05)                 # forward: row-major B[N, K = H]
    Cf = torch.zeros(M, N, dtype=bf, device=DEV)
    ops.gemm_ln_fwd(kw, W, Cf, N, bias=draw(g, N))
    show("gemm_ln_fwd M=%d H=%d N=%d" % (M, H, N), [("C", Cf), ("y", y), ("mean", mean), ("rstd", rstd)])
    Wb = draw(g, H, N, dtype=bf, scale=0.05)                # k-major B: [K = H, N]
    rpb = ops.gemm_ln_rows()
    nblk = (M + rpb - 1) // rpb
    partial = torch.zeros(nblk * 3 * H, device=DEV)
    Cb = torch.zeros(M, N, dtype=bf, device=DEV)
    ops.gemm_ln_bwd(kw, dy, partial, nblk, Wb, Cb, N, dres=dres, dx=dx)
    show("gemm_ln_bwd M=%d H=%d N=%d" % (M, H, N), [("C", Cb), ("dres", dres), ("dx", dx), ("partial", partial)])


def gemv_case(M, K, N):
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    A, B = draw(g, M, K, dtype=bf), draw(g, N, K, dtype=bf, scale=0.05)
    C_, y = torch.zeros(M, N, dtype=bf, device=DEV), torch.zeros(M, K, dtype=bf, device=DEV)
    ops.gemv_ln(A, B, C_, M, N, K, draw(g, K) + 1.0, draw(g, K), 1e-12, y_out=y, bias=draw(g, N))
    show("gemv_ln M=%d K=%d N=%d" % (M, K, N), [("C", C_), ("y", y)])
    C2 = torch.zeros(M, N, dtype=bf, device=DEV)
    ops.gemm(A, B, C2, M, N, K, bias=draw(g, N))
    show("gemv M=%d K=%d N=%d" % (M, K, N), [("C", C2)])


def colsum_case():
    g = torch.Generator().manual_seed(11)
    b = ops.ColsumBatch(torch.device(DEV))
    outs = []
    for i, (nblk, sv, H, nvec) in enumerate([(1, 3, 64, 3), (4, 4, 260, 3), (28, 3, 4, 1), (29, 4, 768, 3), (32, 3, 252, 3), (33, 4, 64, 1),
                                            (61, 4, 1024, 3)]):
        src = draw(g, nblk, sv * H)
        o = [draw(g, H) for _ in range(nvec)] + [None] * (3 - nvec)
        b.add(src.reshape(-1), tuple(o), nblk, sv * H, H, nvec, tuple((i + j) % 2 == 1 for j in range(3)))
        outs += [("out %d.%d" % (i, j), t) for j, t in enumerate(o) if t is not None] + [("keep", src)]
    x = draw(g, 333, 2304, dtype=torch.bfloat16)
    scratch, out = torch.zeros(6, 2304, device=DEV), torch.zeros(2304, device=DEV)
    b.add_slabs(x, 333, 2304, scratch, out, False)
    b.flush()
    show("ColsumBatch one flush", [(k, t) for k, t in outs if k != "keep"] + [("slab out", out), ("scratch", scratch)])


def main():
    rng = ops.Rng(torch.device(DEV), seed=1)
    for mname, mode in MODES:
        for dtype, tn in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
            for H in (256, 768, 1024, 2048):
                for M in (13, 2049, 8193):
                    ln_case(mname, mode, dtype, tn, M, H, rng)
    for M in (77, 400):
        for H in (768, 1024):
            fold_case(M, H, 768, rng)
    gemv_case(5, 768, 768)
    colsum_case()


if __name__ == "__main__":
    main()
