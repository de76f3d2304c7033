#!/usr/bin/env python3
"""SHA-256 of everything the attention kernels write, for a fixed list of small shapes that reaches every route: run it at two
commits and diff the outputs (the kernels use no atomics: two runs of one build agree line for line).
usage: attn_digest.py            every case; the two-part route at a one-pass shape runs in a fresh child process
       attn_digest.py twopart    that case alone (the child: GSTVD_ATTN_ONEPASS is read once per process)
Inputs come from a CPU torch.Generator with a fixed seed, key_mask has its last fifth masked, p = 0.1 with a fixed Rng seed."""
import hashlib, os, subprocess, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from gst_visdial_amd import ops

DEV = "cuda"


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def case(name, dtype, d, Lq, Lk, causal=False, bits=False, bwd=True, p=0.1, B=2, nh=3, kv_group=1, kv_bstride=0):
    g = torch.Generator().manual_seed(20240607)
    H, Bk, kbs = nh * d, B // kv_group, kv_bstride or Lk
    draw = lambda rows: torch.randn(rows, H, generator=g).to(dtype).to(DEV)
    Q, K, V, dO = draw(B * Lq), draw(Bk * kbs), draw(Bk * kbs), draw(B * Lq)
    O, dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    lse = torch.zeros(B * nh * Lq, device=DEV)
    delta = torch.zeros_like(lse)
    mask = torch.ones(Bk, Lk, device=DEV)
    mask[:, int(0.8 * Lk):] = 0
    nbits = ops.attn_keep_bits_shape(B, nh, Lq, Lk, d, dtype, causal, p) if bits else 0
    keep = torch.zeros(nbits, device=DEV, dtype=torch.int64) if nbits else None
    a = ops.attn_desc(Q, K, V, O, lse, mask, B, nh, Lq, Lk, d, causal=causal, mask_neg=-10000.0, drop_p=p, site=5,
                      rng=ops.Rng(torch.device(DEV), seed=1), kv_group=kv_group, kv_bstride=kv_bstride, drop_bits=keep)
    print("%s\n  fwd %s" % (name, ops.attn_kernel_symbol(a)))
    ops.attn_fwd(a)
    out = [("O", O), ("LSE", lse)]
    if bwd:
        ops.attn_bwd(a, dO, dQ, dK, dV, delta)
        print("  bwd %s" % ops.attn_kernel_symbol(a, bwd=True))
        out += [("dQ", dQ), ("dK", dK), ("dV", dV), ("delta", delta)]
    if keep is not None:
        out.append(("drop_bits", keep))
    torch.cuda.synchronize()
    for label, t in out:
        print("  %-9s %s" % (label, sha(t)))


def twopart():
    case("bf16 d64 130x130 GSTVD_ATTN_ONEPASS=0", torch.bfloat16, 64, 130, 130)


def main():
    for dtype, tn in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        for d in (32, 64, 128):
            for Lq, Lk, causal in ((5, 19, False), (37, 67, True), (65, 63, False), (25, 130, False), (130, 25, False)):
                case("%s d%d %dx%d%s" % (tn, d, Lq, Lk, " causal" if causal else ""), dtype, d, Lq, Lk, causal=causal)
    for Lq, Lk in ((64, 65), (70, 256), (130, 130)):
        for bits in (False, True):
            case("bf16 d64 %dx%d%s" % (Lq, Lk, " drop_bits" if bits else ""), torch.bfloat16, 64, Lq, Lk, bits=bits)
    sys.stdout.flush()
    env = dict(os.environ, GSTVD_ATTN_ONEPASS="0")
    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "twopart"], env=env).returncode
    if rc:
        sys.exit("attn_digest: the GSTVD_ATTN_ONEPASS=0 child ended with status %d" % rc)
    # forward only: shared keys (kv_group) behind a batch stride; the decode kernel takes one query and no dropout
    case("bf16 d64 1x77 kv_group=3 kv_bstride=90 p=0", torch.bfloat16, 64, 1, 77, bwd=False, p=0.0, B=6, kv_group=3, kv_bstride=90)
    case("bf16 d64 5x70 kv_group=2 kv_bstride=80", torch.bfloat16, 64, 5, 70, bwd=False, B=4, kv_group=2, kv_bstride=80)


if __name__ == "__main__":
    twopart() if sys.argv[1:] == ["twopart"] else main()
