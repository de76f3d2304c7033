"""Exact layer of the vocabulary arg-max kernels (csrc/vocab_argmax.hip) on a real MI355X.

Operands are integer-valued in [-8, 8] with a bias in halves (tests/exact_mlm.py): every sum is exact in fp32 in any order, so the
device must return the float64 reference's arg-max column AND value to the bit -- no tolerance anywhere in this file.  The table
always has round_up(V, 64) rows whose padding rows, and the bias entries behind V, hold the largest values an operand can
carry: a kernel that read them as candidates would pick them in every row."""
import numpy as np
import pytest
import torch

import exact_mlm as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS = (1, 3, 16, 17, 64, 65)
HS = (64, 768)
VS = (1, 127, 128, 129, 600, 30522)
PAD = 64                      # canary elements in front of and behind every output window
CANARY_I64, CANARY_F32, CANARY_U8 = -0x0123456789ABCDEF, -7.5e37, 0xA5

_CASES = {}


def ops():
    from gst_visdial_amd import ops as o
    return o


def case(H, V):
    """Operands of 65 rows for (H, V), built once: every n of the parametrised tests takes the first n rows."""
    key = (H, V)
    if key not in _CASES:
        x, w, b = X.exact_operands(max(NS), H, V, seed=H * 100003 + V)
        X.poison_padding(w, b, V)
        ref = X.exact_logits(x, w, b, V)
        idx, val = X.argmax_rows(ref, V)
        _CASES[key] = dict(x=x, w=w, b=b, idx=idx, val=val,
                           xd=torch.from_numpy(x).to(DEV), wd=torch.from_numpy(w).to(DEV), bd=torch.from_numpy(b).to(DEV))
        c = _CASES[key]
        c["xb"], c["wb"] = c["xd"].to(torch.bfloat16), c["wd"].to(torch.bfloat16)
        assert torch.equal(c["xb"].float(), c["xd"]) and torch.equal(c["wb"].float(), c["wd"])      # exact in bf16
    return _CASES[key]


class Windows(object):
    """idx / val / workspace windows with canaries on both sides."""

    def __init__(self, n, ws_bytes=0):
        self.n, self.ws_bytes = n, ws_bytes
        self.idx = torch.full((n + 2 * PAD,), CANARY_I64, dtype=torch.int64, device=DEV)
        self.val = torch.full((n + 2 * PAD,), CANARY_F32, dtype=torch.float32, device=DEV)
        self.ws = torch.full((ws_bytes + 2 * PAD,), CANARY_U8, dtype=torch.uint8, device=DEV)

    def views(self):
        return self.idx[PAD:PAD + self.n], self.val[PAD:PAD + self.n], self.ws[PAD:PAD + self.ws_bytes]

    def check(self):
        n, wb = self.n, self.ws_bytes
        for t, canary, k in ((self.idx, CANARY_I64, n), (self.val, CANARY_F32, n), (self.ws, CANARY_U8, wb)):
            assert bool((t[:PAD] == canary).all()) and bool((t[PAD + k:] == canary).all()), "a write outside its window"


def run_fused(xb, wb, bias, V, n):
    o = ops()
    win = Windows(n, o.vocab_argmax_ws_bytes(n, V))
    idx, val, ws = win.views()
    out = o.vocab_argmax_fused(xb[:n], wb, bias, V, n=n, idx=idx, val=val, ws=ws)
    assert out is not None, "the fused kernel refused a bf16 problem with H % 32 == 0"
    torch.cuda.synchronize()
    win.check()
    return out[0].clone(), out[1].clone()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_fused_is_exact_deterministic_and_agrees_with_the_gemm_route(n, H, V):
    c = case(H, V)
    o = ops()
    idx, val = run_fused(c["xb"], c["wb"], c["bd"], V, n)
    assert np.array_equal(idx.cpu().numpy(), c["idx"][:n])
    assert np.array_equal(val.cpu().numpy().astype(np.float64), c["val"][:n])
    assert int(idx.max()) < V
    idx2, val2 = run_fused(c["xb"], c["wb"], c["bd"], V, n)                       # determinism
    assert torch.equal(idx, idx2) and same_bits(val, val2)
    gi, gv = o.vocab_argmax(c["xb"][:n], c["wb"], c["bd"], V, n=n, fused=False)   # the existing GEMM + gstvd_rows_argmax
    assert torch.equal(idx, gi) and same_bits(val, gv)


@pytest.mark.parametrize("V", (129, 30522))
@pytest.mark.parametrize("H", HS)
def test_fp32_operands_take_the_gemm_route(H, V):
    c = case(H, V)
    o = ops()
    n = 17
    assert o.vocab_argmax_fused(c["xd"][:n], c["wd"], c["bd"], V, n=n) is None   # fp32: not the fused kernel's
    idx, val = o.vocab_argmax(c["xd"][:n], c["wd"], c["bd"], V, n=n)
    assert np.array_equal(idx.cpu().numpy(), c["idx"][:n])
    assert np.array_equal(val.cpu().numpy().astype(np.float64), c["val"][:n])


def test_unsupported_width_and_empty_input():
    o = ops()
    x = torch.zeros(3, 48, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(64, 48, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(64, dtype=torch.float32, device=DEV)
    assert o.vocab_argmax_fused(x, w, b, 60) is None                              # H = 48: GSTVD_E_UNSUPPORTED, not an error
    idx, val = o.vocab_argmax(x, w, b, 60)                                        # all logits equal: column 0
    assert idx.tolist() == [0, 0, 0] and val.tolist() == [0.0, 0.0, 0.0]
    idx, val = o.vocab_argmax(x[:0], w, b, 60)
    assert idx.numel() == 0 and val.numel() == 0 and idx.dtype == torch.int64 and val.dtype == torch.float32


@pytest.mark.parametrize("V", (600, 30522))
@pytest.mark.parametrize("H", HS)
def test_planted_ties_and_edges(H, V):
    """Six launches of 17 rows, one per planted case; rows r (the case's number) and 16 (the second 16-row block) are all-8 rows.
    A planted column has an all-8 table row, so against an all-8 x row it reaches 64 H, the largest product there is.  Planted
    columns rest at bias -1; a case raises its own to 0 (or 0.5); every other candidate's bias is at most -0.5."""
    c = case(H, V)
    n = 17
    x, w, b = c["x"][:n].copy(), c["w"].copy(), c["b"].copy()
    X.cap_bias(b, V, -0.5)
    cols = dict(two_tiles=(70, V - 90), one_tile=(130, 170), one_group=(195, 196), by_bias=(10, 300), last=(V - 1,), first=(0,))
    for c_ in sum(cols.values(), ()):
        w[c_] = 8.0
        b[c_] = -1.0
    want = dict(two_tiles=70, one_tile=130, one_group=195, by_bias=300, last=V - 1, first=0)
    o = ops()
    wb = torch.from_numpy(w).to(DEV).to(torch.bfloat16)
    for r, (name, cc) in enumerate(cols.items()):
        xr = x.copy()
        xr[r] = 8.0
        xr[16] = 8.0                                            # a row of the second 16-row block too
        br = b.copy()
        for c_ in cc:
            br[c_] = 0.0
        if name == "by_bias":
            br[cc[0]], br[cc[1]] = 0.0, 0.5                     # equal products: the bias decides, for the LARGER column
        ref = X.exact_logits(xr, w, br, V)
        ridx, rval = X.argmax_rows(ref, V)
        assert ridx[r] == want[name] and ridx[16] == want[name], (name, ridx[r])       # the case is planted as intended
        assert rval[r] == 64.0 * H + (0.5 if name == "by_bias" else 0.0)
        xb, bd = torch.from_numpy(xr).to(DEV).to(torch.bfloat16), torch.from_numpy(br).to(DEV)
        idx, val = run_fused(xb, wb, bd, V, n)
        assert np.array_equal(idx.cpu().numpy(), ridx), name
        assert np.array_equal(val.cpu().numpy().astype(np.float64), rval), name
        gi, gv = o.vocab_argmax(xb, wb, bd, V, n=n, fused=False)
        assert torch.equal(idx, gi) and same_bits(val, gv), name


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("V", (1, 255, 256, 257, 30522))
def test_rows_argmax_alone(V, dtype):
    """Logits already in memory, ld > V, the columns behind V poisoned; ties planted across threads, waves and inside one thread's
    stride."""
    o = ops()
    n, ld = 5, X.round_up(V, 64) + 64
    rng = np.random.RandomState(V)
    z = rng.randint(-100, 101, size=(n, ld)).astype(np.float32)          # integers: exact in bf16 too
    z[:, V:] = 1.0e30
    if V > 1:
        z[1, [V - 1, V // 2]] = 120.0                                    # tie: the smaller column
        z[2, V - 1] = 121.0                                              # the last candidate wins
        z[3, 0] = 122.0                                                  # the first one
        z[4, :V] = -7.0                                                  # all equal: column 0
    if V > 256:
        z[0, [3, 259]] = 125.0                                           # one thread's stride (c, c + 256)
    ridx, rval = X.argmax_rows(z, V)
    zd = torch.from_numpy(z).to(DEV).to(dtype)
    assert torch.equal(zd[:, :V].float().cpu(), torch.from_numpy(z[:, :V]))
    win = Windows(n)
    idx, val, _ = win.views()
    gi, gv = o.rows_argmax(zd, V, idx=idx, val=val)
    torch.cuda.synchronize()
    win.check()
    assert np.array_equal(gi.cpu().numpy(), ridx)
    assert np.array_equal(gv.cpu().numpy(), rval.astype(np.float32))
    gi2, gv2 = o.rows_argmax(zd, V)
    assert torch.equal(gi, gi2) and same_bits(gv, gv2)
