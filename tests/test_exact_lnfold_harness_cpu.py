"""The exact layer of the LayerNorm-folded GEMMs proves itself on the CPU (tests/exact_lnfold.py): every case
of the table runs against a stand-in of the three entry points written in torch -- 16-row blocks, side outputs, refusals -- and
against deliberately wrong stand-ins, each of which must fail the check meant for it.  Nothing here touches a GPU."""
import pytest
import torch

import exact_lnfold as F
from exact_gemm import BF16

CPU = torch.device("cpu")


def _raw(t, rows, cols, ld, extra=0):
    """[rows, cols] elements from the first element of view `t` on, row stride ld -- pointer semantics, as a kernel sees it."""
    return torch.as_strided(t, (rows, cols), (ld, 1), t.storage_offset() + extra)


def _ld(t):
    return t.stride(-2)


class Torch(object):
    """fp32 stand-in of ops.gemm_ln_fwd / gemm_ln_bwd / gemv_ln / colsum_partials with the kernels' geometry.  `defect`: one
    planted error (see DEFECTS)."""

    def __init__(self, defect=None):
        self.device, self.defect = CPU, defect

    def keep(self, n, p, site):
        g = torch.Generator().manual_seed(7919 * site + 1)
        return (torch.rand(n, generator=g) >= p).float() / (1.0 - p)

    def colsum_partials(self, partial, nblk, nvec, H, o0, o1, o2, accumulate):
        s = _raw(partial, nblk, nvec * H, 3 * H).sum(0)
        for j, o in enumerate((o0, o1, o2)):
            if o is not None and j < nvec:
                o.copy_(s[j * H:(j + 1) * H] + (o if accumulate else 0))

    # -- shared pieces
    def _store(self, dst, val, trunc=False):
        if dst.dtype == BF16 and trunc:
            val = (val.contiguous().view(torch.int32) & -65536).view(torch.float32)
        dst.copy_(val)

    def _rows_check(self, kw, B, N, epi):
        M, H = kw["M"], kw["H"]
        if kw["mode"] != "resid" or kw["dtype"] != BF16 or H % 64 or H > 1024 or M > 1024 or kw["p_post"] > 0 or N < 640 or N % 8 \
                or epi == "colsum":
            raise F.Refusal("GSTVD_E_UNSUPPORTED")
        if _ld(B) % 8 or _ld(kw["x"]) % 4:
            raise F.Refusal("GSTVD_E_ALIGN")

    def _h(self, kw):
        M, H = kw["M"], kw["H"]
        x = kw["x"].float()
        if kw["p_pre"] > 0:
            x = x * self.keep(M * H, kw["p_pre"], kw["site_pre"]).view(M, H)
        return x + kw["res"].float() if kw["res"] is not None else x

    def _epilogue(self, acc, C, M, N, bias, addend, aux, epi):
        if bias is not None:
            acc = acc + bias
        if addend is not None:
            acc = acc + addend.float()
        if epi == "gelu":
            u = acc.clone().requires_grad_(True)
            a = torch.nn.functional.gelu(u)
            a.backward(torch.ones_like(a))
            aux.copy_(u.grad)
            acc = a.detach()
        elif epi == "dgelu":
            acc = acc * aux.float()
        C.copy_(acc)
        if self.defect == "c_past_n":                          # one element behind column N - 1 of row 0
            _raw(C, 1, 1, 1, N).fill_(1.0)

    def _product(self, A, B, b_km):
        A = A.to(BF16).float()
        if self.defect == "k_tile":                           # the last 64 columns of the A image never arrive
            A = A.clone()
            A[:, -64:] = 0
        return A @ (B.float() if b_km else B.float().t())

    # -- gemm_ln_fwd
    def gemm_ln_fwd(self, kw, B, C, N, b_km=False, bias=None, addend=None, aux=None, epi=None):
        self._rows_check(kw, B, N, epi)
        M, H = kw["M"], kw["H"]
        h = self._h(kw)
        if self.defect == "mean_cols":                        # the row sum runs over H + 1 columns
            h1 = _raw(kw["x"], M, H + 1, _ld(kw["x"])).float()
            mean = (h.sum(1, keepdim=True) + h1[:, H:]) / (H + 1)
        else:
            mean = h.sum(1, keepdim=True) / H
        var = ((h - mean) ** 2).sum(1, keepdim=True) / H
        rstd = 1.0 / torch.sqrt(var + kw["eps"])
        kw["mean"].copy_(mean[:, 0]), kw["rstd"].copy_(rstd[:, 0])
        y = kw["gamma"] * ((h - mean) * rstd) + kw["beta"]
        kw["y"].copy_(y)
        if self.defect == "y_row_m":                          # the row behind the last one is written as well
            _raw(kw["y"], 1, H, 1, M * _ld(kw["y"])).fill_(0.0)
        self._epilogue(self._product(y, B, b_km), C, M, N, bias, addend, aux, epi)

    # -- gemm_ln_bwd
    def gemm_ln_bwd(self, kw, dy, partial, nblk, B, C, N, dres=None, dx=None, b_km=True, addend=None, aux=None, epi=None):
        self._rows_check(kw, B, N, epi)
        M, H = kw["M"], kw["H"]
        if nblk != (M + F.ROWS - 1) // F.ROWS:
            raise F.Refusal("GSTVD_E_SHAPE")
        pre = self.keep(M * H, kw["p_pre"], kw["site_pre"]).view(M, H) if kw["p_pre"] > 0 else torch.ones(M, H)
        h = self._h(kw)
        rstd = kw["rstd"][:, None]
        xh = (h - kw["mean"][:, None]) * rstd
        dyv = dy.float()
        gy = dyv * kw["gamma"]
        c1 = gy.sum(1, keepdim=True) / H
        c2 = (gy * xh).sum(1, keepdim=True) / H
        if self.defect == "c1_sign":
            c1 = -c1
        dh = (gy - c1 - xh * c2) * rstd
        dxv = dh * pre
        if dres is not None:
            self._store(dres, dh)
        if dx is not None and (dres is None or dx.data_ptr() != dres.data_ptr() or kw["p_pre"] > 0):
            self._store(dx, dxv, trunc=self.defect == "truncate")
        v = torch.cat([dyv * xh, dyv, dxv], 1)
        pad = torch.zeros(nblk * F.ROWS - M, 3 * H)
        if self.defect == "slab_pad_row" and pad.shape[0]:     # the first row behind M counts into the last slab (dy only)
            pad[0, H:2 * H] = _raw(dy, 1, H, 1, M * _ld(dy))[0].float()
        v = torch.cat([v, pad], 0).view(nblk, F.ROWS, 3 * H).sum(1)
        part = _raw(partial, nblk, 3 * H, 3 * H)
        if self.defect == "slab_unwritten":
            part[:, :2 * H].copy_(v[:, :2 * H])
            part[:nblk - 1, 2 * H:].copy_(v[:nblk - 1, 2 * H:])
        else:
            part.copy_(v)
        self._epilogue(self._product(dxv, B, b_km), C, M, N, None, addend, aux, epi)

    # -- gemv_ln
    def gemv_ln(self, A, B, C, M, N, K, gamma, beta, eps, y_out=None, bias=None, addend=None, aux=None, epi=None):
        if N % 4 or K % 8:
            raise F.Refusal("GSTVD_E_SHAPE")
        if M > 16 or K > 1024 or epi in ("dgelu", "colsum"):
            raise F.Refusal("GSTVD_E_UNSUPPORTED")
        if _ld(A) % 8 or _ld(B) % 8 or (y_out is not None and _ld(y_out) % 8):
            raise F.Refusal("GSTVD_E_ALIGN")
        x = A.float()
        s1, s2 = x.sum(1, keepdim=True), (x * x).sum(1, keepdim=True)
        if self.defect == "pad_read":                         # the first pad column counts into the row sum
            s1 = s1 + _raw(A, M, 1, _ld(A), K).float()
        mean, ex2 = s1 / K, s2 / K
        rstd = 1.0 / torch.sqrt((ex2 - mean * mean).clamp(min=0) + eps)
        y = ((x - mean) * rstd * gamma + beta).to(BF16)
        if y_out is not None:
            if self.defect == "y_out_row0":
                y_out[1:].copy_(y[1:])
            else:
                y_out.copy_(y)
        self._epilogue(y.float() @ B.float().t(), C, M, N, bias, addend, aux, epi)


def ids(cs):
    return [c.id for c in cs]


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("c", F.CASES, ids=ids(F.CASES))
def test_harness_accepts_the_stand_in(c):
    """Every case of the table: the stand-in passes, and the reference alone stays inside 2^24 units (exact_range and
    assert_exact_range run inside the problem's construction)."""
    F.run_case(Torch(), c, F.CASES.index(c))


def test_the_table_holds_what_the_issue_lists():
    rs, gs = F.ROWS_CASES, F.GEMV_CASES
    for d in ("fwd", "bwd"):
        r = [c for c in rs if c.dir == d]
        assert {1, 15, 16, 17, 33, 1024} <= set(c.M for c in r) and sum(c.M == 1024 for c in r) == 1
        assert {640, 648, 768} == set(c.N for c in r)
        assert {64, 128, 192, 704, 768, 832, 1024} == set(c.H for c in r)
        assert {0, 1} == set(c.b_km for c in r) and {"bf16", "f32"} == set(c.out for c in r)
        assert {0.0, 0.5} == set(c.p_pre for c in r) and {True, False} == set(c.res for c in r)
    assert {"both", "dres", "dx", "alias"} == set(c.side for c in rs if c.dir == "bwd")
    assert all(c.p_pre == 0 for c in rs if c.side == "alias")
    assert any(c.add and not c.epi for c in rs if c.dir == "bwd") and any(c.epi == "dgelu" for c in rs)
    assert any(c.epi == "gelu" and c.out == o for c in rs for o in ("bf16", "f32"))
    assert {1, 7, 16} == set(c.M for c in gs) and {4, 16, 20, 136} == set(c.N for c in gs)
    assert {8, 32, 40, 200, 1000, 1024} == set(c.K for c in gs)
    for o in ("bf16", "f32"):
        g = [c for c in gs if c.out == o]
        assert any(c.bias for c in g) and any(c.add for c in g) and any(c.yout for c in g) and any(not c.yout for c in g)
        assert any(c.epi == "gelu" for c in g)
    assert len(F.kernel_names()) == 18


def test_every_k_of_the_range_occurs_and_the_backward_needs_rounding():
    """rstd == 2^-k is asserted for k in -1..3; a truncating bf16 store can only be seen where dx is not a bf16 number."""
    p = F.RowsProblem(Torch(), F.rows("bwd", 33, 640, 128, p_pre=0.5), seed=2)
    assert set(p.ln.k.flatten().tolist()) == {-1.0, 0.0, 1.0, 2.0, 3.0}
    dx = p.ln.ref["dx"]
    assert int((dx.to(BF16).double() != dx).sum()) > 20
    g = F.GemvProblem(Torch(), F.gemv(16, 16, 200), seed=1)
    assert len(set(g.k.flatten().tolist())) >= 4


def test_exact_range_guards_refuse_what_leaves_2p24():
    with pytest.raises(AssertionError, match="exact range"):                       # the one-pass sum of squares of a decode row
        F.GemvProblem(Torch(), F.gemv(7, 16, 1024, kmin=11, kmax=11))
    with pytest.raises(AssertionError, match="exact range"):
        F.product_range(torch.full((4, 4), 0.0625, dtype=torch.float64), 2.0 ** 20, "sixteenths")
    F.product_range(torch.full((4, 4), 0.0625, dtype=torch.float64), 2.0 ** 18, "sixteenths")


def test_refusal_checks_accept_the_stand_in():
    be = Torch()
    F.check_rows_refusals(be, "fwd")
    F.check_rows_refusals(be, "bwd")
    F.check_gemv_refusals(be)


def test_refusal_check_rejects_an_entry_point_that_accepts():
    class Lenient(Torch):
        def _rows_check(self, kw, B, N, epi):
            pass
    with pytest.raises(AssertionError, match="accepted|written by a launch"):
        F.check_rows_refusals(Lenient(), "fwd")


def test_invariance_checks_accept_the_stand_in():
    be = Torch()
    for c in (F.rows("fwd", 33, 640, 128, bias=True, p_pre=0.5), F.rows("bwd", 33, 648, 192, add=True, p_pre=0.5), F.gemv(7, 20, 200, bias=True, add=True)):
        F.check_surroundings_do_not_matter(be, c, 3)
        F.check_reproducible(be, c, 4)
        F.check_row_blocks_are_independent(be, c, 1, 5)


def test_row_block_check_rejects_a_stand_in_that_mixes_rows():
    class Mixing(Torch):
        def gemv_ln(self, A, B, C, M, N, K, *a, **kw):
            Torch.gemv_ln(self, A, B, C, M, N, K, *a, **kw)
            C[1].add_(A[0, 0].float().to(C.dtype))
    with pytest.raises(AssertionError, match="changed with the data of the other rows"):
        F.check_row_blocks_are_independent(Mixing(), F.gemv(7, 20, 200), 1, 5, checks=False)


def test_census_check_on_a_synthetic_symbol_list():
    syms = ["_Z16" + k + "v5GemmP6RowProi" for k in F.kernel_names() if "rows" in k] + \
           ["_Z16" + k + "v5GemmP4LnIn" for k in F.kernel_names() if "gemv" in k]
    assert len(syms) == 18
    F.check_census(syms, out=lambda s: None)
    with pytest.raises(AssertionError, match="no case names"):
        F.check_census(syms + ["_Z16gemm_rows_kernelIfLb0ELi3ELi3EEv5GemmP6RowProi"], out=lambda s: None)
    with pytest.raises(AssertionError, match="absent from the library"):
        F.check_census(syms[1:], out=lambda s: None)
    few = [c for c in F.CASES if c.out == "bf16"]
    with pytest.raises(AssertionError, match="no case names"):
        F.check_census(syms, cases=few, out=lambda s: None)


def test_noise_rows_check_against_the_stand_in():
    """The one-pass fp32 variance of the stand-in at |mean| / std = 0.2 and 4 stays within the bound; a variance that loses its
    low bits (computed in bf16) does not."""
    be = Torch()
    for r in (0.2, 4.0):
        assert F.check_noise_rows(be, r, 200, out=lambda s: None) <= 2

    class Coarse(Torch):
        def gemv_ln(self, A, B, C, M, N, K, gamma, beta, eps, **kw):
            Torch.gemv_ln(self, A, B, C, M, N, K, gamma, beta, eps, **kw)
            kw["y_out"].mul_(1.05)
    with pytest.raises(AssertionError, match="from the float64 reference"):
        F.check_noise_rows(Coarse(), 4.0, 200, out=lambda s: None)
    a = torch.tensor([1.0078125, -1.0, 0.0, 2.0 ** -9, 3.0], dtype=BF16)
    b = torch.tensor([1.0, -1.0, -0.0, 0.0, 3.03125], dtype=BF16)
    assert F.bf16_ulps(a, b).tolist() == [1.0, 0.0, 0.0, 16.0, 2.0]


# ------------------------------------------------------------------------------------------ planted defects
FWD = F.rows("fwd", 17, 640, 128, bias=True, p_pre=0.5)
BWD = F.rows("bwd", 17, 640, 128, p_pre=0.5)
GEMV = F.gemv(7, 20, 40, bias=True)
DEFECTS = [
    ("k_tile", FWD, ": C"),                           # one K-tile of the A image dropped
    ("k_tile", BWD, ": C"),
    ("c1_sign", BWD, ": dres"),                       # c1 with the wrong sign
    ("y_row_m", FWD, "outside the"),                  # y written for a row >= M
    ("c_past_n", FWD, "outside the"),                 # one element written past N in C
    ("c_past_n", GEMV, "outside the"),
    ("slab_pad_row", BWD, ": partial"),               # a partial slab that includes a padding row (poison: NaN)
    ("slab_unwritten", BWD, "never written"),         # a partial slab left unwritten
    ("mean_cols", FWD, ": mean"),                     # mean taken over H + 1 columns
    ("truncate", BWD, ": dx"),                        # a bf16 dx that truncates where it should round
    ("y_out_row0", GEMV, "never written"),            # a gemv_ln with no y_out row 0
    ("pad_read", GEMV, ": y_out"),                    # a poisoned padding column read into the row sum
]


@pytest.mark.parametrize("defect,c,match", DEFECTS, ids=["%s-%s" % (d[0], d[1].id) for d in DEFECTS])
def test_planted_defect_fails_the_check_meant_for_it(defect, c, match):
    F.run_case(Torch(), c, 1)                         # (the sound stand-in passes the very same case)
    with pytest.raises(AssertionError, match=match):
        F.run_case(Torch(defect), c, 1)
