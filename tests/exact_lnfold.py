"""Exact layer of the LayerNorm-folded GEMMs: gemm_rows_kernel (csrc/gemm_rows.hip, through
ops.gemm_ln_fwd / ops.gemm_ln_bwd) and gemv16_ln_kernel (csrc/gemv.hip, through ops.gemv_ln), end to end with no tolerance.

The rows are those of exact_ln: h = m + sigma * 2^k gives mean == m, rstd == 2^-k, xhat == sigma bit for bit, with gamma in
{0.5, 1, 2} and integer beta the normalised row is a bf16-exact vector of half-integers, and multiplied by the integer weights of
exact_gemm the product is exact in any accumulation order.  The backward rows are exact_ln's as well (c1, c2, dh and every column
sum exact); the A operand of the folded product is then the bf16 image of dx, a vector of multiples of 1/16.  The decode kernel
forms its variance in one pass, E[x^2] - mean^2: the sums K m and K (m^2 + 4^k) are exact (exact_range refuses a case where they
are not), so var == 4^k there too.  Every activation input (x, res, dy, B, addend, DGELU's aux, the decode rows) sits in a
NaN-poisoned window with ld >= width + 8, every output (y, mean, rstd, dres, dx, partial, C, GELU's aux, y_out) in a canary
window, gamma and beta are 16-byte aligned vectors with poisoned tails, eps = 1e-12 is absorbed.  GELU cases keep the tolerance
of test_gemm_exact_gpu.py (erf is not exact arithmetic) and still get the window checks.

Census.  Every case states the instantiation it expects -- gemm_rows_kernel<OT, BKM, PRO, NV> or gemv16_ln_kernel<F32OUT>.  These
entry points have no kernel-name query and ops.Profiler records no symbol for them, so the mapping from a case to an
instantiation is STATED from the dispatch code (rows_launch: NV = 3 for H <= 768, else 4; the entry points' choice of OT, BKM and
PRO; gemv16_ln_dispatch's out_f32), not observed.  check_census ties the 16 + 2 instantiations of the built library to the table.

Noise rows (gemv_ln only): random bf16 rows with |mean| / std up to 16 against a float64 LayerNorm, since exact rows cannot show
cancellation in the one-pass variance.

Plain helper module: no fixtures, no hooks; everything takes a backend `be` (be.device, be.keep, be.gemm_ln_fwd, be.gemm_ln_bwd,
be.gemv_ln, be.colsum_partials), so tests/test_exact_lnfold_harness_cpu.py proves it on the CPU against a stand-in written in
torch and tests/test_lnfold_exact_gpu.py runs it on the HIP kernels.
"""
import collections
import re

import torch

import exact_gemm as E
import exact_ln as X
from exact_gemm import BF16, F32, Window, integers, reference, rne, assert_bit_equal, assert_exact_range
from exact_ln import balanced_signs, exact_range, vec

FOLD_KERNEL_RE = re.compile(rb"_Z\d+(?:gemm_rows_kernel|gemv16_ln_kernel)\w*")
ROWS = 16                       # rows per block of gemm_rows_kernel (ROWS_BM): one [3][H] partial slab per block
EPS = X.EPS
DT = X.DT
_OT = E._OT
# NV of every H of the table -- stated here from rows_launch (H <= 768: 3), NOT computed: when the threshold moves, the census
# of a case names another kernel than the library's dispatch picks, and the statement has to be revisited.
NV_OF = {64: 3, 128: 3, 192: 3, 704: 3, 768: 3, 832: 4, 1024: 4}
NOISE_Y_BOUND = 2.0 ** -7       # test_ops_gpu.py::test_decode_layernorm_folded_into_the_linear: 2^-7 * max(1, |y|max)
NOISE_C_TOL = 2.0 * 1.2e-2      # test_ops_gpu.py: check(..., bf16, 2.0)


def gelu_tol(dtype):
    import test_gemm_exact_gpu as G          # (imported late: that module's census imports this one)
    return G.GELU_TOL[dtype]


# ---------------------------------------------------------------------------------------------- the tables
_Rows = collections.namedtuple("RowsCase", "dir out b_km M N H p_pre res bias add epi side kmin kmax")


class RowsCase(_Rows):
    """One launch of gemm_ln_fwd (dir "fwd") or gemm_ln_bwd ("bwd").  side (bwd): which of dres / dx the launch is given --
    "both", "dres", "dx" or "alias" (dx is dres, p_pre = 0); epi: None, "gelu" (fwd), "dgelu" (bwd); add: accumulating epilogue."""
    __slots__ = ()

    @property
    def nv(self):
        return NV_OF.get(self.H, 0)          # (0: no kernel takes this H -- the refusal cases)

    @property
    def kernel(self):
        return "gemm_rows_kernelI%sLb%dELi%dELi%dEE" % (_OT[self.out], self.b_km, 1 if self.dir == "fwd" else 2, self.nv)

    @property
    def ln(self):
        return X.case("resid", "bf16", self.M, self.H, p_pre=self.p_pre, res=self.res, alias=self.side == "alias", nv=self.nv,
                      kmin=self.kmin, kmax=self.kmax, bwd=self.dir == "bwd")

    @property
    def id(self):
        s = "%s-%s-%s-%dx%dx%d-nv%d" % (self.dir, self.out, "km" if self.b_km else "rm", self.M, self.N, self.H, self.nv)
        if self.p_pre: s += "-p%g" % self.p_pre
        if not self.res: s += "-nores"
        if self.bias: s += "-bias"
        if self.add: s += "-add"
        if self.epi: s += "-" + self.epi
        if self.side != "both": s += "-" + self.side
        return s


def rows(dir, M, N, H, out="bf16", b_km=None, p_pre=0.0, res=True, bias=False, add=False, epi=None, side="both", kmin=None, kmax=None):
    b_km = (dir == "bwd") if b_km is None else b_km
    # (backward: dx is a vector of multiples of 2^-kmax / 2 up to ~500 * 2^-kmin; the wide rows keep k in 0..2 so that the
    #  product with the weights stays inside 2^24 units -- assert_exact_range checks every case)
    wide = dir == "bwd" and H > 192
    kmin = (0 if wide else -1) if kmin is None else kmin
    kmax = (2 if wide else 3) if kmax is None else kmax
    return RowsCase(dir, out, int(b_km), M, N, H, p_pre, res, bias, add, epi, side, kmin, kmax)


def build_rows_cases():
    c = []
    # -- every instantiation once at the smallest shape of its NV: OT x BKM x PRO x NV
    for out in ("bf16", "f32"):
        for b_km in (False, True):
            for H in (64, 832):
                c.append(rows("fwd", 17, 640, H, out=out, b_km=b_km, bias=True, p_pre=0.5 if b_km else 0.0))
                c.append(rows("bwd", 17, 640, H, out=out, b_km=b_km, p_pre=0.0 if b_km else 0.5))
    # -- rows: a single block (1, 15, 16), two (17), three (33); N = 640 (exactly the five tiles of the side outputs), 648 (a
    #    ragged sixth tile), 768
    for i, M in enumerate((1, 15, 16, 17, 33)):
        N = (640, 648, 768)[i % 3]
        out = ("bf16", "f32")[i % 2]
        c.append(rows("fwd", M, N, 128, out=out, bias=True, add=i % 2 == 1, p_pre=0.5 * (i % 2)))
        c.append(rows("bwd", M, N, 128, out=out, add=i % 2 == 0, p_pre=0.5 * ((i + 1) % 2)))
    # -- columns: H = 64 (KT = 1: fewer K-tiles than the two stages the prologue issues), 128 (as many), 192 (the first refill),
    #    704 / 768 (NV = 3 with and without a ragged last vector), 832 / 1024 (NV = 4)
    for i, H in enumerate((64, 128, 192, 704, 768, 832, 1024)):
        N = (648, 768, 640)[i % 3]
        c.append(rows("fwd", 33, N, H, out=("f32", "bf16")[i % 2], b_km=i % 2 == 1, bias=i % 2 == 0, add=i % 3 == 0, p_pre=0.5 * (i % 2)))
        c.append(rows("bwd", 33, N, H, out=("bf16", "f32")[i % 2], b_km=i % 2 == 0, add=i % 3 == 1, p_pre=0.5 * ((i + 1) % 2)))
    # -- the epilogues: plain accumulate, DGELU alone and with an addend, GELU
    for out in ("bf16", "f32"):
        c += [rows("bwd", 17, 648, 192, out=out, add=True, p_pre=0.5), rows("bwd", 33, 640, 768, out=out, epi="dgelu", p_pre=0.5),
              rows("bwd", 15, 768, 128, out=out, epi="dgelu", add=True, b_km=False),
              rows("fwd", 17, 648, 192, out=out, epi="gelu", bias=True, p_pre=0.5), rows("fwd", 33, 640, 832, out=out, epi="gelu", b_km=True)]
    # -- null pointers: no residual; dres only, dx only, dx is dres at p = 0
    c += [rows("fwd", 17, 640, 192, res=False), rows("fwd", 16, 648, 1024, res=False, out="f32", bias=True),
          rows("bwd", 17, 640, 192, res=False), rows("bwd", 33, 648, 832, res=False, out="f32"),
          rows("bwd", 17, 640, 128, side="dres", p_pre=0.5), rows("bwd", 17, 640, 128, side="dx", p_pre=0.5),
          rows("bwd", 33, 648, 768, side="dres"), rows("bwd", 33, 768, 1024, side="dx", p_pre=0.5, out="f32"),
          rows("bwd", 17, 640, 128, side="alias"), rows("bwd", 33, 648, 704, side="alias", b_km=False, add=True)]
    # -- the largest row count the kernel takes, once per direction
    c += [rows("fwd", 1024, 640, 64, bias=True, p_pre=0.5), rows("bwd", 1024, 640, 64, p_pre=0.5, kmin=0, kmax=1)]
    return c


_Gemv = collections.namedtuple("GemvCase", "M N K out bias add epi yout kmin kmax")


class GemvCase(_Gemv):
    """One launch of gemv_ln.  add: an addend of the OUTPUT's type; yout: y_out is given."""
    __slots__ = ()

    @property
    def kernel(self):
        return "gemv16_ln_kernelILb%dEE" % (self.out == "f32")

    @property
    def id(self):
        s = "gemv-%s-%dx%dx%d" % (self.out, self.M, self.N, self.K)
        for flag, tag in ((self.bias, "-bias"), (self.add, "-add"), (self.epi, "-%s" % self.epi), (not self.yout, "-noy")):
            if flag: s += tag
        return s


def gemv(M, N, K, out="bf16", bias=False, add=False, epi=None, yout=True, kmin=-1, kmax=3):
    return GemvCase(M, N, K, out, bias, add, epi, yout, kmin, kmax)


def build_gemv_cases():
    """K = 8: one 16-lane group live; 32: one wave step; 40: a ragged second step; 200; 1000: the last register slot ragged; 1024:
    every slot live.  N = 4: a quarter of a tile; 16; 20; 136: nine workgroups, the last ragged."""
    c = []
    for i, K in enumerate((8, 32, 40, 200, 1000, 1024)):
        for j, out in enumerate(("bf16", "f32")):
            M, N = (1, 7, 16)[(i + j) % 3], (4, 16, 20, 136)[(i + 2 * j) % 4]
            c.append(gemv(M, N, K, out=out, bias=(i + j) % 2 == 0, add=i % 3 == j, yout=(i + j) % 3 != 2))
    for out in ("bf16", "f32"):
        c += [gemv(16, 136, 1024, out=out, bias=True, add=True), gemv(7, 4, 8, out=out, yout=False), gemv(1, 20, 200, out=out, add=True),
              gemv(16, 4, 1000, out=out, bias=True), gemv(7, 136, 40, out=out, epi="gelu", bias=True), gemv(16, 20, 1024, out=out, epi="gelu", yout=False)]
    return c


ROWS_CASES = build_rows_cases()
GEMV_CASES = build_gemv_cases()
CASES = ROWS_CASES + GEMV_CASES


def kernel_names(cases=None):
    """The instantiations the table names (test_gemm_exact_gpu.py counts them in its census)."""
    return sorted(set(c.kernel for c in (CASES if cases is None else cases)))


def check_census(symbols, cases=None, out=print):
    """Every gemm_rows_kernel / gemv16_ln_kernel instantiation of the built library is named by a case (no exemption), every
    kernel the table names exists, and there are 16 + 2 of them."""
    cs = CASES if cases is None else cases
    named = kernel_names(cs)
    reached = set()
    for s in symbols:
        hits = [n for n in named if n in s]
        assert len(hits) == 1, "%s: named by %r -- an instantiation of the library that no case names" % (s, hits)
        reached.update(hits)
        users = [c for c in cs if c.kernel == hits[0]]
        out("%-64s %d case(s), e.g. %s" % (s, len(users), users[0].id))
    assert reached == set(named), "kernels named by a case but absent from the library: %r" % sorted(set(named) - reached)
    nrows, ngemv = sum("gemm_rows_kernel" in s for s in symbols), sum("gemv16_ln_kernel" in s for s in symbols)
    assert (nrows, ngemv) == (16, 2), "the library carries %d gemm_rows_kernel and %d gemv16_ln_kernel instantiations, not 16 + 2" % (nrows, ngemv)


# ---------------------------------------------------------------------------------------------- small helpers
class Refusal(Exception):
    """What a stand-in raises where the library returns a GSTVD_E_* status."""


def assert_refused(fn, name):
    try:
        fn()
    except Exception as e:                                   # (ops raises GstvdError, a stand-in Refusal)
        assert "GSTVD_E_" in str(e), "%s: failed with %r, not with a status of the library" % (name, e)
        return
    raise AssertionError("%s: accepted, the entry point must refuse it" % name)


def assert_all_canary(win, name):
    """Nothing of an output allocation was written, inside the window or outside."""
    n = int((win.flat.view(E._INT[win.dtype]) != X._canary(win.dtype)).sum().item())
    assert n == 0, "%s: %d element(s) written by a launch that had to be refused" % (name, n)


def product_range(A, peak, name):
    """The product stays where fp32 sums of it are exact in any order: `peak` (exact_gemm.reference's) in units of the smallest
    set bit of the A operand."""
    a = A.abs()
    for e in range(0, 12):
        if bool(((a * 2.0 ** e) == (a * 2.0 ** e).floor()).all()):
            return assert_exact_range(peak * 2.0 ** e, name)
    raise AssertionError(name + ": the A operand is not made of multiples of 2^-11")


def check_gelu(C, aux, pre, name):
    u = pre.float().requires_grad_(True)
    a = torch.nn.functional.gelu(u)
    a.backward(torch.ones_like(a))
    E.assert_close_rel_to_max(C, a.detach(), gelu_tol(C.dtype), name + ": gelu")
    if aux is not None:
        E.assert_close_rel_to_max(aux, u.grad, gelu_tol(aux.dtype), name + ": gelu'")


class _LnBackend(object):
    """What exact_ln.Problem asks of a backend, for the folded kernels' geometry: one partial slab per 16 rows."""

    def __init__(self, be):
        self.be, self.device = be, be.device

    def keep(self, n, p, site):
        return self.be.keep(n, p, site)

    def blocks(self, M, H=None, mode=None):
        return (M + ROWS - 1) // ROWS

    def colsum_partials(self, *a):
        self.be.colsum_partials(*a)


# ---------------------------------------------------------------------------------------------- gemm_ln_fwd / gemm_ln_bwd
class RowsProblem(object):
    """exact_ln.Problem's windows and reference of the LayerNorm (forward rows; backward rows, solved for x and res under the
    known p_pre = 0.5 keep mask) plus the GEMM's: B, bias, addend, aux, C."""

    def __init__(self, be, c, seed=0, decoy=False):
        self.be, self.c = be, c
        p = self.ln = X.Problem(_LnBackend(be), c.ln, seed, decoy=decoy)
        if c.dir == "bwd":
            p.build_backward()
        gen, dev, M, N, H = p.gen, p.dev, c.M, c.N, c.H
        ot = DT[c.out]
        br, bc = (H, N) if c.b_km else (N, H)
        f64 = torch.float64
        p.inp("B", br, bc, BF16, integers((br, bc), E.A_RANGE, gen, f64, dev), ld=bc + 8)
        if c.bias:
            p.inp("bias", 1, N, F32, integers((N,), E.E_RANGE, gen, f64, dev))
        if c.add:
            p.inp("addend", M, N, ot, integers((M, N), E.E_RANGE, gen, f64, dev), ld=N + 16)
        if c.epi == "dgelu":
            p.inp("aux", M, N, BF16, 2.0 ** X.ints((M, N), -1, 1, gen, dev), ld=N + 24)
        elif c.epi == "gelu":
            p.out("aux", M, N, BF16, ld=N + 24)
        p.out("C", M, N, ot, ld=N + 8)
        # the A operand of the product: the bf16 image of y (exact) or of dx (rounded where dh needs nine bits)
        self.A = rne(p.y_ref if c.dir == "fwd" else p.ref["dx"], BF16).double()
        self.C_ref, peak = reference(self.A, p.t["B"].view, False, bool(c.b_km), bias=p.v("bias"), addend=p.v("addend"),
                                     aux=p.v("aux") if c.epi == "dgelu" else None)
        product_range(self.A, peak, c.id)

    def gemm_kw(self):
        p, c = self.ln, self.c
        kw = dict(bias=p.v("bias")[0] if c.bias else None) if c.dir == "fwd" else {}          # (gemm_ln_bwd takes no bias)
        return dict(kw, b_km=bool(c.b_km), addend=p.v("addend"), aux=p.v("aux"), epi=c.epi)

    def launch(self, **over):
        p, c = self.ln, self.c
        if c.dir == "fwd":
            kw = p.fwd_kw(**over.pop("ln", {}))
            self.be.gemm_ln_fwd(kw, p.v("B"), p.v("C"), over.pop("N", c.N), **dict(self.gemm_kw(), **over))
            return
        kw, bw = p.bwd_args()
        kw.update(over.pop("ln", {}))
        dres = p.v("dres") if c.side in ("both", "dres", "alias") else None
        dx = p.v("dres") if c.side == "alias" else (p.v("dx") if c.side in ("both", "dx") else None)
        self.be.gemm_ln_bwd(kw, bw["dy"], bw["partial"], over.pop("nblk", p.nblk), p.v("B"), p.v("C"), over.pop("N", c.N),
                            dres=dres, dx=dx, **dict(self.gemm_kw(), **over))

    def slab_ref(self):
        """partial[mt, 0..2, :]: float64 sums of dy * xhat, dy and dx over the real rows of 16-row block mt."""
        p, c = self.ln, self.c
        dy = p.t["dy"].view.double()
        v = torch.cat([dy * p.sig, dy, p.ref["dx"]], 1)
        pad = torch.zeros(p.nblk * ROWS - c.M, 3 * c.H, dtype=torch.float64, device=v.device)
        return torch.cat([v, pad], 0).view(p.nblk, ROWS, 3 * c.H).sum(1)

    def check(self):
        p, c, n = self.ln, self.c, self.c.id
        if c.dir == "fwd":
            p.check_forward()
        else:
            for name, given in (("dres", c.side != "dx"), ("dx", c.side in ("both", "dx"))):
                if name not in p.t:
                    continue
                if given:
                    X.assert_written(p.t[name], "%s: %s" % (n, name))
                    assert_bit_equal(p.v(name), p.ref["dh" if name == "dres" else "dx"], "%s: %s" % (n, name))
                else:
                    assert_all_canary(p.t[name], "%s: %s (not given to the launch)" % (n, name))
            X.assert_written(p.t["partial"], n + ": partial")
            assert_bit_equal(p.t["partial"].view, self.slab_ref(), n + ": partial slabs, every row")
            p.reduce_and_check()
        X.assert_written(p.t["C"], n + ": C")
        if c.epi == "gelu":
            X.assert_written(p.t["aux"], n + ": aux")
            check_gelu(p.v("C"), p.v("aux"), self.C_ref, n)
        else:
            assert_bit_equal(p.v("C"), self.C_ref, n + ": C")
        p.assert_surroundings()

    def outputs(self):
        o = self.ln.outputs()
        o["C"] = self.ln.t["C"].view3.clone()
        if self.c.epi == "gelu":
            o["aux"] = self.ln.t["aux"].view3.clone()
        return o


def run_rows(be, c, seed=0, decoy=False, checks=True):
    p = RowsProblem(be, c, seed, decoy=decoy)
    p.launch()
    if checks:
        p.check()
    return p


# ---------------------------------------------------------------------------------------------- gemv_ln
class GemvProblem(object):
    """The decode rows A = m + sigma * 2^k (K columns), the weights, and the windows of one gemv_ln launch."""
    inp, out, assert_surroundings = X.Problem.inp, X.Problem.out, X.Problem.assert_surroundings

    def __init__(self, be, c, seed=0, decoy=False, ld_y=None):
        self.be, self.c, self.dev, self.decoy = be, c, be.device, decoy
        self.t, self.wins = {}, []
        dev, M, N, K = self.dev, c.M, c.N, c.K
        gen = E.generator(3000 + seed, dev)
        ot = DT[c.out]
        self.m, self.k = X.ints((M, 1), -3, 3, gen, dev), X.ints((M, 1), c.kmin, c.kmax, gen, dev)
        self.sig = balanced_signs(M, K, gen, dev)
        h = self.m + self.sig * 2.0 ** self.k
        # the one-pass sums the kernel forms: K m and K (m^2 + 4^k)
        exact_range(c.id, row=(h, 1), squares=(h * h, 1))
        gamma, beta = 2.0 ** X.ints((K,), -1, 1, gen, dev), X.ints((K,), -8, 8, gen, dev)
        self.inp("A", M, K, BF16, h, ld=K + 8)
        self.inp("gamma", 1, K, F32, gamma)
        self.inp("beta", 1, K, F32, beta)
        f64 = torch.float64
        self.inp("B", N, K, BF16, integers((N, K), E.A_RANGE, gen, f64, dev), ld=K + 16)
        if c.bias:
            self.inp("bias", 1, N, F32, integers((N,), E.E_RANGE, gen, f64, dev))
        if c.add:
            self.inp("addend", M, N, ot, integers((M, N), E.E_RANGE, gen, f64, dev), ld=N + 16)
        if c.epi == "gelu":
            self.out("aux", M, N, BF16, ld=N + 24)
        self.out("C", M, N, ot, ld=2 * N + 8)                        # strided rows of a wider buffer
        if c.yout:
            self.out("y_out", M, K, BF16, ld=K + 8 if ld_y is None else ld_y)
        self.y_ref = gamma * self.sig + beta
        self.C_ref, peak = reference(rne(self.y_ref, BF16).double(), self.t["B"].view, False, False, bias=self.v("bias"), addend=self.v("addend"))
        product_range(self.y_ref, peak, c.id)

    def v(self, name):
        w = self.t.get(name)
        if w is None:
            return None
        return w.view[0] if name in ("gamma", "beta", "bias") else w.view

    def launch(self, **over):
        c = self.c
        kw = dict(y_out=self.v("y_out"), bias=self.v("bias"), addend=self.v("addend"), aux=self.v("aux"), epi=c.epi)
        kw.update(over)
        self.be.gemv_ln(self.v("A"), self.v("B"), self.v("C"), c.M, c.N, c.K, self.v("gamma"), self.v("beta"), EPS, **kw)

    def check(self):
        c, n = self.c, self.c.id
        if c.yout:
            # y_out == gamma * sigma + beta needs mean == m AND var == 4^k (premise: sqrtf and the division correctly rounded)
            X.assert_written(self.t["y_out"], n + ": y_out")
            assert_bit_equal(self.v("y_out"), self.y_ref, n + ": y_out")
        X.assert_written(self.t["C"], n + ": C")
        if c.epi == "gelu":
            X.assert_written(self.t["aux"], n + ": aux")
            check_gelu(self.v("C"), self.v("aux"), self.C_ref, n)
        else:
            assert_bit_equal(self.v("C"), self.C_ref, n + ": C")
        self.assert_surroundings()

    def outputs(self):
        return dict((k, self.t[k].view3.clone()) for k in ("C", "y_out", "aux") if k in self.t)


def run_gemv(be, c, seed=0, decoy=False, checks=True):
    p = GemvProblem(be, c, seed, decoy=decoy)
    p.launch()
    if checks:
        p.check()
    return p


def run_case(be, c, seed=0, decoy=False, checks=True):
    return (run_gemv if isinstance(c, GemvCase) else run_rows)(be, c, seed, decoy, checks)


# ---------------------------------------------------------------------------------------------- refusals
def check_rows_refusals(be, dir):
    """Each refused as an error of the library, with every output allocation still canary.  Every problem is built at the size it
    names, so a launch that was wrongly accepted would still stay inside its allocations."""
    bad = [("M = 1025", rows(dir, 1025, 640, 64, kmin=0, kmax=1), {}),
           ("N = 632", rows(dir, 17, 632, 64), {}),
           ("N % 8 != 0", rows(dir, 17, 644, 64), {}),
           ("H = 1088", rows(dir, 17, 640, 1088), {}),
           ("H % 64 != 0", rows(dir, 17, 640, 96), {}),
           ("p_post > 0", rows(dir, 17, 640, 64), dict(ln=dict(p_post=0.5))),
           ("COLSUM epilogue", rows(dir, 17, 640, 64), dict(epi="colsum"))]
    for name, c, over in bad:
        _refused(RowsProblem(be, c), over, "gemm_ln_%s, %s" % (dir, name))


def _refused(p, over, name):
    assert_refused(lambda: p.launch(**over), name)
    t = p.ln.t if isinstance(p, RowsProblem) else p.t
    for k in ("y", "mean", "rstd", "dres", "dx", "partial", "C", "y_out"):
        if k in t:
            assert_all_canary(t[k], "%s: %s" % (name, k))
    if "aux" in t and t["aux"].fill == "canary":
        assert_all_canary(t["aux"], name + ": aux")


def check_gemv_refusals(be):
    _refused(GemvProblem(be, gemv(17, 16, 32)), {}, "gemv_ln, M = 17")
    _refused(GemvProblem(be, gemv(7, 16, 1032, kmax=2)), {}, "gemv_ln, K = 1032")
    _refused(GemvProblem(be, gemv(7, 16, 32), ld_y=32 + 4), {}, "gemv_ln, ldy % 8 != 0")


# ---------------------------------------------------------------------------------------------- invariances
assert_same = X.assert_same


def check_surroundings_do_not_matter(be, c, seed=0):
    """Rows >= M and the pad columns of every input: NaN or finite garbage, the outputs are the same bits."""
    a = run_case(be, c, seed).outputs()
    b = run_case(be, c, seed, decoy=True, checks=False).outputs()
    assert_same(a, b, c.id + ": NaN against finite surroundings")


def check_reproducible(be, c, seed=0):
    """Two launches of the same case: the same bits, the partial slabs included."""
    assert_same(run_case(be, c, seed).outputs(), run_case(be, c, seed).outputs(), c.id + ": run to run")


def check_row_blocks_are_independent(be, c, block, seed=0, checks=True):
    """The outputs of row block `block` (16 rows of gemm_rows_kernel; ONE row of the decode kernel) do not depend on the data of
    the other rows: those are replaced by the rows of another draw (finite, no longer an exact case), gamma, beta and the weights
    stay."""
    gemv_ = isinstance(c, GemvCase)
    step = 1 if gemv_ else ROWS
    lo, hi = block * step, min((block + 1) * step, c.M)
    assert 0 <= lo < hi and c.M > step
    p = run_case(be, c, seed, checks=checks)
    mk = GemvProblem if gemv_ else RowsProblem
    q, other = mk(be, c, seed), mk(be, c, seed + 1)
    tq, to = (q.t, other.t) if gemv_ else (q.ln.t, other.ln.t)
    keep = torch.zeros(c.M, dtype=torch.bool, device=be.device)
    keep[lo:hi] = True
    for name in ("A", "x", "res", "dy", "addend", "mean_in", "rstd_in") + (("aux",) if c.epi == "dgelu" else ()):
        if name in tq:
            w, src = tq[name], to[name]
            if name in ("mean_in", "rstd_in"):
                w.view[0][~keep] = src.view[0][~keep]
            else:
                w.view[~keep] = src.view[~keep]
    q.launch()
    a, b = p.outputs(), q.outputs()
    for k in a:
        if k in ("mean", "rstd"):
            x, y = a[k][0, 0, lo:hi], b[k][0, 0, lo:hi]
        elif k == "partial":
            x, y = a[k][0, block], b[k][0, block]
        else:
            x, y = a[k][0, lo:hi], b[k][0, lo:hi]
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), \
            "%s: %s of rows %d..%d changed with the data of the other rows" % (c.id, k, lo, hi - 1)
    (q.ln if not gemv_ else q).assert_surroundings()


# ---------------------------------------------------------------------------------------------- noise rows (gemv_ln)
NOISE_RATIOS, NOISE_K = (0.2, 4.0, 16.0), (200, 1024)


def bf16_ulps(got, ref):
    """|got - ref| in units of the last place of the bf16 number `ref`; a reference below 2^-6 is measured in the ulp of 2^-6
    (next to zero a distance in ulps says nothing about the variance)."""
    r = ref.double()
    ulp = 2.0 ** (torch.floor(torch.log2(r.abs().clamp(min=2.0 ** -6))) - 7)
    return (got.double() - r).abs() / ulp


def check_noise_rows(be, ratio, K, M=16, N=136, seed=0, out=print):
    """Random bf16 rows with |mean| / std = ratio against LayerNorm in float64: y_out within the project's bound
    2^-7 * max(1, |y|max) of rne_bf16(reference), C within the bar of check(..., 2.0).  Returns (and prints) the largest distance
    of y_out in bf16 ulps."""
    dev = be.device
    gen = E.generator(4000 + seed, dev)
    name = "gemv_ln noise rows, |mean| / std = %g, K = %d" % (ratio, K)
    sgn = torch.where(torch.arange(M, device=dev) % 2 == 0, 1.0, -1.0)[:, None]
    z = torch.randn(M, K, generator=gen, device=dev).double()
    z = (z - z.mean(1, keepdim=True)) / z.std(1, keepdim=True)              # (the ratio of every row, not of the distribution)
    x = ((z + ratio * sgn) * 1.7).to(BF16)
    w = (torch.randn(N, K, generator=gen, device=dev) * 0.1).to(BF16)
    gamma = (1.0 + 0.2 * torch.randn(K, generator=gen, device=dev)).float()
    beta, bias = (0.1 * torch.randn(K, generator=gen, device=dev)).float(), torch.randn(N, generator=gen, device=dev).float()
    A = Window(M, K, BF16, dev, "poison", ld=K + 8).set(x)
    Bw = Window(N, K, BF16, dev, "poison", ld=K + 8).set(w)
    g, b, bs = vec(K, F32, dev, "poison", gamma), vec(K, F32, dev, "poison", beta), vec(N, F32, dev, "poison", bias)
    Cw, Y = Window(M, N, BF16, dev, "canary", ld=N + 8), Window(M, K, BF16, dev, "canary", ld=K + 8)
    be.gemv_ln(A.view, Bw.view, Cw.view, M, N, K, g.vector(), b.vector(), EPS, y_out=Y.view, bias=bs.vector(), addend=None, aux=None, epi=None)
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    measured = float((mean.abs() / var.sqrt()).min().item())
    assert measured > 0.8 * ratio, "%s: the rows have |mean| / std = %.2f" % (name, measured)
    yref = rne((xd - mean) / torch.sqrt(var + EPS) * gamma.double() + beta.double(), BF16)
    X.assert_written(Y, name + ": y_out")
    X.assert_written(Cw, name + ": C")
    ulps = float(bf16_ulps(Y.view, yref).max().item())
    err = float((Y.view.double() - yref.double()).abs().max().item())
    bound = NOISE_Y_BOUND * max(1.0, float(yref.double().abs().max().item()))
    out("%s: y_out at most %g bf16 ulp(s) from the float64 reference, |error| %.3e (bound %.3e)" % (name, ulps, err, bound))
    assert err <= bound, "%s: y_out is %.3e from the float64 reference (%g ulps), bound %.3e" % (name, err, ulps, bound)
    E.assert_close_rel_to_max(Cw.view, yref.double() @ w.double().t() + bias.double(), NOISE_C_TOL, name + ": C")
    for tag, win in (("A", A), ("B", Bw), ("gamma", g), ("beta", b), ("bias", bs), ("C", Cw), ("y_out", Y)):
        win.assert_surroundings_untouched("%s: %s" % (name, tag))
    return ulps


def lib_path():
    return E.lib_path()
