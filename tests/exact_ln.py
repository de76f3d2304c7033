"""Exact layer of the LayerNorm tests: inputs whose answer is exact, write windows, a census of every route.

Forward.  Every pre-LayerNorm row is h = m + sigma * 2^k: m a small integer per row, k in -1..3 per row, sigma a balanced +-1
pattern (H / 2 entries of each sign, drawn per row).  The row sum is H * m in any order, the variance exactly 4^k, eps = 1e-12 is
absorbed (4^k + 1e-12 rounds to 4^k in fp32), and with a correctly rounded sqrtf and division rstd = 2^-k and xhat = sigma.  With
gamma in {0.5, 1, 2}, integer beta and p = 0.5 (factor exactly 2) y = keep * 2 * (gamma * sigma + beta) is exact: an fp32 y is
BIT-equal to the float64 reference computed WITHOUT eps, a bf16 y to its round-to-nearest-even image, mean == m and rstd == 2^-k
bit for bit.  That sqrtf and the division behave this way on the hardware is a PREMISE (the library is built without fast-math
flags, so both are the correctly rounded ones); every case asserts it, as the attention layer does for __expf.

Backward.  The post-dropout gradient gy = dy * keep_post * gamma of a row is an integer vector whose sum over the +1 columns and
over the -1 columns are both multiples of H / 4 (a + b * sigma + z of the issue with a, b per-row multiples of 1/4 in [-2, 2],
z zero-sum inside each sign class; with dropout the class sums are dealt over the kept columns only).  Then c1 = S1 / H and
c2 = S2 / H are small multiples of 1/4, dh = (gy - c1 - sigma * c2) * 2^-k is exact, and so is every column sum and every atomic sum into a table, in
any order: bit-equal and bit-reproducible.  A row sum that misses or doubles a column, or a c1 of the wrong sign, shows as a
non-zero multiple of 2^-k / H.  exact_range() computes in float64 the peak of every summed quantity in units of its smallest set
bit and refuses a case that leaves 2^24.

Every output is a window inside a canary-filled allocation, every input a window inside a NaN-poisoned one (exact_gemm.Window),
every activation has a leading dimension of H + 4 (fp32) / H + 8 (bf16) or more, table rows that no id / position / segment names
are NaN.  Every case names the forward and backward kernel it expects.

Plain helper module: no fixtures, no hooks; everything takes a backend `be` (be.device, be.keep, be.ln_fwd, be.ln_bwd, be.blocks,
be.colsum_partials, be.colsum, be.colsum_slabs, be.batch, be.locgrad), so tests/test_exact_ln_harness_cpu.py proves it on the CPU
against a stand-in written in torch and tests/test_ln_exact_gpu.py runs it on the HIP kernels.
"""
import collections
import re

import torch

import exact_gemm as E
from exact_gemm import BF16, CANARY, F32, Window, generator

LN_KERNEL_RE = re.compile(rb"_Z\d+(?:ln_fwd_kernel|ln_bwd_kernel|colsum_\w*kernel|locgrad_kernel)\w*")
DT = {"bf16": BF16, "f32": F32}
_TY = {"bf16": "DF16b", "f32": "f"}
MODES = {"resid": 0, "embed": 1, "image": 2}          # GSTVD_LN_RESID / _EMBED / _IMAGE
EPS = 1e-12
SITE_PRE, SITE_POST = 3, 11
_INT = {BF16: torch.int16, F32: torch.int32}

# ---------------------------------------------------------------------------------------------- the route table
# NV (256-column vectors per lane) of every H of the table -- stated here, NOT computed from the dispatch's thresholds: when those
# move, a case's shape lands on another kernel and its assertion fails.
NV_OF = {4: 1, 64: 1, 96: 1, 252: 1, 256: 1, 260: 3, 764: 3, 768: 3, 772: 4, 832: 4, 1024: 4, 1028: 8, 2044: 8, 2048: 8}

_Case = collections.namedtuple("LnCase", "mode dtype M H nv rw nw wide p_pre p_post res pad alias B T pos_offset type_vocab segs "
                                         "carrier kmin kmax bwd")


class Case(_Case):
    """One forward (+ backward) launch.  nv / rw / nw: the kernel the case expects (nw, rw: backward only); wide: the nblk
    the backward is given -- True: ln_bwd_blocks(M, H, mode); "narrow": ln_bwd_blocks(M), stated explicitly; False: 0 (the
    partials are then sized by ln_bwd_blocks(M) as well); res: RESID has a residual;
    pad: ld = H + pad for every activation; alias: dx is dres (p_pre = 0); EMBED: M = B * T, segs "mix" / "zero" / "none",
    carrier = the table that carries the sign pattern ("word", "pos" or "tt": tt and tt_ext)."""
    __slots__ = ()

    @property
    def fwd_kernel(self):
        return "ln_fwd_kernelI%sLi%dELi%dEE" % (_TY[self.dtype], MODES[self.mode], self.nv)

    @property
    def bwd_kernel(self):
        return "ln_bwd_kernelI%sLi%dELi%dELi%dELi%dEE" % (_TY[self.dtype], MODES[self.mode], self.nv, self.rw, self.nw)

    @property
    def id(self):
        s = "%s-%s-%dx%d-nv%d" % (self.mode, self.dtype, self.M, self.H, self.nv)
        if self.bwd: s += "-rw%dnw%d%s" % (self.rw, self.nw, {True: "-nblk", "narrow": "-nblkM", False: ""}[self.wide])
        else: s += "-fwd"
        if self.p_pre or self.p_post: s += "-p%g.%g" % (self.p_pre, self.p_post)
        if self.mode == "resid" and not self.res: s += "-nores"
        if self.alias: s += "-alias"
        if self.mode == "embed":
            s += "-b%dt%d+%d-tv%d-%s-%s" % (self.B, self.T, self.pos_offset, self.type_vocab, self.segs, self.carrier)
        return s


def case(mode, dtype, M, H, rw=1, nw=4, wide=False, p_pre=0.0, p_post=0.0, res=True, pad=None, alias=False, B=0, T=0, pos_offset=0,
         type_vocab=2, segs="mix", carrier="word", kmin=-1, kmax=3, bwd=True, nv=None):
    if mode == "embed":
        M = B * T
    pad = (8 if dtype == "bf16" else 4) if pad is None else pad
    return Case(mode, dtype, M, H, NV_OF[H] if nv is None else nv, rw, nw, wide, p_pre, p_post, res, pad, alias, B, T, pos_offset,
                type_vocab, segs, carrier, kmin, kmax, bwd)


HS = [4, 64, 252, 256, 260, 764, 768, 772, 1024, 1028, 2044, 2048]
DROPS = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]


def build_cases():
    c = []
    dts = ("f32", "bf16")
    # -- rows per block.  Forward: 4 rows per block; backward, 4 one-row waves: M = 1, 5, 2047 (the last 4-wave shape at H <= 768)
    for i, M in enumerate((1, 3, 4, 5)):
        for dt in dts:
            c.append(case("resid", dt, M, 260, p_post=0.5 * (i % 2), bwd=False))
            c.append(case("image", dt, M, 64, bwd=False))
    for i, M in enumerate((1, 5, 2047)):
        for dt in dts:
            c.append(case("resid", dt, M, 768, p_pre=DROPS[i][0], p_post=DROPS[i][1]))
            c.append(case("image", dt, M, 256))
    # -- backward, 16 one-row waves (M >= 2048, H <= 768, not EMBED), reached only through nblk = ln_bwd_blocks(M, H, mode); the
    #    same shape with nblk = 0 keeps the 4-wave kernel.  M % 16 = 0, 1, 15.  772 columns must not take it, 256 and 768 must.
    for i, M in enumerate((2048, 2049, 2063)):
        for dt in dts:
            H = (768, 256, 764)[i]
            c.append(case("resid", dt, M, H, nw=16, wide=True, p_pre=DROPS[i + 1][0], p_post=DROPS[i + 1][1]))
            c.append(case("resid", dt, M, H, nw=4, wide=False))
            # (the positive count of the 4-wave geometry, where the 16-wave one exists: accepted, and 4 waves)
            c.append(case("resid", dt, M, H, nw=4, wide="narrow", p_pre=DROPS[i][0], p_post=DROPS[i][1]))
            c.append(case("image", dt, M, (256, 768, 260)[i], nw=4, wide="narrow"))
            c.append(case("image", dt, M, (256, 768, 260)[i], nw=16, wide=True))
    for dt in dts:
        c.append(case("resid", dt, 2048, 772, nw=4, wide=True))
        c.append(case("image", dt, 2049, 772, nw=4, wide=True))
    # -- two rows per wave: M > 8192 (8192: the last one-row shape); rv[1] false for the missing second row at M = 8193; at
    #    M = 8200, H = 768 the 16-wave conditions hold as well and the two-row 4-wave kernel is the one taken
    for i, M in enumerate((8192, 8193, 8200)):
        for dt in dts:
            wide = M == 8192
            c.append(case("resid", dt, M, 64, rw=1 if M == 8192 else 2, nw=16 if wide else 4, wide=wide, p_pre=DROPS[i][0], p_post=DROPS[i][1]))
            c.append(case("image", dt, M, 260, rw=1 if M == 8192 else 2, nw=4, kmax=2))
    for dt in dts:
        c.append(case("resid", dt, 8200, 768, rw=2, nw=4, wide=True, p_pre=0.5, p_post=0.5, kmax=2))
        c.append(case("resid", dt, 8200, 2048, rw=2, nw=4, kmax=1))
        c.append(case("image", dt, 8193, 1024, rw=2, nw=4, kmax=2))
        c.append(case("resid", dt, 8193, 772, rw=2, nw=4, kmax=2, res=False))
        c.append(case("image", dt, 8193, 64, rw=2, nw=4, kmax=2, p_post=0.5))
        c.append(case("image", dt, 8200, 1028, rw=2, nw=4, kmax=2))
    # -- columns: every border of the 256-column vectors, M = 13 (three whole blocks and a row)
    for i, H in enumerate(HS):
        for dt in dts:
            pp = DROPS[i % 4]
            c.append(case("resid", dt, 13, H, p_pre=pp[0], p_post=pp[1], res=(i % 3 != 2) or pp[0] > 0))
            c.append(case("image", dt, 13, H, p_post=pp[1]))
    for dt in dts:
        c.append(case("resid", dt, 6, 96, alias=True))
        c.append(case("resid", dt, 7, 832, pad=24))
    # -- embedding
    for dt in dts:
        c += [case("embed", dt, 0, 64, B=3, T=24, p_post=0.5, carrier="word"),                          # no pos_block
              case("embed", dt, 0, 260, B=3, T=24, carrier="pos", pos_offset=2),
              case("embed", dt, 0, 768, B=4, T=3, carrier="pos"),                                      # pos_block, one block per position
              case("embed", dt, 0, 256, B=8, T=5, pos_offset=7, p_post=0.5, carrier="pos"),            # pos_block, two blocks
              case("embed", dt, 0, 1024, B=8, T=5, carrier="tt"),                                      # two blocks per position
              case("embed", dt, 0, 2048, B=4, T=3, carrier="pos", pos_offset=1),                       # non-EXT: direct atomics
              case("embed", dt, 0, 1028, B=3, T=7, carrier="word", p_post=0.5),
              case("embed", dt, 0, 64, B=8, T=1025, rw=2, carrier="pos", kmax=2),                      # two rows per wave, pos_block
              case("embed", dt, 0, 64, B=12, T=683, rw=2, carrier="word", p_post=0.5, kmax=2),         # ... without
              case("embed", dt, 0, 260, B=8, T=1025, rw=2, carrier="tt", kmax=2),
              case("embed", dt, 0, 772, B=8, T=1025, rw=2, carrier="word", kmax=2, type_vocab=1),
              case("embed", dt, 0, 1028, B=8, T=1025, rw=2, carrier="pos", kmax=2, pos_offset=3),       # two rows per wave, direct atomics
              case("embed", dt, 0, 252, B=5, T=1, pos_offset=9, carrier="pos", bwd=False),             # the decode call
              case("embed", dt, 0, 764, B=4, T=6, type_vocab=1, carrier="tt"),
              case("embed", dt, 0, 772, B=4, T=6, type_vocab=1, carrier="word", p_post=0.5),
              case("embed", dt, 0, 4, B=2, T=9, segs="none", carrier="tt"),
              case("embed", dt, 0, 2044, B=2, T=9, segs="zero", carrier="word")]
    # -- production shapes, one launch each (bf16: the type the step runs in)
    c += [case("resid", "bf16", 4096, 768, nw=16, wide=True, p_pre=0.5),
          case("embed", "bf16", 0, 768, B=16, T=256, p_post=0.5, carrier="pos"),
          case("image", "bf16", 592, 1024, p_post=0.5)]
    return c


CASES = build_cases()

# Kernel instantiations no case names, each with its reason.
EXEMPT = {}        # (none: every instantiation is reachable below 8200 x 2048 elements)
# The column reductions and locgrad: named by the check that launches them (tests/test_ln_exact_gpu.py, section "reductions").
# For these eight kernels the census is a CLAIM read off ops.py -- colsum_partials and the final stage of colsum launch the one-entry
# kernel, colsum the slab kernel in front of it, add_slabs the batched slab kernel and colsum_batched -- not an assertion: they have
# no name function, so nothing verifies the launch.
REDUCTIONS = {
    "colsum_entry_kernel": "check_colsum_partials, check_colsum (final stage)",
    "colsum_batched_kernel": "check_colsum_batch",
    "colsum_slab_kernelIf": "check_colsum f32", "colsum_slab_kernelIDF16b": "check_colsum bf16",
    "colsum_slab_batched_kernelIf": "check_add_slabs f32", "colsum_slab_batched_kernelIDF16b": "check_add_slabs bf16",
    "locgrad_kernelIf": "check_locgrad f32", "locgrad_kernelIDF16b": "check_locgrad bf16",
}


def check_census(symbols, cases=None, out=print):
    """Every ln_fwd_kernel / ln_bwd_kernel / colsum* / locgrad instantiation of the built library is named by a case of the table,
    launched by a reduction check, or exempt -- exactly one of the three -- and every kernel the table names exists."""
    cs = CASES if cases is None else cases
    named = sorted(set(c.fwd_kernel for c in cs) | set(c.bwd_kernel for c in cs if c.bwd))
    reached = set()
    for s in symbols:
        hits = [n for n in named if n in s]
        ex = [e for e in EXEMPT if e in s]
        red = [r for r in REDUCTIONS if r in s]
        assert len(hits) + len(ex) + len(red) == 1, "%s: named by %r, exempt as %r, reduction %r" % (s, hits, ex, red)
        reached.update(hits)
        users = [c for c in cs if hits and hits[0] in (c.fwd_kernel, c.bwd_kernel if c.bwd else None)]
        out("%-58s %s" % (s, ("%d case(s), e.g. %s" % (len(users), users[0].id)) if hits else
                          ("EXEMPT: " + EXEMPT[ex[0]]) if ex else "reduction: " + REDUCTIONS[red[0]]))
    assert reached == set(named), "kernels named by a case but absent from the library: %r" % sorted(set(named) - reached)
    assert set(r for r in REDUCTIONS if any(r in s for s in symbols)) == set(REDUCTIONS)


# ---------------------------------------------------------------------------------------------- small helpers
def ints(shape, lo, hi, gen, device):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=torch.device(device)).double()


def balanced_signs(M, H, gen, device):
    """[M, H] of +-1, H / 2 of each per row, drawn per row."""
    idx = torch.rand(M, H, generator=gen, device=torch.device(device)).argsort(dim=1)
    pat = torch.ones(H, dtype=torch.float64, device=idx.device)
    pat[H // 2:] = -1.0
    return torch.empty(M, H, dtype=torch.float64, device=idx.device).scatter_(1, idx, pat.expand(M, H))


def fits(x, dtype, name):
    assert bool((x.to(dtype).double() == x).all()), "%s is not representable in %s" % (name, dtype)
    return x


def units_peak(terms, dim):
    """Peak of sum |terms| over `dim`, in units of the smallest set bit of any term."""
    a = terms.abs()
    for e in range(0, 12):
        if bool(((a * 2.0 ** e) == (a * 2.0 ** e).floor()).all()):
            return float(a.sum(dim).max().item()) * 2.0 ** e
    raise AssertionError("terms are not multiples of 2^-11")


def exact_range(name, **sums):
    """Every summed quantity (value: (terms, dim)) stays where fp32 sums of it are exact in any order."""
    for tag, (terms, dim) in sums.items():
        peak = units_peak(terms, dim)
        assert peak < E.EXACT_LIMIT, "%s: %s sums reach %.0f units of their smallest bit: outside the exact range 2^24" % (name, tag, peak)


assert_bit_equal = E.assert_bit_equal          # (the sign of a zero included: see Problem.build_backward on dy at dropped columns)


def assert_written(win, name):
    """Every element of an output window was written: no canary left, no NaN."""
    v = win.view3.contiguous()
    left = int((v.view(_INT[win.dtype]) == _canary(win.dtype)).sum().item())
    nan = int(torch.isnan(v.float()).sum().item())
    assert left == 0 and nan == 0, "%s: %d element(s) of the window never written (canary left), %d NaN" % (name, left, nan)


def _canary(dtype):
    c = CANARY[dtype]
    return c if dtype != F32 or c < 2 ** 31 else c - 2 ** 32


def vec(n, dtype, device, fill, values=None):
    w = Window(1, n, dtype, device, fill)
    return w.set(values.to(dtype)) if values is not None else w


# ---------------------------------------------------------------------------------------------- one case: inputs and reference
class Problem(object):
    """Windows and float64 reference of one case.  `be.keep(n, p, site)`: the dropout factors (0 or 2) of a site, known before any
    data is drawn."""

    def __init__(self, be, c, seed=0, decoy=False):
        self.c, self.be, dev = c, be, be.device
        self.dev = dev
        gen = self.gen = generator(1000 + seed, dev)
        M, H, dt = c.M, c.H, DT[c.dtype]
        self.ld = H + c.pad
        self.wins = []                                      # (name, window): all checked for untouched surroundings
        self.decoy = decoy                                  # surroundings of the inputs hold finite garbage instead of NaN
        for p in (c.p_pre, c.p_post):
            assert p in (0.0, 0.5)
        self.kpre = be.keep(M * H, c.p_pre, SITE_PRE).view(M, H).double() if c.p_pre > 0 else torch.ones(M, H, dtype=torch.float64, device=dev)
        self.kpost = be.keep(M * H, c.p_post, SITE_POST).view(M, H).double() if c.p_post > 0 else torch.ones(M, H, dtype=torch.float64, device=dev)
        for k in (self.kpre, self.kpost):
            assert bool(((k == 0) | (k == 2) | (k == 1)).all())
        self.gamma = 2.0 ** ints((H,), -1, 1, gen, dev)
        self.beta = ints((H,), -8, 8, gen, dev)
        self.t = {}
        if c.mode == "embed":
            self._embed(gen)
        else:
            self.m = ints((M, 1), -3, 3, gen, dev)
            self.k = ints((M, 1), c.kmin, c.kmax, gen, dev)
            self.sig = balanced_signs(M, H, gen, dev)
        self.h = self.m + self.sig * 2.0 ** self.k
        if c.mode == "resid":
            self._resid(gen)
        elif c.mode == "image":
            self._image(gen)
        self.inp("gamma", 1, H, F32, self.gamma)
        self.inp("beta", 1, H, F32, self.beta)
        self.out("y", M, H, dt, ld=self.ld)
        self.out("mean", 1, M, F32)
        self.out("rstd", 1, M, F32)
        # (the sums the forward kernel forms: the row, the squared deviations)
        exact_range(c.id, row=(self.h, 1), var=((self.sig * 2.0 ** self.k) ** 2, 1))
        self.y_ref = self.kpost * (self.gamma * self.sig + self.beta)
        self.bw = None

    # -- windows
    def inp(self, name, rows, cols, dtype, values, ld=None):
        w = Window(rows, cols, dtype, self.dev, "poison", ld=ld)
        w.set(fits(values, dtype, name).to(dtype))
        if self.decoy:
            w.flat[~w.inside] = 7.0
        self.t[name] = w
        self.wins.append((name, w))
        return w

    def out(self, name, rows, cols, dtype, ld=None, init=None):
        w = Window(rows, cols, dtype, self.dev, "canary", ld=ld)
        if init is not None:
            w.set(init.to(dtype))
        self.t[name] = w
        self.wins.append((name, w))
        return w

    def v(self, name):
        w = self.t.get(name)
        if w is None:
            return None
        return w.view[0] if w.rows == 1 and name in ("gamma", "beta", "mean", "rstd", "b_loc", "mean_in", "rstd_in") else w.view

    # -- the three modes
    def _resid(self, gen):
        c, M, H, dt = self.c, self.c.M, self.c.H, DT[self.c.dtype]
        if not c.res:
            assert c.p_pre == 0
            self.inp("x", M, H, dt, self.h, ld=self.ld)
            return
        r0 = ints((M, H), -4, 4, gen, self.dev)
        res = r0 + (torch.remainder(self.h - r0, 2) == 1).double()          # kept: (h - res) / 2 an integer where h is one
        kept = self.kpre != 0
        res = torch.where(kept, res, self.h)                                 # dropped: the residual alone makes the row
        x = torch.where(kept, (self.h - res) / torch.where(kept, self.kpre, torch.ones_like(self.kpre)), ints((M, H), -3, 3, gen, self.dev))
        self.inp("x", M, H, dt, x, ld=self.ld)
        self.inp("res", M, H, dt, res, ld=self.ld + 8)

    def _image(self, gen):
        c, M, H, dt = self.c, self.c.M, self.c.H, DT[self.c.dtype]
        self.loc = ints((M, 5), 0, 2, gen, self.dev) / 2
        w, b = ints((H, 5), -2, 2, gen, self.dev), ints((H,), -2, 2, gen, self.dev)
        self.inp("loc", M, 5, F32, self.loc)
        self.inp("w_loc", H, 5, F32, w)
        self.inp("b_loc", 1, H, F32, b)
        self.inp("x", M, H, dt, self.h - (self.loc @ w.t() + b), ld=self.ld)

    def _embed(self, gen):
        """One of word / pos / tt + tt_ext carries a row-specific balanced sign pattern x 2^k, the other two a per-row integer
        constant; rows that no id / position / segment of the case names stay NaN."""
        c, dev, H = self.c, self.dev, self.c.H
        V, NX = 13, 4
        self.ids = (torch.randint(1, V - 1, (c.M,), generator=gen, device=dev))                # ids 0 and V - 1 are never named
        if c.segs == "mix":
            self.segs = torch.randint(0, 4, (c.M,), generator=gen, device=dev)
        else:
            self.segs = torch.zeros(c.M, dtype=torch.int64, device=dev)
        self.tpos = torch.arange(c.M, device=dev) % c.T + c.pos_offset
        NP = c.pos_offset + c.T
        tv = c.type_vocab
        rows = {"word": V, "pos": NP, "tt": tv + NX}                                             # tt and tt_ext as one list of rows
        tabs = {}
        for name, n in rows.items():
            if name == c.carrier:
                self.ktab = ints((n, 1), c.kmin, c.kmax, gen, dev)
                self.stab = balanced_signs(n, H, gen, dev)
                tabs[name] = self.stab * 2.0 ** self.ktab
            else:
                tabs[name] = ints((n, 1), -1, 1, gen, dev).expand(n, H).clone()
        self.idx = {"word": self.ids, "pos": self.tpos, "tt": self.segs}
        used = {}
        for name, n in rows.items():
            u = torch.zeros(n, dtype=torch.bool, device=dev)
            u[self.idx[name]] = True
            used[name] = u
            tabs[name][~u] = float("nan")
        self.used = used
        cidx = self.idx[c.carrier]
        self.sig, self.k = self.stab[cidx], self.ktab[cidx]
        self.m = sum(tabs[n][self.idx[n], :1] for n in rows if n != c.carrier)
        for name in ("word", "pos"):
            w = Window(rows[name], H, F32, dev, "poison")
            w.set(tabs[name].float())
            self.t[name] = w
            self.wins.append((name, w))
        for name, part in (("tt", tabs["tt"][:tv]), ("tt_ext", tabs["tt"][tv:])):
            w = Window(part.shape[0], H, F32, dev, "poison")
            w.set(part.float())
            self.t[name] = w
            self.wins.append((name, w))

    # -- keyword arguments of ln_fwd (mode as a string, dtype as a torch dtype: the backend translates)
    def fwd_kw(self, **over):
        c = self.c
        kw = dict(mode=c.mode, dtype=DT[c.dtype], M=c.M, H=c.H, gamma=self.v("gamma"), beta=self.v("beta"), mean=self.v("mean"),
                  rstd=self.v("rstd"), eps=EPS, y=self.v("y"), p_pre=c.p_pre, p_post=c.p_post, site_pre=SITE_PRE, site_post=SITE_POST)
        if c.mode == "resid":
            kw.update(x=self.v("x"), res=self.v("res"))
        elif c.mode == "image":
            kw.update(x=self.v("x"), loc=self.v("loc"), w_loc=self.v("w_loc"), b_loc=self.v("b_loc"))
        else:
            kw.update(ids=self.ids, segs=None if c.segs == "none" else self.segs, T=c.T, type_vocab=c.type_vocab, word=self.v("word"),
                      pos=self.v("pos"), tt=self.v("tt"), tt_ext=self.v("tt_ext"), pos_offset=c.pos_offset)
        kw.update(over)
        return kw

    def check_forward(self):
        n = self.c.id
        assert_bit_equal(self.v("mean"), self.m[:, 0], n + ": mean")
        assert_bit_equal(self.v("rstd"), 2.0 ** -self.k[:, 0], n + ": rstd (premise: sqrtf and the division correctly rounded, eps absorbed)")
        assert_written(self.t["y"], n + ": y")
        assert_bit_equal(self.v("y"), self.y_ref, n + ": y")

    # -- backward
    def build_backward(self):
        """dy such that gy = dy * keep_post * gamma is an integer vector, 0 at dropped columns, whose sums over the kept +1 and the
        kept -1 columns are u H / 4 and w H / 4 (u, w integers in [-4, 4]; the issue's a = (u + w) / 4, b = (u - w) / 4)."""
        c, dev, gen, M, H, dt = self.c, self.dev, self.gen, self.c.M, self.c.H, DT[self.c.dtype]
        u, w = ints((M, 1), -4, 4, gen, dev), ints((M, 1), -4, 4, gen, dev)
        u = torch.where((u == 0) & (w == 0), torch.ones_like(u), u)                              # (not both zero)        # c1 = (u + w) / 4, c2 = (u - w) / 4
        # (c1 + sigma * c2 is u / 2 or w / 2: with |gy| up to 245 -- still 8 bits, so dy is a bf16 number -- dh needs 9 significant
        #  bits wherever u or w is odd and |gy| >= 128, and a bf16 store has to round, half of the time at a tie)
        zmax = 240 if M <= 2100 else 12
        kept, plus = self.kpost != 0, self.sig > 0
        # sorted order of a row: kept +1 columns, kept -1 columns, dropped columns; random inside each group
        key = torch.rand(M, H, generator=gen, device=dev).double() + 2.0 * (~plus).double() + 4.0 * (~kept).double()
        order = key.argsort(dim=1)
        npl, nmi = (kept & plus).sum(1, keepdim=True), (kept & ~plus).sum(1, keepdim=True)
        j = torch.arange(H, device=dev).expand(M, H)
        grp_plus, grp_minus = j < npl, (j >= npl) & (j < npl + nmi)
        n = torch.where(grp_plus, npl, nmi).double().clamp(min=1)
        target = torch.where(grp_plus, u * (H // 4), w * (H // 4))
        target = torch.where(target.abs() <= 8 * n, target, torch.zeros_like(target))          # (few kept columns: keep the elements small)
        l = torch.where(grp_plus, j, j - npl).double()                                          # index inside the group
        base = torch.floor(target / n) + (l < torch.remainder(target, n)).double()
        v = ints((M, H), -zmax, zmax, gen, dev)
        even = (l % 2 == 0)
        vpair = torch.where(even, v, torch.roll(v, 1, dims=1))                                  # the odd member takes its partner's draw
        z = torch.where(even, vpair, -vpair) * ((l - l % 2 + 1) < n).double()                   # a last, unpaired column gets 0
        gy_sorted = (base + z) * (grp_plus | grp_minus).double()
        gy = torch.zeros(M, H, dtype=torch.float64, device=dev).scatter_(1, order, gy_sorted) + 0       # (+ 0: no -0 from the masking)
        assert bool((gy[~kept] == 0).all())
        S1, S2 = gy.sum(1, keepdim=True), (gy * self.sig).sum(1, keepdim=True)
        assert bool((torch.remainder(S1, H // 4) == 0).all()) and bool((torch.remainder(S2, H // 4) == 0).all())
        self.nonzero_c = float(((S1 != 0) | (S2 != 0)).double().mean().item())
        assert self.nonzero_c > 0.5, "%s: c1 and c2 are both zero on %.0f %% of the rows" % (c.id, 100 - 100 * self.nonzero_c)
        kp = torch.where(kept, self.kpost, torch.ones_like(self.kpost))
        # (dropped columns: any finite dy; non-negative, so that 0 * dy is +0 as in the reference and the comparison can keep
        #  the sign of a zero -- every other zero of the backward comes out of a sum, which gives +0 on both sides)
        dy = torch.where(kept, gy / (kp * self.gamma), ints((M, H), 0, 2, gen, dev))
        fits(dy, BF16, c.id + ": dy")
        c1, c2 = S1 / H, S2 / H
        dh = (gy - c1 - self.sig * c2) * 2.0 ** -self.k
        dyv = dy * self.kpost
        dx = dh * self.kpre
        r = self.ref = dict(dh=dh, dx=dx, dgamma=(dyv * self.sig).sum(0), dbeta=dyv.sum(0))
        exact_range(c.id, s1=(gy, 1), dgamma=(dyv, 0), dbias=(dx, 0), dh=(dh, 0))
        self.inp("dy", M, H, dt, dy, ld=self.ld + 16)
        self.inp("mean_in", 1, M, F32, self.m[:, 0])
        self.inp("rstd_in", 1, M, F32, 2.0 ** -self.k[:, 0])
        wide = self.be.blocks(M, H, c.mode)
        self.nblk = wide if c.wide is True else self.be.blocks(M)
        self.nvp = 4 if c.mode == "embed" else 3
        self.out("partial", self.nblk, self.nvp * H, F32)
        if c.mode == "resid":
            self.out("dres", M, H, dt, ld=self.ld + 8)
            if not c.alias:
                self.out("dx", M, H, dt, ld=self.ld + 24)
            r["vec2"] = dx.sum(0)
        elif c.mode == "image":
            self.out("dres", M, H, dt, ld=self.ld + 8)
            r["vec2"] = dh.sum(0)
        else:
            tv = c.type_vocab
            r["vec2"] = (dh * (self.segs == 0)[:, None]).sum(0)
            r["vec3"] = (dh * ((self.segs == 1) & (tv > 1))[:, None]).sum(0)
            for name, key in (("dword", "word"), ("dpos", "pos"), ("dtt_all", "tt")):
                n_rows = self.used[key].shape[0]
                init = ints((n_rows, H), -3, 3, gen, dev)
                r[name] = init.clone().index_add_(0, self.idx[key], dh)
                r[name + "_init"] = init
            self.out("dword", r["dword"].shape[0], H, F32, init=r["dword_init"])
            self.out("dpos", r["dpos"].shape[0], H, F32, init=r["dpos_init"])
            self.out("dtt", tv, H, F32, init=r["dtt_all_init"][:tv])
            self.out("dtt_ext", r["dtt_all"].shape[0] - tv, H, F32, init=r["dtt_all_init"][tv:])
        self.bw = True

    def bwd_args(self):
        c = self.c
        kw = self.fwd_kw(mean=self.v("mean_in"), rstd=self.v("rstd_in"))
        bw = dict(dy=self.v("dy"), partial=self.t["partial"].view, nblk=self.nblk if c.wide else 0)
        if c.mode == "resid":
            bw.update(dres=self.v("dres"), dx=self.v("dres") if c.alias else self.v("dx"))
        elif c.mode == "image":
            bw.update(dres=self.v("dres"))
        else:
            bw.update(dword=self.v("dword"), dpos=self.v("dpos"), dtt=self.v("dtt"), dtt_ext=self.v("dtt_ext"))
        return kw, bw

    def check_backward(self):
        """The row outputs, the partial slabs (all written; their float64 block sum is the reference) and the atomic-fed tables
        (rows 0 / 1 of dtt still lack the slab sums: reduce_and_check adds them)."""
        c, r, n, H = self.c, self.ref, self.c.id, self.c.H
        if c.mode != "embed":
            assert_written(self.t["dres"], n + ": dres")
            assert_bit_equal(self.v("dres"), r["dh"], n + ": dres")
        if c.mode == "resid":
            if not c.alias:
                assert_written(self.t["dx"], n + ": dx")
                assert_bit_equal(self.v("dx"), r["dx"], n + ": dx")
        assert_written(self.t["partial"], n + ": partial")
        part = self.t["partial"].view.double().sum(0).view(self.nvp, H)
        for i, key in enumerate(("dgamma", "dbeta", "vec2", "vec3")[:self.nvp]):
            assert_bit_equal(part[i].float(), r[key], "%s: partial slabs, vector %d (%s)" % (n, i, key))
        if c.mode == "embed":
            assert_bit_equal(self.v("dword"), r["dword"], n + ": dword")
            assert_bit_equal(self.v("dpos"), r["dpos"], n + ": dpos")

    def reduce_and_check(self):
        """The column reductions as the engine issues them: colsum_partials for [nblk][3][H], one ColsumBatch flush (stride 4H, the
        [3H:] view) for the embedding."""
        c, r, n, H, be, dev = self.c, self.ref, self.c.id, self.c.H, self.be, self.dev
        part = self.t["partial"].view
        g = generator(5, dev)
        if c.mode != "embed":
            o0, o1 = vec(H, F32, dev, "canary"), vec(H, F32, dev, "canary")
            init = ints((H,), -3, 3, g, dev)
            o2 = vec(H, F32, dev, "canary", init)
            be.colsum_partials(part, self.nblk, 2, H, o0.vector(), o1.vector(), None, False)
            be.colsum_partials(part[:, 2 * H:], self.nblk, 1, H, o2.vector(), None, None, True)
            assert_bit_equal(o0.vector(), r["dgamma"], n + ": dgamma")
            assert_bit_equal(o1.vector(), r["dbeta"], n + ": dbeta")
            assert_bit_equal(o2.vector(), init + r["vec2"], n + ": dbias / db_loc (accumulated)")
            for tag, w in (("dgamma", o0), ("dbeta", o1), ("dbias", o2)):
                w.assert_surroundings_untouched(n + ": " + tag)
            return
        tv = c.type_vocab
        o0, o1 = vec(H, F32, dev, "canary"), vec(H, F32, dev, "canary")
        dtt = self.v("dtt")
        b = be.batch()
        flat = part.reshape(-1)
        assert flat.data_ptr() == part.data_ptr()
        b.add(flat, (o0.vector(), o1.vector(), dtt[0]), self.nblk, 4 * H, H, 3, (False, False, True))
        if tv > 1:
            b.add(flat[3 * H:], (dtt[1], None, None), self.nblk, 4 * H, H, 1, (True, False, False))
        b.flush()
        assert_bit_equal(o0.vector(), r["dgamma"], n + ": dgamma")
        assert_bit_equal(o1.vector(), r["dbeta"], n + ": dbeta")
        assert_bit_equal(dtt, r["dtt_all"][:tv], n + ": dtt")
        assert_bit_equal(self.v("dtt_ext"), r["dtt_all"][tv:], n + ": dtt_ext")
        o0.assert_surroundings_untouched(n + ": dgamma")
        o1.assert_surroundings_untouched(n + ": dbeta")

    def assert_surroundings(self):
        for name, w in self.wins:
            if not (self.decoy and w.fill == "poison"):
                w.assert_surroundings_untouched("%s: %s" % (self.c.id, name))

    def outputs(self):
        names = ("y", "mean", "rstd", "dres", "dx", "partial", "dword", "dpos", "dtt", "dtt_ext")
        return dict((k, self.t[k].view3.clone()) for k in names if k in self.t)


def run_case(be, c, seed=0, decoy=False, checks=True):
    """Forward, its checks, backward, its checks, the reductions, the surroundings of every window.  Returns the Problem."""
    p = Problem(be, c, seed, decoy=decoy)
    be.ln_fwd(p.fwd_kw(), expect=c.fwd_kernel)
    if checks:
        p.check_forward()
    if c.bwd:
        p.build_backward()
        kw, bw = p.bwd_args()
        be.ln_bwd(kw, bw, expect=c.bwd_kernel)
        if checks:
            p.check_backward()
            p.reduce_and_check()
    p.assert_surroundings()
    return p


def assert_same(a, b, name):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k].view(_INT.get(a[k].dtype, a[k].dtype)), b[k].view(_INT.get(b[k].dtype, b[k].dtype))), "%s: %s differs" % (name, k)


# ---------------------------------------------------------------------------------------------- invariances
def check_surroundings_do_not_matter(be, c, seed=0):
    """Rows >= M and the pad columns of every input: NaN or finite garbage, the outputs are the same bits."""
    a = run_case(be, c, seed).outputs()
    b = run_case(be, c, seed, decoy=True, checks=False).outputs()
    b.pop("dtt", None), a.pop("dtt", None)                  # (rows 0 / 1 of dtt: only the checked run added the slab sums)
    assert_same(a, b, c.id + ": NaN against finite surroundings")


def check_reproducible(be, c, seed=0):
    """Two runs of the same case: the atomic-fed tables (and everything else) bit for bit."""
    assert_same(run_case(be, c, seed).outputs(), run_case(be, c, seed).outputs(), c.id + ": run to run")


def check_segs_none_equals_zeros(be, c, seed=0):
    assert c.mode == "embed" and c.segs == "zero"
    a = run_case(be, c, seed).outputs()
    b = run_case(be, c._replace(segs="none"), seed).outputs()
    assert_same(a, b, c.id + ": segs None against all-zero segs")


def check_alias(be, c, seed=0):
    """dx aliased to dres at p_pre = 0 against separate buffers."""
    assert c.mode == "resid" and c.p_pre == 0 and not c.alias
    a = run_case(be, c, seed).outputs()
    b = run_case(be, c._replace(alias=True), seed).outputs()
    assert torch.equal(a["dx"], a["dres"])
    a.pop("dx")
    assert_same(a, b, c.id + ": dx aliased to dres")


def check_batch_permutation(be, c, seed=0):
    """Embedding input with its batch rows permuted (no dropout: the draws follow the row index): row outputs permuted back are
    the same bits, the table gradients and column sums unchanged."""
    assert c.mode == "embed" and c.p_post == 0
    p = run_case(be, c, seed)
    a = p.outputs()
    perm = torch.randperm(c.B, generator=generator(seed, "cpu")).to(be.device)
    rows = (perm[:, None] * c.T + torch.arange(c.T, device=be.device)[None]).reshape(-1)
    q = Problem(be, c, seed)
    q.build_backward()
    q.ids, q.segs = q.ids[rows].contiguous(), q.segs[rows].contiguous()
    q.t["dy"].view.copy_(p.t["dy"].view[rows])
    q.t["mean_in"].view[0].copy_(p.t["mean_in"].view[0][rows])
    q.t["rstd_in"].view[0].copy_(p.t["rstd_in"].view[0][rows])
    be.ln_fwd(q.fwd_kw(), expect=c.fwd_kernel)
    kw, bw = q.bwd_args()
    be.ln_bwd(kw, bw, expect=c.bwd_kernel)
    q.ref = p.ref
    q.reduce_and_check()
    b = q.outputs()
    for k in ("y", "mean", "rstd"):
        full = a[k].reshape(c.M, -1) if k == "y" else a[k].reshape(c.M, 1)
        assert torch.equal(full[rows].reshape(b[k].shape), b[k]), "%s: %s of the permuted batch" % (c.id, k)
    for k in ("dword", "dpos", "dtt", "dtt_ext"):
        assert torch.equal(a[k], b[k]), "%s: %s changed under a permutation of the batch" % (c.id, k)
    assert torch.equal(a["partial"].double().sum(1), b["partial"].double().sum(1))
    q.assert_surroundings()


# ---------------------------------------------------------------------------------------------- the column reductions
def check_colsum_partials(be, nblk, nvec, H, accumulate, none_out=False, seed=0):
    """out_j[c] (+)= sum_b partial[b][j][c] over a [nblk][3][H] scratch; vectors >= nvec of the scratch are NaN."""
    dev, g = be.device, generator(seed, be.device)
    name = "colsum_partials nblk %d nvec %d H %d acc %d" % (nblk, nvec, H, accumulate)
    src = Window(nblk, 3 * H, F32, dev, "poison")
    vals = ints((nblk, 3 * H), -9, 9, g, dev)
    vals[:, nvec * H:] = float("nan")
    src.set(vals.float())
    exact_range(name, partial=(vals[:, :nvec * H], 0))
    outs, want = [], []
    for j in range(3):
        init = ints((H,), -5, 5, g, dev)
        if j >= nvec or (none_out and j == 1):
            outs.append(None), want.append(None)
            continue
        outs.append(vec(H, F32, dev, "canary", init if accumulate else None))
        want.append(vals[:, j * H:(j + 1) * H].sum(0) + (init if accumulate else 0))
    be.colsum_partials(src.view, nblk, nvec, H, *[o.vector() if o is not None else None for o in outs], accumulate)
    for j, (o, w) in enumerate(zip(outs, want)):
        if o is not None:
            assert_bit_equal(o.vector(), w, "%s: out%d" % (name, j))
            o.assert_surroundings_untouched("%s: out%d" % (name, j))
    src.assert_surroundings_untouched(name + ": partial")


def check_colsum_batch(be, seed=0):
    """ONE ColsumBatch flush: entries of nblk 1, 4, 28, 29, 32, 33 and 61 (the 32-way unrolled loop, its tail, neither), strides
    3H and 4H, nvec 1 and 3, a None output, the [3H:] view of a 4H-strided scratch; then the shared-output re-flush: an entry that
    names an output already queued flushes first, and its sum lands on top."""
    dev, g = be.device, generator(seed, be.device)
    b = be.batch()
    todo, wins = [], []
    spec = [(1, 3, 64, 3), (4, 4, 260, 3), (28, 3, 4, 1), (29, 4, 768, 3), (32, 3, 252, 3), (33, 4, 64, 1), (61, 4, 1024, 3)]
    for i, (nblk, sv, H, nvec) in enumerate(spec):
        stride = sv * H
        src = Window(nblk, stride, F32, dev, "poison")
        vals = ints((nblk, stride), -9, 9, g, dev)
        off = 3 * H if (sv == 4 and nvec == 1) else 0                   # the [3H:] view the embedding uses
        exact_range("ColsumBatch entry %d" % i, partial=(vals, 0))
        src.set(vals.float())
        wins.append(("partial %d" % i, src))
        outs, accs, exp = [], [], []
        for j in range(3):
            if j >= nvec or (i == 3 and j == 1):
                outs.append(None), accs.append(False)
                continue
            acc = (i + j) % 2 == 1
            init = ints((H,), -5, 5, g, dev)
            o = vec(H, F32, dev, "canary", init if acc else None)
            wins.append(("out %d.%d" % (i, j), o))
            outs.append(o.vector()), accs.append(acc)
            todo.append((o, vals[:, off + j * H:off + (j + 1) * H].sum(0) + (init if acc else 0), "entry %d (nblk %d, stride %dH, nvec %d) out%d" % (i, nblk, sv, nvec, j)))
        b.add(src.view.reshape(-1)[off:], tuple(outs), nblk, stride, H, nvec, tuple(accs))
    b.flush()
    for o, want, tag in todo:
        assert_bit_equal(o.vector(), want, "ColsumBatch: " + tag)
    # shared output: two entries accumulate into one vector; the second add() must flush the first
    H = 260
    s1, s2 = ints((5, 3 * H), -9, 9, g, dev), ints((33, 3 * H), -9, 9, g, dev)
    exact_range("ColsumBatch shared output", partial=(torch.cat([s1, s2]), 0))
    w1, w2 = Window(5, 3 * H, F32, dev, "poison").set(s1.float()), Window(33, 3 * H, F32, dev, "poison").set(s2.float())
    o = vec(H, F32, dev, "canary")
    b.add(w1.view.reshape(-1), (o.vector(), None, None), 5, 3 * H, H, 1, (False, False, False))
    b.add(w2.view.reshape(-1), (o.vector(), None, None), 33, 3 * H, H, 1, (True, False, False))
    b.flush()
    assert_bit_equal(o.vector(), s1[:, :H].sum(0) + s2[:, :H].sum(0), "ColsumBatch: shared output, second entry on top of the first")
    for tag, w in wins + [("shared out", o), ("shared 1", w1), ("shared 2", w2)]:
        w.assert_surroundings_untouched("ColsumBatch: " + tag)


COLSUM_M, COLSUM_N = (1, 63, 64, 65, 333), (4, 252, 256, 260, 2304)


def _matrix(be, dtype, M, N, g, pad):
    x = ints((M, N), -6, 6, g, be.device)
    exact_range("%s matrix %dx%d" % (dtype, M, N), columns=(x, 0))
    return x, Window(M, N, DT[dtype], be.device, "poison", ld=N + pad).set(x.to(DT[dtype]))


def check_colsum(be, dtype, M, N, accumulate, seed=0):
    """colsum (slab stage + final stage) and colsum_slabs alone, ld > N, the scratch a canary window that must be fully written."""
    dev, g = be.device, generator(seed, be.device)
    name = "colsum %s %dx%d acc %d" % (dtype, M, N, accumulate)
    x, xw = _matrix(be, dtype, M, N, g, 8)
    nslab = (M + 63) // 64
    init = ints((N,), -5, 5, g, dev)
    out = vec(N, F32, dev, "canary", init if accumulate else None)
    scratch = Window(nslab, N, F32, dev, "canary")
    be.colsum(xw.view, M, N, out.vector(), scratch.view, accumulate)
    assert_bit_equal(out.vector(), x.sum(0) + (init if accumulate else 0), name)
    slabs = torch.stack([x[s * 64:(s + 1) * 64].sum(0) for s in range(nslab)])
    assert_written(scratch, name + ": scratch")
    assert_bit_equal(scratch.view, slabs, name + ": slab scratch")
    s2 = Window(nslab, N, F32, dev, "canary")
    be.colsum_slabs(xw.view, M, N, s2.view)
    assert_bit_equal(s2.view, slabs, name + ": colsum_slabs")
    for tag, w in (("x", xw), ("out", out), ("scratch", scratch), ("scratch of colsum_slabs", s2)):
        w.assert_surroundings_untouched(name + ": " + tag)


def check_add_slabs(be, dtype, shapes, seed=0):
    """ColsumBatch.add_slabs: entries of different M and N in ONE batched slab launch and one batched final reduction."""
    dev, g = be.device, generator(seed, be.device)
    b = be.batch()
    todo = []
    for i, (M, N) in enumerate(shapes):
        x, xw = _matrix(be, dtype, M, N, g, 8 * (i + 1))
        nslab = (M + 63) // 64
        acc = i % 2 == 1
        init = ints((N,), -5, 5, g, dev)
        out = vec(N, F32, dev, "canary", init if acc else None)
        scratch = Window(nslab, N, F32, dev, "canary")
        b.add_slabs(xw.view, M, N, scratch.view, out.vector(), acc)
        todo.append((x, xw, out, scratch, init if acc else 0, "add_slabs %s entry %d (%dx%d)" % (dtype, i, M, N)))
    b.flush()
    for x, xw, out, scratch, init, name in todo:
        assert_bit_equal(out.vector(), x.sum(0) + init, name)
        assert_written(scratch, name + ": scratch")
        for tag, w in (("x", xw), ("out", out), ("scratch", scratch)):
            w.assert_surroundings_untouched(name + ": " + tag)


def check_locgrad(be, dtype, M, H, accumulate, seed=0):
    """dW_loc[h][j] (+)= sum_m dh[m][h] loc[m][j]: 16 row slices, atomics; exact sums, the same bits on a second run."""
    dev, g = be.device, generator(seed, be.device)
    name = "locgrad %s %dx%d acc %d" % (dtype, M, H, accumulate)
    dh, dw_ = _matrix(be, dtype, M, H, g, 8)
    loc = ints((M, 5), 0, 2, g, dev) / 2
    exact_range(name, dw=(dh.abs().t() @ loc, 1))              # (a single term per entry: the peak of sum |dh| loc itself)
    lw = Window(M, 5, F32, dev, "poison").set(loc.float())
    init = ints((H, 5), -5, 5, g, dev)
    got = []
    for _ in range(2):
        out = Window(H, 5, F32, dev, "canary")
        if accumulate:
            out.set(init.float())
        be.locgrad(dw_.view, lw.view, M, H, out.view, accumulate)
        assert_bit_equal(out.view, dh.t() @ loc + (init if accumulate else 0), name)
        out.assert_surroundings_untouched(name + ": dW_loc")
        got.append(out.view.clone())
    assert torch.equal(got[0], got[1]), name + ": not reproducible"
    dw_.assert_surroundings_untouched(name + ": dh")
    lw.assert_surroundings_untouched(name + ": loc")


def autograd_reference(p):
    """float64 autograd of LN WITHOUT eps over the problem's h and dy: (y, dh, dgamma, dbeta) -- what Problem's closed forms
    (y_ref, ref) must equal exactly (tests/test_exact_ln_harness_cpu.py)."""
    h = p.h.clone().requires_grad_(True)
    g, b = p.gamma.clone().requires_grad_(True), p.beta.clone().requires_grad_(True)
    u = h.mean(-1, keepdim=True)
    s = (h - u).pow(2).mean(-1, keepdim=True)
    y = (g * ((h - u) / torch.sqrt(s)) + b) * p.kpost
    y.backward(p.t["dy"].view.double())
    return y.detach(), h.grad, g.grad, b.grad


def lib_path():
    return E.lib_path()
