"""Exact layer of the loss and optimizer tests: csrc/loss.hip -- cross entropy forward, backward and per-row
backward, answer_scores -- csrc/elementwise.hip -- the casts, vl_split -- and csrc/optim.hip -- the three AdamW entries -- on inputs whose answer is known bit for bit.

Cross entropy, pointer rows.  A row has ONE hot column j holding an integer L in [-8, 8]; every other column holds L - 112 - 8k
(k in 0..15 drawn per column; k in 0..1 where L is odd, so that every value keeps within the 8 bits of bf16) or -inf.  exp(-112)
is below half the smallest fp32 denormal, so every cold term is exactly 0 in any denormal mode: s == 1, lse == L, row_loss is 0
(label == j) or the integer L - x[label], stats[0] an integer sum, stats[2] a quotient by a power of two; the gradient of a kept
row is +gs at j, -gs at the label, 0 elsewhere, gs a power of two.  Premises only the hardware can confirm -- __expf(0) == 1,
logf(1) == 0, __expf(x) == 0 for x <= -112 -- have a probe each (premise_*), and no case is skipped on them.
Hot column and label sit on the borders of both loops of the kernels (the 4-element vectors, the 1024-column stride, the scalar
tail at V & ~3).  Noise rows (Gaussian, offset +60, scaled by 20) are judged against float64 log_softmax of the stored values
under the tolerances of tests/test_ops_gpu.py, unchanged.

AdamW.  beta1 = 0.5, beta2 = 0.75, t = 1 (bias correction exactly 1), eps = 2^-4, g * gscale = +-3/16, v = 9/256 (a fixed point:
sqrt 3/16, + eps = 1/4), m a multiple of 3/16, p a multiple of 1/8, lr = 2^-(2..6), wd in {0, 1/2, 1/4, 1/8}: every fp32
operation of the kernel is exact, so the float64 reference is the answer to the last bit; exact_f32() refuses a case one of
whose intermediate values leaves 24 bits.  The reference takes the per-element lr / wd from numpy.searchsorted on the segment
ends -- not from a port of the kernel's lookup.  Premises with a probe each: v_sqrt_f32 exact on 9 * 4^j, v_rcp_f32 exact on
powers of two, powf(b, 1) == b.

Every output is a window inside a canary-filled allocation, every input a window inside a NaN-poisoned one (exact_gemm.Window),
leading dimensions are padded and differ (ldl != ldd), every launch is repeated and must return the same bits.

Plain helper module: no fixtures, no hooks; every check takes a backend `be` (be.device, be.ce_fwd, be.ce_bwd, be.ce_bwd_rows,
be.answer_scores, be.cast, be.cast_ranges, be.vl_split, be.drop_mask, be.adamw, be.adamw_blocks), so
tests/test_exact_loss_harness_cpu.py proves it on the CPU against a stand-in written in torch and tests/test_loss_exact_gpu.py
runs it on the HIP kernels.
"""
import collections

import numpy as np
import torch

import exact_gemm as E
from exact_gemm import BF16, CANARY, F32, Window, generator

I64 = torch.int64
DT = {"bf16": BF16, "f32": F32}
_INT = {BF16: torch.int16, F32: torch.int32, I64: torch.int64}
NEG = -float("inf")


def tol(dtype):
    """tests/test_ops_gpu.py::tol, unchanged."""
    return 2e-5 if dtype == F32 else 1.2e-2


def bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _canary(dtype):
    c = CANARY[dtype]
    return c - 2 ** 32 if dtype == F32 and c >= 2 ** 31 else c


def assert_same_bits(a, b, name):
    assert a.shape == b.shape and a.dtype == b.dtype, name
    bad = bits(a) != bits(b)
    n = int(bad.sum().item())
    if n:
        i = tuple(int(x) for x in torch.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements differ bit for bit; first at %r: %r against %r" % (name, n, bad.numel(), i, a[i].item(), b[i].item()))


def assert_equal_values(got, want, name):
    """Equal BY VALUE (+0 == -0), no NaN anywhere; `want`: float64, compared through its round-to-nearest-even image."""
    w = want.float().to(got.dtype).double().reshape(got.shape)
    g = got.double()
    bad = ~(g == w)
    n = int(bad.sum().item())
    if n:
        idx = [tuple(int(x) for x in i) for i in torch.nonzero(bad)[:6]]
        raise AssertionError("%s: %d of %d elements differ from the exact reference (%d NaN); %s" % (
            name, n, bad.numel(), int(torch.isnan(g).sum().item()), "; ".join("%r: got %r want %r" % (i, g[i].item(), w[i].item()) for i in idx)))


def fits(x, dtype, name):
    ok = (x.to(dtype).double() == x) | torch.isnan(x)
    assert bool(ok.all()), "%s is not representable in %s" % (name, dtype)
    return x


def win_in(values, dtype, dev, pad=0, decoy=None):
    """A [rows, cols] float64 / int64 tensor as a window of `dtype` inside a poisoned allocation (integers: canary -- there is no
    integer NaN), ld = cols + pad.  decoy: finite garbage instead of NaN around it."""
    values = values.reshape(1, -1) if values.dim() == 1 else values
    rows, cols = values.shape
    w = Window(rows, cols, dtype, dev, "canary" if dtype == I64 else "poison", ld=cols + pad)
    if dtype != I64:
        fits(values.double(), dtype, "an input")
    w.set(values.to(dtype))
    if decoy is not None:
        w.flat[~w.inside] = decoy
        w.decoy = True
    return w


def win_out(rows, cols, dtype, dev, pad=0):
    return Window(rows, cols, dtype, dev, "canary", ld=cols + pad)


def surroundings(wins, name):
    for tag, w in wins:
        if w is not None and not getattr(w, "decoy", False):
            w.assert_surroundings_untouched("%s: %s" % (name, tag))


def vec(w):
    return w.view[0]


# ============================================================================================== cross entropy: pointer rows
CE_V = (1, 2, 3, 4, 5, 37, 1023, 1024, 1025, 1030, 2049, 30522)
GSCALES = (1.0, 0.5, -2.0)
OOR = (-5, 0, 3)                        # out-of-range labels: -5, V + 0, V + 3
# (M, one letter per row: k a kept row, i an ignored row, o a row whose label is out of range and not ignore_index); rows that
# count (k and o) are a power of two in number, so that gscale / count is one -- or none at all: stats[2] is then NaN, every row zero
PLANS = ((1, "k"), (5, "kikok"), (8, "kkkkkkko"), (1, "i"), (5, "kkikk"), (8, "kikoikii"))
PLANS_BIG = ((2, "kk"), (2, "ki"), (2, "ko"), (2, "kk"), (2, "ii"), (2, "ko"), (2, "ko"))


def border_columns(V):
    """Columns on the borders of the kernels' loops: the first vectors, both sides of the 1024-column stride, the last vector
    (V4 - 1), the start of the scalar tail (V4) and the last two columns."""
    V4 = V & ~3
    c = [0, 3, 4] + list(range(1019, 1029)) + [V4 - 1, V4, V - 1, V - 2]
    return sorted(set(x for x in c if 0 <= x < V))


def border_pairs(V):
    """(hot column, label): the same column, and neighbouring borders both ways round -- the same 4-vector (1020, 1021),
    neighbouring vectors (3, 4), across the stride (1023, 1024), vector loop against tail (V4 - 1, V4)."""
    b = border_columns(V)
    p = [(x, x) for x in b]
    for x, y in zip(b, b[1:]):
        p += [(x, y), (y, x)]
    return p


_CeCase = collections.namedtuple("CeCase", "dtype V M plan pairs ignore gscale mean seed oor")


class CeCase(_CeCase):
    __slots__ = ()

    """oor: which of OOR the first 'o' row of the plan takes (dealt in turn over the cases of one V and type that have one)."""

    def oor_labels(self):
        return [OOR[(i + self.oor) % 3] if OOR[(i + self.oor) % 3] < 0 else self.V + OOR[(i + self.oor) % 3] for i in range(self.plan.count("o"))]

    @property
    def id(self):
        s = "ce-%s-v%d-m%d-%s-ig%d-gs%g%s-%s" % (self.dtype, self.V, self.M, self.plan, self.ignore, self.gscale, "" if self.mean else "-sum",
                                                ".".join("%d_%d" % p for p in self.pairs))
        return s + "".join("-o%d" % l for l in self.oor_labels())


def build_ce_cases():
    cases = []
    for V in CE_V:
        for dtype in ("f32", "bf16"):
            queue, chunk, noor = border_pairs(V), 0, 0
            plans = PLANS_BIG if V > 4096 else PLANS
            while queue:
                ig = (0, -1)[chunk % 2]
                if all(lab == ig for _, lab in queue):
                    ig = -1
                M, plan = plans[chunk % len(plans)]
                valid = [p for p in border_pairs(V) if p[1] != ig]
                take = []
                for _ in range(plan.count("k")):
                    nxt = [p for p in queue if p[1] != ig]
                    if nxt:
                        queue.remove(nxt[0])
                        take.append(nxt[0])
                    else:
                        take.append(valid[(len(take) * 5 + chunk) % len(valid)])
                cases.append(CeCase(dtype, V, M, plan, tuple(take), ig, GSCALES[chunk % 3], chunk % 4 != 3, len(cases), noor % 3))
                noor += "o" in plan
                chunk += 1
    return cases


CE_CASES = build_ce_cases()


def pointer_rows(M, V, hot, avoid, gen, dev):
    """[M, V] float64 pointer rows and their L; `hot[m]`: the hot column; `avoid[m]`: columns that must stay finite."""
    L = torch.randint(-8, 9, (M, 1), generator=gen, device=dev).double()
    k = torch.randint(0, 16, (M, V), generator=gen, device=dev).double()
    k = torch.where(torch.remainder(L, 2) == 1, torch.remainder(k, 2), k)
    x = L - 112 - 8 * k
    inf = torch.rand(M, V, generator=gen, device=dev) < 0.125
    for m in range(M):
        for c in avoid[m]:
            if 0 <= c < V:
                inf[m, c] = False
    x = torch.where(inf, torch.full_like(x, NEG), x)
    for m in range(M):
        x[m, hot[m]] = L[m, 0]
    return x, L[:, 0]


class CeProblem(object):
    """Windows and exact expectations of one pointer case."""

    def __init__(self, be, c):
        self.c, self.be, dev = c, be, be.device
        self.dev, self.dt = dev, DT[c.dtype]
        gen = generator(7000 + c.seed, dev)
        M, V = c.M, c.V
        b = border_columns(V)
        hot, lab, kept = [], [], []
        it, no = iter(c.pairs), 0
        for m, kind in enumerate(c.plan):
            if kind == "k":
                j, l = next(it)
            elif kind == "i":
                j, l = b[(m + c.seed) % len(b)], c.ignore
            else:
                o = OOR[(no + c.oor) % 3]
                j, l = b[(m + c.seed) % len(b)], (o if o < 0 else V + o)
                no += 1
            hot.append(j), lab.append(l), kept.append(kind == "k")
        x, L = pointer_rows(M, V, hot, [(l,) for l in lab], gen, dev)
        self.x, self.L, self.hot, self.lab, self.kept = x, L, hot, lab, kept
        self.V4 = -(-V // 4) * 4
        self.ldl, self.ldd = self.V4 + 4, self.V4 + 8
        self.logits = win_in(x, self.dt, dev, pad=self.ldl - V)
        self.labels = win_in(torch.tensor(lab, dtype=I64, device=dev), I64, dev)
        self.gs = win_in(torch.tensor([c.gscale], dtype=torch.float64, device=dev), F32, dev)
        self.count = sum(1 for l in lab if l != c.ignore)
        loss = [float(L[m] - x[m, lab[m]]) if kept[m] else 0.0 for m in range(M)]
        self.loss = torch.tensor(loss, dtype=torch.float64, device=dev)
        assert bool(torch.isfinite(self.loss).all()) and bool((self.loss == self.loss.round()).all())
        assert self.count & (self.count - 1) == 0
        gsv = c.gscale / self.count if c.mean and self.count else float("nan") if c.mean else c.gscale      # (no counted row: nothing reads it)
        d = torch.zeros(M, self.ldd, dtype=torch.float64, device=dev)
        for m in range(M):
            if kept[m]:
                d[m, hot[m]] += gsv
                d[m, lab[m]] -= gsv
        self.gsv, self.dl_ref = gsv, d

    def outputs(self):
        dev, M = self.dev, self.c.M
        return win_out(1, M, F32, dev), win_out(1, M, F32, dev), win_out(1, 3, F32, dev)

    def forward(self, name):
        c, be = self.c, self.be
        rl, lse, st = self.outputs()
        be.ce_fwd(self.logits.view, vec(self.labels), c.M, c.V, vec(rl), vec(lse), vec(st), c.ignore)
        E.assert_bit_equal(vec(lse), self.L, name + ": lse == L (premises: __expf(0) == 1, __expf(<= -112) == 0, logf(1) == 0)")
        E.assert_bit_equal(vec(rl), self.loss, name + ": row_loss")
        s = self.loss.sum()
        if self.count:
            want = torch.stack([s, torch.tensor(float(self.count), dtype=torch.float64, device=self.dev), (s.float() / float(self.count)).double()])
            E.assert_bit_equal(vec(st), want, name + ": stats (sum, count, quotient)")
        else:
            E.assert_bit_equal(vec(st)[:2], torch.stack([s, torch.zeros_like(s)]), name + ": stats (sum, count)")
            assert bool(torch.isnan(vec(st)[2])), name + ": stats[2] of a batch without a counted row is NaN"
        surroundings((("row_loss", rl), ("lse", lse), ("stats", st)), name)
        return rl, lse, st

    def backward(self, lse, st, name):
        c, be = self.c, self.be
        dl = win_out(c.M, self.ldd, self.dt, self.dev)
        be.ce_bwd(self.logits.view, vec(self.labels), vec(lse), vec(st), vec(self.gs), c.mean, c.M, c.V, dl.view, c.ignore)
        assert_equal_values(dl.view, self.dl_ref, name + ": dlogits (columns V..ldd zero, ignored and out-of-range rows zero)")
        surroundings((("dlogits", dl),), name)
        return dl

    def backward_rows(self, lse, name, g=None):
        c, be = self.c, self.be
        gv = torch.full((c.M,), self.gsv, dtype=torch.float64, device=self.dev) if g is None else g
        gw = win_in(gv, F32, self.dev)
        dl = win_out(c.M, self.ldd, self.dt, self.dev)
        be.ce_bwd_rows(self.logits.view, vec(self.labels), vec(lse), vec(gw), c.M, c.V, dl.view, c.ignore)
        surroundings((("dlogits of ce_bwd_rows", dl), ("g", gw)), name)
        return dl

    def inputs_untouched(self, name):
        surroundings((("logits", self.logits), ("labels", self.labels), ("gscale", self.gs)), name)
        fits(self.x, self.dt, "x")
        assert torch.equal(self.logits.view.double(), self.x), name + ": the logits were written"


def run_ce_case(be, c):
    """Forward, backward and the per-row backward with g = gscale / count, each launched twice."""
    p = CeProblem(be, c)
    n = c.id
    rl, lse, st = p.forward(n)
    rl2, lse2, st2 = p.forward(n + " (repeated)")
    for tag, a, b in (("row_loss", rl, rl2), ("lse", lse, lse2), ("stats", st, st2)):
        assert_same_bits(a.view, b.view, "%s: %s of the repeated launch" % (n, tag))
    dl = p.backward(lse, st, n)
    dl2 = p.backward(lse, st, n + " (repeated)")
    assert_same_bits(dl.view, dl2.view, n + ": dlogits of the repeated launch")
    dr = p.backward_rows(lse, n)
    assert_same_bits(dr.view, dl.view, n + ": ce_bwd_rows with g = gscale / count against ce_bwd")
    p.inputs_untouched(n)
    return p


# ---------------------------------------------------------------------------------------------- the per-row backward
ROWS_V = (5, 1030, 2049)


def check_ce_bwd_rows(be, dtype, V):
    """g[m] = +-2^k; row 2 has g == 0, row 4 is ignored with g != 0, row 6 has g == 0 AND holds a +inf logit (lse +inf): stored
    as zeros, never multiplied."""
    dev, dt, M = be.device, DT[dtype], 8
    name = "ce_bwd_rows-%s-v%d" % (dtype, V)
    gen = generator(7900 + V, dev)
    b = border_columns(V)
    hot = [b[(3 * m) % len(b)] for m in range(M)]
    lab = [b[(3 * m + (m % 3)) % len(b)] for m in range(M)]
    ignore = -1
    lab[4] = ignore
    x, L = pointer_rows(M, V, hot, [(l,) for l in lab], gen, dev)
    x[6, (hot[6] + 1) % V] = float("inf")
    lse_v = L.clone()
    lse_v[6] = float("inf")
    g = torch.tensor([1.0, -0.5, 0.0, 4.0, 2.0, -0.125, 0.0, 0.25], dtype=torch.float64, device=dev)
    V4 = -(-V // 4) * 4
    ldl, ldd = V4 + 8, V4 + 4
    logits, labels, lse, gw = win_in(x, dt, dev, pad=ldl - V), win_in(torch.tensor(lab, dtype=I64, device=dev), I64, dev), win_in(lse_v, F32, dev), win_in(g, F32, dev)
    ref = torch.zeros(M, ldd, dtype=torch.float64, device=dev)
    for m in range(M):
        if lab[m] != ignore and g[m] != 0:
            ref[m, hot[m]] += g[m]
            ref[m, lab[m]] -= g[m]
    got = []
    for rep in range(2):
        dl = win_out(M, ldd, dt, dev)
        be.ce_bwd_rows(logits.view, vec(labels), vec(lse), vec(gw), M, V, dl.view, ignore)
        assert_equal_values(dl.view, ref, name + ": dlogits (rows 2 and 6: g == 0, row 4: ignored, row 6: a +inf logit)")
        surroundings((("dlogits", dl),), name)
        got.append(dl.view.clone())
    assert_same_bits(got[0], got[1], name + ": repeated launch")
    surroundings((("logits", logits), ("labels", labels), ("lse", lse), ("g", gw)), name)


# ---------------------------------------------------------------------------------------------- premises
def _expf_probe(be, xs):
    """__expf(x) for each x: ce_bwd_rows with lse = 0, g = 1 and the label on another column writes exp(x - 0) - 0."""
    dev = be.device
    V = len(xs) + 1
    x = torch.tensor([list(xs) + [0.0]], dtype=torch.float64, device=dev)
    logits, labels = win_in(x, F32, dev, pad=(-V) % 4 + 4), win_in(torch.tensor([V - 1], dtype=I64, device=dev), I64, dev)
    lse, g = win_in(torch.zeros(1, dtype=torch.float64, device=dev), F32, dev), win_in(torch.ones(1, dtype=torch.float64, device=dev), F32, dev)
    ldd = -(-V // 4) * 4
    dl = win_out(1, ldd, F32, dev)
    be.ce_bwd_rows(logits.view, vec(labels), vec(lse), vec(g), 1, V, dl.view, -1)
    dl.assert_surroundings_untouched("expf probe")
    return dl.view[0, :len(xs)].clone()


def premise_expf_zero(be):
    got = _expf_probe(be, [0.0, -0.0])
    assert bool((bits(got) == 0x3F800000).all()), "premise: __expf(0) == 1; got %r" % got.tolist()


def premise_expf_cold(be):
    xs = [-112.0 - 8 * k for k in range(16)] + [-112.0 - 16 - 8 * k for k in range(16)] + [NEG]
    got = _expf_probe(be, xs)
    assert bool((got == 0).all()), "premise: __expf(x) == 0 for x <= -112; got %r" % got.tolist()


def premise_logf_one(be):
    """lse of a row {0, -inf}: 0 + logf(__expf(0) + __expf(-inf)) must be 0 (given the two premises above: logf(1) == 0)."""
    dev = be.device
    logits = win_in(torch.tensor([[0.0, NEG]], dtype=torch.float64, device=dev), F32, dev, pad=6)
    labels = win_in(torch.tensor([0], dtype=I64, device=dev), I64, dev)
    rl, lse, st = win_out(1, 1, F32, dev), win_out(1, 1, F32, dev), win_out(1, 3, F32, dev)
    be.ce_fwd(logits.view, vec(labels), 1, 2, vec(rl), vec(lse), vec(st), -1)
    assert int(bits(vec(lse))[0]) == 0 and int(bits(vec(rl))[0]) == 0, "premise: logf(1) == 0; lse %r row_loss %r" % (vec(lse).item(), vec(rl).item())


# ---------------------------------------------------------------------------------------------- answer_scores on pointer rows
SCORE_CASES = [(dtype, V, U) for dtype in ("f32", "bf16") for V in (37, 1030) for U in (1, 2, 65)]


def check_answer_scores(be, dtype, V, U):
    """Integer sums over pointer rows: score[row] = - sum of (112 + 8k) over the targets off the hot column, 0 terms on it.
    Target id 0 in the middle and at the end of a row (skipped); the last position contributes nothing; ids[row, 0] is never a
    target.  U = 65: more than one stride of the 64 lanes."""
    dev, dt, rows = be.device, DT[dtype], 3
    name = "answer_scores-%s-v%d-u%d" % (dtype, V, U)
    gen = generator(8100 + V + U, dev)
    M = rows * U
    b = border_columns(V)
    ids = torch.randint(1, V, (rows, U), generator=gen, device=dev)
    bt = torch.tensor(b[1:], device=dev)
    pick = torch.randint(0, len(b) - 1, (rows, U), generator=gen, device=dev)
    ids = torch.where(torch.rand(rows, U, generator=gen, device=dev) < 0.5, bt[pick], ids)          # (half of the targets on a border)
    if U > 2:
        ids[:, U // 2] = 0
        ids[0, U - 1] = 0
        ids[1, 1] = 0
    tgt = torch.zeros_like(ids)
    tgt[:, :-1] = ids[:, 1:]
    hot = [b[(5 * m) % len(b)] if m % 3 else int(tgt.reshape(-1)[m]) for m in range(M)]      # (a third of the rows: the target IS the hot column)
    x, L = pointer_rows(M, V, hot, [(int(tgt.reshape(-1)[m]),) for m in range(M)], gen, dev)
    lp = torch.gather(x, 1, tgt.reshape(-1, 1))[:, 0] - L
    ref = torch.where(tgt.reshape(-1) != 0, lp, torch.zeros_like(lp)).view(rows, U).sum(1)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) < E.EXACT_LIMIT
    logits, lse, idw = win_in(x, dt, dev, pad=(-V) % 4 + 4), win_in(L, F32, dev), win_in(ids, I64, dev)
    got = []
    for rep in range(2):
        sc = win_out(1, rows, F32, dev)
        be.answer_scores(logits.view, vec(lse), idw.view, rows, U, vec(sc))
        E.assert_bit_equal(vec(sc), ref, name)
        sc.assert_surroundings_untouched(name + ": scores")
        got.append(vec(sc).clone())
    assert_same_bits(got[0], got[1], name + ": repeated launch")
    surroundings((("logits", logits), ("lse", lse), ("ids", idw)), name)


# ============================================================================================== cross entropy: noise rows
NOISE_CASES = [(dtype, V, kind) for dtype in ("f32", "bf16") for V in (1025, 2049, 30522) for kind in ("gauss", "offset", "scaled")]
MEASURED = {}                      # id -> dict of measured rel-to-max errors (printed by the GPU module, recorded in DESIGN.md)


def noise_logits(M, V, kind, dtype, gen, dev):
    z = torch.randn(M, V, generator=gen, device=dev, dtype=torch.float64) * 2.0
    z = z + 60.0 if kind == "offset" else z * 10.0 if kind == "scaled" else z         # (scaled: 2 * 10 = 20)
    return z.to(dtype).double()                                                       # the STORED values


def rel_to_max(got, ref):
    got, ref = got.double(), ref.double().reshape(got.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def check_ce_noise(be, dtype, V, kind):
    """M = 3 noise rows against float64 log_softmax of the stored values: row_loss (tol x 5), dlogits (tol(dtype) x 2), scores
    (tol x 10), all relative to the reference maximum as in tests/test_ops_gpu.py, whose fp32 outputs (row_loss, scores) are
    judged under the fp32 tolerance for both logit types.  The columns past V are NaN."""
    dev, dt, M = be.device, DT[dtype], 3
    name = "ce_noise-%s-v%d-%s" % (dtype, V, kind)
    gen = generator(8300 + V, dev)
    x = noise_logits(M, V, kind, dt, gen, dev)
    lab = torch.randint(1, V, (M,), generator=gen, device=dev)
    lab[1] = V - 1
    V4 = -(-V // 4) * 4
    logits, labels = win_in(x, dt, dev, pad=V4 - V + 4), win_in(lab, I64, dev)
    rl, lse, st = win_out(1, M, F32, dev), win_out(1, M, F32, dev), win_out(1, 3, F32, dev)
    be.ce_fwd(logits.view, vec(labels), M, V, vec(rl), vec(lse), vec(st), 0)
    lp = torch.log_softmax(x, -1)
    ref_loss = -torch.gather(lp, 1, lab.view(-1, 1))[:, 0]
    ref_lse = torch.logsumexp(x, -1)
    gs = win_in(torch.ones(1, dtype=torch.float64, device=dev), F32, dev)
    ldd = V4 + 8
    dl = win_out(M, ldd, dt, dev)
    be.ce_bwd(logits.view, vec(labels), vec(lse), vec(st), vec(gs), True, M, V, dl.view, 0)
    ref_d = (lp.exp() - torch.nn.functional.one_hot(lab, V).double()) / M
    ids = torch.cat([torch.ones(1, dtype=I64, device=dev), lab[1:]]).view(1, M)        # targets of positions 0, 1: labels 1, 2
    idw = win_in(ids, I64, dev)
    sc = win_out(1, 1, F32, dev)
    be.answer_scores(logits.view, vec(lse), idw.view, 1, M, vec(sc))
    ref_s = (lp[0, lab[1]] + lp[1, lab[2]]).view(1)
    e = dict(row_loss=rel_to_max(vec(rl), ref_loss), lse=rel_to_max(vec(lse), ref_lse), dlogits=rel_to_max(dl.view[:, :V], ref_d),
             scores=rel_to_max(vec(sc), ref_s), mean=abs(vec(st)[2].item() - ref_loss.mean().item()) / ref_loss.mean().item())
    MEASURED[name] = e
    print("%s: rel-to-max errors %s" % (name, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    assert e["row_loss"] <= tol(F32) * 5, "%s: row_loss %.3e (tol %.1e)" % (name, e["row_loss"], tol(F32) * 5)
    assert e["dlogits"] <= tol(dt) * 2, "%s: dlogits %.3e (tol %.1e)" % (name, e["dlogits"], tol(dt) * 2)
    assert e["scores"] <= tol(F32) * 10, "%s: scores %.3e (tol %.1e)" % (name, e["scores"], tol(F32) * 10)
    assert e["mean"] < 1e-4 and vec(st)[1].item() == M, name + ": stats"
    assert bool((dl.view[:, V:] == 0).all()), name + ": columns V..ldd of dlogits"
    surroundings((("logits", logits), ("labels", labels), ("row_loss", rl), ("lse", lse), ("stats", st), ("dlogits", dl), ("ids", idw), ("scores", sc)), name)


# ---------------------------------------------------------------------------------------------- invariances
INVARIANCE_CASES = [(dtype, V) for dtype in ("f32", "bf16") for V in (1030, 2049)]


def _ce_all(be, x, lab, dt, ldl, ldd, decoy=None):
    """ce_fwd, ce_bwd (sum form, gscale 0.5: no dependence on the count) and ce_bwd_rows over rows x; the outputs, cloned."""
    dev = be.device
    M, V = x.shape
    logits, labels = win_in(x, dt, dev, pad=ldl - V, decoy=decoy), win_in(lab, I64, dev)
    rl, lse, st = win_out(1, M, F32, dev), win_out(1, M, F32, dev), win_out(1, 3, F32, dev)
    be.ce_fwd(logits.view, vec(labels), M, V, vec(rl), vec(lse), vec(st), 0)
    gs = win_in(torch.full((1,), 0.5, dtype=torch.float64, device=dev), F32, dev)
    dl = win_out(M, ldd, dt, dev)
    be.ce_bwd(logits.view, vec(labels), vec(lse), vec(st), vec(gs), False, M, V, dl.view, 0)
    g = win_in(2.0 ** (torch.arange(M, device=dev) % 3 - 1).double(), F32, dev)
    dr = win_out(M, ldd, dt, dev)
    be.ce_bwd_rows(logits.view, vec(labels), vec(lse), vec(g), M, V, dr.view, 0)
    surroundings((("row_loss", rl), ("lse", lse), ("stats", st), ("dlogits", dl), ("dlogits of ce_bwd_rows", dr), ("logits", logits)), "invariance")
    return dict(row_loss=vec(rl).clone(), lse=vec(lse).clone(), dlogits=dl.view[:, :V].clone(), drows=dr.view[:, :V].clone())


def check_ce_invariances(be, dtype, V):
    """A row's row_loss, lse and dlogits are the same bits whatever the other rows are (permutation; M = 1 against M = 8),
    whatever the padding holds (NaN or finite garbage) and whatever ldl and ldd are."""
    dev, dt, M = be.device, DT[dtype], 8
    name = "ce_invariance-%s-v%d" % (dtype, V)
    gen = generator(8500 + V, dev)
    x = noise_logits(M, V, "gauss", dt, gen, dev)
    lab = torch.randint(1, V, (M,), generator=gen, device=dev)
    lab[3] = 0                                                       # one ignored row
    V4 = -(-V // 4) * 4
    base = _ce_all(be, x, lab, dt, V4 + 4, V4 + 8)
    again = _ce_all(be, x, lab, dt, V4 + 4, V4 + 8)
    perm = torch.randperm(M, generator=generator(3, "cpu")).to(dev)
    # (ce_bwd_rows' g follows the row index: compare its output only where the permuted row keeps its g)
    pm = _ce_all(be, x[perm], lab[perm], dt, V4 + 4, V4 + 8)
    decoy = _ce_all(be, x, lab, dt, V4 + 4, V4 + 8, decoy=7.0)
    wide = _ce_all(be, x, lab, dt, V4 + 64, V4 + 20)
    for k in base:
        assert_same_bits(base[k], again[k], "%s: %s, repeated launch" % (name, k))
        assert_same_bits(base[k], decoy[k], "%s: %s, finite against NaN padding" % (name, k))
        assert_same_bits(base[k], wide[k], "%s: %s, other ldl / ldd" % (name, k))
        if k != "drows":
            assert_same_bits(base[k][perm], pm[k], "%s: %s, rows permuted" % (name, k))
    same_g = (torch.arange(M, device=dev) % 3) == (perm % 3)
    assert_same_bits(base["drows"][perm][same_g], pm["drows"][same_g], name + ": ce_bwd_rows, rows permuted")
    for m in (0, 3, 7):
        one = _ce_all(be, x[m:m + 1], lab[m:m + 1], dt, V4 + 4, V4 + 8)
        for k in ("row_loss", "lse", "dlogits"):
            assert_same_bits(base[k][m:m + 1], one[k], "%s: %s of row %d, M = 1 against M = 8" % (name, k, m))


# ============================================================================================== AdamW
B1, B2, EPS, STEP = 0.5, 0.75, 2.0 ** -4, 1.0
G0 = 3.0 / 16
LRS = tuple(2.0 ** -e for e in range(2, 7))
WDS = (0.0, 0.5, 0.25, 0.125)
ODD_LENGTHS = (5, 1, 6, 7, 1, 64, 3, 1021, 2, 9, 130, 1, 1, 2, 255, 4, 11)

_AdamCase = collections.namedtuple("AdamCase", "entry table n begin gscale shadow origin blocks skip")


class AdamCase(_AdamCase):
    """entry: "f32" (gstvd_adamw), "bf16" (gstvd_adamw_bf16grad, gradient slice from `origin`) or "blocks" (gstvd_adamw_blocks:
    `blocks` the list as given, `skip` the modulus of the segments flagged in seg_skip, whose gradients are NaN)."""
    __slots__ = ()

    @property
    def id(self):
        s = "adamw-%s-%s-n%d-b%d-gs%g%s" % (self.entry, self.table, self.n, self.begin, self.gscale, "-shadow" if self.shadow else "")
        if self.entry == "bf16": s += "-o%d" % self.origin
        if self.entry == "blocks": s += "-blk%s-skip%d" % ("_".join(str(b) for b in self.blocks) or "none", self.skip)
        return s


def acase(entry, table, n, begin=0, gscale=1.0, shadow=True, origin=0, blocks=(), skip=0):
    assert begin % 4 == 0 and (begin == 0 or begin % 1024) and n % 4 != 0
    return AdamCase(entry, table, n, begin, gscale, shadow, origin, tuple(blocks), skip)


ADAM_CASES = [
    acase("f32", "one", 4099), acase("f32", "one", 3001, begin=516, gscale=0.5, shadow=False), acase("f32", "one", 7, begin=4),
    acase("f32", "s64", 19203, gscale=0.25), acase("f32", "s64pad", 19203, begin=2052),
    acase("f32", "odd", 5002, gscale=0.5), acase("f32", "oddpad", 5001, begin=1028, shadow=False), acase("f32", "odd", 1027, begin=4, gscale=0.25),
    acase("bf16", "one", 4099, begin=1000, gscale=0.5, origin=1000), acase("bf16", "s64pad", 19203, begin=2052, origin=1000),
    acase("bf16", "s64", 19203, gscale=0.25, shadow=False), acase("bf16", "odd", 5002, gscale=0.25, shadow=False),
    acase("bf16", "oddpad", 5001, begin=1028, gscale=0.5, origin=1000), acase("bf16", "odd", 2051, begin=1000, origin=0),
    acase("blocks", "s64", 19203, begin=2052, blocks=(7, 2, 18, 11, 3), skip=6), acase("blocks", "odd", 5002, begin=516, gscale=0.5, blocks=(4, 0, 2), skip=4),
    acase("blocks", "s64pad", 19203, gscale=0.25, blocks=(18, 0, 9), skip=5, shadow=False), acase("blocks", "oddpad", 5001, begin=1028, blocks=(), skip=3),
]


def segment_table(table, total):
    """(ends, lr, wd) covering [0, total): neighbouring segments always differ in lr AND wd; "...pad": lr == 0 segments."""
    if table == "one":
        ends = [total]
    elif table.startswith("s64"):
        ends = list(range(64, total + 64, 64))                        # ~300 segments, 16 per 1024-block
    else:
        ends, i = [], 0
        while not ends or ends[-1] < total:
            ends.append((ends[-1] if ends else 0) + ODD_LENGTHS[i % len(ODD_LENGTHS)])
            i += 1
        assert set(e % 4 for e in ends) >= {1, 2, 3} and 1 in ODD_LENGTHS
    ns = len(ends)
    lr = [LRS[i % 5] for i in range(ns)]
    wd = [WDS[i % 4] for i in range(ns)]
    if table.endswith("pad"):
        for i in range(ns):
            if i % 7 == 3:
                lr[i] = 0.0
    return np.array(ends, dtype=np.int64), np.array(lr), np.array(wd)


def exact_f32(x, name):
    """The exact_range() guard of this layer: the value is an fp32 number (24 bits, normal range), so the kernel's operation
    that forms it does not round."""
    with np.errstate(over="ignore"):
        ok = (x.astype(np.float32).astype(np.float64) == x) & ((np.abs(x) >= 2.0 ** -126) | (x == 0))
    assert bool(ok.all()), "%s leaves the exact range of fp32 (24 bits) at %d element(s), e.g. %r" % (name, int((~ok).sum()), x[~ok][:3])
    return x


def f32c(x):
    return float(np.float32(x))


def adamw_reference(p, g, m, v, ends, lr, wd, upd, b1, b2, eps, t, gscale, exact=None):
    """float64 AdamW (pytorch_transformers 1.2.0: decay after the update, on the updated weight) of the elements flagged in `upd`;
    per-element lr / wd from numpy.searchsorted on the segment ends; the constants are the kernel's fp32 ones.  exact: a name --
    every intermediate value must then be an fp32 number."""
    n = len(p)
    seg = np.minimum(np.searchsorted(ends, np.arange(n), side="right"), len(ends) - 1)
    lre, wde = lr[seg], wd[seg]
    b1, b2, eps, gscale = f32c(b1), f32c(b2), f32c(eps), f32c(gscale)
    lre, wde = lre.astype(np.float32).astype(np.float64), wde.astype(np.float32).astype(np.float64)
    chk = (lambda x, tag: exact_f32(x[upd], "%s: %s" % (exact, tag))) if exact else (lambda x, tag: x)
    # bc is one of the kernel's fp32 constants (one per launch): formed in fp32 steps like lr * bc below.  At t = 2 the rounding of
    # b2^t alone (2^-25 of 0.998) is 1.5e-5 of 1 - b2^t = 0.002, more than the whole bound of the update term.
    bc = f32c(f32c(np.sqrt(f32c(1.0 - f32c(b2 ** t)))) / f32c(1.0 - f32c(b1 ** t)))
    with np.errstate(invalid="ignore"):
        ge = g * gscale; chk(ge, "g * gscale")
        gc1 = ge * (1.0 - b1); chk(gc1, "g (1 - b1)")
        mm = m * b1 + gc1; chk(mm, "m'")
        gg = ge * ge; chk(gg, "g^2")
        ggc = gg * (1.0 - b2); chk(ggc, "g^2 (1 - b2)")
        vv = v * b2 + ggc; chk(vv, "v'")
        sq = np.sqrt(vv); chk(sq, "sqrt(v')")
        den = sq + eps; chk(den, "sqrt(v') + eps")
        rc = 1.0 / den; chk(rc, "1 / (sqrt(v') + eps)")
        term = mm * rc; chk(term, "m' / (sqrt(v') + eps)")
        ss = lre * bc
        chk(ss, "lr * bc")
        pp = p - ss * term; chk(pp, "p - lr bc term")
        pd = np.where(wde > 0, pp - (lre * wde) * pp, pp); chk(pd, "p'")
    return (np.where(upd, pd, p), np.where(upd, mm, m), np.where(upd, vv, v), term, ss, lre, wde)


class AdamProblem(object):
    """State of one exact case: P, M, V (canary windows: updated in place), G (poisoned), the bf16 shadow (canary), the table."""

    def __init__(self, be, c, seed=0):
        self.c, self.be, dev = c, be, be.device
        rng = np.random.RandomState(9000 + seed)
        n, total = c.n, c.n + 70
        self.total = total
        ends, lr, wd = segment_table(c.table, total)
        self.ends, self.lr, self.wd = ends, lr, wd
        ns = len(ends)
        idx = np.arange(total)
        seg = np.minimum(np.searchsorted(ends, idx, side="right"), ns - 1)
        sign = rng.choice([-1.0, 1.0], total)
        g = sign * G0 / c.gscale
        m = rng.randint(-8, 9, total) * G0
        v = np.full(total, G0 * G0)
        p = rng.randint(-64, 65, total) / 8.0
        self.skip = np.zeros(ns, dtype=np.uint8)
        if c.entry == "blocks" and c.skip:
            self.skip[np.arange(ns) % c.skip == 1] = 1
        inrange = (idx >= c.begin) & (idx < n)
        if c.entry == "blocks":
            listed = np.isin(idx // 1024, np.array(c.blocks, dtype=np.int64))
            inrange &= listed
        pad = lr[seg] == 0
        upd = inrange & ~pad & (self.skip[seg] == 0)
        # what no launch may read or change: padding segments hold NaN in every buffer, skipped segments and everything outside
        # [begin, n) (or the listed blocks) NaN gradients
        g[~upd] = np.nan
        for a in (p, m, v):
            a[pad] = np.nan
        self.upd, self.p0, self.m0, self.v0, self.g0 = upd, p, m, v, g
        pr, mr, vr = adamw_reference(p, g, m, v, ends, lr, wd, upd, B1, B2, EPS, STEP, c.gscale, exact=c.id)[:3]
        self.ref = dict(P=pr, M=mr, V=vr)
        assert upd.any() or not c.blocks
        t = lambda a: torch.from_numpy(a).to(dev)
        self.P, self.M, self.V = (win_out(1, total, F32, dev).set(t(a).float()) for a in (p, m, v))
        gt = BF16 if c.entry == "bf16" else F32
        self.G = win_in(t(g[c.origin:]), gt, dev)
        self.S = win_out(1, total, BF16, dev) if c.shadow else None
        self.seg_end = win_in(t(ends), I64, dev)
        self.hp = win_in(t(np.stack([lr, wd], 1).reshape(-1)), F32, dev)
        self.step = win_in(torch.full((1,), STEP, dtype=torch.float64, device=dev), F32, dev)
        self.blocks = torch.tensor(c.blocks, dtype=torch.int32, device=dev)
        self.skip_dev = torch.from_numpy(self.skip).to(dev)

    def launch(self):
        c, be = self.c, self.be
        args = (vec(self.P), vec(self.G), vec(self.M), vec(self.V), vec(self.S) if self.S is not None else None, vec(self.seg_end), vec(self.hp), vec(self.step))
        if c.entry == "blocks":
            be.adamw_blocks(*args, self.blocks, self.skip_dev, B1, B2, EPS, c.gscale, c.begin, c.n)
        else:
            be.adamw(*args, B1, B2, EPS, c.gscale, c.begin, c.n, c.origin)

    def check(self):
        c, name, dev = self.c, self.c.id, self.be.device
        upd = torch.from_numpy(self.upd).to(dev)
        for tag, w, first in (("param", self.P, self.p0), ("m", self.M, self.m0), ("v", self.V, self.v0)):
            got, ref = vec(w), torch.from_numpy(self.ref[tag[0].upper()]).to(dev)
            if bool(upd.any()):
                E.assert_bit_equal(got[upd], ref[upd], "%s: %s of the updated elements" % (name, tag))
            keep = torch.from_numpy(first).to(dev).float()
            assert_same_bits(got[~upd], keep[~upd], "%s: %s outside the update (below begin, past the end, lr == 0, skipped, unlisted blocks)" % (name, tag))
        if self.S is not None:
            got = vec(self.S)
            if bool(upd.any()):
                E.assert_bit_equal(got[upd], torch.from_numpy(self.ref["P"]).to(dev)[upd], name + ": shadow == bf16(p) by RNE")
            assert bool((bits(got[~upd]) == CANARY[BF16]).all()), name + ": shadow written outside the update"
        surroundings((("param", self.P), ("m", self.M), ("v", self.V), ("grad", self.G), ("shadow", self.S), ("seg_end", self.seg_end), ("hp", self.hp),
                      ("step", self.step)), name)

    def state(self):
        return [w.flat.clone() for w in (self.P, self.M, self.V, self.S) if w is not None]


def run_adam_case(be, c):
    a = AdamProblem(be, c)
    a.launch()
    a.check()
    b = AdamProblem(be, c)
    b.launch()
    for x, y in zip(a.state(), b.state()):
        assert_same_bits(x, y, c.id + ": repeated launch")
    return a


def _adam_probe(be, p, g, m, v, lr, b1, b2, eps, t):
    """One-segment gstvd_adamw launch over a few elements, wd = 0; returns the new p."""
    dev = be.device
    f = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    n = len(p)
    P, M, V = (win_out(1, n, F32, dev).set(f(a).float()) for a in (p, m, v))
    G = win_in(f(g), F32, dev)
    se, hp, st = win_in(torch.tensor([n], dtype=I64, device=dev), I64, dev), win_in(f([lr, 0.0]), F32, dev), win_in(f([t]), F32, dev)
    be.adamw(vec(P), vec(G), vec(M), vec(V), None, vec(se), vec(hp), vec(st), b1, b2, eps, 1.0, 0, n, 0)
    surroundings((("param", P), ("m", M), ("v", V)), "adamw probe")
    return vec(P).clone()


RCP_EXP = tuple(range(-10, 11))
SQRT_EXP = tuple(range(-6, 3))


def premise_rcp_powers_of_two(be):
    """beta1 = beta2 = 0 (bias correction sqrtf(1) / 1), g = 2^-40: sqrt(g^2) is absorbed by eps = 2^k, so p' = -g * rcp(2^k)."""
    for k in RCP_EXP:
        got = _adam_probe(be, [0.0] * 5, [2.0 ** -40] * 5, [0.0] * 5, [0.0] * 5, 1.0, 0.0, 0.0, 2.0 ** k, 1.0)
        assert bool((got.double() == -2.0 ** (-40 - k)).all()), "premise: v_rcp_f32(2^%d) == 2^%d; p' = %r" % (k, -k, got.tolist())


def premise_sqrt_nine_times_four_to_j(be):
    """beta1 = beta2 = 0, g = 3 * 2^j, eps = -2^(j+1): 3 * 2^j - 2^(j+1) is formed without rounding, so sqrt(9 * 4^j) + eps is 2^j
    only if the root is exact -- a root one ulp (2^(j-22)) off either way leaves 2^j +- 2^(j-22), several ulp of 2^j, which no 1-ulp
    reciprocal brings back -- and then p' = -g / 2^j = -3 (given the premise on v_rcp_f32).  A positive eps of 2^j would not do: a
    root one ulp too HIGH gives a tie that rounds back to 2^(j+2)."""
    for j in SQRT_EXP:
        got = _adam_probe(be, [0.0] * 5, [3.0 * 2.0 ** j] * 5, [0.0] * 5, [0.0] * 5, 1.0, 0.0, 0.0, -2.0 ** (j + 1), 1.0)
        assert bool((got.double() == -3.0).all()), "premise: v_sqrt_f32(9 * 4^%d) == 3 * 2^%d; p' = %r" % (j, j, got.tolist())


def premise_powf_one(be):
    """beta1 = 0.5, beta2 = 0.75, t = 1: sqrtf(1 - powf(0.75, 1)) / (1 - powf(0.5, 1)) == 1; with g = 0, m = 1, v = 0, eps = 1:
    p' = -lr * bc * 0.5."""
    got = _adam_probe(be, [0.0] * 5, [0.0] * 5, [1.0] * 5, [0.0] * 5, 1.0, 0.5, 0.75, 1.0, 1.0)
    assert bool((got.double() == -0.5).all()), "premise: powf(b, 1) == b (bias correction exactly 1); p' = %r" % got.tolist()


NOISY_STEPS = (1.0, 2.0, 1000.0)


def check_adamw_noisy(be, t):
    """One noisy multi-segment case: realistic betas, eps and learning rates, step t; float64 reference with the kernel's fp32
    constants; the bounds of tests/test_round5_gpu.py::test_adamw_fast_sqrt_rcp_..., unchanged, judged per element on the UPDATE
    TERM: every other weight is zero, there p' = -lr bc term (1 - lr wd) shows the element's own lr and wd.  The first moment has the
    sign of the gradient: a relative bound on the term presupposes that m' is not a difference of nearly equal numbers."""
    dev, n = be.device, 5003
    name = "adamw-noisy-t%g" % t
    total = n + 70
    rng = np.random.RandomState(77)
    ends = np.array([1602, 1603, 3207, total], dtype=np.int64)
    lr, wd = np.array([2e-5, 1e-3, 5e-4, 1e-4]), np.array([0.01, 0.0, 0.1, 0.01])
    b1, b2, eps = 0.9, 0.999, 1e-6
    p = rng.randn(total)
    p[::2] = 0.0
    g, m, v = rng.randn(total) * 0.1, np.abs(rng.randn(total)) * 0.01, np.abs(rng.randn(total)) * 1e-4
    m = np.copysign(m, g)          # (the sign of g: m' = b1 m + (1 - b1) g does not cancel, so the term's relative error is sqrt's and rcp's)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    p, g, m, v, lr, wd = r32(p), r32(g), r32(m), r32(v), r32(lr), r32(wd)
    upd = (np.arange(total) >= 4) & (np.arange(total) < n)
    pr, mr, vr, term, ss, lre, wde = adamw_reference(p, g, m, v, ends, lr, wd, upd, b1, b2, eps, t, 1.0)
    f = lambda a: torch.from_numpy(a).to(dev)
    P, M, V = (win_out(1, total, F32, dev).set(f(a).float()) for a in (p, m, v))
    G = win_in(f(g), F32, dev)
    S = win_out(1, total, BF16, dev)
    se, hp, st = win_in(f(ends), I64, dev), win_in(f(np.stack([lr, wd], 1).reshape(-1)), F32, dev), win_in(torch.full((1,), t, dtype=torch.float64, device=dev), F32, dev)
    be.adamw(vec(P), vec(G), vec(M), vec(V), vec(S), vec(se), vec(hp), vec(st), b1, b2, eps, 1.0, 4, n, 0)
    u = f(upd)
    gp, gm, gv = vec(P).double(), vec(M).double(), vec(V).double()
    e_m = ((gm - f(mr)).abs()[u].max() / f(mr).abs()[u].max()).item()
    e_v = ((gv - f(vr)).abs() / (1e-6 * f(vr) + 1.2e-38))[u].max().item()
    e_p = (gp - f(pr)).abs()[u].max().item()
    zero = u & (f(p) == 0) & (f(pr).abs() > 1e-20)
    e_t = ((gp - f(pr)).abs() / (f(pr).abs() + 1e-30))[zero].max().item()
    MEASURED[name] = dict(m=e_m, v=e_v, p=e_p, term=e_t)
    print("%s: m %.3e of max|m| (1e-6), v %.3f of its bound, p %.3e (6e-7), update term %.3e relative (5e-6)" % (name, e_m, e_v, e_p, e_t))
    assert bool(torch.isfinite(gp[u]).all()) and bool(torch.isfinite(gv[u]).all())
    assert e_m <= 1e-6, name + ": m"
    assert e_v <= 1.0, name + ": v"
    assert e_p < 6e-7, name + ": p"
    assert e_t < 5e-6, name + ": the update term of the zero weights, per element (an element with its neighbour segment's lr or wd lands here)"
    assert_same_bits(vec(P)[~u], f(p).float()[~u], name + ": p outside [begin, n)")
    assert_same_bits(vec(S)[u], vec(P)[u].to(BF16), name + ": shadow == bf16(p)")
    surroundings((("param", P), ("m", M), ("v", V), ("shadow", S), ("grad", G)), name)


# ============================================================================================== casts
CAST_PAIRS = (("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("bf16", "bf16"))
CAST_N = (1, 3, 4, 5, 1023, 1024, 1025, 2051)
# fp32 bit patterns: +-0, +-inf, NaN, RNE ties with an even (0x3F80) and an odd (0x3F81) upper half and their neighbours, both
# signs; 0x7F7FFFFF (rounds to bf16 inf), the tie 0x7F7F8000 (to even: inf), 0x7F7F7FFF: the largest that does not overflow
SPECIAL_F32 = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF,
               0x3F808001, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7F7FFF, 0xFF7FFFFF, 0x00800000, 0x3F800000)
SPECIAL_BF16 = (0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x7F7F, 0xFF7F, 0x0080, 0x3F80, 0x3F81, 0xBF81, 0x4049)


def _from_bits(pattern, dtype, dev):
    if dtype == F32:
        return torch.tensor([b - 2 ** 32 if b >= 2 ** 31 else b for b in pattern], dtype=torch.int32, device=dev).view(F32)
    return torch.tensor([b - 2 ** 16 if b >= 2 ** 15 else b for b in pattern], dtype=torch.int16, device=dev).view(BF16)


def cast_source(n, dtype, rot, dev):
    """n elements of `dtype`: the specials, rotated by `rot`, in the first 16 positions (the vector path) and in the last 16 (the
    tail: the last n % 4 elements), Gaussian noise between them."""
    sp = _from_bits(SPECIAL_F32 if dtype == F32 else SPECIAL_BF16, dtype, dev)
    x = (torch.randn(n, generator=generator(8700 + n, dev), device=dev) * 3).to(dtype)
    i = torch.arange(n, device=dev)
    special = (i < 16) | (i >= n - 16)
    return torch.where(special, sp[(i + rot) % sp.numel()], x)


def assert_cast_equal(got, src, name):
    """`got` against torch's .to() of `src` on the CPU: NaN where it is NaN (any payload), the same bits elsewhere."""
    want = src.cpu().to(got.dtype).to(got.device)
    nan = torch.isnan(want)
    assert bool((torch.isnan(got) == nan).all()), name + ": NaN positions"
    assert_same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want), name)


def check_cast(be, sdt, ddt, n):
    dev, st, dt = be.device, DT[sdt], DT[ddt]
    nsp = len(SPECIAL_F32 if st == F32 else SPECIAL_BF16)
    for rot in range(0, nsp, 3):
        name = "cast-%s-%s-n%d-rot%d" % (sdt, ddt, n, rot)
        x = cast_source(n, st, rot, dev)
        src = Window(1, n, st, dev, "poison").set(x)
        got = []
        for rep in range(2):
            dst = win_out(1, n, dt, dev)
            be.cast(vec(src), vec(dst), n)
            assert_cast_equal(vec(dst), x, name)
            dst.assert_surroundings_untouched(name + ": dst")
            got.append(vec(dst).clone())
        assert_same_bits(got[0], got[1], name + ": repeated launch")
        src.assert_surroundings_untouched(name + ": src")


def check_cast_denormals(be):
    """fp32 denormals to bf16: the RNE bf16 value or a zero of the same sign.  Returns (rne, flushed): how many of those that
    RNE does not itself round to zero came out each way."""
    dev, n = be.device, 1027
    gen = generator(8800, dev)
    mag = torch.randint(1, 0x00800000, (n,), generator=gen, device=dev, dtype=torch.int64)
    mag[:4] = torch.tensor([1, 0x00008000, 0x007FFFFF, 0x00018000], device=dev)
    mag[-3:] = torch.tensor([0x007F8000, 0x00008001, 0x00400000], device=dev)
    sign = torch.randint(0, 2, (n,), generator=gen, device=dev, dtype=torch.int64) << 31
    b = mag | sign
    x = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(F32)
    src, dst = Window(1, n, F32, dev, "poison").set(x), win_out(1, n, BF16, dev)
    be.cast(vec(src), vec(dst), n)
    got, rne = vec(dst), x.cpu().to(BF16).to(dev)
    zero = torch.where(sign != 0, torch.full_like(rne, -0.0), torch.zeros_like(rne))
    is_rne, is_zero = bits(got) == bits(rne), bits(got) == bits(zero)
    assert bool((is_rne | is_zero).all()), "cast of fp32 denormals: %d element(s) are neither the RNE bf16 value nor a zero of the same sign" % int((~(is_rne | is_zero)).sum())
    dst.assert_surroundings_untouched("cast of denormals: dst")
    tell = bits(rne) != bits(zero)
    return int((is_rne & tell).sum().item()), int((is_zero & tell).sum().item())


RANGE_LENGTHS = (1, 1023, 1024, 1025)


def check_cast_ranges(be, order=(0, 1, 2, 3)):
    """cast_ranges over ranges of 1, 1023, 1024 and 1025 elements (starts multiples of 4, gaps between them): the specials at both
    ends of every range, NaN in the source's gaps, the canary kept in the destination's."""
    dev = be.device
    name = "cast_ranges-%s" % "".join(str(i) for i in order)
    ranges, at = [], 8
    for i in order:
        ranges.append((at, RANGE_LENGTHS[i]))
        at = -(-(at + RANGE_LENGTHS[i] + 5) // 4) * 4
    total = at + 8
    x = torch.full((total,), float("nan"), device=dev)
    inside = torch.zeros(total, dtype=torch.bool, device=dev)
    for r, (a, ln) in enumerate(ranges):
        x[a:a + ln] = cast_source(ln, F32, 3 * r, dev)
        inside[a:a + ln] = True
    src = Window(1, total, F32, dev, "poison").set(x)
    got = []
    for rep in range(2):
        dst = win_out(1, total, BF16, dev)
        be.cast_ranges(ranges, vec(src), vec(dst))
        assert_cast_equal(vec(dst)[inside], x[inside], name)
        assert bool((bits(vec(dst)[~inside]) == CANARY[BF16]).all()), name + ": a gap between two ranges was written"
        dst.assert_surroundings_untouched(name + ": dst")
        got.append(vec(dst).clone())
    assert_same_bits(got[0], got[1], name + ": repeated launch")


# ============================================================================================== vl_split
VL_SHAPES = ((1, 1, 1, 4), (3, 5, 7, 12), (2, 36, 20, 260))
VL_SITES = tuple((s, s + 17) for s in range(21, 21 + 16))


def check_vl_split(be, dtype, shape, p):
    """d_enc [B, R + T, H] of integers split into d_v [B * R, H] and d_t [B * T, H] (windows).  p = 0, rng None: bit-equal to
    slicing.  p = 0.5 (factor exactly 2): bit-equal to slice * ops.dropout_mask(n, p, site) at site_v / site_t -- the masks differ
    and both halves show kept and dropped elements (the first site pair of VL_SITES for which they do)."""
    dev, dt = be.device, DT[dtype]
    B, R, T, H = shape
    name = "vl_split-%s-%dx%dx%dx%d-p%g" % ((dtype,) + tuple(shape) + (p,))
    d = torch.randint(-8, 9, (B, R + T, H), generator=generator(8900 + H, dev), device=dev).double()
    d = torch.where(d == 0, torch.ones_like(d), d)                       # (no zero: a dropped element is told from a kept one)
    src = win_in(d.reshape(B * (R + T), H), dt, dev)
    sv = st = 0
    mv, mt = torch.ones(B * R * H, dtype=torch.float64, device=dev), torch.ones(B * T * H, dtype=torch.float64, device=dev)
    if p > 0:
        assert p == 0.5
        k = min(B * R * H, B * T * H)
        for sv, st in VL_SITES:
            mv, mt = be.drop_mask(B * R * H, p, sv).double(), be.drop_mask(B * T * H, p, st).double()
            if all(bool((x == 0).any()) and bool((x == 2).any()) for x in (mv, mt)) and not torch.equal(mv[:k], mt[:k]):
                break
        else:
            raise AssertionError(name + ": no site pair of the list gives two different masks with kept and dropped elements in both halves")
        assert sv != st and all(bool(((x == 0) | (x == 2)).all()) for x in (mv, mt))
        assert not torch.equal(mv[:k], mt[:k]), name + ": the masks of site_v and site_t are the same"
    ref_v = d[:, :R].reshape(B * R, H) * mv.view(B * R, H)
    ref_t = d[:, R:].reshape(B * T, H) * mt.view(B * T, H)
    got = []
    for rep in range(2):
        dv, dt_ = win_out(B * R, H, dt, dev), win_out(B * T, H, dt, dev)
        be.vl_split(src.view, B, R, T, H, dv.view, dt_.view, p, sv, st)
        E.assert_bit_equal(dv.view, ref_v, name + ": d_v == d_enc[:, :R] * mask_v")
        E.assert_bit_equal(dt_.view, ref_t, name + ": d_t == d_enc[:, R:] * mask_t")
        surroundings((("d_v", dv), ("d_t", dt_)), name)
        got.append((dv.view.clone(), dt_.view.clone()))
    assert_same_bits(got[0][0], got[1][0], name + ": repeated launch, d_v")
    assert_same_bits(got[0][1], got[1][1], name + ": repeated launch, d_t")
    src.assert_surroundings_untouched(name + ": d_enc")


def case_count():
    """How many cases each family of the layer runs (DESIGN.md section 2 quotes it)."""
    return collections.OrderedDict([
        ("ce pointer", len(CE_CASES)), ("ce_bwd_rows", 2 * len(ROWS_V)), ("answer_scores", len(SCORE_CASES)), ("ce noise", len(NOISE_CASES)),
        ("ce invariance", len(INVARIANCE_CASES)), ("adamw exact", len(ADAM_CASES)), ("adamw noisy", len(NOISY_STEPS)),
        ("cast", len(CAST_PAIRS) * len(CAST_N)), ("cast denormals", 1), ("cast_ranges", 2), ("vl_split", 2 * 2 * len(VL_SHAPES)), ("premises", 6)])
