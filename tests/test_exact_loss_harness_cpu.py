"""The exact layer of the loss and optimizer tests proves itself on the CPU (tests/exact_loss.py): every case
runs against a stand-in of csrc/loss.hip, csrc/optim.hip and csrc/elementwise.hip written in torch -- the cross entropy with the kernels' column loops (4-element vectors,
stride 1024, scalar tail), AdamW in emulated fp32 with the kernel's fused steps -- and against deliberately wrong stand-ins, each
of which must fail the case named for it.  Nothing here touches a GPU."""
import numpy as np
import pytest
import torch

import exact_loss as X
from exact_gemm import BF16, F32

CPU = torch.device("cpu")


def r32(x):
    """Round a float64 tensor to fp32 and back: one fp32 operation of the emulation."""
    return x.float().double()


def visit_columns(V, stride=1024, tail=None):
    """The columns the forward kernel's 256 threads visit, with multiplicity: vectors at 4 t + stride i below V4, the scalar tail
    from `tail` (V4) on."""
    V4 = V & ~3
    cols = []
    for t in range(256):
        c = 4 * t
        while c < V4:
            cols += [c, c + 1, c + 2, c + 3]
            c += stride
    cols += list(range(V4 if tail is None else tail, V))
    return torch.tensor(cols, dtype=torch.int64)


class Torch(object):
    """Stand-in of the entries of csrc/loss.hip, csrc/optim.hip and csrc/elementwise.hip.  `defect`: one planted error, by its name in DEFECTS."""

    def __init__(self, defect=None):
        self.device, self.defect = CPU, defect
        self._cols = {}

    # -- cross entropy
    def _visited(self, V):
        if V not in self._cols:
            d = self.defect
            self._cols[V] = visit_columns(V, 1020 if d == "ce stride 1020" else 1024, (V & ~3) + 1 if d == "ce tail from V4 + 1" else None)
        return self._cols[V]

    def ce_fwd(self, logits, labels, M, V, row_loss, lse, stats, ignore_index=0):
        x = logits[:, :V].float()
        xv = x[:, self._visited(V)]
        mx = xv.max(1).values
        s = torch.exp(xv - mx[:, None]).sum(1)
        l = mx + torch.log(s)
        lse.copy_(l)
        keep = (labels != ignore_index) & (labels >= 0) & (labels < V)
        xl = torch.gather(x, 1, labels.clamp(0, V - 1).view(-1, 1))[:, 0]
        if self.defect == "label >= V kept":                      # x[lab] is then read from the row's padding
            keep = (labels != ignore_index) & (labels >= 0)
            wide = torch.as_strided(logits, (M, logits.stride(0)), logits.stride(), logits.storage_offset()).float()
            xl = torch.gather(wide, 1, labels.clamp(0, wide.shape[1] - 1).view(-1, 1))[:, 0]
        row_loss.copy_(torch.where(keep, l - xl, torch.zeros_like(l)))
        n = float(M) if self.defect == "count = M" else float((labels != ignore_index).sum())
        stats[0], stats[1] = row_loss.sum(), n
        stats[2] = stats[0] / stats[1]

    def _bwd(self, logits, labels, lse, g, keep, V, dl):
        d = self.defect
        M, ldd = dl.shape
        x = logits[:, :V].float()
        lab = labels + (-1 if d == "one-hot at c + e + 1" else 0)
        onehot = (torch.arange(V).view(1, -1) == lab.view(-1, 1)).float()
        val = (torch.exp(x - lse.view(-1, 1)) - onehot) * g.view(-1, 1)
        if d == "ignored row multiplied":
            out = torch.where(keep.view(-1, 1), val, (torch.exp(x - lse.view(-1, 1)) - onehot) * 0.0)
        else:
            out = torch.where(keep.view(-1, 1), val, torch.zeros_like(val))
        dl[:, :V] = out.to(dl.dtype)
        if d != "padding not zeroed":
            dl[:, V:] = 0

    def ce_bwd(self, logits, labels, lse, stats, gscale, mean, M, V, dlogits, ignore_index=0):
        gs = gscale[0] if gscale is not None else torch.tensor(1.0)
        if mean:
            gs = gs / stats[1]
        keep = (labels != ignore_index) & (labels >= 0) & (labels < V)
        self._bwd(logits, labels, lse, gs.expand(M), keep, V, dlogits)

    def ce_bwd_rows(self, logits, labels, lse, g, M, V, dlogits, ignore_index=0):
        keep = (labels != ignore_index) & (labels >= 0) & (labels < V) & (g != 0)
        self._bwd(logits, labels, lse, g, keep, V, dlogits)

    def answer_scores(self, logits, lse, dec_ids, rows, U, scores):
        d = self.defect
        flat = dec_ids.reshape(-1)
        for row in range(rows):
            a = torch.zeros((), dtype=torch.float32)
            for u in range(U):
                if d == "scores use ids[u]":
                    tgt = int(dec_ids[row, u])
                elif u + 1 < U:
                    tgt = int(dec_ids[row, u + 1])
                else:
                    tgt = int(flat[(row * U + u + 1) % flat.numel()]) if d == "scores include the last position" else 0
                if tgt != 0:
                    a = a + (logits[row * U + u, tgt].float() - lse[row * U + u])
            scores[row] = a

    # -- casts
    def _convert(self, x, dtype):
        if self.defect == "cast truncates" and x.dtype == F32 and dtype == BF16:
            return (x.view(torch.int32) >> 16).to(torch.int16).view(BF16)
        return x.to(dtype)

    def cast(self, src, dst, n=None):
        n = src.numel() if n is None else n
        m = n - 1 if self.defect == "cast tail off by one" and n % 4 else n
        dst[:m] = self._convert(src[:m], dst.dtype)

    def cast_ranges(self, ranges, src, dst):
        for a, n in ranges:
            self.cast(src[a:a + n], dst[a:a + n], n)

    # -- dropout and vl_split
    def drop_mask(self, n, p, site):
        g = torch.Generator().manual_seed(1234567 + 7919 * int(site))
        return torch.where(torch.rand(n, generator=g) >= p, torch.full((n,), 1.0 / (1.0 - p)), torch.zeros(n))

    def vl_split(self, d_enc, B, R, T, H, d_v, d_t, p, site_v, site_t):
        d = self.defect
        if d == "vl_split sites swapped":
            site_v, site_t = site_t, site_v
        x = d_enc.reshape(B, R + T, H).float()
        for out, n_rows, sl, site in ((d_v, R, slice(0, R), site_v), (d_t, T, slice(R, R + T), site_t)):
            part = x[:, sl]
            if p > 0:
                if d == "vl_split mask index from the d_enc row":
                    full = self.drop_mask(B * (R + T) * H, p, site).view(B, R + T, H)
                    part = part * full[:, sl]
                else:
                    part = part * self.drop_mask(B * n_rows * H, p, site).view(B, n_rows, H)
            out.copy_(part.reshape(B * n_rows, H).to(out.dtype))

    # -- AdamW: fp32 emulated in float64 (one rounding per kernel operation, fused multiply-adds rounded once)
    @staticmethod
    def update(p, g, m, v, lr, wd, b1, b2, eps, t, gscale, wd_first=False):
        f = lambda a: float(np.float32(a))
        b1, b2, eps, gscale = f(b1), f(b2), f(eps), f(gscale)
        lr, wd = r32(lr), r32(wd)
        bc = f(f(np.sqrt(f(1.0 - f(b2 ** t)))) / f(1.0 - f(b1 ** t)))
        c1, c2 = f(1.0 - b1), f(1.0 - b2)
        step_size, decay = r32(lr * bc), r32(-lr * wd)
        if wd_first:
            p = torch.where(wd > 0, r32(decay * p + p), p)
        ge = r32(g * gscale)
        mm = r32(m * b1 + r32(ge * c1))
        vv = r32(v * b2 + r32(r32(ge * ge) * c2))
        den = r32(r32(torch.sqrt(vv)) + eps)
        pp = r32(-step_size * r32(mm * r32(1.0 / den)) + p)
        if not wd_first:
            pp = torch.where(wd > 0, r32(decay * pp + pp), pp)
        return pp, mm, vv

    def _adamw(self, param, grad, m, v, shadow, seg_end, hp, step, b1, b2, eps, gscale, begin, n, origin, blocks=None, seg_skip=None):
        d = self.defect
        total, nseg = param.numel(), seg_end.numel()
        i = torch.arange(total)
        lookup = i
        if d == "segment of i - 1":
            lookup = (i - 1).clamp(min=0)
        elif d == "vector path across a segment end":
            lookup = torch.where((i & ~3) + 3 < n, i & ~3, i)
        seg = torch.bucketize(lookup, seg_end, right=True).clamp(max=nseg - 1)
        lr, wd = hp[0::2][seg].double(), hp[1::2][seg].double()
        lo = (begin // 1024) * 1024 if d == "begin rounded down to 1024" else begin
        act = (i >= lo) & (i < n) & (lr != 0)
        if blocks is not None:
            act &= torch.isin(i // 1024, blocks.long())
            if d != "seg_skip ignored":
                act &= seg_skip[seg] == 0
        gi = i if d == "grad_origin ignored" else i - origin
        g = grad.double()[gi.clamp(0, grad.numel() - 1)]
        pp, mm, vv = self.update(param.double(), g, m.double(), v.double(), lr, wd, b1, b2, eps, float(step[0]),
                                 1.0 if d == "gscale dropped" else gscale, wd_first=(d == "wd before the update"))
        param[act], m[act], v[act] = pp.float()[act], mm.float()[act], vv.float()[act]
        if shadow is not None:
            shadow[act] = pp.float().to(BF16)[act]

    def adamw(self, param, grad, m, v, shadow, seg_end, hp, step, b1, b2, eps, gscale, begin, end, origin):
        self._adamw(param, grad, m, v, shadow, seg_end, hp, step, b1, b2, eps, gscale, begin, end, origin)

    def adamw_blocks(self, param, grad, m, v, shadow, seg_end, hp, step, blocks, seg_skip, b1, b2, eps, gscale, begin, end):
        self._adamw(param, grad, m, v, shadow, seg_end, hp, step, b1, b2, eps, gscale, begin, end, 0, blocks, seg_skip)


BE = Torch()


# ---------------------------------------------------------------------------------------------- the stand-in passes every case
@pytest.mark.parametrize("c", X.CE_CASES, ids=[c.id for c in X.CE_CASES])
def test_pointer_rows(c):
    X.run_ce_case(BE, c)


def test_the_case_table_covers_the_shapes_and_borders():
    cs = X.CE_CASES
    assert set(c.V for c in cs) == set(X.CE_V) and set(c.M for c in cs) == {1, 2, 5, 8}
    assert set(c.M for c in cs if c.V == 30522) == {2}
    for V in X.CE_V:
        for dtype in ("f32", "bf16"):
            mine = [c for c in cs if c.V == V and c.dtype == dtype]
            assert set(p for c in mine for p in c.pairs) >= set(X.border_pairs(V))
            if V > 1:
                assert set(c.ignore for c in mine) == {0, -1}
    assert set(c.gscale for c in cs) == set(X.GSCALES) and set(c.mean for c in cs) == {True, False}
    assert any("i" in c.plan for c in cs) and any(set(c.plan) == {"i"} for c in cs)          # (the second: no counted row at all)
    for V in (37, 1025, 1030, 2049, 30522):                               # every out-of-range label the contract names, in both types
        for dtype in ("f32", "bf16"):
            used = set(l for c in cs if c.V == V and c.dtype == dtype for l in c.oor_labels())
            assert used == {-5, V, V + 3}, (V, dtype, used)
    for c in cs:
        p = X.CeProblem(BE, c)
        assert [l for l, k in zip(p.lab, c.plan) if k == "o"] == c.oor_labels()
    assert {(1020, 1021), (3, 4), (1023, 1024), (1024, 1023), (30519, 30520)} <= set(X.border_pairs(30522))
    for c in cs:                                                          # every value of a pointer row is a bf16 number
        X.CeProblem(BE, c).inputs_untouched(c.id)


def test_premises_hold_in_the_stand_in():
    for f in (X.premise_expf_zero, X.premise_expf_cold, X.premise_logf_one, X.premise_rcp_powers_of_two, X.premise_sqrt_nine_times_four_to_j,
              X.premise_powf_one):
        f(BE)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", X.ROWS_V)
def test_per_row_backward(dtype, V):
    X.check_ce_bwd_rows(BE, dtype, V)


@pytest.mark.parametrize("dtype,V,U", X.SCORE_CASES)
def test_answer_scores(dtype, V, U):
    X.check_answer_scores(BE, dtype, V, U)


@pytest.mark.parametrize("dtype,V,kind", X.NOISE_CASES)
def test_noise_rows(dtype, V, kind):
    X.check_ce_noise(BE, dtype, V, kind)


@pytest.mark.parametrize("dtype,V", X.INVARIANCE_CASES)
def test_invariances(dtype, V):
    X.check_ce_invariances(BE, dtype, V)


@pytest.mark.parametrize("c", X.ADAM_CASES, ids=[c.id for c in X.ADAM_CASES])
def test_adamw_exact(c):
    X.run_adam_case(BE, c)


def test_adamw_tables_are_what_the_layer_claims():
    ends, lr, wd = X.segment_table("s64", 19273)
    assert 290 <= len(ends) <= 310 and bool((np.diff(ends) == 64).all())
    for table in ("s64", "odd"):
        ends, lr, wd = X.segment_table(table, 5072)
        assert bool((lr[1:] != lr[:-1]).all()) and bool((wd[1:] != wd[:-1]).all())
    ends, lr, wd = X.segment_table("oddpad", 5072)
    assert (lr == 0).any() and 1 in np.diff(ends) and set(e % 4 for e in ends) >= {1, 2, 3}
    entries = set((c.entry, c.origin) for c in X.ADAM_CASES)
    assert {("f32", 0), ("bf16", 0), ("bf16", 1000), ("blocks", 0)} <= entries
    assert any(c.entry == "blocks" and not c.blocks for c in X.ADAM_CASES) and any(not c.shadow for c in X.ADAM_CASES)
    assert any(c.entry == "blocks" and list(c.blocks) != sorted(c.blocks) for c in X.ADAM_CASES)


def test_adamw_family_is_exact_in_emulated_fp32_20000_draws():
    """The family of the exact cases, 20000 random elements with an lr and a wd of their own: the emulated fp32 kernel (fused
    steps) equals the float64 reference bit for bit, and exact_f32() accepts every intermediate value."""
    rng = np.random.RandomState(5)
    n = 20000
    for gscale in (1.0, 0.5, 0.25):
        g = rng.choice([-1.0, 1.0], n) * X.G0 / gscale
        m, v, p = rng.randint(-8, 9, n) * X.G0, np.full(n, X.G0 ** 2), rng.randint(-64, 65, n) / 8.0
        lr, wd = np.array(X.LRS)[rng.randint(0, 5, n)], np.array(X.WDS)[rng.randint(0, 4, n)]
        ends = np.arange(1, n + 1)
        pr, mr, vr = X.adamw_reference(p, g, m, v, ends, lr, wd, np.ones(n, dtype=bool), X.B1, X.B2, X.EPS, X.STEP, gscale, exact="family")[:3]
        t = torch.from_numpy
        pp, mm, vv = Torch.update(t(p), t(g), t(m), t(v), t(lr), t(wd), X.B1, X.B2, X.EPS, X.STEP, gscale)
        assert torch.equal(pp, t(pr)) and torch.equal(mm, t(mr)) and torch.equal(vv, t(vr))


def test_exact_range_guard_refuses_a_case_that_leaves_24_bits():
    n = 8
    p, g, m, v = np.full(n, 1.0 + 2.0 ** -20), np.full(n, X.G0), np.zeros(n), np.full(n, X.G0 ** 2)
    with pytest.raises(AssertionError, match="exact range"):
        X.adamw_reference(p, g, m, v, np.array([n]), np.array([2.0 ** -6]), np.array([0.125]), np.ones(n, dtype=bool), X.B1, X.B2, X.EPS, X.STEP, 1.0, exact="guard")


@pytest.mark.parametrize("t", X.NOISY_STEPS)
def test_adamw_noisy(t):
    X.check_adamw_noisy(BE, t)


@pytest.mark.parametrize("n", X.CAST_N)
@pytest.mark.parametrize("sdt,ddt", X.CAST_PAIRS)
def test_casts(sdt, ddt, n):
    X.check_cast(BE, sdt, ddt, n)


def test_cast_denormals_and_ranges():
    rne, flushed = X.check_cast_denormals(BE)
    assert rne > 900 and flushed == 0                       # (torch on the CPU rounds denormals)
    X.check_cast_ranges(BE)
    X.check_cast_ranges(BE, order=(3, 0, 2, 1))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", X.VL_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_vl_split(dtype, shape, p):
    X.check_vl_split(BE, dtype, shape, p)


# ---------------------------------------------------------------------------------------------- every planted defect fails its case
def _ce(cid):
    c = [c for c in X.CE_CASES if c.id == cid]
    assert len(c) == 1, cid
    return lambda be: X.run_ce_case(be, c[0])


def _adam(cid):
    c = [c for c in X.ADAM_CASES if c.id == cid]
    assert len(c) == 1, cid
    return lambda be: X.run_adam_case(be, c[0])


def _first(pred, what):
    c = [c for c in X.CE_CASES if pred(c)]
    assert c, what
    return c[0].id


# defect -> (name of the case that must fail, how to run it)
DEFECTS = {
    "ce stride 1020": _first(lambda c: c.V == 1025 and any(j in (1020, 1021, 1022, 1023) for j, _ in c.pairs), "a hot column in 1020..1023"),
    "ce tail from V4 + 1": _first(lambda c: c.V == 1030 and any(j == 1028 for j, _ in c.pairs), "a hot column at V4"),
    "one-hot at c + e + 1": _first(lambda c: c.V == 37 and c.M == 1, "any kept row"),
    "padding not zeroed": _first(lambda c: c.V == 5, "any case"),
    "label >= V kept": _first(lambda c: c.V == 1030 and any(l >= c.V for l in c.oor_labels()), "an out-of-range label >= V"),
    "count = M": _first(lambda c: "i" in c.plan and c.V == 1024, "a case with an ignored row"),
}
RUN = dict((k, _ce(v)) for k, v in DEFECTS.items())
DEFECTS.update({
    "ignored row multiplied": "ce_bwd_rows-f32-v1030",
    "scores include the last position": "answer_scores-f32-v37-u2",
    "scores use ids[u]": "answer_scores-bf16-v1030-u65",
    "segment of i - 1": "adamw-f32-s64-n19203-b0-gs0.25-shadow",
    "vector path across a segment end": "adamw-f32-odd-n5002-b0-gs0.5-shadow",
    "wd before the update": "adamw-f32-odd-n1027-b4-gs0.25-shadow",
    "gscale dropped": "adamw-f32-one-n3001-b516-gs0.5",
    "begin rounded down to 1024": "adamw-f32-s64pad-n19203-b2052-gs1-shadow",
    "seg_skip ignored": "adamw-blocks-s64-n19203-b2052-gs1-shadow-blk7_2_18_11_3-skip6",
    "grad_origin ignored": "adamw-bf16-one-n4099-b1000-gs0.5-shadow-o1000",
    "cast truncates": "cast-f32-bf16-n5",
    "cast tail off by one": "cast-bf16-f32-n1025",
    "vl_split sites swapped": "vl_split-f32-3x5x7x12-p0.5",
    "vl_split mask index from the d_enc row": "vl_split-bf16-2x36x20x260-p0.5",
})
RUN.update({
    "ignored row multiplied": lambda be: X.check_ce_bwd_rows(be, "f32", 1030),
    "scores include the last position": lambda be: X.check_answer_scores(be, "f32", 37, 2),
    "scores use ids[u]": lambda be: X.check_answer_scores(be, "bf16", 1030, 65),
    "cast truncates": lambda be: X.check_cast(be, "f32", "bf16", 5),
    "cast tail off by one": lambda be: X.check_cast(be, "bf16", "f32", 1025),
    "vl_split sites swapped": lambda be: X.check_vl_split(be, "f32", (3, 5, 7, 12), 0.5),
    "vl_split mask index from the d_enc row": lambda be: X.check_vl_split(be, "bf16", (2, 36, 20, 260), 0.5),
})
RUN.update(dict((k, _adam(v)) for k, v in DEFECTS.items() if v.startswith("adamw-")))


def test_every_defect_has_a_case():
    assert sorted(DEFECTS) == sorted(RUN) and len(DEFECTS) == 20


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_fails_its_named_case(defect):
    RUN[defect](BE)                                          # the case passes on the stand-in ...
    with pytest.raises(AssertionError) as e:                 # ... and fails on the wrong one, under its own name
        RUN[defect](Torch(defect))
    assert DEFECTS[defect] in str(e.value), "%s failed another case: %s" % (defect, str(e.value)[:300])
