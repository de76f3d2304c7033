"""Exact layer of the GEMM tests on a real MI355X (tests/exact_gemm.py): every route of the GEMM dispatch,
through ops.gemm / ops.GemmGroup only, with integer operands (outputs BIT-equal to a float64 reference, no tolerance), outputs
inside canary allocations (nothing outside the M x N windows may change) and inputs inside NaN-poisoned allocations (nothing
outside an operand may reach a result).  Each case names the kernel it expects; the census assertions keep a dispatch change
from silently moving a case onto another kernel.  GELU cases (erf is not exact arithmetic) keep the tolerance of
test_ops_gpu.py::test_gemm_gelu_epilogues and gain the canary / poison checks."""
import pytest
import torch

import exact_gemm as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
GELU_TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2}       # test_ops_gpu.py: tol(dtype), unchanged

# Kernels of the library that no case of the table names, each with its reason and the test that covers it.  None of them is
# reachable through gstvd_gemm, gstvd_gemm_splitk or gstvd_gemm_grouped.
EXEMPT = {
    "gemm_pc256_grouped_adamw_kernel": "own entry point (gstvd_gemm_grouped_adamw), AdamW epilogue is not exact arithmetic: "
                                       "test_fused_update_gpu.py (identity with the unfused path, which this file anchors)",
}
# the grouped launch: (a_km, b_km) x output type, named like the single launches' kernels
GROUPED = [(lay, out) for lay in ("tn", "nt", "nn") for out in ("f32", "bf16")]


def grouped_kernel(lay, out):
    return "gemm_pc256_grouped_kernelI%s%s" % (E._OT[out], E._lb(lay))


def check_census(symbols):
    """Every GEMM kernel instantiation of the built library is named by exactly one kernel name of the tables, or is exempt.
    The LayerNorm-folded kernels (gemm_rows_kernel, gemv16_ln_kernel: own entry points) are named by the table of
    tests/exact_lnfold.py and run by tests/test_lnfold_exact_gpu.py."""
    import exact_lnfold
    folded = exact_lnfold.kernel_names()
    assert len(folded) == 18
    named = sorted(set(c.kernel for c in E.CASES) | set(grouped_kernel(*g) for g in GROUPED) | set(folded))
    reached, lines = set(), []
    for s in symbols:
        hits = [n for n in named if n in s]
        ex = [e for e in EXEMPT if ("%d%s" % (len(e), e)) in s]
        assert len(hits) + len(ex) == 1, "%s: named by %r, exempt as %r" % (s, hits, ex)
        reached.update(hits)
        n = sum(1 for c in E.CASES if c.kernel in s)
        nf = [c.id for c in exact_lnfold.CASES if c.kernel in s]
        lines.append("%-100s %s" % (s, ("%d case(s), e.g. %s" % (n, next(c.id for c in E.CASES if c.kernel in s))) if n
                                    else ("%d case(s) of exact_lnfold, e.g. %s" % (len(nf), nf[0])) if nf
                                    else ("grouped launch" if hits else "EXEMPT: " + EXEMPT[ex[0]])))
    print("\n".join(lines))
    assert reached == set(named), "kernels named by a case but absent from the library: %r" % sorted(set(named) - reached)
    assert len(symbols) >= len(named)


def ops():
    from gst_visdial_amd import ops as o
    return o


def launched(prof):
    """The mangled symbols of the GEMM launches ops.Profiler recorded."""
    return [r[0][5:] for r in prof.records if r[0].startswith("gemm:")]


# ------------------------------------------------------------------------------------------ single launches
@pytest.mark.parametrize("c", E.CASES, ids=lambda c: c.id)
def test_gemm_exact(c):
    o = ops()
    dev = torch.device(DEV, torch.cuda.current_device())
    a_km, b_km = E.LAYOUTS[c.lay]
    splits = o.splitk_plan(o.BF16 if c.inp == "bf16" else o.F32, c.M, c.N, c.K, c.batch, a_km, b_km)
    assert splits == (c.splits or 1), "ops.splitk_plan: %d splits, the case expects %s" % (splits, c.splits)
    p = E.Problem(c, 1000 + E.CASES.index(c), dev)
    kw = p.gemm_kwargs()
    rng, site = None, 11 + E.CASES.index(c)
    if c.drop:
        rng = o.Rng(dev, seed=77)
        kw.update(drop_p=0.5, site=site, rng=rng)
    with o.Profiler() as prof:
        o.gemm(p.A.view, p.B.view, p.C.view, c.M, c.N, c.K, epi=o.EPI_GELU if c.epi == "gelu" else (o.EPI_DGELU if c.epi == "dgelu" else 0), **kw)
    # route census: the dispatch really sent this descriptor to the kernel the case names
    syms = launched(prof)
    assert len(syms) == 1 and c.kernel in syms[0], "launched %r, the case expects %s" % (syms, c.kernel)
    mask = None
    if c.drop:
        mask = o.dropout_mask(c.batch * c.M * c.N, 0.5, site, rng, dev).view(p.C.view.shape)
        assert bool(((mask == 0) | (mask == 2)).all())          # p = 0.5: the scale is exactly 2
    ref, peak = p.expected(mask)
    E.assert_exact_range(peak, c.id)
    if c.epi == "gelu":
        u = ref.float().requires_grad_(True)
        a = torch.nn.functional.gelu(u)
        a.backward(torch.ones_like(a))
        E.assert_close_rel_to_max(p.C.view, a.detach(), GELU_TOL[p.C.dtype], c.id + ": gelu")
        E.assert_close_rel_to_max(p.aux.view, u.grad, GELU_TOL[p.aux.dtype], c.id + ": gelu'")
    else:
        E.assert_bit_equal(p.C.view, ref, c.id)
    p.assert_surroundings(c.id)
    if splits > 1:
        E.assert_counters_zero(o._splitk_scratch(dev), c.id)


def test_census_every_gemm_kernel_of_the_library_is_named_by_a_case_or_exempt():
    """Lists the GEMM kernel instantiations the built library carries and the case that reaches each (run with -s to see it).
    test_gemm_exact / test_grouped_* assert per case that the named kernel is the launched one."""
    assert set(EXEMPT) <= {"gemm_pc256_grouped_adamw_kernel"}
    check_census(E.library_gemm_kernels(E.lib_path()))


# ------------------------------------------------------------------------------------------ grouped launch
# (rows, M, N, accumulate, column sums): dW[M, N] (+)= dy[rows, M]^T x[rows, N]; below / at / across the 256 tile in M and N,
# row counts 1, 77 and 4096, one accumulating into an integer dW, column sums in both forms, one problem without them
WGRAD = [(4096, 128, 256, False, "set"), (77, 256, 520, True, "acc"), (1, 264, 32, False, "set"), (333, 304, 136, False, None),
         (4096, 512, 264, False, "acc"), (77, 8, 8, True, None)]


def wgrad_problems(dev, out=torch.float32, seed=5):
    gen = E.generator(seed, dev)
    probs = []
    for i, (rows, M, N, acc, cs) in enumerate(WGRAD):
        dy = E.Window(rows, M, E.BF16, dev, "poison", ld=M + 8 * (i % 3)).set(E.integers((rows, M), E.A_RANGE, gen, E.BF16, dev))
        x = E.Window(rows, N, E.BF16, dev, "poison", ld=N + 8 * ((i + 1) % 3)).set(E.integers((rows, N), E.A_RANGE, gen, E.BF16, dev))
        dw = E.Window(M, N, out, dev, "canary", ld=N + 4 * (i % 4))
        ref = dy.view.double().t() @ x.view.double()
        if acc:
            dw.set(E.integers((M, N), E.E_RANGE, gen, out, dev))
            ref = ref + dw.view.double()
        gb = gb_ref = None
        if cs is not None:
            gb = E.Window(1, M, E.F32, dev, "canary")
            gb_ref = dy.view.double().sum(0)
            if cs == "acc":
                gb.set(E.integers((M,), E.E_RANGE, gen, E.F32, dev))
                gb_ref = gb_ref + gb.vector().double()
        probs.append(dict(dy=dy, x=x, dw=dw, ref=ref, gb=gb, gb_ref=gb_ref, rows=rows, M=M, N=N, acc=acc, cs=cs))
    return probs


def run_wgrad_group(o, dev, probs):
    grp = o.GemmGroup(dev, a_km=True, b_km=True)
    for q in probs:
        assert grp.colsum_capable(q["dy"].view)
        if q["cs"] is None:
            grp.add(q["dy"].view, q["x"].view, q["dw"].view, q["M"], q["N"], q["rows"], q["acc"])
        else:
            grp.add(q["dy"].view, q["x"].view, q["dw"].view, q["M"], q["N"], q["rows"], q["acc"], colsum_out=q["gb"].vector(),
                    colsum_acc=(q["cs"] == "acc"))
    with o.Profiler() as prof:
        grp.flush()
    return launched(prof)


def check_wgrad(probs, name):
    for i, q in enumerate(probs):
        tag = "%s: problem %d (%d rows, %d x %d)" % (name, i, q["rows"], q["M"], q["N"])
        E.assert_exact_range(q["ref"].abs().max().item() + 16, tag)
        E.assert_bit_equal(q["dw"].view, q["ref"], tag)
        for w in ("dy", "x", "dw", "gb"):
            if q[w] is not None:
                q[w].assert_surroundings_untouched(tag + ": " + w)
        if q["gb"] is not None:
            E.assert_bit_equal(q["gb"].vector(), q["gb_ref"], tag + ": column sums")


@pytest.mark.parametrize("order", [0, 3])
def test_grouped_weight_gradients_exact(order, monkeypatch):
    """GemmGroup(a_km=True, b_km=True).flush() under both tile orders (ops.GROUP_ORDER 0: the library's chunked order, 3: the
    host's per-XCD block map): dW and the column sums are bit-equal to the exact reference, hence to each other."""
    o = ops()
    dev = torch.device(DEV, torch.cuda.current_device())
    monkeypatch.setattr(o, "GROUP_ORDER", order)
    monkeypatch.setattr(o, "GROUP_ORDER_MIN_TILES", 0)
    probs = wgrad_problems(dev)
    syms = run_wgrad_group(o, dev, probs)
    assert len(syms) == 1 and grouped_kernel("tn", "f32") in syms[0], syms
    check_wgrad(probs, "order %d" % order)


@pytest.mark.parametrize("lay,out", GROUPED, ids=["%s-%s" % g for g in GROUPED])
def test_grouped_launch_every_layout_and_output_type_exact(lay, out):
    """Every instantiation gstvd_gemm_grouped can reach (three layouts, fp32 and bf16 output), accumulating problems included."""
    o = ops()
    dev = torch.device(DEV, torch.cuda.current_device())
    a_km, b_km = E.LAYOUTS[lay]
    ot = E.F32 if out == "f32" else E.BF16
    gen = E.generator(31, dev)
    grp = o.GemmGroup(dev, a_km=a_km, b_km=b_km)
    probs = []
    for i, (M, N, K, acc) in enumerate([(128, 256, 72, False), (264, 520, 1032, True), (8, 8, 8, False), (304, 136, 3072, False)]):
        ar, ac = (K, M) if a_km else (M, K)
        br, bc = (K, N) if b_km else (N, K)
        A = E.Window(ar, ac, E.BF16, dev, "poison", ld=ac + 8 * (i % 2)).set(E.integers((ar, ac), E.A_RANGE, gen, E.BF16, dev))
        B = E.Window(br, bc, E.BF16, dev, "poison", ld=bc + 8 * ((i + 1) % 2)).set(E.integers((br, bc), E.A_RANGE, gen, E.BF16, dev))
        Cw = E.Window(M, N, ot, dev, "canary", ld=N + (8 if i == 1 else 4 * (i % 2)))
        prior = None
        if acc:
            Cw.set(E.integers((M, N), E.E_RANGE, gen, ot, dev))
            prior = Cw.view.clone()
        ref, peak = E.reference(A.view, B.view, a_km, b_km, addend=prior)
        grp.add(A.view, B.view, Cw.view, M, N, K, acc)
        probs.append((A, B, Cw, ref, peak))
    with o.Profiler() as prof:
        grp.flush()
    syms = launched(prof)
    assert len(syms) == 1 and grouped_kernel(lay, out) in syms[0], syms
    for i, (A, B, Cw, ref, peak) in enumerate(probs):
        tag = "grouped %s %s: problem %d" % (lay, out, i)
        E.assert_exact_range(peak, tag)
        E.assert_bit_equal(Cw.view, ref, tag)
        for n, w in (("A", A), ("B", B), ("C", Cw)):
            w.assert_surroundings_untouched(tag + ": " + n)


def test_grouped_flush_direct_bf16_exact():
    """flush_direct_bf16: the ranges it reports as written in bf16 hold the round-to-nearest-even image of the exact dW, the fp32
    buffer under them is untouched, and the problems that stay fp32 (accumulating, or with a padded leading dimension) are exact
    fp32; nothing else of either buffer changes."""
    o = ops()
    dev = torch.device(DEV, torch.cuda.current_device())
    gen = E.generator(41, dev)
    # (rows, M, N, offset in the flat gradient buffer, ldc, accumulate)
    plan = [(333, 128, 256, 64, 256, False), (77, 264, 136, 40000, 136, True), (4096, 304, 520, 80000, 520, False),
            (1, 8, 72, 240008, 80, False)]
    total = 241000
    G = torch.empty(total, dtype=E.F32, device=dev)
    Gb = torch.empty(total, dtype=E.BF16, device=dev)
    G.view(torch.int32).fill_(E.CANARY[E.F32])
    Gb.view(torch.int16).fill_(E.CANARY[E.BF16])
    in_f32 = torch.zeros(total, dtype=torch.bool, device=dev)
    in_bf16 = torch.zeros(total, dtype=torch.bool, device=dev)
    grp = o.GemmGroup(dev, a_km=True, b_km=True)
    items, expect_ranges = [], []
    for rows, M, N, off, ldc, acc in plan:
        assert off % 8 == 0
        dy = E.Window(rows, M, E.BF16, dev, "poison", ld=M + 8).set(E.integers((rows, M), E.A_RANGE, gen, E.BF16, dev))
        x = E.Window(rows, N, E.BF16, dev, "poison", ld=N + 16).set(E.integers((rows, N), E.A_RANGE, gen, E.BF16, dev))
        dw = torch.as_strided(G, (M, N), (ldc, 1), off)
        ref = dy.view.double().t() @ x.view.double()
        if acc:
            dw.copy_(E.integers((M, N), E.E_RANGE, gen, E.F32, dev))
            ref = ref + dw.double()
        direct = not acc and ldc == N
        torch.as_strided(in_bf16 if direct else in_f32, (M, N), (ldc, 1), off).fill_(True)
        if direct:
            expect_ranges.append((off, M * N))
        grp.add(dy.view, x.view, dw, M, N, rows, acc)
        items.append((dy, x, dw, torch.as_strided(Gb, (M, N), (ldc, 1), off), ref, direct))
    with o.Profiler() as prof:
        ranges = grp.flush_direct_bf16(G, Gb)
    assert ranges == tuple(sorted(expect_ranges))
    syms = launched(prof)
    assert len(syms) == 2 and grouped_kernel("tn", "f32") in syms[0] and grouped_kernel("tn", "bf16") in syms[1], syms
    for i, (dy, x, dw, dwb, ref, direct) in enumerate(items):
        tag = "flush_direct_bf16: problem %d" % i
        E.assert_exact_range(ref.abs().max().item() + 16, tag)
        E.assert_bit_equal(dwb if direct else dw, ref, tag)
        dy.assert_surroundings_untouched(tag + ": dy")
        x.assert_surroundings_untouched(tag + ": x")
    # the fp32 buffer outside the fp32 problems (under the bf16 ranges included) and the bf16 buffer outside the bf16 ranges
    assert bool((G.view(torch.int32)[~in_f32] == E.CANARY[E.F32]).all()), "fp32 gradient buffer written outside the fp32 problems"
    assert bool((Gb.view(torch.int16)[~in_bf16] == E.CANARY[E.BF16]).all()), "bf16 payload written outside the reported ranges"
