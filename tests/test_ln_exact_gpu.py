"""Exact layer of the LayerNorm tests on a real MI355X (tests/exact_ln.py): every route of gstvd_ln_fwd /
gstvd_ln_bwd, the column reductions and gstvd_locgrad, through ops.ln_fwd / ln_bwd / colsum* / ColsumBatch / locgrad only.  Every
launch names the kernel it expects (the library is asked: ops.ln_kernel_symbol) and runs on canary / NaN-poisoned windows with
padded leading dimensions; y, mean, rstd, dres, dx, the partial slabs, the column sums, the atomic-fed table gradients and dW_loc
are compared bit for bit with a float64 reference computed without eps.  The harness itself is proved on the CPU by
tests/test_exact_ln_harness_cpu.py.

Premises that only the hardware can confirm -- sqrtf(4^k + 1e-12) == 2^k and 1 / 2^k, S / H correctly rounded (so rstd == 2^-k,
mean == m, c1 and c2 multiples of 1/4 exactly) -- are what these tests assert on every case; see the docstring of exact_ln."""
import pytest
import torch

import exact_ln as X

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    """The backend of exact_ln's checks: the HIP kernels, through ops."""

    def __init__(self):
        self.device = torch.device(DEV, torch.cuda.current_device())
        self.rng = ops().Rng(self.device, seed=77)

    def keep(self, n, p, site):
        return ops().dropout_mask(n, p, site, self.rng, self.device)

    def blocks(self, M, H=None, mode=None):
        return ops().ln_bwd_blocks(M) if H is None else ops().ln_bwd_blocks(M, H, X.MODES[mode])

    def _kw(self, kw):
        o = ops()
        return dict(kw, mode=X.MODES[kw["mode"]], dtype=o.BF16 if kw["dtype"] == torch.bfloat16 else o.F32, rng=self.rng)

    def ln_fwd(self, kw, expect=None):
        o, k = ops(), self._kw(kw)
        if expect is not None:
            sym = o.ln_kernel_symbol(k)
            assert expect in sym, "forward would launch %s, the case expects %s" % (sym, expect)
        o.ln_fwd(**k)

    def ln_bwd(self, kw, bw, expect=None):
        o, k = ops(), self._kw(kw)
        if expect is not None:
            sym = o.ln_kernel_symbol(k, bw)
            assert expect in sym, "backward would launch %s, the case expects %s" % (sym, expect)
        o.ln_bwd(k, **bw)

    def colsum_partials(self, *a):
        ops().colsum_partials(*a)

    def colsum(self, *a):
        ops().colsum(*a)

    def colsum_slabs(self, *a):
        ops().colsum_slabs(*a)

    def batch(self):
        return ops().ColsumBatch(self.device)

    def locgrad(self, *a):
        ops().locgrad(*a)


def ids(cs):
    return [c.id for c in cs]


# ------------------------------------------------------------------------------------------ census
def test_census_every_layernorm_kernel_of_the_library_is_named_by_a_case_or_a_reduction_check():
    """Lists the ln_fwd_kernel / ln_bwd_kernel / colsum* / locgrad instantiations the built library carries and what reaches each
    (run with -s).  Every launch of this file asserts that the kernel its case names is the one the library's route decision picks."""
    X.check_census(X.E.library_kernels(X.lib_path(), X.LN_KERNEL_RE))


# ------------------------------------------------------------------------------------------ every case of the table
@pytest.mark.parametrize("c", X.CASES, ids=ids(X.CASES))
def test_layernorm_is_bit_exact_inside_its_windows(c):
    X.run_case(Gpu(), c, X.CASES.index(c))


def test_any_other_positive_nblk_is_refused():
    be, o = Gpu(), ops()
    for c in (X.case("resid", "f32", 2049, 256, nw=16, wide=True), X.case("image", "bf16", 37, 64)):
        p = X.Problem(be, c)
        p.build_backward()
        kw, bw = p.bwd_args()
        for nblk in (1, be.blocks(c.M) + 1, be.blocks(c.M, c.H, c.mode) - 1):
            with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
                o.ln_bwd(be._kw(kw), **dict(bw, nblk=nblk))
            with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
                o.ln_kernel_symbol(be._kw(kw), dict(bw, nblk=nblk))
        p.assert_surroundings()
        assert bool((p.t["partial"].view.view(torch.int32) == X.CANARY[torch.float32]).all())       # nothing was launched


def test_refusals():
    be, o = Gpu(), ops()
    p = X.Problem(be, X.case("resid", "f32", 5, 64))
    p.build_backward()
    kw, bw = p.bwd_args()
    for over in (dict(H=62), dict(H=2052), dict(M=0)):
        with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
            o.ln_fwd(**be._kw(p.fwd_kw(**over)))
        with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
            o.ln_bwd(be._kw(dict(kw, **over)), **bw)
        with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
            o.ln_kernel_symbol(be._kw(p.fwd_kw(**over)))
    q = X.Problem(be, X.case("embed", "f32", 0, 64, B=2, T=3))
    q.build_backward()
    kw, bw = q.bwd_args()
    for tab in ("word", "pos", "tt", "tt_ext"):
        with pytest.raises(Exception, match="GSTVD_E_NULL"):
            o.ln_fwd(**be._kw(q.fwd_kw(**{tab: None})))
        with pytest.raises(Exception, match="GSTVD_E_NULL"):
            o.ln_bwd(be._kw(kw), **dict(bw, **{"d" + tab: None}))
    x = torch.zeros(8, 8, device=be.device)
    out, scratch = torch.zeros(8, device=be.device), torch.zeros(64, device=be.device)
    for N in (6, 7):
        with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
            o.colsum(x, 8, N, out, scratch, False)
        with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
            o.colsum_slabs(x, 8, N, scratch)
    for pr in (p, q):
        pr.assert_surroundings()


# ------------------------------------------------------------------------------------------ invariances
def _pick(pred, n=1):
    return [c for c in X.CASES if pred(c)][:n]


INV = (_pick(lambda c: c.mode == "resid" and c.bwd and c.res and c.nw == 16 and c.p_pre > 0, 2) +
       _pick(lambda c: c.mode == "resid" and c.bwd and c.M == 13 and c.H in (260, 2048)) +
       _pick(lambda c: c.mode == "image" and c.bwd and c.M == 13 and c.H in (772, 1028), 2) +
       _pick(lambda c: c.mode == "embed" and c.bwd and c.M < 200 and c.H in (256, 2048), 4))
REPRO = _pick(lambda c: c.mode == "embed" and c.bwd and c.M < 5000, 40)
PERM = [X.case("embed", dt, 0, H, B=B, T=T, pos_offset=po, carrier=car) for dt in ("f32", "bf16")
        for H, B, T, po, car in ((64, 3, 24, 0, "word"), (768, 8, 5, 7, "pos"), (1024, 8, 5, 0, "tt"), (2048, 4, 3, 1, "word"))]
ZERO = [X.case("embed", dt, 0, H, B=B, T=T, segs="zero", carrier=car) for dt in ("f32", "bf16")
        for H, B, T, car in ((260, 4, 3, "pos"), (1028, 3, 5, "tt"))]
ALIAS = [X.case("resid", dt, M, H, nw=nw, wide=nw == 16, p_post=pp) for dt in ("f32", "bf16")
         for M, H, nw, pp in ((9, 260, 4, 0.0), (2049, 768, 16, 0.5), (7, 2048, 4, 0.0))]


@pytest.mark.parametrize("c", INV, ids=ids(INV))
def test_rows_behind_m_and_pad_columns_of_the_inputs_do_not_matter(c):
    X.check_surroundings_do_not_matter(Gpu(), c, 3)


@pytest.mark.parametrize("c", REPRO, ids=ids(REPRO))
def test_atomic_fed_tables_are_the_same_bits_run_to_run(c):
    X.check_reproducible(Gpu(), c, 4)


@pytest.mark.parametrize("c", ZERO, ids=ids(ZERO))
def test_segs_none_equals_all_zero_segs(c):
    X.check_segs_none_equals_zeros(Gpu(), c, 5)


@pytest.mark.parametrize("c", PERM, ids=ids(PERM))
def test_permuting_the_batch_rows_of_an_embedding_input(c):
    X.check_batch_permutation(Gpu(), c, 6)


@pytest.mark.parametrize("c", ALIAS, ids=ids(ALIAS))
def test_dx_aliased_to_dres_at_p_zero(c):
    X.check_alias(Gpu(), c, 7)


# ------------------------------------------------------------------------------------------ reductions
# (28 .. 61: the loop with eight loads in flight, entered from nblk = 29 on, its tail, and the last count without it)
@pytest.mark.parametrize("nblk", [1, 3, 4, 5, 28, 29, 32, 33, 61])
def test_colsum_partials(nblk):
    be = Gpu()
    for nvec in (1, 2, 3):
        for acc in (False, True):
            for H in (4, 260):
                X.check_colsum_partials(be, nblk, nvec, H, acc, none_out=(nvec == 3 and not acc), seed=nblk)


def test_colsum_batch_one_flush_and_the_shared_output_reflush():
    X.check_colsum_batch(Gpu(), 1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_colsum_and_colsum_slabs(dtype):
    be = Gpu()
    for i, M in enumerate(X.COLSUM_M):
        for j, N in enumerate(X.COLSUM_N):
            X.check_colsum(be, dtype, M, N, (i + j) % 2 == 1, seed=i * 7 + j)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_colsum_final_stage_with_32_and_33_slabs(dtype):
    """The final stage of colsum runs the one-entry kernel: 32 / 33 slabs reach its loop with eight loads in flight and the tail."""
    be = Gpu()
    for i, nslab in enumerate((28, 29, 32, 33)):
        X.check_colsum(be, dtype, 64 * nslab, 8, i % 2 == 1, seed=nslab)
        X.check_colsum(be, dtype, 64 * nslab - 63, 8, i % 2 == 0, seed=nslab + 1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_add_slabs_entries_of_different_shape_in_one_launch(dtype):
    be = Gpu()
    X.check_add_slabs(be, dtype, [(63, 256), (333, 260)], 1)
    X.check_add_slabs(be, dtype, [(65, 2304), (1, 4), (64, 252), (333, 2304), (130, 260)], 2)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_locgrad(dtype):
    be = Gpu()
    for i, M in enumerate((1, 15, 16, 17, 400)):
        for j, H in enumerate((4, 256, 260, 1024)):
            for acc in (False, True):
                X.check_locgrad(be, dtype, M, H, acc, seed=i * 5 + j)
