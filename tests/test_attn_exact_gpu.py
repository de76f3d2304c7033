"""Exact layer of the attention tests on a real MI355X (tests/exact_attn.py): every route of
gstvd_attn_fwd / gstvd_attn_bwd through ops.attn_fwd / ops.attn_bwd only.  Every launch names the kernels it expects (the library
is asked: ops.attn_kernel_symbol) and runs on canary / NaN-poisoned windows with padded leading dimensions.  One-hot attention
(C), the power-of-two part of uniform attention (D), the invariances (E), the recovered dropout masks (F), uniform attention on
disjoint Q / K columns (H: a nonzero dK) and subset attention (I: ties, P = 2^-j) are compared bit for bit; the only tolerances
are test_ops_gpu.py's tol (restated as exact_attn.TOL), one ulp of the output type, the derived bound of the fully masked row
(G) and, for the graded rows that walk the online-softmax rescale (J), exact_attn.J_K x the first-order rounding bound of
exact_attn.tent_bounds, element by element.  The harness itself is proved on the CPU by tests/test_exact_attn_harness_cpu.py.

Premises of C and D that only the hardware can confirm -- __expf(0) == 1, __expf(x) == 0 for x <= -104, __logf(1) == 0, forward
and backward score expressions rounding alike, __expf(-__logf(2^k)) == 2^-k -- are what these tests assert on every case; see
the docstrings of check_onehot / check_uniform."""
import pytest
import torch

import exact_attn as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
SITE = 29


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    """The backend of exact_attn's checks: the HIP kernels, through ops.attn_desc / attn_fwd / attn_bwd."""

    def __init__(self):
        self.device = torch.device(DEV, torch.cuda.current_device())
        self.rng = ops().Rng(self.device, seed=77)

    def run(self, p):
        o, c = ops(), p.c
        a = o.attn_desc(p._Q, p._K, p._V, p._O, p.t("LSE"), p.km, c.B, c.nh, c.Lq, c.Lk, c.d, causal=c.causal, mask_neg=c.neg,
                        scale=p.scale_arg, drop_p=c.p, site=SITE, rng=self.rng, ldq=p.ld_in, ldk=p.ld_kv, ldv=p.ld_kv, ldo=p.ld_o, kv_group=c.kv_group,
                        kv_bstride=c.kv_bstride, drop_bits=p.bits)
        sym = o.attn_kernel_symbol(a, False)
        assert c.fwd_kernel in sym, "%s: forward would launch %s, the case expects %s" % (c.id, sym, c.fwd_kernel)
        o.attn_fwd(a)
        if c.bwd is None:
            return
        args = (a, p._dO, p._dQ, p._dK, p._dV, p.t("delta"))
        kw = dict(lddo=p.ld_do, lddq=p.ld_dq, lddk=p.ld_dkv, lddv=p.ld_dkv)
        if c.bwd == "refuse":
            with pytest.raises(Exception, match="GSTVD_E_UNSUPPORTED"):
                o.attn_bwd(*args, **kw)
            with pytest.raises(Exception, match="GSTVD_E_UNSUPPORTED"):
                o.attn_kernel_symbol(a, True)
            return
        o.attn_bwd(*args, **kw)
        sym = o.attn_kernel_symbol(a, True)
        want = c.bwd_kernel + ("" if c.dq_first is None else " dq_first=%d" % c.dq_first)
        assert c.bwd_kernel in sym and (sym.endswith(" dq_first=%d" % c.dq_first) if c.dq_first is not None else "dq_first" not in sym), \
            "%s: backward launched %s, the case expects %s" % (c.id, sym, want)

    def keep(self, p):
        c = p.c
        Lkp = A.round4(c.Lk)
        m = ops().dropout_mask(c.B * c.nh * c.Lq * Lkp, c.p, SITE, self.rng, self.device)
        assert bool(((m == 0) | (m == 2)).all())                 # p = 0.5: the factor is exactly 2
        return m.view(c.B, c.nh, c.Lq, Lkp)[..., :c.Lk] != 0


def ids(cs):
    return [c.id for c in cs]


# ------------------------------------------------------------------------------------------ A. census
def test_census_every_attention_kernel_of_the_library_is_named_by_a_case_or_exempt():
    """Lists the attention kernel instantiations the built library carries and the cases that reach each (run with -s).  Every
    launch of this file asserts that the kernel its case names is the one the library's route decision picks."""
    A.check_census(E_symbols())


def E_symbols():
    return A.E.library_kernels(A.lib_path(), A.ATTN_KERNEL_RE)


def test_backward_refuses_shared_keys_and_batch_strides():
    be = Gpu()
    cs = [c for c in A.CASES if c.bwd == "refuse"]
    assert len(cs) == 6
    for c in cs:
        A.check_onehot(be, c, 1)


# ------------------------------------------------------------------------------------------ C, D: every case of the table
RUNNABLE = [c for c in A.CASES if c.bwd != "refuse"]


@pytest.mark.parametrize("c", RUNNABLE, ids=ids(RUNNABLE))
def test_onehot_attention_is_bit_exact(c):
    A.check_onehot(Gpu(), c, A.CASES.index(c))


@pytest.mark.parametrize("c", RUNNABLE, ids=ids(RUNNABLE))
def test_uniform_attention_counts_every_allowed_key_once(c):
    A.check_uniform(Gpu(), c, A.CASES.index(c), out=print)


def test_uniform_attention_has_bit_exact_backward_cases_in_both_types():
    """The constructions of check_uniform are not vacuous: the table holds bit-exact backward cases in fp32 and in bf16 mode."""
    be = Gpu()
    for dt in ("f32", "bf16"):
        c = next(c for c in RUNNABLE if c.dtype == dt and c.d == 64 and c.has_bwd and not c.causal and c.p == 0 and c.Lk == 17)
        assert A.check_uniform(be, c, 0) == "exact", c.id


# ------------------------------------------------------------------------------------------ H, I, J
H_CASES = [c for c in RUNNABLE if c.has_bwd]
ONEPASS_BORDERS = [c for c in RUNNABLE if c.dtype == "bf16" and c.d == 64 and not c.causal and c.has_bwd and c.p > 0 and not c.fused and c.nh <= 2
                   and ((c.Lk in (64, 65, 256, 257) and c.Lq in (64, 100)) or (c.Lq in (63, 64) and c.Lk == 200))]
I_CASES = A.first_per_kernel(RUNNABLE, per=2)
I_CASES += [c for c in ONEPASS_BORDERS + [c for c in RUNNABLE if c.nh > 2] if c not in I_CASES]
J_CASES = [c for c in RUNNABLE if A.tent_case(c)]


@pytest.mark.parametrize("c", H_CASES, ids=ids(H_CASES))
def test_uniform_attention_on_disjoint_columns_has_an_exact_nonzero_dk(c):
    A.check_uniform_dk(Gpu(), c, A.CASES.index(c), out=print)


@pytest.mark.parametrize("c", I_CASES, ids=ids(I_CASES))
def test_subset_attention_is_bit_exact_with_ties(c):
    A.check_subset(Gpu(), c, A.CASES.index(c), out=print)


@pytest.mark.parametrize("c", J_CASES, ids=ids(J_CASES))
def test_graded_rows_through_the_softmax_rescale_stay_inside_the_rounding_bound(c):
    A.check_tent(Gpu(), c, A.CASES.index(c), out=print)


def test_disjoint_columns_and_subsets_reach_a_bit_exact_dk_in_both_types():
    """The constructions of H and I are not vacuous: a nonzero dK is compared bit for bit in fp32 and in bf16 mode."""
    be = Gpu()
    for dt in ("f32", "bf16"):
        c = next(c for c in RUNNABLE if c.dtype == dt and c.d == 64 and c.has_bwd and not c.causal and c.p == 0 and c.Lk == 17)
        assert A.check_uniform_dk(be, c, 0) == "exact", c.id
        assert A.check_subset(be, c, 0) == "exact", c.id


# ------------------------------------------------------------------------------------------ E. invariances
E_ALL = A.first_per_kernel(RUNNABLE, lambda c: c.has_bwd and c.Lq > 1 and c.Lk > 16) + A.first_per_kernel(RUNNABLE, lambda c: c.fwd == "decode" and c.Lk > 16)
E_NODROP = A.first_per_kernel(RUNNABLE, lambda c: c.p == 0 and c.Lk > 16 and c.kv_group == 1 and c.Lk % 64 not in (0, 63) and not c.fused)
E_CAUSAL = A.first_per_kernel(RUNNABLE, lambda c: c.causal and c.Lq > 8)
E_BITS = [c for c in RUNNABLE if c.bits and c.B * c.nh * c.Lq <= 4096]


@pytest.mark.parametrize("c", E_ALL, ids=ids(E_ALL))
def test_key_mask_none_equals_all_ones(c):
    A.check_mask_none_vs_ones(Gpu(), c, A.CASES.index(c))


@pytest.mark.parametrize("c", E_ALL, ids=ids(E_ALL))
def test_masked_keys_contribute_nothing_whatever_their_rows_hold(c):
    A.check_masked_rows_do_not_matter(Gpu(), c, A.CASES.index(c))


@pytest.mark.parametrize("c", E_CAUSAL, ids=ids(E_CAUSAL))
def test_causal_queries_do_not_depend_on_later_keys(c):
    A.check_causal_later_keys(Gpu(), c, A.CASES.index(c))


@pytest.mark.parametrize("c", E_NODROP, ids=ids(E_NODROP))
def test_appended_masked_keys_change_nothing(c):
    A.check_appended_masked_keys(Gpu(), c, 1 if c.Lk % 2 else 2, A.CASES.index(c))


@pytest.mark.parametrize("c", E_NODROP, ids=ids(E_NODROP))
def test_permuting_batch_rows_and_heads_permutes_the_outputs(c):
    A.check_permutation(Gpu(), c, A.CASES.index(c))


@pytest.mark.parametrize("c", E_BITS, ids=ids(E_BITS))
def test_keep_bits_equal_hashed_draws_at_the_onepass_borders(c):
    A.check_keep_bits_vs_hash(Gpu(), c, A.CASES.index(c))


# ------------------------------------------------------------------------------------------ F. the dropout masks applied
def _f(dt, d, Lq, Lk, causal=False):
    one = dt == "bf16" and d == 64 and not causal and 64 < Lk <= 256 and 64 <= Lq <= 1024
    return A.case(dt, d, Lq, Lk, "tiled", "onepass" if one else A.two(Lq, Lk), causal=causal, p=0.5)


# E32 (bf16) and fp32 routes, d = 32 / 64 / 128, causal and not, odd Lk, Lk % 4 != 0, Lq and Lk on both sides of 64, a one-pass shape
F_CASES = [_f(dt, d, Lq, Lk, causal) for dt in ("bf16", "f32") for d, Lq, Lk, causal in
           [(32, 65, 63, False), (32, 37, 67, True), (64, 63, 65, False), (64, 70, 70, True), (64, 64, 130, False),
            (128, 66, 61, False), (128, 61, 66, True)]]


@pytest.mark.parametrize("c", F_CASES, ids=ids(F_CASES))
def test_every_consumer_applies_the_draws_of_the_mask_probe(c):
    A.check_dropout_masks(Gpu(), c, F_CASES.index(c))


# ------------------------------------------------------------------------------------------ G. a fully masked row
G_CASES = A.first_per_kernel(RUNNABLE, lambda c: c.B >= 2 and c.kv_group == 1 and c.neg == -10000.0 and c.p == 0 and c.Lk > 16) + \
          A.first_per_kernel(RUNNABLE, lambda c: c.B >= 2 and c.kv_group == 1 and c.neg == -10000.0 and c.p > 0 and c.Lk > 16 and c.Lq > 1)
G_CASES_1E9 = A.first_per_kernel(RUNNABLE, lambda c: c.B >= 2 and c.kv_group == 1 and c.neg < -1e8 and c.p == 0 and c.Lk > 16)


@pytest.mark.parametrize("c", G_CASES, ids=ids(G_CASES))
def test_a_fully_masked_row_is_the_softmax_of_the_raw_scores(c):
    A.check_all_masked_row(Gpu(), c, A.CASES.index(c), out=print)


@pytest.mark.parametrize("c", G_CASES_1E9, ids=ids(G_CASES_1E9))
def test_a_fully_masked_row_under_minus_1e9_stays_finite_and_normalised(c):
    A.check_all_masked_row(Gpu(), c, A.CASES.index(c), out=print)
