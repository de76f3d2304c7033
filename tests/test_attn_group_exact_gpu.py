"""Exact layer of the grouped cross-attention backward on a real MI355X (tests/exact_attn_group.py): gstvd_attn_group_bwd through
ops.attn_desc / ops.attn_fwd / ops.attn_group_bwd only, on canary / NaN-poisoned windows with padded leading dimensions, K / V
and dK / dV also as column slices of a wide buffer.  dQ and delta are compared bit for bit with gstvd_attn_bwd's two-part kernel
on replicated K / V, dK and dV with a float64 reference at 4 x exact_attn.TOL and bit for bit between runs, against exact integer
sums (one-hot, uniform attention; uniform attention on disjoint Q / K columns for a nonzero dK) and against the draws the grouped forward applied.  The checks themselves are proved on the CPU
by tests/test_exact_attn_group_harness_cpu.py."""
import pytest
import torch

import exact_attn_group as X

A = X.A
pytestmark = pytest.mark.gpu

SITE = 31


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    """The backend of exact_attn_group's checks: the HIP kernels."""

    def __init__(self):
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.rng = ops().Rng(self.device, seed=78)

    def _desc(self, p, **over):
        o, c = ops(), p.c
        kw = dict(causal=c.causal, mask_neg=c.neg, scale=p.scale_arg, drop_p=c.p, site=SITE, rng=self.rng, ldq=p.ld_in, ldk=p.ld_kv, ldv=p.ld_kv, ldo=p.ld_o,
                  kv_group=c.kv_group, kv_bstride=c.kv_bstride)
        B = c.B - over.pop("B_minus", 0)
        kw.update(over)
        return o.attn_desc(p._Q, p._K, p._V, p._O, p.t("LSE"), p.km, B, c.nh, c.Lq, c.Lk, c.d, **kw)

    @staticmethod
    def _bwd_args(p, a, null=None):
        t = dict(dO=p._dO, dQ=p._dQ, dK=p._dK, dV=p._dV, delta=p.t("delta"))
        if null:
            t[null] = None
        return (a, t["dO"], t["dQ"], t["dK"], t["dV"], t["delta"]), dict(lddo=p.ld_do, lddq=p.ld_dq, lddk=p.ld_dkv, lddv=p.ld_dkv)

    def run(self, p):
        o = ops()
        a = self._desc(p)
        o.attn_fwd(a)
        args, kw = self._bwd_args(p, a)
        o.attn_group_bwd(*args, **kw)

    def run_plain(self, p):
        o = ops()
        assert p.c.kv_group == 1
        a = self._desc(p)
        o.attn_fwd(a)
        args, kw = self._bwd_args(p, a)
        o.attn_bwd(*args, **kw)
        sym = o.attn_kernel_symbol(a, True)
        assert "attn_bwd_kernel" in sym, "%s: the comparison ran %s, not the two-part kernel" % (p.c.id, sym)

    def keep(self, p):
        c = p.c
        Lkp = A.round4(c.Lk)
        m = ops().dropout_mask(c.B * c.nh * c.Lq * Lkp, c.p, SITE, self.rng, self.device)
        return m.view(c.B, c.nh, c.Lq, Lkp)[..., :c.Lk] != 0

    def refuse(self, p, null=None, **change):
        a = self._desc(p, **change)
        args, kw = self._bwd_args(p, a, null)
        with pytest.raises(Exception, match="GSTVD_E_NULL" if null else "GSTVD_E_UNSUPPORTED"):
            ops().attn_group_bwd(*args, **kw)


def ids(cs):
    return [c.id for c in cs]


EXACT = [c._replace(p=0.5 if c.p else 0.0) for c in X.CASES]       # the exact families: the dropout factor is 1 or 2
ONE = [c for c in X.CASES if c.kv_group == 1]
MASKED = [c for c in X.CASES if c.B // c.kv_group >= 2]
TYPES = [(dt, d) for dt in ("bf16", "f32") for d in (32, 64, 128)]
DRAWS = [X.case(dt, d, X.SHAPES[i % 2], p=0.5) for i, (dt, d) in enumerate(TYPES)] + \
        [X.case("bf16", 64, X.SHAPES[2], p=0.5), X.case("f32", 32, X.SHAPES[4], p=0.5)]
REFUSE = [X.case(dt, d, X.SHAPES[1]) for dt, d in TYPES]


def test_symbols_the_census_of_exact_attn_does_not_see_the_new_kernels_and_every_one_is_reached():
    syms = X.E.library_kernels(X.E.lib_path(), X.GROUP_KERNEL_RE)
    want = set(X.kernel_of(c) for c in X.CASES)
    assert len(want) == 6
    for s in syms:
        assert sum(1 for w in want if w in s) == 1, "%s: no case reaches this instantiation" % s
    assert all(any(w in s for s in syms) for w in want), (sorted(want), syms)
    assert not any(A.ATTN_KERNEL_RE.search(s.encode()) for s in syms)


@pytest.mark.parametrize("c", ONE, ids=ids(ONE))
def test_a_group_of_one_is_the_two_part_backward_bit_for_bit(c):
    X.check_group_of_one(Gpu(), c, X.CASES.index(c))


@pytest.mark.parametrize("c", X.CASES, ids=ids(X.CASES))
def test_dq_and_delta_equal_the_backward_on_replicated_keys_bit_for_bit(c):
    X.check_dq_matches_replicated(Gpu(), c, X.CASES.index(c))


@pytest.mark.parametrize("c", X.CASES, ids=ids(X.CASES))
def test_dk_dv_are_the_group_sums_deterministic_and_blind_to_zero_members(c):
    X.check_dkv(Gpu(), c, X.CASES.index(c), out=print)


@pytest.mark.parametrize("c", EXACT, ids=ids(EXACT))
def test_onehot_attention_sums_the_group_exactly(c):
    X.check_onehot(Gpu(), c, EXACT.index(c))


@pytest.mark.parametrize("c", EXACT, ids=ids(EXACT))
def test_uniform_attention_sums_the_group_exactly(c):
    X.check_uniform(Gpu(), c, EXACT.index(c))


@pytest.mark.parametrize("c", EXACT, ids=ids(EXACT))
def test_uniform_attention_on_disjoint_columns_sums_a_nonzero_dk_over_the_group_exactly(c):
    X.check_uniform_dk(Gpu(), c, EXACT.index(c), out=print)


def test_disjoint_columns_reach_a_bit_exact_grouped_dk_in_both_types():
    be = Gpu()
    for dt in ("f32", "bf16"):
        c = next(c for c in EXACT if c.dtype == dt and c.kv_group > 1 and c.p == 0 and c.Lk < 256 and c.Lq > 1)
        assert X.check_uniform_dk(be, c, EXACT.index(c)) == "exact", c.id


@pytest.mark.parametrize("c", MASKED, ids=ids(MASKED))
def test_a_fully_masked_key_row_is_the_softmax_of_the_raw_scores(c):
    X.check_all_masked_row(Gpu(), c, X.CASES.index(c), out=print)


@pytest.mark.parametrize("c", DRAWS, ids=ids(DRAWS))
def test_the_backward_applies_the_draws_of_the_grouped_forward(c):
    X.check_dropout_masks(Gpu(), c, DRAWS.index(c))


@pytest.mark.parametrize("c", REFUSE, ids=ids(REFUSE))
def test_unsupported_descriptors_are_refused_and_nothing_is_written(c):
    X.check_refusals(Gpu(), c, REFUSE.index(c))
