"""Exact layer of the attention-map tests on a real MI355X (tests/exact_attn_maps.py): gstvd_attn_probs through ops.attn_desc /
ops.attn_probs only, with V, O, LSE and the RNG left out of the descriptor.  P sits in a canary window and is NaN before every
launch.  One-hot maps, the uniform maps' equalities, the invariances and the head-mean rule are compared bit for bit; the only
tolerance is the derived (Lk + 8) * 2^-24 of the integer-score family (1.8e-5 at 293 keys, exact_attn.TOL[F32]).  The checks
themselves are proved on the CPU against a torch stand-in by tests/test_attn_maps_cpu.py."""
import re

import pytest
import torch

import exact_attn_maps as M

pytestmark = pytest.mark.gpu

PMAP_KERNEL_RE = re.compile(rb"_Z\d+pmap_kernel\w*")
_TY = {"bf16": "DF16b", "f32": "f"}


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    """The backend of exact_attn_maps' checks: the HIP kernel.  The descriptor carries no V, O, LSE or RNG."""

    def __init__(self):
        self.device = torch.device("cuda", torch.cuda.current_device())

    def run(self, p, scale=None, drop_p=0.0, q_bstride=0, kv_bstride=0):
        o, c = ops(), p.c
        a = o.attn_desc(p.Q, p.K, None, None, None, p.km, c.B, c.nh, c.Lq, c.Lk, c.d, causal=c.causal, mask_neg=c.neg, scale=scale,
                        drop_p=drop_p, ldq=p.ldq, ldk=p.ldk, ldv=0, ldo=0, kv_group=c.kv_group, q_bstride=q_bstride, kv_bstride=kv_bstride)
        o.attn_probs(a, p.P, head_mean=c.mean)


def ids(cs):
    return [c.id for c in cs]


def test_census_every_map_kernel_of_the_library_is_reached_by_a_case():
    syms = M.E.library_kernels(M.E.lib_path(), PMAP_KERNEL_RE)
    want = set("pmap_kernelI%sLi%dELb%dEE" % (_TY[c.dtype], c.d, int(c.mean)) for c in M.CASES)
    assert len(want) == 12
    for s in syms:
        assert sum(1 for w in want if w in s) == 1, "%s: no case reaches this instantiation" % s
    assert all(any(w in s for s in syms) for w in want), (sorted(want), syms)
    assert not any(M.A.ATTN_KERNEL_RE.search(s.encode()) for s in syms)      # (the census of tests/test_attn_exact_gpu.py does not see them)


@pytest.mark.parametrize("c", M.CASES, ids=ids(M.CASES))
def test_onehot_maps_are_bit_exact(c):
    M.check_onehot(Gpu(), c, M.CASES.index(c))


@pytest.mark.parametrize("c", M.CASES, ids=ids(M.CASES))
def test_uniform_maps_count_every_allowed_key_once(c):
    M.check_uniform(Gpu(), c, M.CASES.index(c))


@pytest.mark.parametrize("c", M.CASES, ids=ids(M.CASES))
def test_integer_scores_match_the_float64_softmax(c):
    M.check_integer_scores(Gpu(), c, M.CASES.index(c), out=print)


E_CASES = [c for i, c in enumerate(M.CASES) if c.Lk > 16 and (i % 3 == 0 or c.nh > 4 or c.fused or c.kv_group > 1 or c.causal)]


@pytest.mark.parametrize("c", E_CASES, ids=ids(E_CASES))
def test_invariances_hold_bit_for_bit(c):
    M.check_invariances(Gpu(), c, M.CASES.index(c))


R_CASES = [M.case(dt, d, 17, 70, mean=mean) for dt in ("bf16", "f32") for d, mean in ((32, False), (64, True), (128, False))]


@pytest.mark.parametrize("c", R_CASES, ids=ids(R_CASES))
def test_dropout_and_batch_strides_are_refused_and_nothing_is_written(c):
    def refused(fn):
        with pytest.raises(Exception, match="GSTVD_E_UNSUPPORTED"):
            fn()
    M.check_refusals(Gpu(), c, refused)
