"""Exact layer of the soft pseudo-label tests on a real MI355X (tests/exact_distill.py): csrc/distill.hip
through gst_visdial_amd.ops -- the teacher's top-K on integer rows (ids and logp bit-exact: borders of the loops, ties, rows with
fewer than K finite values), the student's backward on pointer rows (bit-exact), alpha == 0 against gstvd_ce_bwd bit for bit, forward
and backward at tau in {0.5, 2} on noise rows against float64, lse_tau at tau = 1 against gstvd_ce_fwd's lse bit for bit (the one
row log-sum-exp of csrc/ce_row.h under both of its pre-scales) -- every output in a canary window, every input in a poisoned one,
every launch repeated.  The harness itself is proved on the CPU by tests/test_exact_distill_harness_cpu.py; the premises of the
pointer rows (__expf(0) == 1, logf(1) == 0, __expf(x) == 0 for x <= -112) have their tests in tests/test_loss_exact_gpu.py."""
import pytest
import torch

import exact_distill as D
import exact_loss as X

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    def __init__(self):
        self.device = torch.device(DEV, torch.cuda.current_device())

    def ce_fwd(self, logits, labels, M, V, row_loss, lse, stats, ignore_index):
        ops().ce_fwd(logits, labels, M, V, row_loss, lse, stats, ignore_index=ignore_index)

    def ce_bwd(self, logits, labels, lse, stats, gscale, mean, M, V, dlogits, ignore_index):
        ops().ce_bwd(logits, labels, lse, stats, gscale, mean, M, V, dlogits, ignore_index=ignore_index)

    def topk_logp(self, logits, lse, M, V, K, ids, logp):
        ops().topk_logp(logits, lse, M, V, K, ids=ids, logp=logp)

    def distill_fwd(self, logits, labels, sid, slp, M, V, alpha, tau, ce_row_loss, row_loss, row_kd, lse_tau, stats, ignore_index):
        ops().distill_fwd(logits, labels, sid, slp, M, V, alpha, tau, ce_row_loss, row_loss, row_kd, lse_tau, stats, ignore_index=ignore_index)

    def distill_bwd(self, logits, labels, sid, slp, lse, lse_tau, stats, gscale, M, V, alpha, tau, dlogits, ignore_index):
        ops().distill_bwd(logits, labels, sid, slp, lse, lse_tau, stats, gscale, M, V, alpha, tau, dlogits, ignore_index=ignore_index)


@pytest.mark.parametrize("dtype,V,K", D.TOPK_CASES)
def test_topk_ids_and_logp_are_exact(dtype, V, K):
    D.check_topk(Gpu(), dtype, V, K)


@pytest.mark.parametrize("dtype,V,rot", D.BWD_CASES)
def test_pointer_rows_with_half_half_soft_labels_are_exact(dtype, V, rot):
    D.check_bwd_exact(Gpu(), dtype, V, rot)


@pytest.mark.parametrize("dtype,V", D.ALPHA0_CASES)
def test_alpha_zero_is_the_cross_entropy_bit_for_bit(dtype, V):
    D.check_alpha_zero(Gpu(), dtype, V)


@pytest.mark.parametrize("dtype,V,kind,tau", D.NOISE_CASES)
def test_noise_rows_against_float64(dtype, V, kind, tau):
    D.check_noise(Gpu(), dtype, V, kind, tau)


@pytest.mark.parametrize("dtype,V", D.LSE1_CASES)
def test_lse_tau_at_tau_one_is_the_cross_entropy_lse_bit_for_bit(dtype, V):
    D.check_lse_tau_one(Gpu(), dtype, V)


def test_refusals_come_before_any_launch():
    """K outside 1..16 or above V, alpha outside [0, 1], inv_tau not positive, ldl < V: GSTVD_E_SHAPE; V above 32768 for the top-K:
    GSTVD_E_UNSUPPORTED; a misaligned logits / dlogits pointer: GSTVD_E_ALIGN; a dtype that is neither: GSTVD_E_DTYPE.  Only return
    codes are read; the outputs keep their canary."""
    from gst_visdial_amd import _lib as Lb
    lib = Lb.load()
    dev = Gpu().device
    M, V, K = 3, 37, 4
    status = Lb.status_name
    for dt, align in ((X.F32, 16), (X.BF16, 8)):
        code = ops().dt(torch.empty(0, dtype=dt))
        es = torch.empty((), dtype=dt).element_size()
        lg = X.Window(M, V, dt, dev, "poison", ld=40)
        dl = X.win_out(M, 40, dt, dev)
        lab = torch.ones(M, dtype=torch.int64, device=dev)
        sid = torch.zeros(M, 16, dtype=torch.int64, device=dev)
        slp = torch.zeros(M, 16, dtype=torch.float32, device=dev)
        ids = X.win_out(M, 16, X.I64, dev)
        f = [X.win_out(1, n, X.F32, dev) for n in (M * 16, M, M, M, M, 3, M)]
        logp, rl, l, kd, lt, st, lse = f
        p = lambda w: w.view.data_ptr()

        def topk(lp=None, ldl=40, v=V, k=K, c=code):
            return status(lib.gstvd_topk_logp(p(lg) if lp is None else lp, ldl, p(lse), M, v, k, c, p(ids), p(logp), None))

        def fwd(lp=None, ldl=40, k=K, a=0.5, it=1.0, c=code):
            return status(lib.gstvd_distill_fwd(p(lg) if lp is None else lp, ldl, lab.data_ptr(), sid.data_ptr(), slp.data_ptr(), M, V, k, 0, a, it,
                                                c, p(rl), p(l), p(kd), p(lt), p(st), None))

        def bwd(lp=None, ldl=40, dp=None, ldd=40, k=K, a=0.5, it=1.0, c=code):
            return status(lib.gstvd_distill_bwd(p(lg) if lp is None else lp, ldl, lab.data_ptr(), sid.data_ptr(), slp.data_ptr(), p(lse), p(lt),
                                                p(st), None, M, V, k, 0, a, it, c, p(dl) if dp is None else dp, ldd, None))

        for k in (0, 17, -1):
            assert topk(k=k) == fwd(k=k) == bwd(k=k) == "GSTVD_E_SHAPE", k
        assert topk(v=3, ldl=4, k=4) == "GSTVD_E_SHAPE"                      # K > V
        assert topk(ldl=36) == fwd(ldl=36) == bwd(ldl=36) == bwd(ldd=36) == "GSTVD_E_SHAPE"
        assert topk(ldl=42) == fwd(ldl=42) == bwd(ldl=42) == bwd(ldd=42) == "GSTVD_E_SHAPE"
        for a in (-0.25, 1.5, float("nan")):
            assert fwd(a=a) == bwd(a=a) == "GSTVD_E_SHAPE", a
        for it in (0.0, -1.0, float("inf"), float("nan")):
            assert fwd(it=it) == bwd(it=it) == "GSTVD_E_SHAPE", it
        assert topk(v=32772, ldl=32772) == "GSTVD_E_UNSUPPORTED"
        assert topk(c=7) == fwd(c=7) == bwd(c=7) == "GSTVD_E_DTYPE"
        for off in range(es, align, es):
            assert topk(lp=p(lg) + off) == fwd(lp=p(lg) + off) == bwd(lp=p(lg) + off) == bwd(dp=p(dl) + off) == "GSTVD_E_ALIGN", (dt, off)
        torch.cuda.synchronize()
        for w in [dl, ids] + f[:6]:                                       # nothing was launched: every output still holds its canary
            assert bool((X.bits(w.flat) == X._canary(w.dtype)).all())


def test_case_count():
    n = D.case_count()
    print("cases: %s; total %d" % (", ".join("%s %d" % kv for kv in n.items()), sum(n.values())))
    assert sum(n.values()) == 92
