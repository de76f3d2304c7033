"""Exact layer of the loss and optimizer tests on a real MI355X (tests/exact_loss.py): csrc/loss.hip,
csrc/optim.hip and csrc/elementwise.hip through gst_visdial_amd.ops -- cross entropy forward / backward / per-row backward on pointer rows (bit-exact) and noise rows (float64
reference, the tolerances of tests/test_ops_gpu.py), answer_scores, AdamW's three entries on inputs every fp32 operation of which
is exact, the four casts, cast_ranges, vl_split -- every output in a canary window, every input in a poisoned one, every launch
repeated.  The harness itself is proved on the CPU by tests/test_exact_loss_harness_cpu.py.

Premises that only the hardware can confirm have a test each: __expf(0) == 1, logf(1) == 0, __expf(x) == 0 for x <= -112;
v_sqrt_f32 exact on 9 * 4^j, v_rcp_f32 exact on powers of two, powf(b, 1) == b."""
import pytest
import torch

import exact_loss as X

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    def __init__(self):
        self.device = torch.device(DEV, torch.cuda.current_device())
        self.rng = ops().Rng(self.device, seed=20240607)

    def ce_fwd(self, logits, labels, M, V, row_loss, lse, stats, ignore_index):
        ops().ce_fwd(logits, labels, M, V, row_loss, lse, stats, ignore_index=ignore_index)

    def ce_bwd(self, logits, labels, lse, stats, gscale, mean, M, V, dlogits, ignore_index):
        ops().ce_bwd(logits, labels, lse, stats, gscale, mean, M, V, dlogits, ignore_index=ignore_index)

    def ce_bwd_rows(self, logits, labels, lse, g, M, V, dlogits, ignore_index):
        ops().ce_bwd_rows(logits, labels, lse, g, M, V, dlogits, ignore_index=ignore_index)

    def answer_scores(self, logits, lse, dec_ids, rows, U, scores):
        ops().answer_scores(logits, lse, dec_ids, rows, U, scores)

    def cast(self, src, dst, n):
        ops().cast(src, dst, n)

    def cast_ranges(self, ranges, src, dst):
        ops().CastRanges(ranges, self.device).run(src, dst)

    def drop_mask(self, n, p, site):
        return ops().dropout_mask(n, p, site, self.rng, self.device)

    def vl_split(self, d_enc, B, R, T, H, d_v, d_t, p, site_v, site_t):
        ops().vl_split(d_enc, B, R, T, H, d_v, d_t, p, site_v, site_t, self.rng if p > 0 else None)

    def adamw(self, param, grad, m, v, shadow, seg_end, hp, step, b1, b2, eps, gscale, begin, end, origin):
        ops().adamw(param, grad, m, v, shadow, seg_end, hp, step, b1, b2, eps, gscale, begin=begin, end=end, grad_origin=origin)

    def adamw_blocks(self, param, grad, m, v, shadow, seg_end, hp, step, blocks, seg_skip, b1, b2, eps, gscale, begin, end):
        ops().adamw_blocks(param, grad, m, v, shadow, seg_end, hp, step, blocks, seg_skip, b1, b2, eps, gscale, begin=begin, end=end)


# ---------------------------------------------------------------------------------------------- premises
def test_premise_expf_of_zero_is_one():
    X.premise_expf_zero(Gpu())


def test_premise_expf_is_zero_from_minus_112_down():
    X.premise_expf_cold(Gpu())


def test_premise_logf_of_one_is_zero():
    X.premise_logf_one(Gpu())


def test_premise_rcp_is_exact_on_powers_of_two():
    X.premise_rcp_powers_of_two(Gpu())


def test_premise_sqrt_is_exact_on_nine_times_four_to_the_j():
    X.premise_sqrt_nine_times_four_to_j(Gpu())


def test_premise_powf_of_exponent_one_returns_the_base():
    X.premise_powf_one(Gpu())


# ---------------------------------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("c", X.CE_CASES, ids=[c.id for c in X.CE_CASES])
def test_pointer_rows_are_exact(c):
    X.run_ce_case(Gpu(), c)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", X.ROWS_V)
def test_per_row_backward_stores_zero_rows(dtype, V):
    X.check_ce_bwd_rows(Gpu(), dtype, V)


@pytest.mark.parametrize("dtype,V,U", X.SCORE_CASES)
def test_answer_scores_are_exact_integer_sums(dtype, V, U):
    X.check_answer_scores(Gpu(), dtype, V, U)


@pytest.mark.parametrize("dtype,V,kind", X.NOISE_CASES)
def test_noise_rows_against_float64(dtype, V, kind):
    X.check_ce_noise(Gpu(), dtype, V, kind)


@pytest.mark.parametrize("dtype,V", X.INVARIANCE_CASES)
def test_a_row_does_not_depend_on_its_neighbours_padding_or_strides(dtype, V):
    X.check_ce_invariances(Gpu(), dtype, V)


# ---------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("c", X.ADAM_CASES, ids=[c.id for c in X.ADAM_CASES])
def test_adamw_is_exact_per_segment(c):
    X.run_adam_case(Gpu(), c)


@pytest.mark.parametrize("t", X.NOISY_STEPS)
def test_adamw_noisy_update_term_per_element(t):
    X.check_adamw_noisy(Gpu(), t)


# ---------------------------------------------------------------------------------------------- casts, vl_split
@pytest.mark.parametrize("n", X.CAST_N)
@pytest.mark.parametrize("sdt,ddt", X.CAST_PAIRS)
def test_casts_round_to_nearest_even(sdt, ddt, n):
    X.check_cast(Gpu(), sdt, ddt, n)


def test_cast_of_fp32_denormals_rounds_or_flushes_to_a_zero_of_the_same_sign():
    rne, flushed = X.check_cast_denormals(Gpu())
    print("fp32 denormals to bf16: %d rounded to nearest even, %d flushed to a zero of their sign" % (rne, flushed))


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 0, 2, 1)])
def test_cast_ranges_keep_the_gaps(order):
    X.check_cast_ranges(Gpu(), order)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", X.VL_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_vl_split_is_slicing_times_the_masks_of_its_sites(dtype, shape, p):
    X.check_vl_split(Gpu(), dtype, shape, p)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_cross_entropy_entries_come_before_any_launch():
    """ldl < V: GSTVD_E_SHAPE; a logits / dlogits pointer off its vector alignment (16 bytes fp32, 8 bytes bf16): GSTVD_E_ALIGN.
    Only return codes are read; the outputs keep their canary."""
    from gst_visdial_amd import _lib as Lb
    lib, o = Lb.load(), ops()
    dev = Gpu().device
    M, V = 3, 37
    for dt, align in ((X.F32, 16), (X.BF16, 8)):
        code = o.dt(torch.empty(0, dtype=dt))
        es = torch.empty((), dtype=dt).element_size()
        lg = X.Window(M, V, dt, dev, "poison", ld=40)
        dl = X.win_out(M, 40, dt, dev)
        lab = torch.ones(M, dtype=torch.int64, device=dev)
        rl, lse, st, g = (X.win_out(1, n, X.F32, dev) for n in (M, M, 3, M))
        p = lambda w: w.view.data_ptr()
        status = Lb.status_name

        def fwd(lp, ldl):
            return status(lib.gstvd_ce_fwd(lp, ldl, lab.data_ptr(), M, V, 0, code, p(rl), p(lse), p(st), None))

        def bwd(lp, ldl, dp, ldd):
            return status(lib.gstvd_ce_bwd(lp, ldl, lab.data_ptr(), p(lse), p(st), None, 1, M, V, 0, code, dp, ldd, None))

        def rows(lp, ldl, dp, ldd):
            return status(lib.gstvd_ce_bwd_rows(lp, ldl, lab.data_ptr(), p(lse), p(g), M, V, 0, code, dp, ldd, None))

        assert "GSTVD_E_SHAPE" in str(fwd(p(lg), 36)) and "GSTVD_E_SHAPE" in str(bwd(p(lg), 36, p(dl), 40)) and "GSTVD_E_SHAPE" in str(rows(p(lg), 36, p(dl), 40))
        assert "GSTVD_E_SHAPE" in str(bwd(p(lg), 40, p(dl), 36)) and "GSTVD_E_SHAPE" in str(rows(p(lg), 40, p(dl), 36))
        for off in range(es, align, es):
            assert "GSTVD_E_ALIGN" in str(fwd(p(lg) + off, 40)), (dt, off)
            assert "GSTVD_E_ALIGN" in str(bwd(p(lg) + off, 40, p(dl), 40)) and "GSTVD_E_ALIGN" in str(bwd(p(lg), 40, p(dl) + off, 40)), (dt, off)
            assert "GSTVD_E_ALIGN" in str(rows(p(lg) + off, 40, p(dl), 40)) and "GSTVD_E_ALIGN" in str(rows(p(lg), 40, p(dl) + off, 40)), (dt, off)
        torch.cuda.synchronize()
        for w in (dl, rl, lse, st):                              # nothing was launched: every output still holds its canary
            assert bool((X.bits(w.flat) == X._canary(dt if w is dl else X.F32)).all())


def test_case_count():
    n = X.case_count()
    print("cases: %s; total %d" % (", ".join("%s %d" % kv for kv in n.items()), sum(n.values())))
    assert n["ce pointer"] == len(X.CE_CASES) >= 150
