"""Exact layer of the LayerNorm-folded GEMMs on a real MI355X (tests/exact_lnfold.py): gemm_rows_kernel and
gemv16_ln_kernel through ops.gemm_ln_fwd / gemm_ln_bwd / gemv_ln / colsum_partials / dropout_mask / Rng only.  Every launch runs
on canary / NaN-poisoned windows with padded leading dimensions; y, mean, rstd, dres, dx, every partial slab, the column sums,
y_out and C (bf16 and fp32) are compared bit for bit with a float64 reference computed without eps.  The harness itself is proved
on the CPU by tests/test_exact_lnfold_harness_cpu.py.

Premise that only the hardware can confirm -- sqrtf(4^k + 1e-12) == 2^k and 1 / 2^k == 2^-k for the k range used, S / H
correctly rounded -- is asserted by a test of its own through the kernels (rstd of gemm_ln_fwd, y_out of gemv_ln)."""
import pytest
import torch

import exact_lnfold as F
import exact_ln as X

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    """The backend of exact_lnfold's checks: the HIP kernels, through ops."""

    def __init__(self):
        self.device = torch.device(DEV, torch.cuda.current_device())
        self.rng = ops().Rng(self.device, seed=77)

    def keep(self, n, p, site):
        return ops().dropout_mask(n, p, site, self.rng, self.device)

    def _kw(self, kw):
        o = ops()
        return dict(kw, mode=X.MODES[kw["mode"]], dtype=o.BF16 if kw["dtype"] == torch.bfloat16 else o.F32, rng=self.rng)

    def _epi(self, epi):
        o = ops()
        return {None: 0, "gelu": o.EPI_GELU, "dgelu": o.EPI_DGELU, "colsum": 32}[epi]          # (32: GSTVD_EPI_COLSUM)

    def gemm_ln_fwd(self, kw, B, C, N, epi=None, **opt):
        ops().gemm_ln_fwd(self._kw(kw), B, C, N, epi=self._epi(epi), **opt)

    def gemm_ln_bwd(self, kw, dy, partial, nblk, B, C, N, epi=None, **opt):
        ops().gemm_ln_bwd(self._kw(kw), dy, partial, nblk, B, C, N, epi=self._epi(epi), **opt)

    def gemv_ln(self, A, B, C, M, N, K, gamma, beta, eps, epi=None, **opt):
        ops().gemv_ln(A, B, C, M, N, K, gamma, beta, eps, epi=self._epi(epi), **opt)

    def colsum_partials(self, *a):
        ops().colsum_partials(*a)


def ids(cs):
    return [c.id for c in cs]


# ------------------------------------------------------------------------------------------ census and premise
def test_census_every_folded_kernel_of_the_library_is_named_by_a_case():
    """Lists the 16 gemm_rows_kernel and 2 gemv16_ln_kernel instantiations the built library carries and a case of each (run
    with -s).  The tie from a case to an instantiation is stated from the dispatch code, not observed: see exact_lnfold."""
    F.check_census(F.E.library_kernels(F.lib_path(), F.FOLD_KERNEL_RE))


def test_premise_sqrtf_and_the_division_give_rstd_of_two_to_minus_k():
    """On this hardware sqrtf(4^k + 1e-12) == 2^k and 1 / 2^k == 2^-k for every k the tables use: rstd of a forward launch whose
    rows cover k = -1..3, and y_out of the decode kernel (its rstd is not an output; y_out == gamma * sigma + beta needs it)."""
    be = Gpu()
    p = F.run_rows(be, F.rows("fwd", 33, 640, 128), seed=2)
    ks = set(p.ln.k.flatten().tolist())
    assert ks == {-1.0, 0.0, 1.0, 2.0, 3.0}
    F.assert_bit_equal(p.ln.v("rstd"), 2.0 ** -p.ln.k[:, 0], "rstd == 2^-k")
    g = F.run_gemv(be, F.gemv(16, 16, 200), seed=1)
    assert set(g.k.flatten().tolist()) >= {-1.0, 3.0}


# ------------------------------------------------------------------------------------------ every case of the tables
@pytest.mark.parametrize("c", F.ROWS_CASES, ids=ids(F.ROWS_CASES))
def test_folded_layernorm_gemm_is_bit_exact_inside_its_windows(c):
    F.run_rows(Gpu(), c, F.CASES.index(c))


@pytest.mark.parametrize("c", F.GEMV_CASES, ids=ids(F.GEMV_CASES))
def test_decode_layernorm_gemv_is_bit_exact_inside_its_windows(c):
    F.run_gemv(Gpu(), c, F.CASES.index(c))


@pytest.mark.parametrize("dir", ["fwd", "bwd"])
def test_gemm_ln_refusals_leave_every_output_untouched(dir):
    F.check_rows_refusals(Gpu(), dir)


def test_gemv_ln_refusals_leave_every_output_untouched():
    F.check_gemv_refusals(Gpu())


# ------------------------------------------------------------------------------------------ invariances
INV = [F.rows("fwd", 33, 648, 192, bias=True, add=True, p_pre=0.5), F.rows("bwd", 33, 648, 192, add=True, p_pre=0.5),
       F.gemv(7, 20, 200, bias=True, add=True)]


@pytest.mark.parametrize("c", INV, ids=ids(INV))
def test_what_surrounds_the_windows_does_not_matter(c):
    F.check_surroundings_do_not_matter(Gpu(), c, 3)


@pytest.mark.parametrize("c", INV, ids=ids(INV))
def test_two_launches_give_the_same_bits(c):
    F.check_reproducible(Gpu(), c, 4)


@pytest.mark.parametrize("c", INV, ids=ids(INV))
def test_a_row_block_does_not_depend_on_the_other_row_blocks(c):
    F.check_row_blocks_are_independent(Gpu(), c, 1, 5)


# ------------------------------------------------------------------------------------------ noise rows
@pytest.mark.parametrize("K", F.NOISE_K)
@pytest.mark.parametrize("ratio", F.NOISE_RATIOS)
def test_decode_one_pass_variance_on_rows_with_a_large_mean(ratio, K):
    """gemv16_ln_kernel forms var = E[x^2] - mean^2 in one fp32 pass: random bf16 rows with |mean| / std = ratio against LayerNorm
    in float64.  Prints the largest distance of y_out in bf16 ulps (run with -s).
    Measured on an MI355X: see the comment of the kernel (csrc/gemv.hip)."""
    F.check_noise_rows(Gpu(), ratio, K, seed=int(ratio * 10) + K)
