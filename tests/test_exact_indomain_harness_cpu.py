"""The in-domain filter's rule (tests/exact_indomain.py) proven on the CPU.

1. Against tests/golden/indomain.npz, recorded from the reference's own cov_mean and MultivariateNormal.log_prob
   (tools/make_golden_indomain.py).  Measured on the machine that recorded it (torch CPU, float64):
       case a (N 400, D 32):  mean and cov equal to the reference's bit for bit;  log-prob max relative deviation 2.44e-15
       case b (N 300, D 64):  mean and cov equal bit for bit;                      log-prob max relative deviation 3.96e-15
   The log-prob assertion stands at 16x the measured value (a torch build whose CPU BLAS orders its sums differently moves the last
   bits).  16 x 0 leaves no such room for mean and cov, so those are held to the any-order bound computed from the data
   (exact_indomain.fit_bounds: ~5e-14 and ~7e-14 here), and the measured zero is printed.
2. The exact cases have teeth: a float64 torch stand-in that walks the kernels' structure (row slabs, 16-row blocks, the f64
   accumulator's row map, the mirror, tail tiles) equals the rule bit for bit on every exact case -- and each planted defect is
   caught, by name, by the same comparison the GPU tests make."""
import os

import numpy as np
import pytest
import torch

import exact_indomain as X
from gst_visdial_amd.indomain import factor
from gst_visdial_amd._lib import GstvdError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indomain.npz")
MEASURED_LOGPROB_REL = {"a": 2.44e-15, "b": 3.96e-15}
CANARY = -4321.5


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("case,n,d", [("a", 400, 32), ("b", 300, 64)])
def test_rule_reproduces_the_reference_fixture(golden, case, n, d):
    fit, score, ref_lp = golden[case + "_fit"], golden[case + "_score"], golden[case + "_log_prob"]
    assert fit.shape == (n, d) and fit.dtype == np.float16 and score.shape == (50, d) and ref_lp.dtype == np.float64
    assert int(golden["seed"]) == 20261020
    cond = np.linalg.cond(golden[case + "_cov"])
    assert 1e2 <= cond <= 1e3 and np.abs(golden[case + "_mean"]).max() > 0.1
    mean, cov = X.fit_rule(fit)
    dm, dc = X.fit_bounds(fit)
    dev_mean, dev_cov = np.abs(mean - golden[case + "_mean"]), np.abs(cov - golden[case + "_cov"])
    print("case %s: max |mean - ref| %.3e  max |cov - ref| %.3e" % (case, dev_mean.max(), dev_cov.max()))
    assert (dev_mean <= dm).all() and (dev_cov <= dc).all()
    assert np.array_equal(cov, cov.T)
    w, hld = factor(torch.from_numpy(cov))
    lp = X.logprob_rule(score, mean, w.numpy(), X.klog2pi(d), hld)
    rel = (np.abs(lp - ref_lp) / np.abs(ref_lp)).max()
    print("case %s: max relative deviation of the rule's log-probs from the reference's %.3e" % (case, rel))
    assert rel <= 16 * MEASURED_LOGPROB_REL[case]


def test_rule_reproduces_torch_float64_at_512_features():
    """The D = 512, N = 1100 case of tests/test_indomain_gpu.py.  Measured: mean equal bit for bit, max |cov - ref| 1.1e-16 (bound
    1.7e-13), log-prob max relative deviation 1.13e-15; asserted at 16x that."""
    fit, score = X.big_case()
    ref_mean, ref_cov, ref_lp = X.host_reference(fit, score)
    mean, cov = X.fit_rule(fit)
    dm, dc = X.fit_bounds(fit)
    assert (np.abs(mean - ref_mean) <= dm).all() and (np.abs(cov - ref_cov) <= dc).all()
    w, hld = factor(torch.from_numpy(cov))
    rel = (np.abs(X.logprob_rule(score, mean, w.numpy(), X.klog2pi(512), hld) - ref_lp) / np.abs(ref_lp)).max()
    print("D = 512: max relative deviation of the rule's log-probs from torch float64 %.3e" % rel)
    assert rel <= 16 * 1.13e-15


def test_factor_names_the_failing_minor():
    c = np.diag([1.0, 2.0, 3.0, 4.0])
    c[2, 2] = -1.0
    with pytest.raises(GstvdError, match="leading minor of order 3"):
        factor(torch.from_numpy(c))
    w, hld = factor(torch.from_numpy(np.diag([4.0, 9.0])))
    assert np.array_equal(w.numpy(), np.diag([0.5, 1.0 / 3.0])) and hld == float(np.log(2.0) + np.log(3.0))


def test_pack_order_is_the_documented_one():
    from gst_visdial_amd import ops
    w = np.tril(np.arange(48 * 48, dtype=np.float64).reshape(48, 48) + 1)
    p = X.pack_w(w)
    assert p.size == 128 * 3 * 4
    for t, s, c, r in ((0, 0, 0, 0), (1, 7, 3, 15), (2, 11, 2, 9), (2, 0, 1, 4)):
        assert p[128 * t * (t + 1) + 64 * s + 16 * c + r] == w[16 * t + r, 4 * s + c]
    assert np.array_equal(ops.gauss_pack_w(torch.from_numpy(w)).numpy(), p)


# ---- the stand-in: the kernels' structure in float64 torch, with switches for the defects ----------------------------------------
def f32_row_map(tile_rows):
    """Where the f32 C/D formula puts the f64 accumulator's rows: the value of true row (g + 4 reg) lands in row (4 g + reg)."""
    out = torch.empty_like(tile_rows)
    for g in range(4):
        for reg in range(4):
            out[4 * g + reg] = tile_rows[g + 4 * reg]
    return out


def standin_fit(x, defect=None):
    xd = torch.from_numpy(np.asarray(x).astype(np.float64))
    n, d = xd.shape
    nslab = (n + X.SLAB - 1) // X.SLAB
    colsum = torch.zeros(d, dtype=torch.float64)
    for s in range(nslab):
        colsum += xd[s * X.SLAB:(s + 1) * X.SLAB].sum(0)
    mean = colsum / n
    S = torch.zeros(d, d, dtype=torch.float64)
    for s in range(nslab - 1 if defect == "last_slab_dropped" else nslab):
        rows = xd[s * X.SLAB:(s + 1) * X.SLAB]
        xc = rows if defect == "mean_not_subtracted" else rows - mean
        S += xc.t() @ xc
    if defect == "f32_row_map":
        for i0 in range(0, d, 16):
            S[i0:i0 + 16] = f32_row_map(S[i0:i0 + 16].clone())
    fact = 1.0 / n if defect == "one_over_n" else 1.0 / (n - 1)
    low = torch.tril(fact * S)
    cov = torch.full((d, d), CANARY, dtype=torch.float64)
    il = torch.tril_indices(d, d)
    cov[il[0], il[1]] = low[il[0], il[1]]
    if defect != "upper_unmirrored":
        cov[il[1], il[0]] = low[il[0], il[1]]
    return mean.numpy(), cov.numpy()


def standin_logprob(x, mean, w, kl2pi, hld, defect=None):
    xd = torch.from_numpy(np.asarray(x).astype(np.float64))
    m, d = xd.shape
    wt = torch.from_numpy(np.tril(w).copy())
    xc = xd if defect == "mean_not_subtracted" else xd - torch.from_numpy(mean)
    q = torch.zeros(m, dtype=torch.float64)
    for t in range(d // 16):
        last = 16 * t if defect == "diagonal_kstep_skipped" else 16 * t + 16          # K-steps of block row t: up to the diagonal block
        z = xc[:, :last] @ wt[16 * t:16 * t + 16, :last].t()
        if defect == "f32_row_map":
            z = f32_row_map(z.t().contiguous()).t()                                   # rows of z move; q adds them all: no effect
        q += (z * z).sum(1)
    out = torch.full((m,), CANARY, dtype=torch.float64)
    written = m - m % 16 if defect == "tail_rows_unwritten" else m
    out[:written] = ((-0.5 * (kl2pi + q)) - hld)[:written]
    return out.numpy()


def fit_mismatches(defect):
    bad = []
    for n, d in X.FIT_CASES:
        if d == 512 and n not in (2, X.SLAB + 1):
            continue                                             # the CPU harness keeps the two D = 512 cases that cost least and most
        x = X.exact_fit_features(n, d, np.float16)
        want_mean, want_cov = X.fit_rule(x)
        mean, cov = standin_fit(x, defect)
        if not (np.array_equal(mean, want_mean) and np.array_equal(cov, want_cov)):
            bad.append((n, d))
    return bad


def score_mismatches(defect):
    bad = []
    for m, d in X.SCORE_CASES:
        x, mean, w = X.exact_score_problem(m, d, np.float16)
        want = X.logprob_rule(x, mean, w, X.klog2pi(d), X.HALF_LOG_DET)
        got = standin_logprob(x, mean, w, X.klog2pi(d), X.HALF_LOG_DET, defect)
        if got.tobytes() != want.tobytes():
            bad.append((m, d))
    return bad


def test_standin_without_defect_equals_the_rule_on_every_exact_case():
    assert fit_mismatches(None) == [] and score_mismatches(None) == []


FIT_WALKED = [(n, d) for n, d in X.FIT_CASES if d != 512 or n in (2, X.SLAB + 1)]


@pytest.mark.parametrize("defect", ["f32_row_map", "mean_not_subtracted", "one_over_n", "upper_unmirrored", "last_slab_dropped"])
def test_fit_defect_is_caught(defect):
    bad = fit_mismatches(defect)
    assert bad == FIT_WALKED                                     # every case shows it ...
    assert (X.SLAB + 1, 512) in bad and (X.SLAB + 1, 16) in bad  # ... the one-row second slab too: its row carries a deviation


@pytest.mark.parametrize("defect", ["diagonal_kstep_skipped", "mean_not_subtracted", "tail_rows_unwritten"])
def test_logprob_defect_is_caught(defect):
    bad = score_mismatches(defect)
    if defect == "tail_rows_unwritten":
        assert bad == [(m, d) for m, d in X.SCORE_CASES if m % 16]
    else:
        assert bad == X.SCORE_CASES


def test_row_map_cannot_show_in_a_sum_over_rows():
    """q adds every row of z, so the accumulator's row map is invisible to the log-prob; the fit's tiles are what catch it."""
    assert score_mismatches("f32_row_map") == []


def test_case_table_brackets_the_slab_and_the_tile():
    assert X.SLAB == 4096 and set(X.FIT_ROWS) == {2, 17, 64, 4095, 4096, 4097}
    assert set(X.DIMS) == {16, 32, 80, 512} and set(X.SCORE_ROWS) == {1, 15, 16, 17, 67}
    import gst_visdial_amd._lib as L
    assert L.GAUSS_FIT_SLAB == X.SLAB and L.GAUSS_MAX_D == 1024
