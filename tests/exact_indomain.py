"""The in-domain filter's rule restated in numpy, independently of the kernels, and the case table both layers walk.

The rule (include/gstvd_hip.h states it for the library): features x[n, :] in fp16 or fp32, every sum in float64.
  fit      mean[i] = (sum_n x[n, i]) / N;  S[i, j] = sum_n (x[n, i] - mean[i]) (x[n, j] - mean[j]);  cov = (1.0 / (N - 1)) * S, the
           factor applied once behind the sum; the lower triangle is computed and the upper one is its copy.
  log-prob z = W (x - mean), q = sum_i z_i^2, out = (-0.5 * (klog2pi + q)) - half_log_det, W lower triangular.
  keep     out >= threshold; NaN is never kept.
The rule does not fix the order of a sum.  The exact cases below are therefore built so that every order gives the same bits:
small integers (and halves), column sums that are multiples of N, so every partial sum is an exactly representable number.

Used by tests/test_exact_indomain_harness_cpu.py (against the reference's fixture, and a stand-in with planted defects) and
tests/test_indomain_exact_gpu.py / tests/test_indomain_gpu.py (against the device)."""
import math

import numpy as np

SLAB = 4096                       # rows of a slab of the fit (GSTVD_GAUSS_FIT_SLAB)
U = 2.0 ** -53                    # unit roundoff of float64

DIMS = (16, 32, 80, 512)
SCORE_ROWS = (1, 15, 16, 17, 67)
FIT_ROWS = (2, 17, 64, SLAB - 1, SLAB, SLAB + 1)   # one slab not full, one slab full, a second slab of a single row
FIT_CASES = [(n, d) for d in DIMS for n in FIT_ROWS]
SCORE_CASES = [(m, d) for d in DIMS for m in SCORE_ROWS]


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def fit_rule(x):
    """(mean [D], cov [D, D]) of the rows of x, float64."""
    xd = np.asarray(x).astype(np.float64)
    n = xd.shape[0]
    mean = xd.sum(axis=0) / n
    xc = xd - mean
    s = np.tril(xc.T @ xc)
    s = s + np.tril(s, -1).T
    return mean, (1.0 / (n - 1)) * s


def logprob_rule(x, mean, w, klog2pi, half_log_det):
    """float64 [M]: the Gaussian log density of every row of x; w = L^-1, lower triangular."""
    with np.errstate(invalid="ignore", over="ignore"):
        z = (np.asarray(x).astype(np.float64) - mean) @ np.tril(w).T
        q = (z * z).sum(axis=1)
        return (-0.5 * (klog2pi + q)) - half_log_det


def keep_rule(scores, threshold):
    with np.errstate(invalid="ignore"):
        return (scores >= threshold).astype(np.uint8)


def klog2pi(d):
    return d * math.log(2 * math.pi)


def pack_w(w):
    """The operand order of the library: packed[128 t (t + 1) + 64 s + 16 c + r] = W[16 t + r, 4 s + c], s < 4 t + 4."""
    d = w.shape[0]
    out = []
    for t in range(d // 16):
        for s in range(4 * t + 4):
            for c in range(4):
                out.append(w[16 * t:16 * t + 16, 4 * s + c])
    return np.concatenate(out).astype(np.float64)


# ---- error bounds computed from the data ----------------------------------------------------------------------------------------
def logprob_bound(x, mean, w, kl2pi, half_log_det):
    """Per output, a bound on |kernel - rule| when both use this mean and W: twice the first-order bound of a float64 sum of n
    terms taken in any order (n * 2^-53 * sum |terms|) for every z_i, carried through q = sum z_i^2 (whose own sum gets the same
    bound), plus two roundings of the result."""
    xc = np.asarray(x).astype(np.float64) - mean
    d = xc.shape[1]
    wl = np.tril(w)
    z = xc @ wl.T
    ez = 2.0 * d * U * (np.abs(xc) @ np.abs(wl).T)
    q = (z * z).sum(axis=1)
    dq = (2.0 * np.abs(z) * ez + ez * ez).sum(axis=1) + 2.0 * d * U * q
    out = (-0.5 * (kl2pi + q)) - half_log_det
    return 0.5 * dq + 4.0 * U * (np.abs(out) + abs(half_log_det) + 0.5 * (kl2pi + q))


def fit_bounds(x):
    """(bound on |mean - rule|  [D], bound on |cov - rule| [D, D]) for sums taken in any order: twice n * 2^-53 * sum |terms| for the
    column sums and for the products' sums, plus what the mean's own error moves the centred products by."""
    xd = np.asarray(x).astype(np.float64)
    n = xd.shape[0]
    mean = xd.sum(axis=0) / n
    dm = 2.0 * n * U * np.abs(xd).sum(axis=0) / n + U * np.abs(mean)
    xc = np.abs(xd - mean)
    fact = 1.0 / (n - 1)
    col = xc.sum(axis=0)
    s_abs = xc.T @ xc
    ds = 2.0 * n * U * s_abs + np.outer(dm, col) + np.outer(col, dm) + n * np.outer(dm, dm)
    return dm, fact * ds + 2.0 * U * fact * s_abs


# ---- exact cases ---------------------------------------------------------------------------------------------------------------
def exact_fit_features(n, d, dtype, seed=0):
    """Integer-and-a-half features whose sums are exact in any order: x[r, i] = base[i] + dev[r, i] with the deviations in +/-
    pairs of rows (an odd N leaves ROW 0 without a deviation, so the last row -- a slab of its own at N = SLAB + 1 -- has one), so
    mean == base exactly and S is a sum of small integers.  Pair 0 carries +/- (i + 1): the rows of S, and its columns, all differ,
    so a moved, transposed or permuted tile shows.  Returns x in `dtype` (np.float16 / np.float32)."""
    rng = np.random.RandomState(1000 * d + n + seed)
    base = (rng.randint(-8, 9, size=d) + 0.5 * rng.randint(0, 2, size=d)).astype(np.float64)
    pairs = n // 2
    v = rng.randint(-3, 4, size=(pairs, d)).astype(np.float64)
    v[0] = np.arange(1, d + 1)
    if pairs > 1:
        v[-1] = rng.randint(1, 4, size=d)                       # the last pair is nowhere zero
    dev = np.zeros((n, d))
    first = n % 2
    dev[first::2] = v
    dev[first + 1::2] = -v
    x = (base + dev).astype(dtype)
    assert np.array_equal(x.astype(np.float64), base + dev)     # representable
    mean, cov = fit_rule(x)
    assert np.array_equal(mean, base)
    s = cov * (n - 1)
    assert len({r.tobytes() for r in np.round(s)}) == d         # every row of S (= every column) differs from every other
    return x


def exact_score_problem(m, d, dtype, seed=0):
    """(x [m, d] in dtype, mean [d], W [d, d]) with integer features, a mean of halves and an integer lower-triangular W with a
    non-zero diagonal: every z and q is an exactly representable integer (or quarter) in any order of the sums, and every row's q is
    different."""
    rng = np.random.RandomState(77 * d + m + seed)
    w = np.tril(rng.randint(-2, 3, size=(d, d))).astype(np.float64)
    w[np.arange(d), np.arange(d)] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=d)
    mean = 0.5 * rng.randint(-6, 7, size=d)
    for _ in range(20):
        x = rng.randint(-8, 9, size=(m, d)).astype(dtype)
        q = (((x.astype(np.float64) - mean) @ w.T) ** 2).sum(axis=1)
        if len(set(q.tolist())) == m:
            return x, mean, w
    raise AssertionError("no draw with distinct q")


def big_case():
    """(fit [1100, 512], score [67, 512]) fp16 features with unequal variances and a non-zero mean: the D = 512 case of
    tests/test_indomain_gpu.py, whose reference is torch float64 on the host (host_reference)."""
    rng = np.random.RandomState(512)
    d, n = 512, 1100
    scale = np.exp(rng.uniform(np.log(0.1), np.log(0.5), size=d))
    loc = rng.uniform(-0.5, 0.5, size=d)
    fit = (rng.standard_normal((n, d)) * scale + loc).astype(np.float16)
    score = (rng.standard_normal((67, d)) * scale * 1.2 + loc).astype(np.float16)
    return fit, score


def host_reference(fit, score):
    """torch float64 on the host, the statements of the reference's script: mean, centred product scaled by 1/(N-1),
    MultivariateNormal(loc, covariance_matrix).log_prob.  Returns (mean, cov, log_prob) as numpy."""
    import torch
    m = torch.from_numpy(fit).double().t()
    mean = m.mean(dim=1, keepdim=True)
    mc = m - mean
    cov = (1.0 / (m.shape[1] - 1)) * mc.matmul(mc.t())
    dist = torch.distributions.MultivariateNormal(loc=mean.squeeze(), covariance_matrix=cov)
    return mean.squeeze().numpy(), cov.numpy(), dist.log_prob(torch.from_numpy(score).double()).numpy()


HALF_LOG_DET = 1.2345678901234567    # any double: the rule and the kernel apply it in the same two roundings
