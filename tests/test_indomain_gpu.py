"""InDomainFilter (gst_visdial_amd/indomain.py) on the device: the fixture recorded from the reference's cov_mean and
MultivariateNormal.log_prob, and a D = 512, N = 1100 case made here whose independent reference is torch float64 on the host.

Bounds are computed from the data (tests/exact_indomain.py), not picked.  The kernel is held to the rule evaluated with the kernel's
OWN mean and W: per output, twice the first-order bound of a float64 sum of n terms in any order (n 2^-53 sum |terms|), carried
through q.  Against the reference the same bound is used plus the deviation tests/test_exact_indomain_harness_cpu.py measured for
the rule itself, at its 16x (2.44e-15, 3.96e-15 and, for D = 512, 1.13e-15 relative).  That comparison scores with the HOST's fit
by the rule loaded into the filter (load_state_dict), so that it rests on nothing the device computed but the scores; the
deviation of the whole pipeline (device fit, host factor, device scores) from the reference is printed beside it.
Error paths: covariance not positive definite (N <= D), N < 2, D = 24, dtype and device mismatches; state_dict round trip
bit-equal; score_batches records in the reference's order."""
import os

import numpy as np
import pytest
import torch

import exact_indomain as X
from gst_visdial_amd import ops
from gst_visdial_amd._lib import GstvdError
from gst_visdial_amd.indomain import InDomainFilter, factor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indomain.npz")
RULE_VS_REFERENCE_REL = {"a": 16 * 2.44e-15, "b": 16 * 3.96e-15, "big": 16 * 1.13e-15}     # measured by the CPU harness, at its 16x


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def unpack_w(packed, d):
    w = np.zeros((d, d))
    for t in range(d // 16):
        k = 16 * t + 16
        w[16 * t:16 * t + 16, :k] = packed[128 * t * (t + 1):128 * (t + 1) * (t + 2)].reshape(k, 16).T
    return w


def check_against_rule(f, fit, score, lp):
    """The device's fit within the any-order bounds of the rule's; its log-probs within the bound of the rule evaluated with the
    device's own mean and W."""
    d = fit.shape[1]
    mean, cov = f.mean.cpu().numpy(), f.cov.cpu().numpy()
    want_mean, want_cov = X.fit_rule(fit)
    dm, dc = X.fit_bounds(fit)
    print("fit: max |mean - rule| %.3e (bound %.3e)  max |cov - rule| %.3e (bound %.3e)"
          % (np.abs(mean - want_mean).max(), dm.max(), np.abs(cov - want_cov).max(), dc.max()))
    assert (np.abs(mean - want_mean) <= dm).all() and (np.abs(cov - want_cov) <= dc).all()
    assert np.array_equal(cov, cov.T)
    w = unpack_w(f.w.cpu().numpy(), d)
    want = X.logprob_rule(score, mean, w, f.klog2pi, f.half_log_det)
    bound = X.logprob_bound(score, mean, w, f.klog2pi, f.half_log_det)
    print("log-prob: max |kernel - rule| %.3e, max of the bound %.3e, worst ratio %.3f"
          % (np.abs(lp - want).max(), bound.max(), (np.abs(lp - want) / bound).max()))
    assert (np.abs(lp - want) <= bound).all()
    return want, bound


def check_against_reference(case, f, fit, score, ref, lp):
    """The device's scores under the host's fit (the rule's mean, cov and the host factor of it) against the reference's."""
    d = fit.shape[1]
    mean, cov = X.fit_rule(fit)
    w, hld = factor(torch.from_numpy(cov))
    g = InDomainFilter(DEV).load_state_dict({"mean": torch.from_numpy(mean), "cov": torch.from_numpy(cov), "w_packed": ops.gauss_pack_w(w),
                                             "half_log_det": torch.tensor(hld, dtype=torch.float64)})
    got = g.log_prob(torch.from_numpy(score).to(DEV)).cpu().numpy()
    bound = X.logprob_bound(score, mean, w.numpy(), X.klog2pi(d), hld)
    dev = np.abs(got - ref)
    print("%s: max relative deviation from the reference's log-probs: scores under the host's fit %.3e, whole pipeline %.3e"
          % (case, (dev / np.abs(ref)).max(), (np.abs(lp - ref) / np.abs(ref)).max()))
    assert (dev <= bound + RULE_VS_REFERENCE_REL[case] * np.abs(ref)).all()


@pytest.mark.parametrize("case", ["a", "b"])
def test_filter_on_the_reference_fixture(golden, case):
    fit, score, ref = golden[case + "_fit"], golden[case + "_score"], golden[case + "_log_prob"]
    f = InDomainFilter(DEV).fit(torch.from_numpy(fit).to(DEV))
    lp = f.log_prob(torch.from_numpy(score).to(DEV)).cpu().numpy()
    assert lp.dtype == np.float64 and lp.shape == (50,)
    check_against_rule(f, fit, score, lp)
    check_against_reference(case, f, fit, score, ref, lp)
    assert (np.abs(f.cov.cpu().numpy() - golden[case + "_cov"]) <= X.fit_bounds(fit)[1]).all()     # the harness measured 0 for the rule


@pytest.fixture(scope="module")
def big():
    """D = 512, N = 1100 (exact_indomain.big_case) and its reference, torch float64 on the host."""
    fit, score = X.big_case()
    return fit, score, X.host_reference(fit, score)[2]


def test_filter_on_512_features(big):
    fit, score, ref = big
    f = InDomainFilter(DEV).fit(torch.from_numpy(fit).to(DEV))
    lp, keep = f.select(torch.from_numpy(score).to(DEV), float(np.median(ref)))
    lp, keep = lp.cpu().numpy(), keep.cpu().numpy()
    check_against_rule(f, fit, score, lp)
    assert np.array_equal(keep, X.keep_rule(lp, float(np.median(ref)))) and f.n_kept() == int(keep.sum())
    check_against_reference("big", f, fit, score, ref, lp)


def test_state_dict_round_trip_is_bit_equal(golden):
    fit, score = golden["a_fit"], torch.from_numpy(golden["a_score"]).to(DEV)
    f = InDomainFilter(DEV).fit(torch.from_numpy(fit).to(DEV))
    state = f.state_dict()
    assert set(state) == {"mean", "cov", "w_packed", "half_log_det"} and all(v.device.type == "cpu" for v in state.values())
    g = InDomainFilter(DEV).load_state_dict(state)
    for k in ("mean", "cov", "w"):
        assert torch.equal(getattr(f, k), getattr(g, k))
    assert g.half_log_det == f.half_log_det and g.klog2pi == f.klog2pi
    assert f.log_prob(score).cpu().numpy().tobytes() == g.log_prob(score).cpu().numpy().tobytes()
    out = torch.full((50,), 7.0, dtype=torch.float64, device=DEV)
    assert g.log_prob(score, out=out) is out and torch.equal(out, f.log_prob(score))


def test_score_batches_gives_the_reference_records_in_order(golden):
    fit, score = golden["b_fit"], torch.from_numpy(golden["b_score"]).to(DEV)
    f = InDomainFilter(DEV).fit(torch.from_numpy(fit).to(DEV))
    ids = [900 - 7 * i for i in range(50)]
    recs = f.score_batches([score[:16], score[16:17], score[17:]], torch.tensor(ids))
    whole = f.log_prob(score).cpu().tolist()
    assert recs == [{"image_id": i, "log_prob": s} for i, s in zip(ids, whole)]
    assert all(type(r["image_id"]) is int and type(r["log_prob"]) is float for r in recs)
    with pytest.raises(GstvdError, match="49 image ids for 50"):
        f.score_batches([score], ids[:49])
    # select over a loop, one host read behind it
    total = 0
    for part in (score[:20], score[20:]):
        lp, keep = f.select(part, whole[3])
        total += int(keep.sum().item())
    assert f.n_kept() == total == sum(1 for s in whole if s >= whole[3])


def test_error_paths(golden):
    fit = torch.from_numpy(golden["a_fit"]).to(DEV)
    f = InDomainFilter(DEV)
    with pytest.raises(GstvdError, match="not positive definite: its leading minor of order"):
        f.fit(fit[:32])                                          # N <= D: rank N - 1 < D
    with pytest.raises(GstvdError, match="at least 2 rows"):
        f.fit(fit[:1])
    with pytest.raises(GstvdError, match="multiple of 16"):
        f.fit(torch.zeros(100, 24, device=DEV))
    with pytest.raises(GstvdError, match="float16 or float32"):
        f.fit(fit.to(torch.bfloat16))
    with pytest.raises(GstvdError, match="GPU tensors"):
        f.fit(fit.cpu())
    assert f.mean is None                                        # no failed fit left a half state behind
    f.fit(fit)
    with pytest.raises(GstvdError, match="mean must be a contiguous float64 tensor of shape \\[64\\]"):
        f.log_prob(torch.zeros(4, 64, dtype=torch.float16, device=DEV))
    with pytest.raises(GstvdError, match="out must be"):
        f.log_prob(fit[:4], out=torch.zeros(4, device=DEV))
    with pytest.raises(GstvdError, match="out lives on cpu"):
        f.log_prob(fit[:4], out=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(GstvdError, match="keep must be"):
        ops.gauss_logprob(fit[:4], f.mean, f.w, f.klog2pi, f.half_log_det, threshold=0.0, keep=torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(GstvdError, match="need a threshold"):
        ops.gauss_logprob(fit[:4], f.mean, f.w, f.klog2pi, f.half_log_det, keep=torch.zeros(4, dtype=torch.uint8, device=DEV))
    with pytest.raises(GstvdError, match="workspace must be"):
        ops.gauss_fit(fit, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(GstvdError, match="cov must be"):
        ops.gauss_fit(fit, cov=torch.zeros(32, 31, dtype=torch.float64, device=DEV))
