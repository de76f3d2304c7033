"""In-domain image filter: the first stage of GST (preprocessing/clip_in_domain_filtering.py) from the feature matrix on.

The reference fits a multivariate normal to the CLIP features of the VisDial images (cov_mean, MultivariateNormal), scores every
CC12M image by its log density and writes {"image_id", "log_prob"} records; the cut is left to the user.  Here the fit and the
scoring run on the device in float64 (ops.gauss_fit, ops.gauss_logprob; the rule is stated in include/gstvd_hip.h), the one
D x D Cholesky factorisation per fit runs on the host in torch's CPU linalg, and a fit is made once and kept (state_dict) instead of
once per scoring run.  The CLIP network itself is not part of this package: the filter starts at its output.

Two departures, both stated in INTEGRATION.md: a NaN or Inf feature gives a NaN or Inf score instead of raising, and "score at or
above the threshold is in-domain" is this project's reading of the reference's `-threshold`, which it parses and never reads.
"""
import math

import torch

from . import ops
from ._lib import GstvdError


def factor(cov):
    """Host side of a fit: cov float64 [D, D] (any device) -> (W = L^-1 lower triangular, half_log_det = sum log diag L) for
    cov = L L^T, in torch's CPU linalg.  A covariance that is not positive definite raises GstvdError naming the failing minor."""
    c = cov.detach().to("cpu", torch.float64)
    L, info = torch.linalg.cholesky_ex(c)
    if int(info) != 0:
        raise GstvdError("InDomainFilter: the covariance is not positive definite: its leading minor of order %d is not positive "
                         "(a fit needs more rows than features, and no constant or dependent feature)" % int(info))
    piv = torch.diagonal(L) ** 2                                # a pivot lost in the rounding of the others is no pivot: rank-deficient fits
    tiny = piv <= c.shape[0] * 2.0 ** -52 * float(torch.diagonal(c).max())
    if bool(tiny.any()):
        raise GstvdError("InDomainFilter: the covariance is not positive definite: its leading minor of order %d is zero to rounding "
                         "(a fit needs more rows than features, and no constant or dependent feature)" % (int(tiny.nonzero()[0]) + 1))
    W = torch.linalg.solve_triangular(L, torch.eye(c.shape[0], dtype=torch.float64), upper=False)
    return torch.tril(W), float(torch.log(torch.diagonal(L)).sum())


class InDomainFilter(object):
    """Gaussian in-domain score of image features.  fit() once on the dialog data's features; log_prob() / select() /
    score_batches() on any number of others."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.mean = self.cov = self.w = None
        self.half_log_det = self.klog2pi = None
        self._n_kept = None

    # ---- fit
    def fit(self, feats):
        """feats fp16 or fp32 [N, D] on the device.  Device: mean and covariance; host: Cholesky, W = L^-1, the log determinant."""
        mean, cov = ops.gauss_fit(feats)
        W, hld = factor(cov)                                   # the one D x D copy to the host ...
        self._set(mean, cov, ops.gauss_pack_w(W).to(feats.device), hld)   # ... and the one back
        return self

    def _set(self, mean, cov, w, half_log_det):
        self.mean, self.cov, self.w = mean, cov, w
        self.half_log_det = float(half_log_det)
        self.klog2pi = mean.numel() * math.log(2 * math.pi)
        self._n_kept = torch.zeros(1, dtype=torch.int64, device=mean.device)

    def _fitted(self):
        if self.mean is None:
            raise GstvdError("InDomainFilter: fit() or load_state_dict() first")

    # ---- score
    def log_prob(self, feats, out=None):
        """float64 [M]: the log density of every row of feats."""
        self._fitted()
        return ops.gauss_logprob(feats, self.mean, self.w, self.klog2pi, self.half_log_det, out=out)

    def select(self, feats, threshold):
        """(log_prob float64 [M], keep uint8 [M]): keep[m] = log_prob[m] >= threshold; the kept rows are added to the device counter
        n_kept() reads.  No host synchronisation."""
        self._fitted()
        keep = torch.empty(feats.shape[0], dtype=torch.uint8, device=feats.device) if isinstance(feats, torch.Tensor) and feats.dim() == 2 \
            else None
        lp = ops.gauss_logprob(feats, self.mean, self.w, self.klog2pi, self.half_log_det, threshold=threshold, keep=keep,
                               n_kept=self._n_kept)
        return lp, keep

    def n_kept(self):
        """Rows kept by every select() since the fit (or reset_n_kept): the one host read, to be made behind a loop."""
        self._fitted()
        return int(self._n_kept.item())

    def reset_n_kept(self):
        self._fitted()
        self._n_kept.zero_()

    def score_batches(self, batches, image_ids):
        """The reference's output: a list of {"image_id": int, "log_prob": float}, one per row of every batch, in order.  `batches`
        yields feature matrices, `image_ids` the ids of all their rows in the same order (a sequence or tensor).  One device-to-host
        copy at the end."""
        self._fitted()
        scores = [self.log_prob(b) for b in batches]
        lp = torch.cat(scores).cpu().tolist() if scores else []
        ids = image_ids.reshape(-1).tolist() if isinstance(image_ids, torch.Tensor) else [int(i) for i in image_ids]
        if len(ids) != len(lp):
            raise GstvdError("InDomainFilter.score_batches: %d image ids for %d scored rows" % (len(ids), len(lp)))
        return [{"image_id": i, "log_prob": s} for i, s in zip(ids, lp)]

    # ---- state
    def state_dict(self):
        self._fitted()
        return {"mean": self.mean.detach().cpu().clone(), "cov": self.cov.detach().cpu().clone(), "w_packed": self.w.detach().cpu().clone(),
                "half_log_det": torch.tensor(self.half_log_det, dtype=torch.float64)}

    def load_state_dict(self, state):
        for k in ("mean", "cov", "w_packed", "half_log_det"):
            if k not in state:
                raise GstvdError("InDomainFilter.load_state_dict: missing %r" % k)
        mean, cov, w = (state[k].to(self.device, torch.float64).contiguous() for k in ("mean", "cov", "w_packed"))
        D = mean.numel()
        if mean.dim() != 1 or tuple(cov.shape) != (D, D) or D % 16 or w.dim() != 1 or w.numel() != 128 * (D // 16) * (D // 16 + 1):
            raise GstvdError("InDomainFilter.load_state_dict: shapes do not belong to one fit")
        self._set(mean, cov, w, float(state["half_log_det"]))
        return self
