"""The exact layer of the soft pseudo-label tests proves itself on the CPU (tests/exact_distill.py): every
case runs against a stand-in of csrc/distill.hip written in torch -- fp32 arithmetic, the rule of include/gstvd_hip.h -- and against
deliberately wrong stand-ins, each of which must fail a case named for it.  Nothing here touches a GPU."""
import pytest
import torch

import exact_distill as D
from exact_gemm import F32

CPU = torch.device("cpu")


class Torch(object):
    """Stand-in of gstvd_ce_fwd / gstvd_ce_bwd (mean form) and of the entries of csrc/distill.hip.  `defect`: one planted error."""

    def __init__(self, defect=None):
        self.device, self.defect = CPU, defect

    # -- the cross entropy the distillation entries build on
    @staticmethod
    def _keep(labels, V, ignore):
        return (labels != ignore) & (labels >= 0) & (labels < V)

    def ce_fwd(self, logits, labels, M, V, row_loss, lse, stats, ignore_index=0):
        x = logits[:, :V].float()
        mx = x.max(1).values
        l = mx + torch.log(torch.exp(x - mx[:, None]).sum(1))
        lse.copy_(l)
        keep = self._keep(labels, V, ignore_index)
        xl = torch.gather(x, 1, labels.clamp(0, V - 1).view(-1, 1))[:, 0]
        row_loss.copy_(torch.where(keep, l - xl, torch.zeros_like(l)))
        stats[0], stats[1] = row_loss.sum(), float((labels != ignore_index).sum())
        stats[2] = stats[0] / stats[1]

    def _ce_rows(self, logits, labels, lse, gs, V, ignore):
        x = logits[:, :V].float()
        onehot = (torch.arange(V).view(1, -1) == labels.view(-1, 1)).float()
        val = (torch.exp(x - lse.view(-1, 1)) - onehot) * gs
        return torch.where(self._keep(labels, V, ignore).view(-1, 1), val, torch.zeros_like(val))

    def ce_bwd(self, logits, labels, lse, stats, gscale, mean, M, V, dlogits, ignore_index=0):
        gs = (gscale[0] if gscale is not None else torch.tensor(1.0)) / stats[1]
        dlogits[:, :V] = self._ce_rows(logits, labels, lse, gs, V, ignore_index).to(dlogits.dtype)
        dlogits[:, V:] = 0

    # -- the teacher
    def topk_logp(self, logits, lse, M, V, K, ids, logp):
        x = logits[:, :V].float()
        if self.defect == "ties to the larger id":
            vals, idx = torch.sort(x.flip(1), dim=1, descending=True, stable=True)
            idx = V - 1 - idx
        else:
            vals, idx = torch.sort(x, dim=1, descending=True, stable=True)
        if self.defect == "-inf entries dropped":
            idx = torch.where(torch.isinf(vals), torch.zeros_like(idx), idx)
        ids.copy_(idx[:, :K])
        logp.copy_(vals[:, :K] - lse.view(-1, 1))

    # -- the student
    def _soft(self, labels, sid, V, ignore):
        ok = (sid[:, 0] >= 0) & ((sid >= 0) & (sid < V)).all(-1)
        if self.defect == "out-of-range id used":
            ok = sid[:, 0] >= 0
        return self._keep(labels, V, ignore) & ok

    def _q(self, slp, inv_tau):
        s = slp * inv_tau
        s = s - s.max(-1, keepdim=True).values
        e = torch.exp(s)
        z = e.sum(-1, keepdim=True)
        return e / z, s - torch.log(z)

    def distill_fwd(self, logits, labels, sid, slp, M, V, alpha, tau, ce_row_loss, row_loss, row_kd, lse_tau, stats, ignore_index=0):
        inv_tau = torch.tensor(1.0 / tau, dtype=F32)
        x = logits[:, :V].float() * inv_tau
        soft = self._soft(labels, sid, V, ignore_index)
        mx = x.max(1).values
        lt = mx + torch.log(torch.exp(x - mx[:, None]).sum(1))
        q, lq = self._q(slp, inv_tau)
        wide = torch.as_strided(logits, (M, logits.stride(0)), logits.stride(), logits.storage_offset()).float() * inv_tau
        at = torch.gather(wide, 1, sid.clamp(0, wide.shape[1] - 1)) - lt[:, None]
        term = torch.where(q > 0, q * (lq - at), torch.zeros_like(q))
        kd = torch.where(soft, term.sum(-1), torch.zeros_like(lt))
        a = torch.where(soft, torch.full_like(lt, alpha), torch.zeros_like(lt))
        row_kd.copy_(kd)
        lse_tau.copy_(torch.where(soft, lt, torch.zeros_like(lt)))
        mixed = (1 - a) * ce_row_loss + a * (tau * tau) * kd
        row_loss.copy_(torch.where(a == 0, ce_row_loss, mixed))
        stats[0], stats[1] = row_loss.sum(), float((labels != ignore_index).sum())
        stats[2] = stats[0] / stats[1]

    def distill_bwd(self, logits, labels, sid, slp, lse, lse_tau, stats, gscale, M, V, alpha, tau, dlogits, ignore_index=0):
        d = self.defect
        inv_tau = torch.tensor(1.0 / tau, dtype=F32)
        gs = (gscale[0] if gscale is not None else torch.tensor(1.0)) / stats[1]
        x = logits[:, :V].float()
        soft = self._soft(labels, sid, V, ignore_index) & (alpha != 0)
        q, _ = self._q(slp, inv_tau)
        qd = torch.zeros(M, V)
        if d == "duplicate ids merged":
            qd.scatter_(1, sid.clamp(0, V - 1), q * soft[:, None])
        else:
            qd.scatter_add_(1, sid.clamp(0, V - 1), q * soft[:, None])
        onehot = (torch.arange(V).view(1, -1) == labels.view(-1, 1)).float()
        wk = alpha * tau if d != "tau squared in the gradient" else alpha * tau * tau
        val = gs * ((1 - alpha) * (torch.exp(x - lse.view(-1, 1)) - onehot) + wk * (torch.exp(x * inv_tau - lse_tau.view(-1, 1)) - qd))
        out = torch.where(soft.view(-1, 1), val, self._ce_rows(logits, labels, lse, gs, V, ignore_index))
        if d == "ignored row multiplied":
            out = torch.where(self._keep(labels, V, ignore_index).view(-1, 1), out, x * 0.0 + gs)
        dlogits[:, :V] = out.to(dlogits.dtype)
        if d != "padding not zeroed":
            dlogits[:, V:] = 0


CPU_V = (5, 1023, 1025, 4099)


@pytest.mark.parametrize("dtype,V,K", [c for c in D.TOPK_CASES if c[1] in CPU_V])
def test_topk_cases_pass_on_the_stand_in(dtype, V, K):
    D.check_topk(Torch(), dtype, V, K)


def test_topk_case_at_the_full_vocabulary_passes_on_the_stand_in():
    D.check_topk(Torch(), "bf16", 30522, 16)


@pytest.mark.parametrize("dtype,V,rot", [c for c in D.BWD_CASES if c[1] in CPU_V])
def test_exact_backward_cases_pass_on_the_stand_in(dtype, V, rot):
    D.check_bwd_exact(Torch(), dtype, V, rot)


@pytest.mark.parametrize("dtype,V,kind,tau", [c for c in D.NOISE_CASES if c[1] in (1025,)])
def test_noise_cases_pass_on_the_stand_in(dtype, V, kind, tau):
    D.check_noise(Torch(), dtype, V, kind, tau)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_alpha_zero_case_passes_on_the_stand_in(dtype):
    D.check_alpha_zero(Torch(), dtype, 1030)


@pytest.mark.parametrize("dtype,V", [c for c in D.LSE1_CASES if c[1] <= 1025])
def test_lse_at_tau_one_cases_pass_on_the_stand_in(dtype, V):
    D.check_lse_tau_one(Torch(), dtype, V)


DEFECTS = {
    "ties to the larger id": lambda be: D.check_topk(be, "f32", 1025, 4),
    "-inf entries dropped": lambda be: D.check_topk(be, "bf16", 1023, 16),
    "out-of-range id used": lambda be: D.check_bwd_exact(be, "f32", 1025, 0),
    "duplicate ids merged": lambda be: D.check_bwd_exact(be, "f32", 1025, 1),
    "tau squared in the gradient": lambda be: D.check_noise(be, "f32", 1025, "gauss", 2.0),
    "ignored row multiplied": lambda be: D.check_bwd_exact(be, "bf16", 5, 2),
    "padding not zeroed": lambda be: D.check_bwd_exact(be, "f32", 4099, 2),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_planted_defect_fails_its_case(defect):
    DEFECTS[defect](Torch())                                   # the case passes on the sound stand-in ...
    with pytest.raises(AssertionError):
        DEFECTS[defect](Torch(defect))                         # ... and catches the defect


def test_case_count():
    n = D.case_count()
    assert n["top-k"] == 28 and n["backward exact"] == 24 and n["noise"] == 24 and n["alpha 0"] == 4
