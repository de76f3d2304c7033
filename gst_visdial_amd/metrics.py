"""Retrieval metrics of the generative evaluation (utils/visdial_metrics.py:21-195): integer rank work on the host,
bit-exact with the reference (ties resolved by torch.sort exactly as there)."""
import torch


def scores_to_ranks(scores):
    """[B, rounds, options] scores -> 1-based rank of every option (descending score)."""
    b, r, o = scores.shape
    order = scores.reshape(-1, o).sort(1, descending=True)[1]
    ranks = torch.empty_like(order)
    ranks.scatter_(1, order, torch.arange(o, device=order.device).expand_as(order))
    return (ranks + 1).view(b, r, o)


class SparseGTMetrics(object):
    """R@1/5/10, mean rank, MRR against one ground-truth option per round (visdial_metrics.py:41-117)."""

    def __init__(self):
        self._ranks = []

    def observe(self, predicted_scores, target_ranks):
        ranks = scores_to_ranks(predicted_scores.detach())
        b, r, o = ranks.shape
        flat = ranks.view(b * r, o)
        gt = target_ranks.reshape(b * r).long().to(flat.device)
        self._ranks.extend(flat[torch.arange(b * r, device=flat.device), gt].cpu().tolist())

    def retrieve(self, reset=True):
        out = {}
        if self._ranks:
            r = torch.tensor(self._ranks).float()
            out = {"r@1": (r <= 1).float().mean().item(), "r@5": (r <= 5).float().mean().item(),
                   "r@10": (r <= 10).float().mean().item(), "mean": r.mean().item(), "mrr": r.reciprocal().mean().item()}
        if reset:
            self.reset()
        return out

    def reset(self):
        self._ranks = []


class NDCG(object):
    """visdial_metrics.py:119-195."""

    def __init__(self):
        self._num, self._den = 0.0, 0.0

    def observe(self, predicted_scores, target_relevance):
        ranks = scores_to_ranks(predicted_scores.detach().unsqueeze(1)).squeeze(1)
        rel = target_relevance.to(ranks.device)
        k = (rel != 0).sum(-1)
        rankings = torch.sort(ranks, dim=-1)[1]
        best = torch.sort(rel, dim=-1, descending=True)[1]
        for b in range(ranks.shape[0]):
            n = int(k[b])
            disc = torch.log2(torch.arange(n).float() + 2)
            dcg = (rel[b][rankings[b][:n]].cpu().float() / disc).sum()
            ideal = (rel[b][best[b][:n]].cpu().float() / disc).sum()
            self._num += float(dcg / ideal)
        self._den += ranks.shape[0]

    def retrieve(self, reset=True):
        out = {"ndcg": float(self._num / self._den)} if self._den > 0 else {}
        if reset:
            self.reset()
        return out

    def reset(self):
        self._num, self._den = 0.0, 0.0


class NDCGBatchSum(NDCG):
    """NDCG whose accumulator follows visdial_metrics.py:160-174 to the bit: the per-dialog ratios of one observe() call are
    summed as fp32 tensors and the numerator stays an fp32 tensor (NDCG above adds Python floats -- the same value to ~1e-8,
    which is what the generative gate asks; the discriminative evaluation is held to bit equality with the reference)."""

    def observe(self, predicted_scores, target_relevance):
        ranks = scores_to_ranks(predicted_scores.detach().unsqueeze(1)).squeeze(1)
        rel = target_relevance.to(ranks.device)
        k = (rel != 0).sum(-1)
        rankings = torch.sort(ranks, dim=-1)[1]
        best = torch.sort(rel, dim=-1, descending=True)[1]
        ratios = []
        for b in range(ranks.shape[0]):
            n = int(k[b])
            disc = torch.log2(torch.arange(n).float() + 2)
            dcg = (rel[b][rankings[b][:n]].cpu().float() / disc).sum(-1)
            ideal = (rel[b][best[b][:n]].cpu().float() / disc).sum(-1)
            ratios.append(dcg / ideal)
        self._num = self._num + sum(ratios)
        self._den += ranks.shape[0]


# ---- the same metrics on the device (gstvd_rank_metrics; the rule is stated in include/gstvd_hip.h) ------------------------------
# Ranks follow the STABLE descending sort (tied options keep their index order; NaN first), the NDCG sums are sequential float64
# sums of fp32 terms, and everything a loop accumulates lives in one int64 device vector that is only added to: no host
# synchronisation before retrieve().  The classes above are untouched and stay the default of every loop.
_DISCOUNTS = {}


def _discounts(device, options):
    """log2(p + 2) for p < options, computed on the host once per (device, options) and uploaded: no device log2 in a result."""
    key = (str(device), int(options))
    if key not in _DISCOUNTS:
        _DISCOUNTS[key] = torch.log2(torch.arange(int(options)).float() + 2).to(device)
    return _DISCOUNTS[key]


def _flat_scores(scores):
    if scores.dim() != 3:
        raise ValueError("scores must be [B, rounds, options] (got %s)" % (tuple(scores.shape),))
    return scores.detach().reshape(-1, scores.shape[2])


def scores_to_ranks_device(scores):
    """[B, rounds, options <= 128] fp32 scores on the device -> int64 1-based ranks there, one launch, no synchronisation.  Tied
    options are ranked in index order (torch.sort(..., descending=True, stable=True)); scores_to_ranks leaves that to torch.sort."""
    from . import ops
    flat = _flat_scores(scores)
    ranks = torch.empty(flat.shape, dtype=torch.int64, device=flat.device)
    ops.rank_metrics(flat, ranks=ranks)
    return ranks.view(scores.shape)


class DeviceRankMetrics(object):
    """R@1/5/10, mean rank, MRR and NDCG accumulated on the device.  observe() is one library call and returns without waiting;
    state() is the one device-to-host copy; retrieve() turns a state into the dict SparseGTMetrics + NDCG give."""

    def __init__(self, device, max_options=128):
        from . import ops
        if not 1 <= int(max_options) <= ops.RANK_MAX_OPTIONS:
            raise ValueError("max_options must lie in [1, %d]" % ops.RANK_MAX_OPTIONS)
        self.device, self.max_options = torch.device(device), int(max_options)
        self.acc = torch.zeros(ops.RANK_ACC_SLOTS, dtype=torch.int64, device=self.device)

    def observe(self, scores, gt_index, relevance=None, round_id=None):
        """scores [B, R, O] fp32 on the device; gt_index [B, R] (any device: uploaded once) or None; relevance [B, O] with
        round_id [B] (1-based): the relevance row of dialog b belongs to list (b, round_id[b] - 1).  Without round_id, R must be 1.
        Returns the per-list outputs written (gt_rank int32 [B * R], ndcg fp32 [B * R]: NaN where a list has no relevance row)."""
        from . import ops
        flat = _flat_scores(scores)
        B, R, O = scores.shape
        if O > self.max_options:
            raise ValueError("scores have %d options, more than max_options = %d" % (O, self.max_options))
        dev, n = flat.device, B * R
        kw = {}
        if gt_index is not None:
            kw["gt_index"] = gt_index.reshape(n).to(device=dev, dtype=torch.int64, non_blocking=True)
            kw["gt_rank"] = torch.empty(n, dtype=torch.int32, device=dev)
        if relevance is not None:
            kw["relevance"] = relevance.reshape(B, O).to(device=dev, dtype=torch.float32, non_blocking=True)
            kw["discounts"] = _discounts(dev, O)
            kw["ndcg"] = torch.empty(n, dtype=torch.float32, device=dev)
            if round_id is not None:
                rid = round_id.reshape(B).to(device=dev, dtype=torch.int64, non_blocking=True)
                b = torch.arange(B, device=dev)
                slot = torch.where((rid >= 1) & (rid <= R), b * R + rid - 1, torch.full_like(rid, n))   # a bad round: no list
                rel_index = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
                rel_index[slot] = b.to(torch.int32)
                kw["rel_index"] = rel_index[:n]
            elif R != 1:
                raise ValueError("relevance for %d rounds per dialog needs round_id" % R)
        return ops.rank_metrics(flat, acc=self.acc, **kw)

    def state(self):
        """The accumulator on the host: {"slots": RANK_ACC_SLOTS Python ints (the sum's slot 0), "ndcg_sum": float}."""
        from . import ops
        host = self.acc.cpu()
        slots = host.tolist()
        slots[ops.RANK_NDCG_SUM] = 0
        return {"slots": slots, "ndcg_sum": float(host[ops.RANK_NDCG_SUM:ops.RANK_NDCG_SUM + 1].view(torch.float64)[0])}

    @staticmethod
    def merge(states):
        """Sum of states, pure host code: the integer slots added exactly, ndcg_sum added in float64 in the order given."""
        states = list(states)
        out = {"slots": [0] * len(states[0]["slots"]), "ndcg_sum": 0.0}
        for s in states:
            out["slots"] = [x + y for x, y in zip(out["slots"], s["slots"])]
            out["ndcg_sum"] = out["ndcg_sum"] + s["ndcg_sum"]
        return out

    @staticmethod
    def metrics(state):
        """A state -> the metric dict.  The histogram is expanded to the list of ground-truth ranks in ascending rank order and
        goes through the torch expressions of SparseGTMetrics.retrieve, in float32 like there -- counts and the integer rank sum
        are exact in any order below 2**24; from sum(rank) >= 2**24 on the expressions run in float64 instead.  ndcg = ndcg_sum /
        n_ndcg over the lists with a finite ratio.  gt_skipped, ndcg_empty and rel_skipped appear only when they are nonzero."""
        from . import ops
        slots = state["slots"]
        hist = slots[ops.RANK_HIST:ops.RANK_HIST + ops.RANK_MAX_OPTIONS + 1]
        out = {}
        if sum(hist) > 0:
            big = sum(r * c for r, c in enumerate(hist)) >= 2 ** 24
            r = torch.repeat_interleave(torch.arange(len(hist)), torch.tensor(hist))
            r = r.double() if big else r.float()
            as_f = (lambda x: x.double()) if big else (lambda x: x.float())
            out = {"r@1": as_f(r <= 1).mean().item(), "r@5": as_f(r <= 5).mean().item(), "r@10": as_f(r <= 10).mean().item(),
                   "mean": r.mean().item(), "mrr": r.reciprocal().mean().item()}
        if slots[ops.RANK_N_NDCG] > 0:
            out["ndcg"] = float(state["ndcg_sum"] / slots[ops.RANK_N_NDCG])
        for name, slot in (("gt_skipped", ops.RANK_N_GT_SKIPPED), ("ndcg_empty", ops.RANK_N_NDCG_EMPTY), ("rel_skipped", ops.RANK_N_REL_SKIPPED)):
            if slots[slot]:
                out[name] = slots[slot]
        return out

    def retrieve(self, reset=True):
        out = self.metrics(self.state())
        if reset:
            self.reset()
        return out

    def reset(self):
        self.acc.zero_()
