"""gstvd_rank_metrics (csrc/rank_metrics.hip) on the case table of tests/exact_rank_metrics.py and on the fixture recorded from the
reference's metric classes: equal to the rule bit for bit on ranks, gt_rank, ndcg (NaNs by position) and every accumulator slot,
the float64 sum included; every output inside a poisoned canary window, strided rows with their gaps untouched; each nullable
output left out in turn; a second call; the replay of a captured graph on other contents; the library's refusals."""
import struct

import numpy as np
import pytest
import torch

import exact_rank_metrics as X
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
POISON = {torch.int64: -7777777, torch.int32: -99, torch.float32: 1234.5}
BY_ID = {c["id"]: c for c in X.CASES}


class Window(object):
    """`rows` rows of `cols` elements at row stride `ld` inside a poisoned buffer with PAD elements in front and behind."""

    def __init__(self, rows, cols, dtype, ld=None, fill=None):
        self.rows, self.cols, self.ld = rows, cols, (ld or cols)
        self.poison = POISON[dtype] if fill is None else fill
        self.buf = torch.full((2 * PAD + rows * self.ld,), self.poison, dtype=dtype, device=DEV)
        self.view = self.buf.as_strided((rows, cols), (self.ld, 1), PAD)

    def vector(self):
        return self.buf[PAD:PAD + self.rows * self.cols] if self.ld == self.cols else None

    def put(self, array):
        self.view.copy_(torch.as_tensor(np.asarray(array)).to(self.view.dtype))
        return self

    def surroundings_untouched(self):
        b = self.buf.cpu()
        inside = torch.zeros(b.numel(), dtype=torch.bool)
        inside.as_strided((self.rows, self.cols), (self.ld, 1), PAD).fill_(True)
        rest = b[~inside]
        return bool((rest == self.poison).all()) if self.poison == self.poison else bool(torch.isnan(rest).all())


def _device_case(case, omit=()):
    """The case's operands on the device: inputs in windows whose gaps hold NaN / poison (a stray read would show), outputs poisoned."""
    n, o = case["scores"].shape
    st = case["strides"] or (o, o, o)
    d = {"scores": Window(n, o, torch.float32, st[0], fill=float("nan")).put(case["scores"]), "w": {}}
    kw = {}
    if case["gt_index"] is not None:
        kw["gt_index"] = torch.as_tensor(case["gt_index"]).to(DEV)
        if "gt_rank" not in omit:
            d["w"]["gt_rank"] = Window(n, 1, torch.int32)
            kw["gt_rank"] = d["w"]["gt_rank"].vector()
    if case["relevance"] is not None and "ndcg" not in omit:
        rel = case["relevance"]
        kw["relevance"] = Window(rel.shape[0], o, torch.float32, st[2], fill=float("nan")).put(rel).view
        kw["discounts"] = torch.as_tensor(case["discounts"]).to(DEV)
        if case["rel_index"] is not None:
            kw["rel_index"] = torch.as_tensor(case["rel_index"]).to(DEV)
        d["w"]["ndcg"] = Window(n, 1, torch.float32)
        kw["ndcg"] = d["w"]["ndcg"].vector()
    if "ranks" not in omit:
        d["w"]["ranks"] = Window(n, o, torch.int64, st[1])
        kw["ranks"] = d["w"]["ranks"].view
    if "acc" not in omit:
        d["w"]["acc"] = Window(X.ACC_SLOTS, 1, torch.int64)
        kw["acc"] = d["w"]["acc"].vector()
        kw["acc"].zero_()
    d["kw"] = kw
    return d


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _same_float_bits(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def _check(case, d, want, acc_want, calls=1):
    cid, w = case["id"], d["w"]
    if "ranks" in w:
        assert np.array_equal(w["ranks"].view.cpu().numpy(), want["ranks"]), cid
    if "gt_rank" in w:
        assert np.array_equal(w["gt_rank"].vector().cpu().numpy(), want["gt_rank"]), cid
    if "ndcg" in w:
        assert _same_float_bits(w["ndcg"].vector().cpu().numpy(), want["ndcg"]), cid
    if "acc" in w:
        got = w["acc"].vector().cpu().tolist()
        s = struct.unpack("<d", struct.pack("<q", got[X.NDCG_SUM]))[0]
        got[X.NDCG_SUM] = 0
        assert got == [v * calls for v in acc_want["slots"]], (cid, got[:8], acc_want["slots"][:8])
        total = acc_want["ndcg_sum"]
        assert struct.pack("<d", s) == struct.pack("<d", total if calls == 1 else total + total), (cid, s, total)
    for k, win in w.items():
        assert win.surroundings_untouched(), (cid, k)


def _rule(case, omit=()):
    c = dict(case)
    if "ndcg" in omit:
        c["relevance"] = c["rel_index"] = None
    acc = X.empty_acc()
    return X.run_rule(c, acc), acc


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_rank_metrics_case_table(cid):
    from gst_visdial_amd import ops
    case = BY_ID[cid]
    d = _device_case(case)
    written = ops.rank_metrics(d["scores"].view, **d["kw"])
    assert set(written) == set(d["w"])
    _check(case, d, *_rule(case))


@pytest.mark.parametrize("omit", ["ranks", "gt_rank", "ndcg", "acc"])
@pytest.mark.parametrize("cid", ["strided_O100_L5", "O128_L5_mixed", "O100_L257_null"])
def test_rank_metrics_each_nullable_output_left_out(cid, omit):
    """Leaving an output out changes nothing else (ndcg leaves with its relevance: the entry refuses one without the other)."""
    from gst_visdial_amd import ops
    case = BY_ID[cid]
    d = _device_case(case, omit=(omit,))
    assert omit not in ops.rank_metrics(d["scores"].view, **d["kw"])
    _check(case, d, *_rule(case, omit=(omit,)))


def test_case_ids_used_above_exist():
    assert {"strided_O100_L5", "O128_L5_mixed", "O100_L257_null", "O100_L5_mixed"} <= set(BY_ID)


@pytest.mark.parametrize("cid", ["O100_L257_null", "strided_O100_L5"])
def test_rank_metrics_second_call_adds_again(cid):
    from gst_visdial_amd import ops
    case = BY_ID[cid]
    d = _device_case(case)
    ops.rank_metrics(d["scores"].view, **d["kw"])
    first = {k: w.buf.clone() for k, w in d["w"].items() if k != "acc"}
    ops.rank_metrics(d["scores"].view, **d["kw"])
    for k, b in first.items():
        assert torch.equal(b.view(torch.int32) if b.dtype == torch.float32 else b,
                           d["w"][k].buf.view(torch.int32) if b.dtype == torch.float32 else d["w"][k].buf), k
    _check(case, d, *_rule(case), calls=2)


def test_rank_metrics_replays_from_a_captured_graph_on_other_contents():
    from gst_visdial_amd import ops
    from gst_visdial_amd.graph import capture
    c0 = X.make_case("graph_a", 100, 9, 201, "mixed")
    c1 = X.make_case("graph_b", 100, 9, 202, "mixed")
    assert c0["relevance"].shape == c1["relevance"].shape
    d = _device_case(c0)
    call = lambda: ops.rank_metrics(d["scores"].view, **d["kw"])
    call()                                                                                   # eager once: library loaded, nothing lazy left
    g = torch.cuda.CUDAGraph()
    with capture(g):
        call()
    for c in (c1, c0):
        d["scores"].view.copy_(torch.as_tensor(c["scores"]))
        d["kw"]["gt_index"].copy_(torch.as_tensor(c["gt_index"]))
        d["kw"]["relevance"].copy_(torch.as_tensor(c["relevance"]))
        d["kw"]["rel_index"].copy_(torch.as_tensor(c["rel_index"]))
        for k, w in d["w"].items():
            w.view.fill_(0 if k == "acc" else w.poison)
        g.replay()
        torch.cuda.synchronize()
        _check(c, d, *_rule(c))


def test_rank_metrics_reproduces_the_reference_fixture():
    from gst_visdial_amd.metrics import DeviceRankMetrics, scores_to_ranks_device
    g = load_npz("rank_metrics.npz")
    m = DeviceRankMetrics(DEV)
    for i in range(g["scores"].shape[0]):
        scores = g["scores"][i].to(DEV)
        assert torch.equal(scores_to_ranks_device(scores).cpu(), g["ranks"][i])
        out = m.observe(scores, g["gt_option_inds"][i], g["gt_relevance"][i], g["round_id"][i])
        assert torch.equal(out["gt_rank"].cpu().long(), g["gt_ranks"][i])
        want = X.run_rule(dict(scores=g["scores"][i].reshape(40, 100).numpy(), gt_index=g["gt_option_inds"][i].reshape(-1).numpy(),
                               relevance=g["gt_relevance"][i].numpy(), discounts=X.discounts_host(100),
                               rel_index=np.asarray([b if l == b * 10 + int(g["round_id"][i][b]) - 1 else -1
                                                     for b in range(4) for l in range(b * 10, b * 10 + 10)], dtype=np.int32)))
        assert _same_float_bits(out["ndcg"].cpu().numpy(), want["ndcg"])
    got = m.retrieve()
    names = ("r@1", "r@5", "r@10", "mean", "mrr", "ndcg")
    ref = dict(zip(names, g["metrics_final"].tolist()))
    assert set(got) == set(names) and all(np.float32(got[k]) == np.float32(ref[k]) for k in names[:4])
    assert abs(got["mrr"] - ref["mrr"]) <= 120 * 2.0 ** -24 * ref["mrr"] and abs(got["ndcg"] - ref["ndcg"]) <= 2 * 101 * 2.0 ** -24


def test_rank_metrics_refusals_write_nothing():
    import ctypes as C
    from gst_visdial_amd import _lib
    lib = _lib.load()
    case = BY_ID["O100_L5_mixed"]
    d = _device_case(case)
    kw, p = d["kw"], (lambda t: t.data_ptr())

    def desc():
        a = _lib.RankMetricsDesc()
        a.scores, a.ld_scores, a.gt_index, a.L, a.O = p(d["scores"].view), 100, p(kw["gt_index"]), 5, 100
        a.relevance, a.ld_rel, a.n_rel = p(kw["relevance"]), 100, kw["relevance"].shape[0]
        a.rel_index = p(kw["rel_index"])
        a.discounts, a.n_discounts = p(kw["discounts"]), 100
        a.ranks, a.ld_ranks, a.gt_rank, a.ndcg, a.acc = p(kw["ranks"]), 100, p(kw["gt_rank"]), p(kw["ndcg"]), p(kw["acc"])
        return a

    kw["acc"].fill_(POISON[torch.int64])
    assert lib.gstvd_rank_metrics(None, None) == -4 and lib.gstvd_rank_metrics(C.byref(_lib.RankMetricsDesc()), None) == -4
    for field in ("discounts", "ndcg", "gt_index", "relevance"):                             # each leaves an operand without its partner
        a = desc()
        setattr(a, field, None)
        assert lib.gstvd_rank_metrics(C.byref(a), None) == -4, field
    for field, value in (("O", 129), ("O", 0), ("L", 0), ("L", 2 ** 31), ("ld_scores", 99), ("ld_ranks", 99), ("ld_rel", 99),
                         ("n_discounts", 99), ("n_rel", 0)):
        a = desc()
        setattr(a, field, value)
        assert lib.gstvd_rank_metrics(C.byref(a), None) == -2, field
    a = desc()
    a.rel_index, a.n_rel = None, 4                                                           # NULL rel_index needs one row per list
    assert lib.gstvd_rank_metrics(C.byref(a), None) == -2
    torch.cuda.synchronize()
    for k, w in d["w"].items():
        assert bool((w.buf == w.poison).all()), k
