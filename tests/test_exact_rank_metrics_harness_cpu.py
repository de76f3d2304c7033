"""The exact layer of the device ranking metrics proves itself on the CPU (tests/exact_rank_metrics.py, DESIGN.md section 8,
"Ranking metrics"): the numpy rule reproduces the reference's fixture and torch's stable sort, DeviceRankMetrics' host half turns
an accumulator filled by the rule into the reference's metric dict, the entry point is declared everywhere, the argument checks
name what is wrong, and the three evaluation loops take the switch."""
import math
import os
import struct

import numpy as np
import pytest
import torch

import exact_rank_metrics as X
from conftest import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("r@1", "r@5", "r@10", "mean", "mrr", "ndcg")
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return {k: v.numpy() for k, v in load_npz("rank_metrics.npz").items()}


def _fixture_case(g, i):
    """Batch i of the fixture as a case of the rule: 40 lists, the relevance row of dialog b at list (b, round_id[b] - 1)."""
    b, r, o = g["scores"].shape[1:]
    idx = np.full(b * r, -1, dtype=np.int32)
    idx[np.arange(b) * r + g["round_id"][i] - 1] = np.arange(b)
    return dict(scores=g["scores"][i].reshape(b * r, o), gt_index=g["gt_option_inds"][i].reshape(-1), relevance=g["gt_relevance"][i],
                rel_index=idx, discounts=X.discounts_host(o))


def _acc_tensor(acc):
    slots = list(acc["slots"])
    slots[X.NDCG_SUM] = struct.unpack("<q", struct.pack("<d", acc["ndcg_sum"]))[0]
    return torch.tensor(slots, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ the rule against the reference
def test_fixture_preconditions(golden):
    s = golden["scores"].reshape(-1, golden["scores"].shape[-1])
    assert all(np.unique(row).size == row.size for row in s)               # no list holds two equal scores
    assert int((golden["gt_relevance"] != 0).sum(-1).min()) >= 1           # every relevance row has k >= 1


def test_rule_reproduces_reference_ranks_and_gt_ranks(golden):
    for i in range(golden["scores"].shape[0]):
        out = X.run_rule(_fixture_case(golden, i))
        assert np.array_equal(out["ranks"].reshape(golden["ranks"][i].shape), golden["ranks"][i])
        assert np.array_equal(out["gt_rank"].astype(np.int64), golden["gt_ranks"][i])


def test_rule_ndcg_within_the_fp32_sum_bound(golden):
    """Two fp32 sums of k non-negative terms and one division separate the reference's ratio from the rule's: 2 (k + 1) 2^-24."""
    worst = 0.0
    for i in range(golden["scores"].shape[0]):
        case = _fixture_case(golden, i)
        out = X.run_rule(case)
        lists = np.flatnonzero(case["rel_index"] >= 0)
        assert np.array_equal(case["rel_index"][lists], np.arange(len(lists)))
        for b, l in enumerate(lists):
            err, k = abs(float(out["ndcg"][l]) - float(golden["ndcg"][i, b])), int(out["k"][l])
            worst = max(worst, err / (2 * (k + 1) * EPS))
            assert err <= 2 * (k + 1) * EPS, (i, b, err, k)
        assert np.isnan(np.delete(out["ndcg"], lists)).all()
    print("ndcg: worst error / bound = %.3f" % worst)


def test_rule_equals_torch_stable_sort_on_the_case_table():
    for case in X.CASES:
        x = torch.from_numpy(case["scores"])
        order = torch.sort(x, dim=1, descending=True, stable=True)[1]
        ranks = torch.empty_like(order)
        ranks.scatter_(1, order, torch.arange(x.shape[1]).expand_as(order))
        assert np.array_equal(X.ranks_rule(case["scores"]), (ranks + 1).numpy()), case["id"]


def test_case_table_covers_what_it_names():
    assert {c["scores"].shape[1] for c in X.CASES} >= set(X.O_VALUES) and {c["scores"].shape[0] for c in X.CASES} >= set(X.L_VALUES)
    acc = X.empty_acc()
    seen_nan = seen_k0 = seen_kO = False
    for case in X.CASES:
        out = X.run_rule(case, acc)
        o = case["scores"].shape[1]
        seen_nan |= bool(np.isnan(case["scores"]).any())
        if out["ndcg"] is not None:
            idx = case["rel_index"] if case["rel_index"] is not None else np.arange(len(out["k"]))
            valid = (idx >= 0) & (idx < case["relevance"].shape[0])
            seen_k0 |= bool((out["k"][valid] == 0).any())
            seen_kO |= bool((out["k"][valid] == o).any())
    s = acc["slots"]
    assert seen_nan and seen_k0 and seen_kO
    assert all(s[i] > 0 for i in (X.N_SPARSE, X.N_GT_SKIPPED, X.N_NDCG, X.N_NDCG_EMPTY, X.N_REL_SKIPPED)) and s[X.N_CALLS] == len(X.CASES)
    assert sum(s[X.HIST:]) == s[X.N_SPARSE] and s[X.HIST] == 0 and s[X.HIST + 128] > 0
    assert any(c["strides"] for c in X.CASES) and any(c["rel_index"] is None and c["relevance"] is not None for c in X.CASES)


# -------------------------------------------------------------------------------- retrieve on an accumulator filled by the rule
def test_retrieve_on_rule_accumulator_gives_the_reference_dict(golden):
    from gst_visdial_amd.metrics import DeviceRankMetrics
    acc, n, k_max = X.empty_acc(), 0, 0
    for i in range(golden["scores"].shape[0]):
        out = X.run_rule(_fixture_case(golden, i), acc)
        n += out["ranks"].shape[0]
        k_max = max(k_max, int(out["k"].max()))
        m = DeviceRankMetrics("cpu")
        m.acc.copy_(_acc_tensor(acc))
        got = m.retrieve(reset=True)
        assert int(m.acc.abs().sum()) == 0
        want = dict(zip(NAMES, golden["metrics"][i].tolist()))
        assert set(got) == set(NAMES)                                       # no skipped / empty key: those counts are zero
        for key in ("r@1", "r@5", "r@10", "mean"):                          # counts and integer rank sums < 2^24: exact in any order
            assert np.float32(got[key]) == np.float32(want[key]), (i, key, got[key], want[key])
        assert abs(got["mrr"] - want["mrr"]) <= n * EPS * want["mrr"], (i, got["mrr"], want["mrr"])
        assert abs(got["ndcg"] - want["ndcg"]) <= 2 * (k_max + 1) * EPS, (i, got["ndcg"], want["ndcg"])
    assert want == dict(zip(NAMES, golden["metrics_final"].tolist()))


def test_retrieve_reports_skips_and_switches_to_float64():
    from gst_visdial_amd.metrics import DeviceRankMetrics
    st = X.empty_acc()
    st["slots"][X.N_GT_SKIPPED], st["slots"][X.N_NDCG_EMPTY], st["slots"][X.N_REL_SKIPPED] = 3, 2, 1
    assert DeviceRankMetrics.metrics(st) == {"gt_skipped": 3, "ndcg_empty": 2, "rel_skipped": 1}
    assert DeviceRankMetrics.metrics(X.empty_acc()) == {}
    big = X.empty_acc()
    big["slots"][X.HIST + 100], big["slots"][X.HIST + 3], big["slots"][X.N_SPARSE] = 200000, 1, 200001      # sum(rank) > 2^24
    got = DeviceRankMetrics.metrics(big)
    assert got["mean"] == (200000 * 100 + 3) / 200001.0 and got["r@5"] == 1 / 200001.0      # fp32 would round both


def test_merge_of_batch_states_equals_one_run(golden):
    from gst_visdial_amd.metrics import DeviceRankMetrics
    whole, parts = X.empty_acc(), []
    for i in range(golden["scores"].shape[0]):
        X.run_rule(_fixture_case(golden, i), whole)
        one = X.empty_acc()
        X.run_rule(_fixture_case(golden, i), one)
        parts.append(one)
    merged = DeviceRankMetrics.merge(parts)
    assert merged == whole and all(isinstance(v, int) for v in merged["slots"])
    other = DeviceRankMetrics.merge([parts[2], parts[0], parts[1]])
    assert other["slots"] == whole["slots"] and abs(other["ndcg_sum"] - whole["ndcg_sum"]) <= 4 * 2.0 ** -52 * whole["ndcg_sum"]
    assert parts[0]["slots"][X.N_CALLS] == 1                                # merge is pure: its inputs are as they were


# ------------------------------------------------------------------------------------------------------------- the entry point
def test_entry_point_in_header_bindings_and_makefile():
    import re
    from gst_visdial_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gstvd_rank_metrics_t;", hdr).group(1)
    names = [re.split(r"[\s\*]+", d.strip())[-1] for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert names == [f[0] for f in _lib.RankMetricsDesc._fields_]
    assert "int gstvd_rank_metrics(const gstvd_rank_metrics_t* a, gstvd_stream_t s);" in hdr
    assert "gstvd_rank_metrics" in _lib.SIGNATURES and _lib.ABI_VERSION == 9
    assert "rank_metrics.hip" in open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "Makefile")).read()
    assert "rank_metrics_kernel 0" in open(os.path.join(ROOT, "tools", "kernel_resources.expect")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%d entry points" % len(_lib.SIGNATURES) in design and "### Ranking metrics" in design
    # the header's slot numbers = the bindings' = this harness's own
    enum = dict((k, int(v)) for k, v in re.findall(r"GSTVD_RANK_([A-Z_]+) = (\d+)", hdr))
    assert enum["MAX_OPTIONS"] == ops.RANK_MAX_OPTIONS == X.MAX_OPTIONS and ops.RANK_ACC_SLOTS == X.ACC_SLOTS == 8 + 128 + 1
    for name in ("N_SPARSE", "N_GT_SKIPPED", "N_NDCG", "N_NDCG_EMPTY", "N_REL_SKIPPED", "N_CALLS", "NDCG_SUM", "HIST"):
        assert enum[name] == getattr(ops, "RANK_" + name) == getattr(X, name), name


def test_argument_checks_name_what_is_wrong():
    from gst_visdial_amd import ops
    from gst_visdial_amd._lib import GstvdError
    s, rel, disc = torch.zeros(4, 100), torch.zeros(4, 100), torch.ones(100)
    with pytest.raises(GstvdError, match="no CPU path"):
        ops.rank_metrics(s, ranks=torch.zeros(4, 100, dtype=torch.int64))
    with pytest.raises(GstvdError, match="scores"):
        ops.rank_metrics(torch.zeros(4, 129))
    with pytest.raises(GstvdError, match="scores"):
        ops.rank_metrics(s.half())
    with pytest.raises(GstvdError, match="discounts"):
        ops.rank_metrics(s, relevance=rel, ndcg=torch.zeros(4))
    with pytest.raises(GstvdError, match="ndcg"):
        ops.rank_metrics(s, relevance=rel, discounts=disc)
    with pytest.raises(GstvdError, match="discounts"):
        ops.rank_metrics(s, relevance=rel, discounts=torch.ones(99), ndcg=torch.zeros(4))
    with pytest.raises(GstvdError, match="gt_index"):
        ops.rank_metrics(s, gt_index=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(GstvdError, match="gt_index"):
        ops.rank_metrics(s, gt_index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(GstvdError, match="relevance"):
        ops.rank_metrics(s, relevance=torch.zeros(3, 100), discounts=disc, ndcg=torch.zeros(4))
    with pytest.raises(GstvdError, match="rel_index"):
        ops.rank_metrics(s, relevance=rel, discounts=disc, ndcg=torch.zeros(4), rel_index=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(GstvdError, match="ndcg"):
        ops.rank_metrics(s, relevance=rel, discounts=disc, ndcg=torch.zeros(5))
    with pytest.raises(GstvdError, match="ranks"):
        ops.rank_metrics(s, ranks=torch.zeros(4, 99, dtype=torch.int64))
    with pytest.raises(GstvdError, match="acc"):
        ops.rank_metrics(s, acc=torch.zeros(ops.RANK_ACC_SLOTS - 1, dtype=torch.int64))
    with pytest.raises(GstvdError, match="gt_rank needs gt_index"):
        ops.rank_metrics(s, gt_rank=torch.zeros(4, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the loops
class _Recorder(object):
    """Stands in for metrics.DeviceRankMetrics: counts what the loops do with it."""
    made = []

    def __init__(self, device, max_options=128):
        self.device, self.calls = device, []
        _Recorder.made.append(self)

    def observe(self, scores, gt_index, relevance=None, round_id=None):
        self.calls.append((tuple(scores.shape), gt_index is not None, relevance is not None, round_id is not None))

    def state(self):
        return X.empty_acc()

    metrics = staticmethod(lambda state: {"r@1": 0.5})
    merge = staticmethod(lambda states: states[0])

    def retrieve(self, reset=True):
        return {"r@1": 0.5}


def _forbid(*a, **k):
    raise AssertionError("the host metric classes must not be touched with metrics='device'")


def _stable_ranks(scores):
    order = torch.sort(scores, dim=-1, descending=True, stable=True)[1]
    ranks = torch.empty_like(order)
    ranks.scatter_(-1, order, torch.arange(scores.shape[-1]).expand_as(order))
    return ranks + 1


def _patch(monkeypatch, module):
    from gst_visdial_amd import metrics
    _Recorder.made = []
    monkeypatch.setattr(metrics, "DeviceRankMetrics", _Recorder)
    monkeypatch.setattr(metrics, "scores_to_ranks_device", _stable_ranks)
    for name in ("SparseGTMetrics", "NDCG", "NDCGBatchSum", "scores_to_ranks"):
        if hasattr(module, name):
            monkeypatch.setattr(module, name, _forbid)


def _gen_batches(n, rounds, options, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [dict(scores=torch.randn(2, rounds, options, generator=g), gt_option_inds=torch.randint(0, options, (2, rounds), generator=g),
                 round_id=torch.randint(1, rounds + 1, (2, 1), generator=g), gt_relevance=torch.rand(2, options, generator=g),
                 image_id=torch.tensor([10 * i, 10 * i + 1])) for i in range(n)]


def test_evaluate_takes_the_switch(monkeypatch):
    from gst_visdial_amd import evaluate as E
    batches = _gen_batches(3, 10, 5)
    scorer = lambda model, batch, device: batch["scores"]
    host = E.evaluate(object(), batches, {"device": "cpu"}, scorer=scorer)              # default = "host": today's path
    assert set(host[1]) == set(NAMES)
    _patch(monkeypatch, E)
    json_, m = E.evaluate(object(), batches, {"device": "cpu"}, scorer=scorer, metrics="device")
    assert json_ == [] and m == {"r@1": 0.5} and len(_Recorder.made) == 1
    assert _Recorder.made[0].calls == [((2, 10, 5), True, True, True)] * 3              # one observe per batch
    test_batches = _gen_batches(2, 1, 5, seed=1)
    json_, m = E.evaluate(object(), test_batches, {"device": "cpu"}, mode="vd_eval_test", scorer=scorer, metrics="device")
    assert m == {} and _Recorder.made[-1].calls == []
    assert [e["image_id"] for e in json_] == [0, 1, 10, 11] and [e["round_id"] for e in json_] == [int(b["round_id"][j]) for b in test_batches for j in range(2)]
    assert [e["ranks"] for e in json_] == [_stable_ranks(b["scores"])[j, 0].tolist() for b in test_batches for j in range(2)]
    with pytest.raises(ValueError, match="metrics"):
        E.evaluate(object(), batches, {"device": "cpu"}, scorer=scorer, metrics="gpu")


def test_host_is_the_default_and_never_makes_the_device_class(monkeypatch):
    from gst_visdial_amd import evaluate as E, metrics
    monkeypatch.setattr(metrics, "DeviceRankMetrics", _forbid)
    monkeypatch.setattr(metrics, "scores_to_ranks_device", _forbid)
    batches = _gen_batches(2, 10, 5)
    scorer = lambda model, batch, device: batch["scores"]
    a = E.evaluate(object(), batches, {"device": "cpu"}, scorer=scorer)
    b = E.evaluate(object(), batches, {"device": "cpu"}, scorer=scorer, metrics="host")
    assert a == b and set(a[1]) == set(NAMES)


class _Encoder(object):
    def eval(self):
        return self


def test_evaluate_disc_takes_the_switch(monkeypatch):
    from gst_visdial_amd import evaluate_disc as D
    batches = _gen_batches(3, 10, 5)
    for b in batches:
        b["tokens"] = torch.zeros(2, 10, 5, 4, dtype=torch.int64)
    monkeypatch.setattr(D, "score_batch", lambda encoder, batch, params, rows_per_call=200: batch["scores"])
    from gst_visdial_amd import metrics
    monkeypatch.setattr(metrics, "DeviceRankMetrics", _forbid)                          # the default never makes the device class
    host = D.evaluate_disc(_Encoder(), batches, {"mode": "vd_eval_val", "device": "cpu"})
    assert set(host) == set(NAMES)
    _patch(monkeypatch, D)
    assert D.evaluate_disc(_Encoder(), batches, {"mode": "vd_eval_val", "device": "cpu"}, metrics="device") == {"r@1": 0.5}
    assert len(_Recorder.made) == 1 and _Recorder.made[0].calls == [((2, 10, 5), True, True, True)] * 3
    test_batches = _gen_batches(2, 1, 5, seed=2)
    json_ = D.evaluate_disc(_Encoder(), test_batches, {"mode": "vd_eval_test", "device": "cpu"}, metrics="device")
    assert [e["ranks"] for e in json_] == [_stable_ranks(b["scores"])[j, 0].tolist() for b in test_batches for j in range(2)]
    with pytest.raises(ValueError, match="metrics"):
        D.evaluate_disc(_Encoder(), batches, {"mode": "vd_eval_val", "device": "cpu"}, metrics="gpu")


def test_evaluate_attack_takes_the_switch(monkeypatch):
    from gst_visdial_amd import attack as A
    rounds, options, T = 2, 50, 3
    batches = _gen_batches(2, rounds, options)
    for b in batches:
        for k in ("enc_input_ids", "enc_segments", "enc_sep_indices", "enc_mlm_labels", "enc_att_mask", "dec_input_ids", "dec_att_mask"):
            b[k] = torch.zeros(2, rounds, options, T, dtype=torch.int64)
        b["enc_image_feat"], b["enc_image_loc"], b["enc_image_mask"] = torch.zeros(2, 3, 4), torch.zeros(2, 3, 5), torch.zeros(2, 3)
    g = torch.Generator().manual_seed(5)
    monkeypatch.setattr(A, "score_chunk", lambda model, item, params, epsilon, textattack=None, coref=None: torch.randn(A.ROWS_PER_CALL, generator=g))
    params = {"attack": "fgsm", "device": "cpu"}
    from gst_visdial_amd import metrics
    monkeypatch.setattr(metrics, "DeviceRankMetrics", _forbid)                          # the default never makes the device class
    host = A.evaluate_attack(_Encoder(), batches, params)
    assert set(host[1]) == set(NAMES)
    _patch(monkeypatch, A)
    json_, m = A.evaluate_attack(_Encoder(), batches, params, metrics="device")
    assert json_ == [] and m == {"r@1": 0.5}
    assert len(_Recorder.made) == 1 and _Recorder.made[0].calls == [((2, rounds, options), True, True, True)] * 2
    with pytest.raises(ValueError, match="metrics"):
        A.evaluate_attack(_Encoder(), batches, params, metrics="gpu")


def test_ndcg_sum_slot_round_trips_through_state():
    """state() reads the float64 out of its int64 slot, and merge adds it as a float: no bit is lost on the way."""
    from gst_visdial_amd.metrics import DeviceRankMetrics
    acc = X.empty_acc()
    acc["ndcg_sum"], acc["slots"][X.N_NDCG] = 0.1 + 0.2, 2
    m = DeviceRankMetrics("cpu")
    m.acc.copy_(_acc_tensor(acc))
    st = m.state()
    assert st["ndcg_sum"] == 0.1 + 0.2 and st["slots"] == acc["slots"] and not math.isnan(st["ndcg_sum"])
