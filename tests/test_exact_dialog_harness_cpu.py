"""CPU proof of tests/exact_dialog.py: the numpy rows rule reproduces the fixture recorded from the reference's encode_input bit
for bit, the numpy append rule equals generate.append_to_context, and the harness itself runs (and catches wrong backends) on a
numpy stand-in."""
import os

import numpy as np
import pytest
import torch

import exact_dialog as X
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    from gst_visdial_amd.selfcheck import read_npz
    return X.fixture_cases(read_npz(os.path.join(GOLDEN, "selftrain_rows.npz")))


def test_rows_rule_reproduces_the_reference_fixture(fixture):
    assert sorted(c.name for c, _ in fixture) == ["cut", "full", "noise", "r12"]
    for c, want in fixture:
        got = X.rows_rule(c.cap, c.ques, c.ans, c.ppl, c.T, c.Ud, c.select_data, c.threshold, c.mask_prob, c.valid, c.u_tok)
        for k in X.ROWS_OUT:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (c.name, k)
            assert np.array_equal(got[k], want[k]), (c.name, k, np.argwhere(got[k] != want[k])[:5])


def test_fixture_covers_what_it_promises(fixture):
    f = {c.name: (c, w) for c, w in fixture}
    c, w = f["cut"]
    assert c.T == 32 and w["enc_ids"][0, 2, 31] == X.SEP                                   # fits exactly
    assert w["enc_sep"][1, 2, 5] == 32 and X.SEP != w["enc_ids"][1, 2, 31] != 0            # the final [SEP] is lost, its position listed
    assert w["enc_sep"][2, 2, 5] > 32 and w["enc_ids"][2, 2, 31] not in (0, X.SEP)          # cut inside the question
    thr = np.float32(c.threshold)
    below = np.nextafter(thr, np.float32(0))
    for b, j in np.ndindex(*c.ppl.shape):
        assert bool(w["dec_labels"][b, j].any()) == (not c.ppl[b, j] >= thr), (b, j)
    assert {float(thr), float(below), float("inf")} <= set(float(x) for x in c.ppl.flat)
    c, w = f["noise"]
    assert c.mask_prob == 0.15 and c.Ud == 6 and (w["dec_att"].sum(-1) <= 6).all() and (w["dec_att"].sum(-1) == 6).any()
    assert (c.ques[:, :, 0] == X.SEP).any()                                                 # an empty question
    assert any(int(s) in c.ques or int(s) in c.ans for s in (100, 101, 103))
    assert ((c.ans != 0).sum(-1) == 18).any() and not (c.ans[(c.ans != 0).sum(-1) == 18] == X.SEP).any()
    u = c.u_tok
    hit = (w["enc_mlm"] >= 0)
    assert hit[u[..., :32] == np.float32(0.14)].any() and not hit[u[..., :32] >= np.float32(0.15)].any()
    c, w = f["r12"]
    assert (w["enc_sep"][:, 11, :24] != 0).all() and (w["enc_sep"][:, 11, 24] == 0).all() and w["enc_sep"].shape[-1] == 25 and (w["enc_sep"] >= 32).any()
    assert c.valid is not None and not w["dec_labels"][c.valid == 0].any()
    c, w = f["full"]
    assert c.T == 256 and c.Ud == 25 and w["enc_ids"].shape == (2, 10, 256)


def _host_append(c):
    from gst_visdial_amd.generate import append_to_context
    ids, ln, new = torch.as_tensor(c.ctx_ids).clone(), torch.as_tensor(c.ctx_len).clone(), torch.as_tensor(c.new_ids)
    seg = None if c.segments is None else torch.as_tensor(c.segments).clone()
    n, bad = append_to_context(ids, ln, new, c.sep_id, segments=seg, segment_value=c.segment_value if seg is not None else None)
    return ids, ln, seg, n, bad


def _assert_same_as_host(c):
    ids, ln, seg, n, bad = _host_append(c)
    r = X.append_rule(c.ctx_ids, c.ctx_len, c.new_ids, c.sep_id, c.segments, c.segment_value,
                      (np.asarray(c.ctx_ids) != 0).astype(np.float32))
    assert np.array_equal(r["ctx_ids"], ids.numpy()) and np.array_equal(r["ctx_len"], ln.numpy()), c.name
    assert np.array_equal(r["n_out"], n.numpy()) and np.array_equal(np.nonzero(r["abnormal"])[0], bad.numpy()), c.name
    assert seg is None or np.array_equal(r["segments"], seg.numpy()), c.name
    assert np.array_equal(r["att_mask"], (ids != 0).float().numpy()) and not r["full"].any(), c.name


def test_append_rule_equals_append_to_context_on_random_cases():
    cases = X.append_random_cases(200)
    assert sum(len(c.ctx_len) for c in cases) == 200
    overflow = 0
    for c in cases:
        _assert_same_as_host(c)
        overflow += int(((c.new_ids != 0).sum(-1) + c.ctx_len > c.ctx_ids.shape[1]).sum())
    assert 10 < overflow < 190                                  # both branches are exercised


def test_append_rule_equals_append_to_context_on_the_edge_table():
    for c in X.append_edge_cases():
        T = c.ctx_ids.shape[1]
        n = (c.new_ids != 0).sum(-1)
        kinds = set(zip((c.ctx_len + n - T).tolist(), n.tolist()))
        assert (0, 4) in kinds and (1, 4) in kinds and (1, 2) in kinds and any(k[1] == 0 for k in kinds)
        assert (c.ctx_len == T).any() and (c.new_ids[5, :4] == 0).any()
        r = X.append_rule(c.ctx_ids, c.ctx_len, c.new_ids, c.sep_id, c.segments, c.segment_value, None, c.abnormal, c.full)
        full = c.ctx_len >= T
        assert np.array_equal(r["full"], full.astype(np.int32)) and r["abnormal"][3] == 1
        assert np.array_equal(r["ctx_ids"][full], c.ctx_ids[full]) and (r["n_out"][full] == 0).all()
        with pytest.raises(RuntimeError, match="context already full"):
            _host_append(c)                                     # the host function raises where the rule records `full`
        keep = ~full                                            # the same table without the full row: equal to the host function
        sub = c._replace(ctx_ids=c.ctx_ids[keep], ctx_len=c.ctx_len[keep], new_ids=c.new_ids[keep],
                         segments=None if c.segments is None else c.segments[keep])
        _assert_same_as_host(sub)


def test_harness_passes_on_the_rules_and_catches_wrong_backends(fixture):
    be = X.NumpyBackend()
    for c in X.append_edge_cases() + X.append_random_cases(16, allow_full=True):
        X.run_append_case(be, c)
    for c in X.rows_cases()[:4]:
        X.run_rows_case(be, c)
    X.run_rows_case(be, fixture[0][0], fixture[0][1])

    class SkipsPadding(X.NumpyBackend):                         # leaves the zero tail to a pre-zeroed buffer: poison stays
        def rows(self, *a, out=None, **k):
            keep = out["enc_seg"].clone()
            X.NumpyBackend.rows(self, *a, out=out, **k)
            out["enc_seg"][out["enc_ids"] == 0] = keep[out["enc_ids"] == 0]

    class WritesPastRow(X.NumpyBackend):
        def rows(self, *a, out=None, **k):
            X.NumpyBackend.rows(self, *a, out=out, **k)
            torch.as_strided(out["dec_ids"], (1,), (1,), out["dec_ids"].storage_offset() + out["dec_ids"].shape[1]).fill_(0)

    class ClearsFlags(X.NumpyBackend):
        def append(self, ctx_ids, ctx_len, new_ids, sep_id, abnormal, full, **k):
            abnormal.zero_()
            X.NumpyBackend.append(self, ctx_ids, ctx_len, new_ids, sep_id, abnormal, full, **k)

    class CountsThenCopiesNonZero(X.NumpyBackend):              # copies the n non-zero ids instead of the first n entries
        def append(self, ctx_ids, ctx_len, new_ids, sep_id, abnormal, full, **k):
            packed = torch.zeros_like(new_ids)
            for b in range(new_ids.shape[0]):
                nz = new_ids[b][new_ids[b] != 0]
                packed[b, :nz.numel()] = nz
            X.NumpyBackend.append(self, ctx_ids, ctx_len, packed, sep_id, abnormal, full, **k)

    c = X.rows_cases()[1]
    for bad in (SkipsPadding(), WritesPastRow()):
        with pytest.raises(AssertionError):
            X.run_rows_case(bad, c)
    for bad in (ClearsFlags(), CountsThenCopiesNonZero()):
        with pytest.raises(AssertionError):
            X.run_append_case(bad, X.append_edge_cases()[1])
