"""CPU proof of tests/exact_disc_rows.py: the numpy rules reproduce the fixture recorded from the reference's own loader bit for
bit (rows, labels, image_label, zeroed features), the case table covers what it promises, and the harness itself runs (and
catches wrong backends) on a numpy stand-in."""
import os

import numpy as np
import pytest
import torch

import exact_disc_rows as X
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    from gst_visdial_amd.selfcheck import read_npz
    return X.fixture_cases(read_npz(os.path.join(GOLDEN, "disc_rows.npz")))


def test_rows_rule_reproduces_the_reference_fixture(fixture):
    assert sorted(c.name for c, _, _ in fixture) == ["eval_a", "eval_b", "full_eval", "full_train", "train_a", "train_b"]
    for c, want, _ in fixture:
        got = X.rule_of(c)
        for k, w in want.items():
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, (c.name, k, got[k].dtype, w.dtype, got[k].shape, w.shape)
            bits = (lambda a: a.view(np.int32)) if w.dtype == np.float32 else (lambda a: a)
            assert np.array_equal(bits(got[k]), bits(w)), (c.name, k, np.argwhere(got[k] != w)[:5])
        assert set(want) == set(X.ROWS_OUT) - (set() if c.train else {"nsp_labels"})


def test_image_rule_reproduces_the_reference_fixture(fixture):
    seen = 0
    for c, _, img in fixture:
        if img is None:
            continue
        feats, label = X.image_rule(img["feats"], img["image_mask"], img["u_img"], img["forced_region"], c.mask_prob)
        assert np.array_equal(label, img["out_label"]) and label.dtype == img["out_label"].dtype, c.name
        assert np.array_equal(feats.view(np.int32), img["out_feats"].view(np.int32)), c.name
        seen += 1
    assert seen == 3


def test_fixture_covers_what_it_promises(fixture):
    f = {c.name: (c, w, img) for c, w, img in fixture}
    kinds = set()
    for name in ("train_a", "train_b", "full_train"):
        c, w, img = f[name]
        assert c.mask_prob == 0.15 and (w["mask"] >= 0).any()
        for r in range(c.rows.shape[1]):
            d, j, slot = (int(x) for x in c.rows[:, r])
            if slot:
                C, F = X.feasible(c.cap, c.ques, c.ans, c.opts, c.gt, d, j, c.T, c.num_options)
                kinds.add("none" if not F else "all" if len(F) == len(C) else "some")
        u, hit = c.u_tok, w["mask"] >= 0
        assert not hit[u >= np.float32(0.15)].any() and hit[u == np.nextafter(np.float32(0.15), np.float32(0))].any()
        assert (u == 0).any() and not hit[:, 0].any()                                       # a draw of 0 where no token sits
    assert kinds == {"none", "all", "some"}
    c, w, img = f["train_a"]
    assert img["image_mask"][1, 30] == 0 and img["out_label"][1, 30] == 1 and (img["out_label"][:, 0] == 0).all()   # forced padding
    assert (img["out_feats"][0][img["out_label"][0] == 1] == 0).all(-1).any()
    c, w, img = f["train_b"]
    assert c.tot_rounds == 3 and c.num_options == 4 < c.opts.shape[2] and c.dense is not None
    assert set(np.unique(w["segments"][:, 0])) == {0, 1} and w["hist_len"].max() == 5
    neg = w["neg_option"] >= 0
    assert np.array_equal(w["nsp_labels"][neg, 0], c.dense[c.rows[0, neg], c.rows[1, neg], w["neg_option"][neg]].astype(np.float32))
    c, w, _ = f["eval_a"]
    assert (w["sep_indices"][np.arange(len(w["hist_len"])), w["hist_len"]] >= c.T).any() and "nsp_labels" not in w
    c, w, _ = f["eval_b"]
    assert c.tot_rounds == 2 and w["hist_len"].max() == 3 and c.num_options == 4
    for name in ("full_train", "full_eval"):
        c, w, _ = f[name]
        assert c.T == 256 and c.opts.shape[1:3] == (10, 100) and w["tokens"].shape == (24, 256)
    assert (f["full_eval"][1]["neg_option"] >= 64).any()                                   # the second ballot


def test_eval_relevance_is_reordered_like_the_loader(fixture):
    from gst_visdial_amd.selfcheck import read_npz
    from gst_visdial_amd.disc_rows import eval_option_order
    g = read_npz(os.path.join(GOLDEN, "disc_rows.npz"))
    for name in ("eval_a", "eval_b", "full_eval"):
        gt, no = torch.as_tensor(g[name + "::gt"]), int(g[name + "::num_options"])
        order = eval_option_order(gt, g[name + "::opts"].shape[2], no)
        for (d, j), _ in np.ndenumerate(g[name + "::gt"]):
            assert order[d, j].tolist() == [X.eval_option(int(gt[d, j]), k) for k in range(no)]
        rid = torch.as_tensor(g[name + "::round_id"])
        rel = torch.gather(torch.as_tensor(g[name + "::gt_relevance"]), 1, order[torch.arange(gt.shape[0]), rid - 1])
        assert torch.equal(rel, torch.as_tensor(g[name + "::out_gt_relevance"]))


def test_case_table_covers_what_it_promises():
    cases = {c.name: c for c in X.cases()}
    c = cases["eval_tr11_no5"]
    w = X.rule_of(c)
    row = lambda d, j, s: next(r for r in range(c.rows.shape[1]) if tuple(c.rows[:, r]) == (d, j, s))
    last = lambda r: int(w["sep_indices"][r, w["hist_len"][r]])
    assert c.T == 32 and c.ques.shape == (3, 3, 18) and c.opts.shape[2] == 5
    assert c.gt[0].tolist() == [0, 4, 2] and sorted(c.gt[1].tolist()) == sorted(c.gt[2].tolist()) == [0, 2, 4]
    # dialog 0, round 2 (gt 2: slots 0..4 are options 2, 0, 1, 3, 4 of 8, 2, 3, 0, 1 tokens)
    assert [int(w["neg_option"][row(0, 2, s)]) for s in range(5)] == [2, 0, 1, 3, 4]
    assert last(row(0, 2, 1)) == 31 and w["tokens"][row(0, 2, 1), 31] == X.SEP                       # fits exactly
    assert last(row(0, 2, 2)) == 32 and w["tokens"][row(0, 2, 2), 31] not in (0, X.SEP)              # loses its final [SEP]
    assert last(row(0, 2, 0)) == 37 and w["tokens"][row(0, 2, 0), 31] not in (0, X.SEP)              # cut inside the option
    r = row(0, 2, 3)
    assert last(r) == 29 and w["tokens"][r, 28] == w["tokens"][r, 29] == X.SEP                        # an empty option: a lone [SEP]
    r = row(1, 2, 0)
    assert w["sep_indices"][r, 5] == w["sep_indices"][r, 4] + 1                                      # an empty question
    assert (w["att"].sum(-1) == np.minimum(w["sep_indices"][np.arange(45), w["hist_len"]] + 1, 32)).all()
    assert (w["segments"][:, 0] == 1).all() and (w["hist_len"] == 2 * c.rows[1] + 2).all()            # tot_rounds 11: nothing pruned
    w2 = X.rule_of(cases["eval_tr2_no3"])
    j = cases["eval_tr2_no3"].rows[1]
    assert (w2["segments"][j >= 1, 0] == 0).all() and (w2["segments"][j == 0, 0] == 1).all()
    assert (w2["hist_len"][j >= 1] == 3).all() and (w2["hist_len"][j == 0] == 2).all() and cases["eval_tr2_no3"].num_options == 3 < 5
    # negatives: all feasible, exactly one, none (cut to len(a_j) = 2, 18 and 0)
    c = cases["train_tr11_no5_p15"]
    F = lambda d, j: X.feasible(c.cap, c.ques, c.ans, c.opts, c.gt, d, j, c.T, c.num_options)
    assert len(F(1, 0)[1]) == 4 and F(1, 1)[1] == [2] and F(1, 2)[1] == [] and F(2, 0)[1] == [] and F(2, 1)[1] == []
    assert [len(X.utt(c.ans[d, j])) for d, j in ((1, 2), (2, 0), (2, 1))] == [2, 18, 0]
    w = X.rule_of(c)
    rows = [r for r in range(c.rows.shape[1]) if tuple(c.rows[:2, r]) == (2, 1) and c.rows[2, r] > 0]
    assert all(w["sep_indices"][r, 4] == w["sep_indices"][r, 3] + 1 for r in rows)                   # the negative cut to nothing
    assert sorted(set(int(w["neg_option"][r]) for r in rows)) == [0, 1, 3, 4]                        # draws 0, .3, .5, 1 - ulp over C = [0, 1, 3, 4]
    rows = [r for r in range(c.rows.shape[1]) if tuple(c.rows[:2, r]) == (1, 2) and c.rows[2, r] > 0]
    assert all(w["sep_indices"][r, 6] - w["sep_indices"][r, 5] - 1 == 2 for r in rows)
    hit = w["mask"] >= 0
    assert not hit[c.u_tok == np.float32(0.15)].any() and hit[c.u_tok < np.float32(0.15)].any()
    c = cases["train_tr2_no4_dense"]
    w = X.rule_of(c)
    neg = w["neg_option"] >= 0
    s = c.dense[c.rows[0, neg], c.rows[1, neg], w["neg_option"][neg]]
    assert (w["nsp_labels"][neg, 1] != (np.float32(1) - s.astype(np.float32))).all()                 # not the fp32 subtraction
    assert np.array_equal(w["nsp_labels"][neg, 1], (1.0 - s).astype(np.float32))
    assert cases["train_full_T256_O100"].rows.shape == (3, 24) and cases["eval_full_T256_O100"].opts.shape[1:3] == (10, 100)
    w = X.rule_of(cases["train_full_T256_O100"])
    assert (w["neg_option"] >= 64).any() and (0 <= w["neg_option"]).any() and (w["neg_option"][w["neg_option"] >= 0] < 64).any()
    w = X.rule_of(cases["eval_invalid_rows"])
    assert w["tokens"][0, 0] == X.CLS and not w["tokens"][1:6].any() and w["tokens"][6, 0] == 0 and (w["mask"][1:] == -1).all()


def test_harness_passes_on_the_rule_and_catches_wrong_backends(fixture):
    be = X.NumpyBackend()
    for c in X.cases():
        X.run_case(be, c)
    for c, want, _ in fixture[:2] + fixture[4:5]:
        X.run_case(be, c, want)

    class SkipsOneElement(X.NumpyBackend):                      # leaves one padding element to a pre-zeroed buffer: poison stays
        def rows(self, *a, out=None, **k):
            keep = out["segments"][3, -1].clone()
            X.NumpyBackend.rows(self, *a, out=out, **k)
            out["segments"][3, -1] = keep

    class WritesPastRow(X.NumpyBackend):
        def rows(self, *a, out=None, **k):
            X.NumpyBackend.rows(self, *a, out=out, **k)
            torch.as_strided(out["mask"], (1,), (1,), out["mask"].storage_offset() + out["mask"].shape[1]).fill_(-1)

    class ReadsThePadColumns(X.NumpyBackend):                   # takes the option row's stride for its width
        def rows(self, cap, ques, ans, opts, *a, **k):
            wide = torch.as_strided(opts, opts.shape[:3] + (opts.stride(2),), opts.stride(), opts.storage_offset())
            return X.NumpyBackend.rows(self, cap, ques, ans, wide, *a, **k)

    class SubtractsInFp32(X.NumpyBackend):
        def rows(self, *a, out=None, **k):
            X.NumpyBackend.rows(self, *a, out=out, **k)
            neg = out["neg_option"] >= 0
            out["nsp_labels"][neg, 1] = 1 - out["nsp_labels"][neg, 0]

    c = {c.name: c for c in X.cases()}
    for bad, name in ((SkipsOneElement(), "eval_tr11_no5"), (WritesPastRow(), "eval_tr11_no5"),
                      (ReadsThePadColumns(), "train_full_T256_O100"), (SubtractsInFp32(), "train_tr2_no4_dense")):
        with pytest.raises(AssertionError):
            X.run_case(bad, c[name])
