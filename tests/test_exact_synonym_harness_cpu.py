"""The numpy rules of tests/exact_synonym.py checked on the host: `topk_rule` against what the reference's
pick_most_similar_words_batch returned on tests/golden/tiny_synonym.npz (tools/make_golden_synonym.py), and both rules on
hand-written cases."""
import numpy as np

import exact_synonym as X


def test_topk_rule_equals_the_reference_where_the_fixture_checks():
    fx = X.load_fixture()
    emb = fx["emb"].astype(np.float64)
    ehat = np.asarray(emb / np.linalg.norm(emb, axis=1, keepdims=True), "float32").astype(np.float64)
    V = ehat.shape[0]
    K, thr = int(fx["K"]), float(fx["threshold"])
    idx, val = X.topk_rule(ehat @ ehat.T, np.arange(V), K, thr)
    chk = fx["checked"]
    assert chk.shape == (V, K) and fx["ref_idx"].shape == (V, K)
    assert np.array_equal(idx[chk], fx["ref_idx"][chk])
    assert np.abs(val - fx["ref_val"])[chk].max() <= 2e-5
    assert np.array_equal((idx >= 0).sum(1), fx["ref_count"])                     # nothing lies near the cut: the counts agree
    assert len(set(fx["words"].tolist())) == V


def test_fixture_leaves_at_most_five_percent_unchecked():
    fx = X.load_fixture()
    left_out = 1.0 - fx["checked"].mean()
    used = fx["ref_idx"] >= 0
    print("unchecked: %.3f %% of all positions, %.3f %% of the used ones" % (100 * left_out, 100 * (1.0 - fx["checked"][used].mean())))
    assert left_out <= 0.05 and 1.0 - fx["checked"][used].mean() <= 0.05
    assert fx["ref_count"].min() >= 1 and float(fx["gap"]) == 4e-5


def test_topk_rule_by_hand():
    d = np.array([[1.0, 0.5, 0.75, 0.5, 0.25],
                  [0.5, 1.0, 0.5, 0.5, 0.5],
                  [0.0, 0.0, 0.0, 0.0, 0.0]])
    idx, val = X.topk_rule(d, [0, 1, 9], 3)
    assert idx.tolist() == [[2, 1, 3], [0, 2, 3], [-1, -1, -1]]                   # ties to the smaller index; row 9: outside
    assert val.tolist() == [[0.75, 0.5, 0.5], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0]]
    idx, val = X.topk_rule(d, [0, 1, 2], 3, 0.5)
    assert idx.tolist() == [[2, 1, 3], [0, 2, 3], [-1, -1, -1]]                   # a value equal to the threshold is kept
    idx, _ = X.topk_rule(d, [0, 1, 2], 3, 0.500001)
    assert idx.tolist() == [[2, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    d2 = np.array([[1.0, 1.0, 1.0]])
    idx, val = X.topk_rule(d2, [1], 4)                                            # a duplicate of the source is kept, the source not
    assert idx.tolist() == [[0, 2, -1, -1]] and val.tolist() == [[1.0, 1.0, 0.0, 0.0]]
    E = X.exact_unit_rows(9, 300, 0)
    assert np.all(np.abs(E).sum(1) == 4.0) and np.all((E.astype(np.float64) ** 2).sum(1) == 1.0)
    assert np.all((E.astype(np.float64) @ E.T.astype(np.float64)) * 16 % 1 == 0)


def test_replace_rule_by_hand():
    C, S, P = 101, 102, 0
    ids = np.array([[C, 5, 6, S, 7, 5, S, 5, S, P, P, P]])
    out, n = X.replace_rule(ids, [[(0, [5], [8, 9])]], S, P)
    assert out.tolist() == [[C, 8, 9, 6, S, 7, 5, S, 5, S, P, P]] and n.tolist() == [1]
    out, n = X.replace_rule(ids, [[(1, [7, 5], [4])]], S, P)
    assert out.tolist() == [[C, 5, 6, S, 4, S, 5, S, P, P, P, P]] and n.tolist() == [1]
    out, n = X.replace_rule(ids, [[(3, [5], [4])]], S, P)                         # fewer than 4 separators
    assert np.array_equal(out, ids) and n.tolist() == [0]
    out, n = X.replace_rule(ids, [[(1, [5, S], [4])]], S, P)                      # never across a separator
    assert np.array_equal(out, ids) and n.tolist() == [0]
    out, n = X.replace_rule(ids, [[(0, [5], [1, 2, 3, 4, 1, 2])]], S, P)          # growth drops the tail
    assert out.tolist() == [[C, 1, 2, 3, 4, 1, 2, 6, S, 7, 5, S]] and n.tolist() == [1]
    out, n = X.replace_rule(np.array([[C, 3, 3, 3, S]]), [[(0, [3, 3], [1])]], S, P)
    assert out.tolist() == [[C, 1, 3, S, P]] and n.tolist() == [1]                # greedy, left to right, no overlap
    out, n = X.replace_rule(np.array([[C, 3, 3, 3, S, P, P, P, P]]), [[(0, [3], [1, 2]), (0, [2, 1], [9])]], S, P)
    assert out.tolist() == [[C, 1, 9, 9, 2, S, P, P, P]] and n.tolist() == [5]             # the second sees the first one's output
    cont = np.zeros(50, np.uint8)
    cont[40:] = 1
    ids = np.array([[C, 5, 40, 5, S, 41, 5, S]])
    out, n = X.replace_rule(ids, [[(0, [5], [7]), (1, [5], [7])]], S, P, cont)
    assert out.tolist() == [[C, 5, 40, 7, S, 41, 7, S]] and n.tolist() == [2]
    out, n = X.replace_rule(ids, [[(1, [41, 5], [7])]], S, P, cont)               # may not start on a ## piece
    assert n.tolist() == [0]
    seg, sepi, att = X.refresh_rule(np.array([[C, 5, S, 6, 7, S, 8, S, P, P]]), S, P, 4, [1])
    assert seg.tolist() == [[1, 1, 1, 0, 0, 0, 1, 1, 0, 0]] and sepi.tolist() == [[2, 5, 7, 0]]
    assert att.tolist() == [[1, 1, 1, 1, 1, 1, 1, 1, 0, 0]]
    _, sepi, _ = X.refresh_rule(np.array([[C, S, S, S, P]]), S, P, 2)
    assert sepi.tolist() == [[1, 2]]
