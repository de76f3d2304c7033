"""gstvd_cos_topk on a real MI355X, bit for bit against tests/exact_synonym.py's `topk_rule`.

Exact-sum inputs: rows of +-0.25 (16 non-zeros: norm exactly 1; every dot product a multiple of 1/16, exact in any summation
order), hence many ties -- which is the point: the order among equal values is part of the rule.  Random inputs (the fixture,
gaussian V = 2048, D = 300): indices equal wherever the float64 gaps on both sides exceed 4e-5, values within 2e-5 -- the error
of a D-term fp32 sum is <= (D - 1) * 2^-24 * sum|a b| <= 1.8e-5 for unit rows."""
import numpy as np
import pytest
import torch

import exact_synonym as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON_I, GUARD = -77, 2
ROUTES = ("many", "few")


def run(E, src, K, threshold, route, V=None, D=None, ld_pad=4, row_pad=3):
    """Launch inside poisoned windows: the table has NaN in `ld_pad` padding columns and `row_pad` rows behind V; idx / val sit
    between guard rows, the workspace between guard bytes; all guards are checked afterwards."""
    from gst_visdial_amd import ops
    V = E.shape[0] if V is None else V
    D = E.shape[1] if D is None else D
    tab = torch.full((V + row_pad, D + ld_pad), float("nan"), dtype=torch.float32)
    tab[:V, :D] = torch.from_numpy(E[:V, :D])
    tab = tab.to(DEV)
    n = V if src is None else len(src)
    s = None if src is None else torch.tensor(src, dtype=torch.int32, device=DEV)
    idx_buf = torch.full((n + 2 * GUARD, K), POISON_I, dtype=torch.int32, device=DEV)
    val_buf = torch.full((n + 2 * GUARD, K), float("nan"), dtype=torch.float32, device=DEV)
    need = ops.cos_topk_ws_bytes(n, V, K)
    ws_buf = torch.full((need + 128,), 0xAB, dtype=torch.uint8, device=DEV)
    idx, val = ops.cos_topk(tab, s, K=K, threshold=threshold, route=route, V=V, D=D, idx=idx_buf[GUARD:GUARD + n],
                            val=val_buf[GUARD:GUARD + n], ws=ws_buf[64:64 + need])
    torch.cuda.synchronize()
    for g in (idx_buf[:GUARD], idx_buf[GUARD + n:]):
        assert bool((g == POISON_I).all()), "idx guard rows written"
    for g in (val_buf[:GUARD], val_buf[GUARD + n:]):
        assert bool(torch.isnan(g).all()), "val guard rows written"
    assert bool((ws_buf[:64] == 0xAB).all()) and bool((ws_buf[64 + need:] == 0xAB).all()), "workspace guard bytes written"
    return idx.cpu().numpy(), val.cpu().numpy()


def check(E, src, K, threshold, V=None, D=None):
    V = E.shape[0] if V is None else V
    D = E.shape[1] if D is None else D
    E64 = E[:V, :D].astype(np.float64)
    rows = np.arange(V) if src is None else np.asarray(src)
    dots = np.zeros((len(rows), V))
    ok = (rows >= 0) & (rows < V)
    dots[ok] = E64[rows[ok]] @ E64.T
    want_i, want_v = X.topk_rule(dots, rows, K, threshold)
    out = []
    for route in ROUTES:
        got_i, got_v = run(E, src, K, threshold, route, V, D)
        assert np.array_equal(got_i, want_i), (route, V, D, K, len(rows))
        assert np.array_equal(got_v, want_v.astype(np.float32)), (route, V, D, K, len(rows))
        out.append((got_i, got_v))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()


def sources(V, n, seed):
    """n source rows, unordered, with repeats, and (from 5 on) one entry outside the table."""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, V, size=n)
    if n >= 2:
        src[-1] = src[0]
    if n >= 5:
        src[2] = V if seed % 2 else -1
    return src.tolist()


@pytest.mark.parametrize("D", [4, 8, 300])
@pytest.mark.parametrize("V", [1, 15, 16, 17, 63, 64, 65, 130])
def test_shape_grid(V, D):
    E = X.exact_unit_rows(V, D, seed=V * 1000 + D)
    for K in (1, 3, 10, 16):                               # K > V - 1 at the small V: the tail stays unused
        check(E, None, K, None)                            # all rows
    for i, n in enumerate((1, 5, 64, 65)):
        check(E, sources(V, n, seed=V + n), (10, 3, 16, 1)[i], None)


def test_threshold():
    E = X.exact_unit_rows(130, 300, seed=1)
    E[1] = E[0]
    E[2, :] = E[0]
    nz = np.nonzero(E[0])[0]
    E[2, nz[0]] = -E[0, nz[0]]                              # dot(0, 2) = 14/16 exactly
    src = [0, 5, 77]
    check(E, src, 10, 2.0)                                  # nothing passes
    idx, _ = run(E, src, 10, 2.0, "few")
    assert (idx == -1).all()
    check(E, src, 16, float("-inf"))                        # everything passes
    check(E, src, 16, None)
    check(E, src, 10, 0.875)                                # a value exactly equal to the threshold is kept
    idx, val = run(E, src, 10, 0.875, "many")
    assert idx[0, :2].tolist() == [1, 2] and val[0, :2].tolist() == [1.0, 0.875] and idx[0, 2] == -1
    check(E, None, 10, 0.0625)
    check(E, None, 10, 0.0)


def test_self_exclusion_and_duplicates():
    E = X.exact_unit_rows(65, 300, seed=2)
    E[40] = E[3]
    E[64] = E[3]
    check(E, None, 3, None)
    idx, val = run(E, [3, 40, 64], 3, 0.5, "few")
    assert idx[0, :2].tolist() == [40, 64] and idx[1, :2].tolist() == [3, 64] and idx[2, :2].tolist() == [3, 40]
    assert (val[:, :2] == 1.0).all()
    assert not (idx == np.array([[3], [40], [64]])).any()   # the source itself never


def test_routes_census_and_determinism():
    from gst_visdial_amd import ops
    E = X.exact_unit_rows(130, 300, seed=3)
    before = dict(ops.COS_TOPK_CENSUS)
    a = [run(E, None, 10, None, r) for r in ROUTES]
    b = [run(E, None, 10, None, r) for r in ROUTES]
    assert ops.COS_TOPK_CENSUS["many"] == before["many"] + 2 and ops.COS_TOPK_CENSUS["few"] == before["few"] + 2
    for (ia, va), (ib, vb) in zip(a, b):
        assert np.array_equal(ia, ib) and va.tobytes() == vb.tobytes()
    assert np.array_equal(a[0][0], a[1][0]) and a[0][1].tobytes() == a[1][1].tobytes()
    assert ops.cos_topk_route(8, 65713) == "few" and ops.cos_topk_route(65713, 65713) == "many"
    # the route chosen without forcing is one of the two and gives the same bits
    tab = torch.from_numpy(E).to(DEV)
    idx, val = ops.cos_topk(tab, None, K=10, threshold=None)
    assert np.array_equal(idx.cpu().numpy(), a[0][0]) and val.cpu().numpy().tobytes() == a[0][1].tobytes()


def random_case(ehat, K, threshold, gap, label):
    """Indices equal wherever the float64 gaps on both sides (and to the cut) exceed `gap`; values within 2e-5; both routes equal
    bits; at most 5 % of the used positions left out."""
    V = ehat.shape[0]
    exact = ehat.astype(np.float64) @ ehat.astype(np.float64).T
    want_i, want_v = X.topk_rule(exact, np.arange(V), K, threshold)
    outs = [run(ehat, None, K, threshold, r) for r in ROUTES]
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1].tobytes() == outs[1][1].tobytes()
    got_i, got_v = outs[0]
    order = np.sort(np.where(np.eye(V, dtype=bool), -np.inf, exact), axis=1)[:, ::-1]        # self excluded, descending
    checked = np.ones((V, K), bool)
    for k in range(K):
        up = order[:, k - 1] - order[:, k] if k else np.full(V, np.inf)
        down = order[:, k] - order[:, k + 1]
        checked[:, k] = (up > gap) & (down > gap)
        if threshold is not None:
            checked[:, k] &= np.abs(order[:, k] - threshold) > gap
    used = want_i >= 0
    left_out = 1.0 - checked[used].mean() if used.any() else 0.0
    same = used & (got_i == want_i)
    err = np.abs(got_v[same] - want_v[same]).max()
    print("%s: %d used positions, %.2f %% left out, value error %.3e" % (label, int(used.sum()), 100 * left_out, err))
    assert left_out <= 0.05
    assert np.array_equal(got_i[checked], want_i[checked])
    assert err <= 2e-5
    return got_i, got_v


def test_fixture_against_the_reference():
    fx = X.load_fixture()
    emb = fx["emb"].astype(np.float64)
    ehat = np.asarray(emb / np.linalg.norm(emb, axis=1, keepdims=True), "float32")
    K, thr, gap = int(fx["K"]), float(fx["threshold"]), float(fx["gap"])
    got_i, got_v = random_case(ehat, K, thr, gap, "fixture")
    chk = fx["checked"]
    assert 1.0 - chk.mean() <= 0.05
    assert np.array_equal(got_i[chk], fx["ref_idx"][chk])
    assert np.abs(got_v - fx["ref_val"])[chk].max() <= 2e-5


def test_gaussian_2048():
    rng = np.random.RandomState(11)
    e = rng.standard_normal((2048, 300))
    ehat = np.asarray(e / np.linalg.norm(e, axis=1, keepdims=True), "float32")
    random_case(ehat, 10, None, 4e-5, "gaussian V 2048")


def test_refusals():
    from gst_visdial_amd import ops, _lib
    tab = torch.zeros(8, 12, device=DEV)
    with pytest.raises(_lib.GstvdError):
        ops.cos_topk(tab, None, K=17)
    with pytest.raises(_lib.GstvdError):
        ops.cos_topk(tab, None, K=3, D=6)                   # D % 4
    with pytest.raises(_lib.GstvdError):
        ops.cos_topk(torch.zeros(4, 516, device=DEV), None, K=3)          # a D the kernel cannot hold
    with pytest.raises(_lib.GstvdError):
        ops.cos_topk(tab, None, K=3, route="both")
