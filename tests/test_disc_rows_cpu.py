"""CPU side of the discriminative rows: the negative rule draws the distribution of the loader's choice / remove loop (exact
fractions), the bin edges of floor(u * n), the error paths (there is no CPU path) and the dispatch of a batch on its keys."""
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_disc_rows as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_everywhere():
    from gst_visdial_amd import _lib, ops, disc_rows
    assert "gstvd_disc_rows" in _lib.SIGNATURES and callable(ops.disc_rows) and callable(disc_rows.eval_item)
    assert "disc_rows.hip" in open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "Makefile")).read()
    assert _lib.ABI_VERSION == 9                                        # an entry point was added, no signature changed


def _loop_distribution(fits):
    """The loader's loop (dataloader_visdial_disc.py:165-177) over candidates 0..n-1, in this test's own words: draw uniformly from
    what is left; a candidate that fits ends the loop; one that does not is removed; when nothing is left, the last draw stands.
    -> {candidate: probability}, exact, by walking every order in which the loop can draw."""
    dist = {}

    def walk(left, p, last):
        if not left:
            dist[last] = dist.get(last, 0) + p
            return
        for c in left:
            q = p * Fraction(1, len(left))
            if fits[c]:
                dist[c] = dist.get(c, 0) + q
            else:
                walk([x for x in left if x != c], q, c)
    walk(list(range(len(fits))), Fraction(1), None)
    return dist


def test_the_negative_rule_draws_the_distribution_of_the_choice_remove_loop():
    """Every feasibility pattern of |C| <= 5.  The rule: uniform over the feasible candidates, or over all of them when none is
    feasible -- its bins [k / n, (k + 1) / n) have measure 1 / n each, and X.pick maps a draw inside bin k to element k."""
    seen = 0
    for n in range(1, 6):
        for fits in itertools.product((False, True), repeat=n):
            pool = [c for c in range(n) if fits[c]] or list(range(n))
            want = {c: Fraction(1, len(pool)) for c in pool}
            assert _loop_distribution(fits) == want, fits
            assert [pool[X.pick(np.float32((k + 0.5) / len(pool)), len(pool))] for k in range(len(pool))] == pool
            seen += 1
    assert seen == 2 + 4 + 8 + 16 + 32


def test_pick_at_the_bin_edges_is_the_exact_floor_of_the_fp32_draw_times_n():
    top = np.nextafter(np.float32(1), np.float32(0))
    for n in range(1, 101):
        assert X.pick(np.float32(0), n) == 0 and X.pick(top, n) == n - 1
        for k in range(1, n):
            edge = np.float32(k / n)
            for u in (edge, np.nextafter(edge, np.float32(0))):
                exact = Fraction(float(u)) * n                           # float(fp32) and Fraction(float) are both exact
                assert X.pick(u, n) == min(exact.numerator // exact.denominator, n - 1), (n, k, float(u))
    assert X.pick(np.float32(0.25), 4) == 1 and X.pick(np.nextafter(np.float32(0.25), np.float32(0)), 4) == 0
    assert X.pick(np.float32(1 / 3), 3) == 1                             # fp32(1/3) lies above 1/3: the edge belongs to bin 1


def _cpu_pools():
    cap, ques, ans, opts, gt = X.edge_pools()
    t = lambda x: torch.as_tensor(x)
    return dict(cap=t(cap), ques=t(ques), ans=t(ans), opts=t(opts), gt_index=t(gt), image_feat=torch.zeros(3, 7, 4),
                image_loc=torch.zeros(3, 7, 5), image_mask=torch.ones(3, 7, dtype=torch.long), image_target=torch.zeros(3, 7, 6))


PARAMS = dict(max_seq_len=32, visdial_tot_rounds=11, num_options=5, num_negative_samples=2, batch_size=4, mask_prob=0.15)


def test_cpu_tensors_and_disabled_uniforms_raise():
    from gst_visdial_amd import ops, disc_rows
    from gst_visdial_amd._lib import GstvdError
    b = _cpu_pools()
    rows = [torch.zeros(2, dtype=torch.int32)] * 3
    with pytest.raises(GstvdError, match="no CPU path"):
        ops.disc_rows(b["cap"], b["ques"], b["ans"], b["opts"], b["gt_index"], *rows, 32, 11, 5, False)
    with pytest.raises(GstvdError, match="no CPU path"):
        disc_rows.eval_item(b, 0, 10, PARAMS)
    with pytest.raises(GstvdError, match="no CPU path"):
        disc_rows.train_batch(b, b, dict(PARAMS, mask_prob=0.0))
    with pytest.raises(GstvdError, match="needs u_tok"):
        ops.disc_rows(b["cap"], b["ques"], b["ans"], b["opts"], b["gt_index"], *rows, 32, 11, 5, False, mask_prob=0.15)
    with pytest.raises(GstvdError, match="needs u_neg"):
        ops.disc_rows(b["cap"], b["ques"], b["ans"], b["opts"], b["gt_index"], *rows, 32, 11, 5, True)
    # the uniforms explicitly disabled: raised before anything is looked at, whatever device the pools are on
    b = {k: _FakeCuda(v) for k, v in b.items()}
    for off in ("u_tok", "u_img"):
        with pytest.raises(GstvdError, match="needs the uniforms u_tok"):
            disc_rows.train_batch(b, b, PARAMS, **{off: False})
    with pytest.raises(GstvdError, match="need the uniforms u_neg"):
        disc_rows.train_batch(b, b, dict(PARAMS, mask_prob=0.0), u_neg=False)


class _FakeCuda(object):
    """A pool tensor that claims to be on the GPU: enough for the argument checks that run in front of any device work."""

    def __init__(self, t):
        self.t, self.is_cuda, self.device, self.shape = t, True, "cuda:0", t.shape


def test_over_limit_shapes_raise():
    from gst_visdial_amd import ops
    from gst_visdial_amd._lib import GstvdError
    z = lambda *s: torch.zeros(*s, dtype=torch.int64)
    rows = [torch.zeros(2, dtype=torch.int32)] * 3

    def call(D=2, R=3, O=5, U=18, Lc=8, T=32, tot_rounds=11, num_options=5):
        return ops.disc_rows(z(D, Lc), z(D, R, U), z(D, R, U), z(D, R, O, U), z(D, R), *rows, T, tot_rounds, num_options, False)
    for kw, msg in ((dict(U=65), "U, Lc <= 64"), (dict(Lc=65), "U, Lc <= 64"), (dict(R=13), "separators"), (dict(O=101, num_options=100), "O <= 100"),
                    (dict(num_options=6), "num_options <= O"), (dict(num_options=1), "2 <= num_options"), (dict(tot_rounds=0), "tot_rounds >= 1"),
                    (dict(T=1), "T >= 2")):
        with pytest.raises(GstvdError, match=msg):
            call(**kw)
    with pytest.raises(GstvdError, match="no CPU path"):                # within the limits: only the device is wrong
        call(R=12, O=100, num_options=100, U=64, Lc=64)
    with pytest.raises(GstvdError, match="do not belong together"):
        ops.disc_rows(z(2, 8), z(2, 3, 18), z(2, 3, 17), z(2, 3, 5, 18), z(2, 3), *rows, 32, 11, 5, False)
    with pytest.raises(GstvdError, match="one stride"):
        ops.disc_rows(z(2, 8), z(2, 3, 18), z(2, 3, 18), z(2, 3, 18, 5).permute(0, 1, 3, 2), z(2, 3), *rows, 32, 11, 5, False)


def test_batches_are_dispatched_on_their_keys(monkeypatch):
    from gst_visdial_amd import evaluate_disc as ED, disc_rows
    b = _cpu_pools()
    assert disc_rows.is_pooled(b) and not disc_rows.is_pooled(dict(b, tokens=torch.zeros(1))) and not disc_rows.is_pooled(dict(tokens=1))
    calls = []

    class Enc(object):
        def eval(self):
            return self

        def nsp_scores(self, tokens, features, spatials, segments, att, image_mask):
            calls.append(("nsp", tuple(tokens.shape), att.dtype))
            return None, torch.arange(tokens.shape[0], dtype=torch.float32)

    def fake_eval_item(pools, start, end, params):
        calls.append(("eval_item", start, end))
        n = end - start
        return dict(tokens=torch.ones(n, 32, dtype=torch.long), segments=torch.zeros(n, 32, dtype=torch.long),
                    sep_indices=torch.zeros(n, 25, dtype=torch.long), mask=torch.zeros(n, 32, dtype=torch.long),
                    hist_len=torch.zeros(n, dtype=torch.long), att=torch.ones(n, 32), image_feat=torch.zeros(n, 7, 4),
                    image_loc=torch.zeros(n, 7, 5), image_mask=torch.ones(n, 7))
    monkeypatch.setattr(disc_rows, "eval_item", fake_eval_item)
    params = dict(PARAMS, device=torch.device("cpu"), mode="vd_eval_val")
    out = ED.score_batch(Enc(), b, params, rows_per_call=20)            # 3 x 3 x 5 = 45 rows: chunks of 20, 20, 5
    assert tuple(out.shape) == (3, 3, 5)
    assert [c for c in calls if c[0] == "eval_item"] == [("eval_item", 0, 20), ("eval_item", 20, 40), ("eval_item", 40, 45)]
    assert [c[2] for c in calls if c[0] == "nsp"] == [torch.float32] * 3                    # the kernel's mask is handed through
    # the same batch with `tokens`: the tensor path, untouched -- the pooled builder is not called
    del calls[:]
    w = X.rule_of(X.cases()[0])
    shape = lambda k: torch.as_tensor(w[k]).view(3, 3, 5, -1)
    tb = dict(b, tokens=shape("tokens"), segments=shape("segments"), sep_indices=shape("sep_indices"), mask=shape("mask"),
              hist_len=torch.as_tensor(w["hist_len"]).view(3, 3, 5))
    out = ED.score_batch(Enc(), tb, params, rows_per_call=20)
    assert tuple(out.shape) == (3, 3, 5) and [c[0] for c in calls] == ["nsp"] * 3 and calls[0][2] == torch.bool
    # metrics side of a pooled batch: the ground truth is slot 0, the relevance follows the slot order
    rel = torch.arange(15, dtype=torch.float32).view(3, 5)
    gi, gr = disc_rows.eval_targets(dict(b, gt_relevance=rel, round_id=torch.tensor([[1], [2], [3]])), params)
    assert not gi.any() and tuple(gi.shape) == (3, 3)
    gt = b["gt_index"]
    assert gr.tolist() == [[float(rel[d, X.eval_option(int(gt[d, d]), k)]) for k in range(5)] for d in range(3)]


def test_image_labels_equal_the_numpy_rule_on_the_cpu():
    """disc_rows.image_labels is plain torch: it runs wherever its tensors live, so the rule is pinned here without a GPU."""
    from gst_visdial_amd.disc_rows import image_labels
    gen = np.random.default_rng(2)
    feats = gen.standard_normal((4, 9, 5)).astype(np.float32)
    mask = np.ones((4, 9), np.int64)
    mask[1, 6:], mask[2, 1:], mask[3] = 0, 0, 0
    u = gen.random((4, 9))
    u[0, :4] = (0.15, np.float64(np.nextafter(np.float32(0.15), np.float32(0))), 0.135, np.nextafter(0.135, 0))
    forced = np.array([1, 8, 8, 4], np.int64)
    for p in (0.15, 0.0):
        f, lab = image_labels(torch.as_tensor(feats), torch.as_tensor(mask), torch.as_tensor(u), torch.as_tensor(forced), p)
        wf, wl = X.image_rule(feats, mask, u, forced, p)
        assert np.array_equal(lab.numpy(), wl) and np.array_equal(f.numpy(), wf), p
    assert wl[1, 8] == 1 and mask[1, 8] == 0 and (wl[:, 0] == 0).all()                      # a forced padding region keeps its 1
