"""CPU proof of tests/exact_gen_rows.py: the numpy rule reproduces the fixture recorded from the reference's own loader bit for bit,
the case table covers what it promises, the harness itself runs (and catches wrong backends) on a numpy stand-in, the entry point
is declared in every layer, and the host layers refuse what they must without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import exact_gen_rows as X
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def golden():
    from gst_visdial_amd.selfcheck import read_npz
    return read_npz(os.path.join(GOLDEN, "gen_rows.npz"))


@pytest.fixture(scope="module")
def fixture(golden):
    return X.fixture_cases(golden)


def test_rows_rule_reproduces_the_reference_fixture(fixture):
    assert sorted(c.name for c, _ in fixture) == sorted(X.FIXTURE_CASES)
    for c, want in fixture:
        got = X.rule_of(c)
        assert set(want) == set(X.out_names(c)) - ({"dec_option"} if c.mode.startswith("train") else set()), (c.name, sorted(want))
        for k, w in want.items():
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, (c.name, k, got[k].dtype, w.dtype, got[k].shape, w.shape)
            bits = (lambda a: a.view(np.int32)) if w.dtype == np.float32 else (lambda a: a)
            assert np.array_equal(bits(got[k]), bits(w)), (c.name, k, np.argwhere(got[k] != w)[:5])


def test_fixture_covers_what_it_promises(fixture):
    f = {c.name: (c, w) for c, w in fixture}
    for c, w in fixture:
        assert (c.T, c.Ud, c.ques.shape) == (256, 25, (2, 10, 18)), c.name
        last = w["sep_indices"][np.arange(len(w["hist_len"])), w["hist_len"]]
        assert (last >= c.T).any() and (last < c.T).any(), c.name                      # rows cut at T next to rows that fit
        assert (w["segments"][:, 0] == 1).all()
    c, w = f["eval"]
    assert c.opts.shape == (2, 10, 100, 18) and c.num_options == 100 and c.enc.shape == (2, 20) and c.dec.shape[1] >= 40
    assert (w["hist_len"] == 2 * c.enc[1] + 1).all() and (w["mlm"] == -1).all() and (w["dec_option"] >= 64).any()
    assert (w["dec_ids"][:, 0] == X.CLS).all() and ((w["dec_ids"] == X.SEP).sum(-1) == 1).all() and (w["dec_att"] == (w["dec_ids"] != 0)).all()
    c, w = f["eval_noise"]
    assert c.mask_prob == 0.15 and c.enc.shape[1] == c.dec.shape[1] == c.u_tok.shape[0] and np.array_equal(c.enc, c.dec[:2])
    hit = w["mlm"] >= 0
    assert hit.any() and (w["tokens"][hit] == X.MASK).all() and not hit[c.u_tok >= np.float32(0.15)].any()
    assert hit[c.u_tok == np.nextafter(np.float32(0.15), np.float32(0))].any() and (c.u_tok == 0).any() and not hit[:, 0].any()
    c, w = f["test"]
    assert c.opts.shape == (2, 1, 100, 18) and c.gt is None and c.enc[1].tolist() == [9, 3] and (w["dec_option"] == c.dec[2]).all()
    c, w = f["train_a"]
    assert (w["hist_len"] == 2 * c.enc[1] + 1).all() and not (w["dec_ids"] == X.SEP).any() and (w["dec_labels"] == X.SEP).any()
    assert (w["dec_att"].sum(-1) == (w["dec_labels"] != 0).sum(-1) + 1).all()
    c, w = f["train_q"]
    assert (w["hist_len"] == 2 * c.enc[1]).all() and w["hist_len"].min() == 0
    assert (f["train_a"][1]["dec_labels"] != w["dec_labels"]).any()


def test_eval_relevance_is_reordered_like_the_loader(golden):
    from gst_visdial_amd import gen_rows as GR
    t = lambda k: torch.as_tensor(golden[k])
    batch = dict(gt_index=t("pools::gt"), opts=t("pools::opts"), gt_relevance=t("eval::gt_relevance"), round_id=t("eval::round_id").view(-1, 1))
    gt_inds, rel = GR.eval_targets(batch, dict(num_options=100))
    assert torch.equal(rel, t("eval::out_gt_relevance")) and tuple(gt_inds.shape) == (2, 10) and not gt_inds.any()
    assert GR.eval_targets({k: v for k, v in batch.items() if k != "gt_relevance"}, None)[1] is None


def test_case_table_covers_what_it_promises():
    """A self-check of the table and the numpy rule only: it runs no library code and says nothing about the kernel, which
    tests/test_gen_rows_exact_gpu.py holds to this table."""
    cases = {c.name: c for c in X.cases()}
    assert set(c.mode for c in cases.values()) == set(X.MODES)
    c = cases["eval_no6"]
    w = X.rule_of(c)
    assert (c.T, c.Ud, c.ques.shape, c.opts.shape, c.cap.shape) == (32, 8, (3, 4, 8), (3, 4, 6, 8), (3, 8))
    erow = lambda d, j: next(r for r in range(c.enc.shape[1]) if tuple(c.enc[:, r]) == (d, j))
    drow = lambda d, j, s: next(r for r in range(c.dec.shape[1]) if tuple(c.dec[:, r]) == (d, j, s))
    last = lambda r: int(w["sep_indices"][r, w["hist_len"][r]])
    assert [last(erow(0, j)) + 1 for j in range(4)] == [14, 23, 32, 41]
    assert [last(erow(1, j)) + 1 for j in range(4)] == [6, 24, 33, 44] and [last(erow(2, j)) + 1 for j in range(4)] == [5, 10, 21, 32]
    r = erow(0, 2)
    assert w["tokens"][r, 31] == X.SEP and w["att"][r].all()                                       # ends exactly at T
    r = erow(1, 2)
    assert w["tokens"][r, 31] not in (0, X.SEP) and w["sep_indices"][r, 5] == 32                   # one past T: the last [SEP] is lost
    r = erow(0, 3)
    assert w["sep_indices"][r, 7] == 40 and w["sep_indices"][r, 6] == 36 and w["att"][r].all()      # far past T, positions still listed
    assert 0 not in c.cap[0] and 0 not in c.ques[1, 1] and 0 not in c.ans[1, 0]                     # rows without a terminating 0
    r = erow(1, 0)
    assert w["sep_indices"][r, 1] == w["sep_indices"][r, 0] + 1 and w["tokens"][r, 4] == w["tokens"][r, 5] == X.SEP   # an empty question
    assert w["tokens"][erow(2, 0), :2].tolist() == [X.CLS, X.SEP]                                   # an empty caption
    assert (w["hist_len"] == 2 * c.enc[1] + 1).all() and (w["segments"][:, 0] == 1).all() and (w["mlm"] == -1).all()
    assert (w["att"] == (w["tokens"] != 0)).all()
    lens = [[len(X.utt(c.opts[d, j, o])) for o in range(6)] for d in range(3) for j in range(4)]
    assert any(6 in l for l in lens) and any(7 in l for l in lens) and any(8 in l for l in lens) and any(0 in l for l in lens)
    assert {0, 5} <= set(c.gt[0].tolist()) and {0, 5} <= set(c.gt[1].tolist()) and {0, 5} <= set(c.gt[2].tolist())
    for d in range(3):
        for j in range(4):
            g = int(c.gt[d, j])
            assert [int(w["dec_option"][drow(d, j, s)]) for s in range(6)] == [g] + [o for o in range(6) if o != g]
    full = [r for r in range(c.dec.shape[1]) if len(X.utt(c.opts[c.dec[0, r], c.dec[1, r], w["dec_option"][r]])) >= 6]
    assert full and all(w["dec_ids"][r, 7] == X.SEP and w["dec_att"][r].all() for r in full)        # cut to Ud - 2: [SEP] in the last slot
    empty = [r for r in range(c.dec.shape[1]) if len(X.utt(c.opts[c.dec[0, r], c.dec[1, r], w["dec_option"][r]])) == 0]
    assert empty and all(w["dec_ids"][r].tolist() == [X.CLS, X.SEP] + [0] * 6 for r in empty)
    assert cases["eval_no4"].num_options == 4 < 6 and cases["eval_no4"].dec.shape[1] == 48
    n = cases["eval_noise_row_per_option"]
    wn = X.rule_of(n)
    hit = wn["mlm"] >= 0
    assert n.enc.shape[1] == 72 and hit.any() and not hit[n.u_tok == np.float32(0.15)].any()
    assert hit[(n.u_tok == np.nextafter(np.float32(0.15), np.float32(0))) & (wn["segments"] + wn["att"] > 0) & (wn["tokens"] == X.MASK)].all()
    assert (wn["tokens"][0] != wn["tokens"][1]).any() or (wn["tokens"][6] != wn["tokens"][7]).any()  # the copies of one context differ
    t1, tR = cases["test_Ro1"], cases["test_RoR_no5"]
    assert t1.opts.shape == (3, 1, 6, 8) and t1.gt is None and t1.enc[1].tolist() == [3, 1, 0] and tR.opts.shape[1] == 4
    w1 = X.rule_of(t1)
    assert (w1["dec_option"] == t1.dec[2]).all()
    for s in range(6):                                                                              # dialog 0 scores its round 3, original order
        assert w1["dec_ids"][s].tolist() == ([X.CLS] + X.utt(c.opts[0, 3, s])[:6] + [X.SEP] + [0] * 8)[:8]
    a, q = cases["train_a"], cases["train_q"]
    wa, wq = X.rule_of(a), X.rule_of(q)
    assert a.opts is None and (wa["hist_len"] == 2 * a.enc[1] + 1).all() and (wq["hist_len"] == 2 * q.enc[1]).all()
    assert not (wa["dec_ids"] == X.SEP).any() and (wa["dec_labels"][:, -1] == 0).all() and (wa["dec_option"] == -1).all()
    assert (wa["dec_labels"][:, :-1] == np.where(wa["dec_att"][:, 1:] > 0, np.where(wa["dec_ids"][:, 1:] == 0, X.SEP, wa["dec_ids"][:, 1:]), 0)).all()
    assert (wq["tokens"][0] == wa["tokens"][0]).sum() < 32 and wq["tokens"][0, :10].tolist() == wa["tokens"][0, :10].tolist()
    assert (X.rule_of(cases["train_q_noise"])["mlm"] >= 0).any()
    for name in ("eval_enc_only", "train_a_enc_only"):
        assert cases[name].dec is None and set(X.rule_of(cases[name])) == set(X.ENC_OUT)
    for name in ("eval_dec_only", "train_q_dec_only"):
        assert cases[name].enc is None and set(X.rule_of(cases[name])) == set(X.DEC_OUT)
    # every way a row can name nothing
    b = cases["eval_invalid_rows"]
    wb = X.rule_of(b)
    assert wb["tokens"][0, 0] == X.CLS and not wb["tokens"][1:5].any() and wb["tokens"][5, 0] == X.CLS and (wb["mlm"][1:5] == -1).all()
    assert not wb["sep_indices"][1:5].any() and not wb["hist_len"][1:5].any()
    assert wb["dec_option"].tolist() == [0, -1, -1, -1, -1, -1, -1, -1, -1, 2, 2] and not wb["dec_ids"][1:9].any()
    assert b.gt[1, 1] == 6 and b.gt[2, 2] == -1 and b.num_options == 4
    assert X.rule_of(cases["test_invalid_rows"])["dec_option"].tolist() == [0, -1, -1, -1, -1, 1, -1, -1, 0, 3, 3]
    wt = X.rule_of(cases["train_a_invalid_rows"])
    assert [bool(x) for x in wt["dec_ids"][:, 0]] == [True, False, False, False, False, False, False, False, True, False, False]
    # the widest rows and the most separators
    u = cases["eval_U64_Ud70"]
    wu = X.rule_of(u)
    assert u.ques.shape[2] == u.cap.shape[1] == 64 and 0 not in u.opts and wu["dec_ids"][0, 65] == X.SEP and wu["dec_att"][0, :66].all()
    assert wu["sep_indices"][1, :4].tolist() == [65, 130, 195, 260] and wu["tokens"][1, 199] != 0
    wv = X.rule_of(cases["train_a_U64_Ud25"])
    assert wv["dec_labels"][0, 23] == X.SEP and wv["dec_ids"][0, 24] == 0 and wv["dec_att"][0].all()
    r12 = X.rule_of(cases["eval_R12"])
    assert r12["hist_len"].max() == 23 and (r12["sep_indices"][11, :24] > 0).all() and r12["sep_indices"][11, 24] == 0
    assert X.rule_of(cases["train_q_R12"])["hist_len"].max() == 22
    e = cases["eval_full"]
    assert (e.T, e.Ud, e.opts.shape, e.num_options) == (256, 25, (2, 10, 100, 18), 100) and e.dec.shape == (3, 48)
    assert (X.rule_of(e)["dec_option"] >= 64).any() and cases["eval_full_noise"].u_tok.shape == (24, 256)


def test_harness_passes_on_the_rule_and_catches_wrong_backends(fixture):
    be = X.NumpyBackend()
    for c in X.cases():
        X.run_case(be, c)
    for c, want in fixture:
        X.run_case(be, c, dict(X.rule_of(c), **want))

    class SkipsOneElement(X.NumpyBackend):                      # leaves one padding element to a pre-zeroed buffer: poison stays
        def rows(self, *a, out=None, **k):
            keep = out["segments"][3, -1].clone()
            X.NumpyBackend.rows(self, *a, out=out, **k)
            out["segments"][3, -1] = keep

    class WritesPastRow(X.NumpyBackend):
        def rows(self, *a, out=None, **k):
            X.NumpyBackend.rows(self, *a, out=out, **k)
            torch.as_strided(out["dec_ids"], (1,), (1,), out["dec_ids"].storage_offset() + out["dec_ids"].shape[1]).fill_(0)

    class ReadsThePadColumns(X.NumpyBackend):                   # takes the option row's stride for its width
        def rows(self, cap, ques, ans, opts, *a, **k):
            wide = torch.as_strided(opts, opts.shape[:3] + (opts.stride(2),), opts.stride(), opts.storage_offset())
            X.NumpyBackend.rows(self, cap, ques, ans, wide, *a, **k)

    class WritesLabelsInEval(X.NumpyBackend):
        def rows(self, *a, out=None, **k):
            X.NumpyBackend.rows(self, *a, out=out, **k)
            out["dec_labels"].zero_()

    class KeepsSepInTrainIds(X.NumpyBackend):
        def rows(self, *a, out=None, **k):
            X.NumpyBackend.rows(self, *a, out=out, **k)
            out["dec_ids"][:, 1:] = torch.where(out["dec_att"][:, 1:] > 0, out["dec_labels"][:, :-1], out["dec_ids"][:, 1:])

    c = {c.name: c for c in X.cases()}
    for bad, name in ((SkipsOneElement(), "eval_no6"), (WritesPastRow(), "eval_no6"), (ReadsThePadColumns(), "eval_U64_Ud70"),
                      (WritesLabelsInEval(), "test_Ro1"), (KeepsSepInTrainIds(), "train_q")):
        with pytest.raises(AssertionError):
            X.run_case(bad, c[name])


def test_entry_point_is_declared_in_every_layer():
    from gst_visdial_amd import _lib, ops, gen_rows, evaluate
    assert _lib.ABI_VERSION == 9
    assert "gstvd_gen_rows" in _lib.SIGNATURES and _lib.SIGNATURES["gstvd_gen_rows"][1][0]._type_ is _lib.GenRowsDesc
    assert (_lib.GEN_EVAL, _lib.GEN_TEST, _lib.GEN_TRAIN_A, _lib.GEN_TRAIN_Q) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    assert "int gstvd_gen_rows(const gstvd_gen_rows_t* a, gstvd_stream_t s);" in header
    assert re.search(r"GSTVD_GEN_EVAL = 0, GSTVD_GEN_TEST = 1, GSTVD_GEN_TRAIN_A = 2, GSTVD_GEN_TRAIN_Q = 3", header)
    struct = header[header.index("gstvd_disc_rows(const"):header.index("} gstvd_gen_rows_t;")]
    struct = struct[struct.rindex("typedef struct {"):]
    fields = re.findall(r"(\w+);", struct)
    assert fields == [n for n, _ in _lib.GenRowsDesc._fields_], (fields, [n for n, _ in _lib.GenRowsDesc._fields_])
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "gen_rows.hip" in srcs and os.path.exists(os.path.join(ROOT, "gst_visdial_amd", "csrc", "gen_rows.hip"))
    assert "gen_rows_kernel 0" in open(os.path.join(ROOT, "tools", "kernel_resources.expect")).read().splitlines()
    src = open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "gen_rows.hip")).read()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")
    assert callable(ops.gen_rows) and callable(gen_rows.eval_rounds) and callable(gen_rows.test_rounds) and callable(gen_rows.train_batch)
    assert callable(evaluate.score_batch)


def _cpu_pools(D=2, R=3, O=5, U=6, Lc=7):
    z = lambda *s: torch.ones(s, dtype=torch.int64)
    return dict(cap=z(D, Lc), ques=z(D, R, U), ans=z(D, R, U), opts=z(D, R, O, U), gt_index=torch.zeros(D, R, dtype=torch.int64))


def test_host_layers_refuse_cpu_tensors_and_bad_shapes():
    from gst_visdial_amd import ops, gen_rows as GR
    from gst_visdial_amd._lib import GstvdError
    p = _cpu_pools()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    enc, dec = (i32(0, 1), i32(0, 2)), (i32(0, 1), i32(0, 2), i32(0, 4))
    args = lambda **k: [k.get(n, p[n]) for n in ("cap", "ques", "ans", "opts", "gt_index")]
    with pytest.raises(GstvdError, match="no CPU path"):
        ops.gen_rows(*args(), "eval", 32, 8, enc, dec)
    bad = [
        (args(), dict(mode="valid"), "mode must be one of"),
        (args(ques=p["ques"].int()), {}, "ques must be an int64 tensor of 3 dimensions"),
        (args(opts=p["opts"][:, :, :, 0]), {}, "opts must be an int64 tensor of 4 dimensions"),
        (args(gt_index=None), {}, "gt_index must be an int64 tensor of 2 dimensions"),
        (args(ans=p["ans"][:, :2]), {}, "do not belong together"),
        (args(opts=p["opts"][:, :2]), {}, r"opts must be \[D, R or 1, O, U\]"),
        (args(opts=p["opts"].transpose(1, 2).contiguous().transpose(1, 2)), {}, "dense rows of one stride"),
        # the test split's [D, 1, O, U] as a slice of a larger pool: its dialog stride is that of R rounds, not of one
        (args(opts=p["opts"][:, -1:], gt_index=None), dict(mode="test"), "dense rows of one stride"),
        (args(opts=p["opts"][:, :1]), {}, "dense rows of one stride"),
        (args(cap=torch.ones(2, 65, dtype=torch.int64)), {}, "1 <= U, Lc <= 64"),
        (args(), dict(T=1), "T >= 2"),
        (args(), dict(Ud=2), "Ud >= 3"),
        (args(), dict(S=5), "more than max_sep_len = 5 allows"),
        (args(), dict(num_options=6), "2 <= num_options <= O"),
        (args(), dict(num_options=1), "2 <= num_options <= O"),
        (args(), dict(enc=(i32(0, 1), i32(0))), r"enc_rows\[1\] must be a contiguous int32 vector of 2 elements"),
        (args(), dict(dec=(i32(0, 1), i32(0, 1))), "dec_rows must be 3 int32 vectors"),
        (args(), dict(mask_prob=0.15), "mask_prob = 0.15 needs u_tok"),
        (args(), dict(mask_prob=0.15, u_tok=torch.zeros(3, 32)), r"u_tok must be fp32 \[n_enc = 2, T = 32\]"),
        (args(), dict(out=dict()), None),
    ]
    for a, k, msg in bad:
        kw = dict(mode="eval", T=32, Ud=8, enc=enc, dec=dec)
        kw.update(k)
        call = lambda: ops.gen_rows(*a, kw.pop("mode"), kw.pop("T"), kw.pop("Ud"), kw.pop("enc"), kw.pop("dec"), **kw)
        if msg is None:
            with pytest.raises(KeyError):
                call()
        else:
            with pytest.raises(GstvdError, match=msg):
                call()
    # the train modes take no option pool and no ground truth; the test mode no ground truth: they get as far as the device check
    for mode, a in (("train_a", args(opts=None, gt_index=None)), ("train_q", args(opts=None, gt_index=None)), ("test", args(gt_index=None))):
        with pytest.raises(GstvdError, match="no CPU path"):
            ops.gen_rows(*a, mode, 32, 8, enc, (dec[0], dec[1], i32(0, 0)))
    with pytest.raises(GstvdError, match="no CPU path"):              # a dense [D, 1, O, U] pool of its own passes the stride check
        ops.gen_rows(*args(opts=p["opts"][:, -1:].contiguous(), gt_index=None), "test", 32, 8, enc, dec)
    params = dict(max_seq_len=32, max_utt_len=8, num_options=5)
    image = dict(enc_image_feat=torch.zeros(2, 4, 8), enc_image_loc=torch.zeros(2, 4, 5), enc_image_mask=torch.ones(2, 4))
    with pytest.raises(GstvdError, match=r"eval_rounds needs GPU tensors \(cap is on cpu\)"):
        GR.eval_rounds(p, 0, 6, params)
    with pytest.raises(GstvdError, match="the pooled batch has no 'n_rounds'"):
        GR.test_rounds(p, 0, 2, params)
    with pytest.raises(GstvdError, match=r"test_rounds needs GPU tensors \(cap is on cpu\)"):
        GR.test_rounds(dict(p, n_rounds=torch.tensor([3, 1])), 0, 2, params)
    with pytest.raises(GstvdError, match=r"train_batch needs GPU tensors \(cap is on cpu\)"):
        GR.train_batch(p, image, params)
    with pytest.raises(GstvdError, match="model must be"):
        GR.train_batch(p, image, params, model="enc_only_a")
    with pytest.raises(GstvdError, match="the pooled batch has no 'ans'"):
        GR.eval_rounds({k: v for k, v in p.items() if k != "ans"}, 0, 6, params)


def test_is_pooled_dispatch(monkeypatch):
    from gst_visdial_amd import evaluate as EV, gen_rows as GR
    p = _cpu_pools()
    assert GR.is_pooled(p) and not GR.is_pooled(dict(p, enc_input_ids=torch.zeros(1))) and not GR.is_pooled(dict(enc_input_ids=torch.zeros(1)))
    assert GR.noise_prob(dict(attack="random_token", mask_prob=0.15)) == 0.15 and GR.noise_prob(dict(mask_prob=0.15)) == 0.0
    assert GR.noise_prob(None) == 0.0
    seen = []
    monkeypatch.setattr(EV, "_score_batch_pooled", lambda model, batch, rounds_per_call, params: seen.append((rounds_per_call, params)) or "pooled")
    assert EV.score_batch(None, p, "cpu", params=dict(num_options=5)) == "pooled" and seen == [(20, dict(num_options=5))]
    # a loader-shaped batch does not reach the pooled route: it runs score_batch's own code (one encoder row per round)
    calls = []

    class Model(object):
        def score_candidates(self, feat, loc, imask, ids, seg, att, dec_ids, dec_att, group):
            calls.append((tuple(ids.shape), tuple(dec_ids.shape), group))
            return torch.zeros(dec_ids.shape[0])

    B, R, O, T, U = 2, 3, 4, 10, 5
    ids = torch.arange(B * R * T).view(B, R, 1, T).expand(B, R, O, T).contiguous()
    lb = dict(enc_input_ids=ids, enc_segments=torch.zeros_like(ids), enc_att_mask=torch.ones(B, R, O, T), dec_input_ids=torch.ones(B, R, O, U).long(),
              dec_att_mask=torch.ones(B, R, O, U), enc_image_feat=torch.zeros(B, 3, 4), enc_image_loc=torch.zeros(B, 3, 5),
              enc_image_mask=torch.ones(B, 3))
    out = EV.score_batch(Model(), lb, "cpu", rounds_per_call=4)
    assert tuple(out.shape) == (B, R, O) and calls == [((4, T), (16, U), O), ((2, T), (8, U), O)] and len(seen) == 1
