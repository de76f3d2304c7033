"""Exact layer of the discriminative-rows tests: the rule of csrc/disc_rows.hip stated in numpy, case tables,
and a harness that runs a backend on them inside canary-filled windows.

The kernel is integer work on token ids, so there is no tolerance anywhere: every output must be torch.equal to the rule, the
label floats bit for bit.

  rows_rule    gstvd_disc_rows: dataloader/dataloader_visdial_disc.py (train rows :125-288, eval rows :299-401) through
               utils/data_utils.encode_input, on token-id pools.  tests/test_exact_disc_rows_harness_cpu.py pins it, bit for bit, to
               tests/golden/disc_rows.npz, which tools/make_golden_disc_rows.py records from the reference's own loader.
  image_rule   utils/data_utils.encode_image_input's labels and feature zeroing (gst_visdial_amd.disc_rows.image_labels).

Windows as in tests/exact_dialog.py: every array the kernel writes is a window inside a larger allocation that holds a canary
pattern, pre-filled with POISON (a value no rule produces): an element the launch skips shows up, and so does a write outside.
The pools are strided too (caption rows and option rows with pad columns that hold ids, which must not be read as tokens).

Plain helper module: no fixtures, no hooks.  Everything takes a backend `be` (be.device, be.rows(...) with the signature of
ops.disc_rows), so the CPU harness test proves the harness on a numpy stand-in and tests/test_disc_rows_exact_gpu.py runs it on the
HIP kernel.
"""
import collections
import math

import numpy as np
import torch

from exact_dialog import CLS, SEP, MASK, POISON, S_MAX, V0, V1, _t, _window, _i32_vec, _i32_intact
from exact_gemm import Window

ROWS_OUT = ("tokens", "segments", "mask", "att", "sep_indices", "hist_len", "neg_option", "nsp_labels")


# ------------------------------------------------------------------------------------------------------------------ the rule
def utt(row):
    """The utterance of a 0-padded pool row: the ids in front of its first 0."""
    row = [int(v) for v in row]
    return row[:row.index(0)] if 0 in row else row


def eval_option(gt, slot):
    """Option of eval slot `slot`: the ground truth first, then the other indices in increasing order."""
    return gt if slot == 0 else (slot - 1 if slot - 1 < gt else slot)


def candidates(gt, O, num_options):
    return [c for c in range(O) if c != gt][:num_options - 1]


def pick(u, n):
    """min(floor((double)u * n), n - 1) of an fp32 draw (a negative product counts as 0)."""
    return min(max(int(math.floor(float(np.float64(np.float32(u))) * n)), 0), n - 1)


def tot_len(cap, ques, ans, d, j):
    """The loader's running length when it draws the negatives of round j: [CLS] caption [SEP], then every round up to and
    including j with BOTH its question and its ground-truth answer, one [SEP] each."""
    return len(utt(cap[d])) + 2 + sum(len(utt(ques[d, k])) + 1 + len(utt(ans[d, k])) + 1 for k in range(j + 1))


def feasible(cap, ques, ans, opts, gt, d, j, T, num_options):
    """(C, F): the candidate options of round j and those of them that fit."""
    C = candidates(int(gt[d, j]), opts.shape[2], num_options)
    n = tot_len(cap, ques, ans, d, j)
    return C, [c for c in C if T >= n + len(utt(opts[d, j, c])) + 1]


def negative(cap, ques, ans, opts, gt, d, j, u, T, num_options):
    """(option index, its tokens) of the negative the draw u selects."""
    C, F = feasible(cap, ques, ans, opts, gt, d, j, T, num_options)
    if F:
        c = F[pick(u, len(F))]
        return c, utt(opts[d, j, c])
    c = C[pick(u, len(C))]
    return c, utt(opts[d, j, c])[:len(utt(ans[d, j]))]


def rows_rule(cap, ques, ans, opts, gt, row_dialog, row_round, row_slot, T, tot_rounds, num_options, train, mask_prob=0.0, u_tok=None,
              u_neg=None, dense=None, cls=CLS, sep=SEP, mask=MASK, S=S_MAX):
    """numpy statement of gstvd_disc_rows.  Returns the eight output arrays over the N rows (nsp_labels all zero in eval mode,
    where the kernel does not write it)."""
    cap, ques, ans, opts, gt = (np.asarray(x) for x in (cap, ques, ans, opts, gt))
    D, R, U = ques.shape
    O = opts.shape[2]
    N = len(row_dialog)
    assert R >= 1 and 2 * R + 1 <= S <= 64 and U <= 64 and cap.shape[1] <= 64 and T >= 2 and 2 <= num_options <= O <= 100 and tot_rounds >= 1
    assert mask_prob == 0 or u_tok is not None
    o = dict(tokens=np.zeros((N, T), np.int64), segments=np.zeros((N, T), np.int64), mask=np.full((N, T), -1, np.int64),
             att=np.zeros((N, T), np.float32), sep_indices=np.zeros((N, S), np.int64), hist_len=np.zeros(N, np.int64),
             neg_option=np.full(N, -1, np.int32), nsp_labels=np.zeros((N, 2), np.float32))
    for r in range(N):
        d, j, slot = int(row_dialog[r]), int(row_round[r]), int(row_slot[r])
        if not (0 <= d < D and 0 <= j < R and 0 <= slot and (train or slot < num_options) and 0 <= int(gt[d, j]) < O):
            continue                                                       # a row that names nothing: padding
        g = int(gt[d, j])
        if not train:
            c = eval_option(g, slot)
            x = utt(opts[d, j, c])
            o["neg_option"][r] = c
        elif slot == 0:
            x = utt(ans[d, j])
            o["nsp_labels"][r] = (1.0, 0.0)
        else:
            c, x = negative(cap, ques, ans, opts, gt, d, j, u_neg[r], T, num_options)
            o["neg_option"][r] = c
            s = None if dense is None else float(dense[d, j, c])
            o["nsp_labels"][r] = (0.0, 1.0) if s is None else (np.float32(s), np.float32(1.0 - s))
        utts = [utt(cap[d])]
        for k in range(j):
            utts += [utt(ques[d, k]), utt(ans[d, k])]
        utts += [utt(ques[d, j]), x]
        cur = 1
        if j + 2 > tot_rounds:                                             # pruneRounds: the oldest utterances go, the caption first
            utts, cur = utts[len(utts) - 2 * tot_rounds:], 0
        ids, seg, mlm, seps = [cls], [cur], [-1], []
        for ut in utts:
            for t in ut:
                p = len(ids)
                hit = u_tok is not None and p < T and float(np.float64(np.float32(u_tok[r, p]))) < float(mask_prob)
                ids.append(mask if hit else t), seg.append(cur), mlm.append(t if hit else -1)
            ids.append(sep), seg.append(cur), mlm.append(-1)
            seps.append(len(ids) - 1)
            cur ^= 1
        n = min(len(ids), T)
        o["tokens"][r, :n], o["segments"][r, :n], o["mask"][r, :n] = ids[:n], seg[:n], mlm[:n]
        o["sep_indices"][r, :len(seps)] = seps
        o["hist_len"][r] = len(utts) - 1
        o["att"][r] = np.arange(T) < seps[-1] + 1
    return o


def image_rule(feats, image_mask, u_img, forced_region, mask_prob):
    """numpy statement of disc_rows.image_labels, per dialog: -> (features, image_label)."""
    feats, label = np.array(feats), np.full(np.asarray(image_mask).shape, -1, np.int64)
    for d in range(label.shape[0]):
        for i in range(label.shape[1]):
            if image_mask[d, i] != 0 and mask_prob > 0:
                u = float(u_img[d, i])
                if u < mask_prob:
                    label[d, i] = 1
                    if u / mask_prob < 0.9:
                        feats[d, i] = 0
        label[d, int(forced_region[d])] = 1
        label[d, 0] = 0
    return feats, label


# ------------------------------------------------------------------------------------------------------------------ the cases
DiscCase = collections.namedtuple("DiscCase", "name cap ques ans opts gt dense rows T tot_rounds num_options train mask_prob u_tok u_neg")


def _row(U, n, gen):
    row = np.zeros(U, np.int64)
    row[:n] = gen.integers(V0, V1, n)
    return row


def edge_pools():
    """D = 3, R = 3, O = 5, U = 18, Lc = 8 at T = 32.  The lengths are chosen so that (tests/test_exact_disc_rows_harness_cpu.py
    asserts each on the rule's output)
      dialog 0, round 2: 29 tokens in front of the option; options of 2 / 3 / 8 / 0 tokens fit exactly, lose the final [SEP], are
                         cut inside, are empty;
      dialog 1: the negatives of round 0 are all feasible, of round 1 exactly one is, of round 2 none (cut to len(a_2) = 2); q_2 empty;
      dialog 2: a full-width caption and question (no 0 in the row), round 0 has no feasible negative and an 18-token answer,
                round 1 none and an EMPTY answer (the negative is cut to nothing).
    gt_index holds 0, O - 1 and a middle value in every dialog; ans[d, j] = opts[d, j, gt]."""
    gen = np.random.default_rng(41)
    cap_len = [5, 3, 8]
    q_len = [[4, 5, 3], [4, 6, 0], [18, 2, 5]]
    gt = np.array([[0, 4, 2], [2, 0, 4], [4, 2, 0]], np.int64)
    o_len = [[[3, 1, 4, 2, 6], [4, 3, 5, 1, 2], [2, 3, 8, 0, 1]],
             [[5, 17, 3, 0, 9], [5, 6, 4, 9, 18], [7, 5, 3, 6, 2]],
             [[2, 9, 1, 4, 18], [4, 1, 0, 6, 3], [1, 2, 3, 4, 5]]]
    cap = np.stack([_row(8, n, gen) for n in cap_len])
    ques = np.stack([np.stack([_row(18, n, gen) for n in q]) for q in q_len])
    opts = np.stack([np.stack([np.stack([_row(18, n, gen) for n in o]) for o in rnd]) for rnd in o_len])
    ans = np.stack([np.stack([opts[d, j, gt[d, j]] for j in range(3)]) for d in range(3)])
    return cap, ques, ans, opts, gt


def soft_scores(shape, gen):
    """float64 scores in [0, 1] whose fp32 `1 - s` (both operands fp32) differs from the double subtraction rounded once."""
    out = []
    while len(out) < int(np.prod(shape)):
        s = float(gen.random())
        if np.float32(1.0) - np.float32(s) != np.float32(1.0 - s):
            out.append(s)
    return np.array(out, np.float64).reshape(shape)


def _noise(n, T, gen):
    u = gen.random((n, T)).astype(np.float32)
    u[:, 1::5] = np.float32(0.15)                                          # the strict comparison: never masked
    u[:, 2::5] = np.nextafter(np.float32(0.15), np.float32(0))             # its neighbour below, side by side: masked
    return u


def _all_rows(D, R, slots):
    d, j, s = np.meshgrid(np.arange(D), np.arange(R), np.arange(slots), indexing="ij")
    return np.stack([d.ravel(), j.ravel(), s.ravel()]).astype(np.int32)


U_NEG = (0.0, 0.3, 0.5, float(np.nextafter(np.float32(1), np.float32(0))))


def big_pools(seed=43, D=2, R=10, O=100, U=18, Lc=38):
    gen = np.random.default_rng(seed)
    cap = np.stack([_row(Lc, n, gen) for n in (38, 11)[:D]])
    ques = np.stack([np.stack([_row(U, int(gen.integers(3, U + 1)), gen) for _ in range(R)]) for _ in range(D)])
    opts = np.stack([np.stack([np.stack([_row(U, int(gen.integers(0, U + 1)), gen) for _ in range(O)]) for _ in range(R)]) for _ in range(D)])
    gt = gen.integers(0, O, (D, R)).astype(np.int64)
    gt[0, 0], gt[0, 1], gt[1, 9] = 0, O - 1, 70
    ans = np.stack([np.stack([opts[d, j, gt[d, j]] for j in range(R)]) for d in range(D)])
    return cap, ques, ans, opts, gt


def cases():
    """The table of the exact harness (every rule at the smallest shape at which it can go wrong) plus the production shape
    R = 10, O = 100, T = 256 for N = 24 sampled rows, where the options fill both ballots."""
    gen = np.random.default_rng(47)
    cap, ques, ans, opts, gt = edge_pools()
    T = 32
    ev = lambda no: _all_rows(3, 3, no)
    tr = _all_rows(3, 3, 1 + len(U_NEG))                                   # slot 0, then one negative per draw of U_NEG
    u_neg = np.array([0.0 if s == 0 else U_NEG[s - 1] for s in tr[2]], np.float32)
    dense = soft_scores((3, 3, 5), gen)
    out = [
        DiscCase("eval_tr11_no5", cap, ques, ans, opts, gt, None, ev(5), T, 11, 5, False, 0.0, None, None),
        DiscCase("eval_tr2_no3", cap, ques, ans, opts, gt, None, ev(3), T, 2, 3, False, 0.0, None, None),
        DiscCase("train_tr11_no5_p15", cap, ques, ans, opts, gt, None, tr, T, 11, 5, True, 0.15, _noise(tr.shape[1], T, gen), u_neg),
        DiscCase("train_tr2_no4_dense", cap, ques, ans, opts, gt, dense, tr, T, 2, 4, True, 0.0, None, u_neg),
        DiscCase("train_tr2_no2_p15_dense", cap, ques, ans, opts, gt, dense, tr, T, 2, 2, True, 0.15, _noise(tr.shape[1], T, gen), u_neg),
    ]
    # the bin edges of floor(u * n): k / n as fp32 and its neighbour below, for n = 4 and n = 3, over feasible sets and over C
    for no, n in ((5, 4), (4, 3)):
        edges = [np.float32(k / n) for k in range(1, n)]
        us = np.array(edges + [np.nextafter(e, np.float32(0)) for e in edges], np.float32)
        rows = np.concatenate([np.stack([np.full(len(us), d), np.full(len(us), j), np.arange(1, len(us) + 1)]) for d, j in ((1, 0), (2, 1))], 1)
        out.append(DiscCase("train_bin_edges_n%d" % n, cap, ques, ans, opts, gt, None, rows.astype(np.int32), T, 11, no, True, 0.0, None,
                            np.concatenate([us, us])))
    # rows that name nothing (dialog, round, slot out of range; a ground truth outside the options) next to good ones
    bad_gt = gt.copy()
    bad_gt[1, 1] = 5
    rows = np.array([[0, 3, -1, 1, 2, 1, 0], [0, 0, 0, 3, -1, 1, 2], [0, 0, 0, 0, 0, 1, 5]], np.int32)
    out.append(DiscCase("eval_invalid_rows", cap, ques, ans, opts, bad_gt, None, rows, T, 11, 5, False, 0.0, None, None))
    out.append(DiscCase("train_invalid_rows", cap, ques, ans, opts, bad_gt, None, rows, T, 11, 5, True, 0.0, None,
                        np.full(rows.shape[1], 0.5, np.float32)))
    # the production shape, 24 sampled rows each
    bcap, bques, bans, bopts, bgt = big_pools()
    pickr = gen.permutation(2 * 10 * 100)[:24]
    erows = np.stack([pickr // 1000, pickr // 100 % 10, pickr % 100]).astype(np.int32)
    erows[:, 0], erows[:, 1], erows[:, 2] = (0, 0, 99), (0, 1, 99), (1, 9, 71)                      # gt 0 / O - 1 / 70 at the far slots
    out.append(DiscCase("eval_full_T256_O100", bcap, bques, bans, bopts, bgt, None, erows, 256, 11, 100, False, 0.0, None, None))
    pickt = gen.permutation(2 * 10 * 3)[:24]
    trows = np.stack([pickt // 30, pickt // 3 % 10, pickt % 3]).astype(np.int32)
    out.append(DiscCase("train_full_T256_O100", bcap, bques, bans, bopts, bgt, soft_scores((2, 10, 100), gen), trows, 256, 11, 100, True, 0.15,
                        _noise(24, 256, gen), gen.random(24).astype(np.float32)))
    return out


def rule_of(c):
    return rows_rule(c.cap, c.ques, c.ans, c.opts, c.gt, c.rows[0], c.rows[1], c.rows[2], c.T, c.tot_rounds, c.num_options, c.train,
                     c.mask_prob, c.u_tok, c.u_neg, c.dense)


# ------------------------------------------------------------------------------------------------------------------ the harness
def _strided_opts(opts, device, pad=3):
    """opts [D, R, O, U] as a view of a [D, R, O, U + pad] tensor whose pad columns hold ordinary ids (never to be read)."""
    o = torch.as_tensor(np.asarray(opts), dtype=torch.int64)
    D, R, O, U = o.shape
    big = torch.full((D, R, O, U + pad), V1 + 7, dtype=torch.int64)
    big[..., :U] = o
    big = big.to(device)
    return big, big[..., :U]


def rows_windows(N, T, device, S=S_MAX):
    """The outputs as windows: POISON inside, canaries around; the four [N, T] arrays share one row stride."""
    w = {}
    for k, cols, pad in (("tokens", T, 3), ("segments", T, 3), ("mask", T, 3), ("att", T, 3), ("sep_indices", S, 2)):
        w[k] = Window(N, cols, torch.float32 if k == "att" else torch.int64, device, "canary", ld=cols + pad)
    w["hist_len"] = Window(1, N, torch.int64, device, "canary", guard=1)
    w["nsp_labels"] = Window(1, 2 * N, torch.float32, device, "canary", guard=1)
    for v in w.values():
        v.view.fill_(POISON)
    return w


def run_case(be, c, want=None):
    """`be.rows` on case c into poisoned windows with strided pools, against rows_rule (or the recorded `want`); twice: same bits."""
    dev = be.device
    if want is None:
        want = rule_of(c)
    N = c.rows.shape[1]
    capw = _window(c.cap, torch.int64, dev, 3)
    capw.flat[~capw.inside.to(capw.flat.device)] = V1 + 9                   # ids, not canaries, behind every caption row
    big, opts = _strided_opts(c.opts, dev)
    ins = dict(cap=capw.view, ques=_t(c.ques, dev, torch.int64), ans=_t(c.ans, dev, torch.int64), opts=opts, gt=_t(c.gt, dev, torch.int64),
               rd=_t(c.rows[0], dev, torch.int32), rj=_t(c.rows[1], dev, torch.int32), rs=_t(c.rows[2], dev, torch.int32),
               u_tok=_t(c.u_tok, dev, torch.float32), u_neg=_t(c.u_neg, dev, torch.float32), dense=_t(c.dense, dev, torch.float64))
    keep = {k: v.clone() for k, v in ins.items() if v is not None}
    big0 = big.clone()
    got = []
    names = [k for k in ROWS_OUT if c.train or k != "nsp_labels"]
    for rep in range(2):
        w = rows_windows(N, c.T, dev)
        neg_buf, neg = _i32_vec(np.full(N, POISON), dev)
        out = dict(tokens=w["tokens"].view, segments=w["segments"].view, mask=w["mask"].view, att=w["att"].view,
                   sep_indices=w["sep_indices"].view, hist_len=w["hist_len"].vector(), neg_option=neg,
                   nsp_labels=w["nsp_labels"].vector().view(N, 2))
        be.rows(ins["cap"], ins["ques"], ins["ans"], ins["opts"], ins["gt"], ins["rd"], ins["rj"], ins["rs"], c.T, c.tot_rounds,
                c.num_options, c.train, mask_prob=c.mask_prob, u_tok=ins["u_tok"], u_neg=ins["u_neg"], dense_scores=ins["dense"], out=out)
        for k in names:
            v = out[k].cpu()
            assert not bool((v == POISON).any()), "%s: %s has elements the launch did not write" % (c.name, k)
            ref = torch.as_tensor(want[k]).reshape(v.shape).to(v.dtype)
            same = torch.equal(v.view(torch.int32), ref.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(v, ref)
            assert same, "%s: %s differs from the rule at %s" % (c.name, k, (v != ref).nonzero()[:6].tolist())
        if not c.train:
            assert bool((out["nsp_labels"] == POISON).all()), c.name + ": nsp_labels was written in eval mode"
        for k, win in w.items():
            win.assert_surroundings_untouched("%s %s" % (c.name, k))
        _i32_intact(neg_buf, N, c.name + " neg_option")
        got.append({k: out[k].cpu().clone() for k in names})
    for k in names:
        assert torch.equal(got[0][k], got[1][k]), "%s: %s differs between two launches" % (c.name, k)
    for k, v in keep.items():
        assert torch.equal(ins[k], v), "%s: input %s was written" % (c.name, k)
    assert torch.equal(big, big0), c.name + ": the option pool was written"
    return got[0]


def derived_u_neg(c, r, chosen):
    """u_neg = (rank + 0.5) / |F| (or / |C| when nothing is feasible) of the option the reference's loop settled on."""
    d, j, slot = (int(x) for x in c.rows[:, r])
    if slot == 0:
        return 0.0
    C, F = feasible(c.cap, c.ques, c.ans, c.opts, c.gt, d, j, c.T, c.num_options)
    pool = F or C
    return (pool.index(int(chosen)) + 0.5) / len(pool)


def fixture_cases(g):
    """The cases of tests/golden/disc_rows.npz (a dict of numpy arrays) as (DiscCase, recorded outputs, image record) triples.
    The image record (feats, image_mask, u_img, forced_region, out_feats, out_label) is None for the eval cases."""
    names = sorted(set(k.split("::")[0] for k in g))
    out = []
    for n in names:
        f = lambda k: np.asarray(g["%s::%s" % (n, k)])
        opt = lambda k: f(k) if ("%s::%s" % (n, k)) in g else None
        c = DiscCase(n, f("cap"), f("ques"), f("ans"), f("opts"), f("gt"), opt("dense"), f("rows").astype(np.int32), int(f("T")),
                     int(f("tot_rounds")), int(f("num_options")), bool(f("train")), float(f("mask_prob")), opt("u_tok"), opt("u_neg"))
        want = {k: f("out_" + k) for k in ROWS_OUT if opt("out_" + k) is not None}
        if c.train:                                                        # the draw that selects the recorded option: mid-bin
            c = c._replace(u_neg=np.array([derived_u_neg(c, r, want["neg_option"][r]) for r in range(c.rows.shape[1])], np.float32))
        img = None if opt("img_feats") is None else {k: f("img_" + k) for k in ("feats", "image_mask", "u_img", "forced_region",
                                                                                "out_feats", "out_label")}
        out.append((c, want, img))
    return out


class NumpyBackend(object):
    """Stand-in backend: the rule itself, written into the caller's tensors (proves the harness without a GPU)."""
    device = "cpu"

    def rows(self, cap, ques, ans, opts, gt, rd, rj, rs, T, tot_rounds, num_options, train, mask_prob=0.0, u_tok=None, u_neg=None,
             dense_scores=None, out=None):
        n = lambda x: None if x is None else x.numpy()
        r = rows_rule(n(cap), n(ques), n(ans), n(opts), n(gt), n(rd), n(rj), n(rs), T, tot_rounds, num_options, train, mask_prob,
                      n(u_tok), n(u_neg), n(dense_scores))
        for k in ROWS_OUT:
            if train or k != "nsp_labels":
                out[k].copy_(torch.as_tensor(r[k]).reshape(out[k].shape))
        return out
