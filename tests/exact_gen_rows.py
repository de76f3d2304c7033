"""Exact layer of the generative-rows tests: the rule of csrc/gen_rows.hip stated in numpy, a case table, and
a harness that runs a backend on the cases inside canary-filled windows.

The kernel is integer work on token ids, so there is no tolerance anywhere: every output must be torch.equal to the rule, the 0 / 1
floats bit for bit.

  rows_rule    gstvd_gen_rows: dataloader/dataloader_visdial_gen.py (eval rows :295-458, test rows :507-603, teacher rows :123-293)
               through utils/data_utils.encode_input, on token-id pools.  tests/test_exact_gen_rows_harness_cpu.py pins it, bit for
               bit, to tests/golden/gen_rows.npz, which tools/make_golden_gen_rows.py records from the reference's own loader.

Windows as in tests/exact_disc_rows.py: every array the kernel writes is a window inside a larger allocation that holds a canary
pattern, pre-filled with POISON (a value no rule produces): an element the launch skips shows up, and so does a write outside.
The pools are strided too (caption rows and option rows with pad columns that hold ids, which must not be read as tokens).

Plain helper module: no fixtures, no hooks.  Everything takes a backend `be` (be.device, be.rows(...) with the signature of
ops.gen_rows), so the CPU harness test proves the harness on a numpy stand-in and tests/test_gen_rows_exact_gpu.py runs it on the
HIP kernel.
"""
import collections

import numpy as np
import torch

from exact_dialog import CLS, SEP, MASK, POISON, S_MAX, V0, V1, _t, _window, _i32_vec, _i32_intact
from exact_disc_rows import _row, _strided_opts, big_pools, eval_option, utt
from exact_gemm import Window

MODES = ("eval", "test", "train_a", "train_q")
ENC_OUT = ("tokens", "segments", "mlm", "att", "sep_indices", "hist_len")
DEC_OUT = ("dec_ids", "dec_att", "dec_labels", "dec_option")


def out_names(c):
    train = c.mode in ("train_a", "train_q")
    return (ENC_OUT if c.enc is not None else ()) + (tuple(k for k in DEC_OUT if train or k != "dec_labels") if c.dec is not None else ())


# ------------------------------------------------------------------------------------------------------------------ the rule
def encode(utts, max_len, max_sep, mask_prob, draws, cls, sep, mask):
    """utils/data_utils.encode_input with start_segment 1 on id lists; `draws(p)` is the uniform of row position p (asked for
    p < max_len only: a draw behind the cut changes nothing).  -> ids, segments, mlm labels (each cut / padded to max_len), the
    separator positions padded to max_sep, att."""
    ids, seg, lab, seps, cur = [cls], [1], [-1], [], 1
    for ut in utts:
        for t in ut:
            p = len(ids)
            hit = mask_prob > 0 and p < max_len and float(np.float64(np.float32(draws(p)))) < float(mask_prob)
            ids.append(mask if hit else t), seg.append(cur), lab.append(t if hit else -1)
        ids.append(sep), seg.append(cur), lab.append(-1)
        seps.append(len(ids) - 1)
        cur ^= 1
    pad = lambda x, n, fill: (list(x) + [fill] * n)[:n]
    ids = pad(ids, max_len, 0)
    return ids, pad(seg, max_len, 0), pad(lab, max_len, -1), pad(seps, max_sep, 0), [1.0 if t != 0 else 0.0 for t in ids]


def context(cap, ques, ans, d, j, mode):
    utts = [utt(cap[d])]
    for k in range(j):
        utts += [utt(ques[d, k]), utt(ans[d, k])]
    return utts if mode == "train_q" else utts + [utt(ques[d, j])]


def rows_rule(cap, ques, ans, opts, gt, mode, enc, dec, T, Ud, num_options=None, mask_prob=0.0, u_tok=None, cls=CLS, sep=SEP, mask=MASK,
              S=S_MAX):
    """numpy statement of gstvd_gen_rows.  enc [2, n_enc] / dec [3, n_dec] int (or None) -> a dict of the output arrays of the
    lists that are there (dec_labels all zero outside the train modes, where the kernel does not write it)."""
    assert mode in MODES
    cap, ques, ans = (np.asarray(x) for x in (cap, ques, ans))
    D, R, U = ques.shape
    train = mode in ("train_a", "train_q")
    assert R >= 1 and 2 * R <= S <= 64 and U <= 64 and cap.shape[1] <= 64 and T >= 2 and Ud >= 3
    assert mask_prob == 0 or u_tok is not None
    o = {}
    if not train:
        opts = np.asarray(opts)
        Ro, O = opts.shape[1:3]
        num_options = O if num_options is None else num_options
        assert Ro in (R, 1) and 2 <= num_options <= O <= 100
    if enc is not None:
        n = len(enc[0])
        o.update(tokens=np.zeros((n, T), np.int64), segments=np.zeros((n, T), np.int64), mlm=np.full((n, T), -1, np.int64),
                 att=np.zeros((n, T), np.float32), sep_indices=np.zeros((n, S), np.int64), hist_len=np.zeros(n, np.int64))
        for r in range(n):
            d, j = int(enc[0][r]), int(enc[1][r])
            if not (0 <= d < D and 0 <= j < R):
                continue                                                   # a row that names nothing: padding
            utts = context(cap, ques, ans, d, j, mode)
            ids, seg, lab, seps, att = encode(utts, T, S, mask_prob, (lambda p: u_tok[r, p]), cls, sep, mask)
            o["tokens"][r], o["segments"][r], o["mlm"][r], o["sep_indices"][r], o["att"][r] = ids, seg, lab, seps, att
            o["hist_len"][r] = len(utts) - 1
    if dec is not None:
        n = len(dec[0])
        o.update(dec_ids=np.zeros((n, Ud), np.int64), dec_att=np.zeros((n, Ud), np.float32), dec_labels=np.zeros((n, Ud), np.int64),
                 dec_option=np.full(n, -1, np.int32))
        for r in range(n):
            d, j, slot = (int(dec[i][r]) for i in range(3))
            if not (0 <= d < D and 0 <= j < R and 0 <= slot and (slot == 0 if train else slot < num_options)):
                continue
            if mode == "eval":
                g = int(np.asarray(gt)[d, j])
                if not 0 <= g < O:
                    continue
                c = eval_option(g, slot)
            elif mode == "test":
                c = slot
            if train:
                x = utt((ans if mode == "train_a" else ques)[d, j])
            else:
                x = utt(opts[d, j if Ro == R else 0, c])
                o["dec_option"][r] = c
            ids, _, _, _, att = encode([x[:Ud - 2]], Ud, S, 0.0, None, cls, sep, mask)
            ids = np.array(ids, np.int64)
            o["dec_att"][r] = att
            if train:
                o["dec_labels"][r, :-1] = ids[1:]
                ids[ids == sep] = 0
            o["dec_ids"][r] = ids
    return o


def expand_eval(cap, ques, ans, opts, gt, T, Ud, num_options, mask_prob=0.0, u_tok=None):
    """The eval loader's batch of the pools, on the host: enc_* [D, R, num_options, T] (every option's copy of the context; with
    noise each copy has its own draws, u_tok [D * R * num_options, T]), dec_* [D, R, num_options, Ud]."""
    D, R = np.asarray(ques).shape[:2]
    d, j, s = np.meshgrid(np.arange(D), np.arange(R), np.arange(num_options), indexing="ij")
    rows = np.stack([d.ravel(), j.ravel(), s.ravel()]).astype(np.int32)
    w = rows_rule(cap, ques, ans, opts, gt, "eval", rows[:2], rows, T, Ud, num_options, mask_prob, u_tok)
    sh = lambda k: torch.as_tensor(w[k]).view(D, R, num_options, -1)
    return dict(enc_input_ids=sh("tokens"), enc_segments=sh("segments"), enc_att_mask=sh("att"), enc_mlm_labels=sh("mlm"),
                enc_sep_indices=sh("sep_indices"), enc_hist_len=torch.as_tensor(w["hist_len"]).view(D, R, num_options),
                dec_input_ids=sh("dec_ids"), dec_att_mask=sh("dec_att"), gt_option_inds=torch.zeros(D, R, dtype=torch.long))


# ------------------------------------------------------------------------------------------------------------------ the cases
GenCase = collections.namedtuple("GenCase", "name cap ques ans opts gt mode enc dec T Ud num_options mask_prob u_tok")

EDGE_GT = np.array([[0, 5, 2, 3], [5, 0, 3, 1], [2, 4, 0, 5]], np.int64)


def edge_pools():
    """D = 3, R = 4, O = 6, U = 8, Lc = 8 for T = 32, Ud = 8.  Lengths (tests/test_exact_gen_rows_harness_cpu.py asserts each on the
    rule's output), the untruncated length of the context of round j in brackets:
      dialog 0: a full-width caption (8, no 0 in the row); q 3 5 5 3, a 2 2 4 6: [14, 23, 32 = T exactly, 41 far past T];
      dialog 1: caption 3; q 0 (empty) 8 (full width) 6 7, a 8 (full width) 1 2 7: [6, 24, 33 = one past T: the last [SEP] is lost, 44];
      dialog 2: an empty caption; q 2 3 1 4, a 0 (empty) 8 5 3: [5, 10, 21, 32].
    Every round has options of 0, 1, 3, 6 (= Ud - 2), 7 and 8 (> Ud - 2) tokens except where the ground truth's length (the answer)
    replaces one; gt_index holds 0 and O - 1 in every dialog."""
    gen = np.random.default_rng(53)
    cap_len = [8, 3, 0]
    q_len = [[3, 5, 5, 3], [0, 8, 6, 7], [2, 3, 1, 4]]
    a_len = [[2, 2, 4, 6], [8, 1, 2, 7], [0, 8, 5, 3]]
    base = [3, 7, 6, 0, 8, 1]
    cap = np.stack([_row(8, n, gen) for n in cap_len])
    ques = np.stack([np.stack([_row(8, n, gen) for n in q]) for q in q_len])
    o_len = [[[a_len[d][j] if c == EDGE_GT[d, j] else base[(c + d + j) % 6] for c in range(6)] for j in range(4)] for d in range(3)]
    opts = np.stack([np.stack([np.stack([_row(8, n, gen) for n in o]) for o in rnd]) for rnd in o_len])
    ans = np.stack([np.stack([opts[d, j, EDGE_GT[d, j]] for j in range(4)]) for d in range(3)])
    return cap, ques, ans, opts, EDGE_GT.copy()


def _noise(n, T, gen, p=0.15):
    u = gen.random((n, T)).astype(np.float32)
    u[:, 1::5] = np.float32(p)                                             # the strict comparison: never masked
    u[:, 2::5] = np.nextafter(np.float32(p), np.float32(0))                # its neighbour below, side by side: masked
    return u


def _grid(*dims):
    g = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    return np.stack([x.ravel() for x in g]).astype(np.int32)


def _full_rows(U, shape, gen):
    return gen.integers(V0, V1, tuple(shape) + (U,)).astype(np.int64)      # no 0 anywhere: every utterance fills its row


def cases():
    """The table of the exact harness: every rule at the smallest shape at which it can go wrong, the widest utterances, the most
    separators, and the production shape R = 10, O = 100, T = 256, Ud = 25 for sampled rows."""
    gen = np.random.default_rng(59)
    cap, ques, ans, opts, gt = edge_pools()
    T, Ud = 32, 8
    enc, dec6, dec4 = _grid(3, 4), _grid(3, 4, 6), _grid(3, 4, 4)
    dec0 = np.concatenate([enc, np.zeros((1, 12), np.int32)])
    n_rounds = np.array([4, 2, 1])
    tenc = np.stack([np.arange(3), n_rounds - 1]).astype(np.int32)
    tdec = np.stack([np.repeat(tenc[0], 6), np.repeat(tenc[1], 6), np.tile(np.arange(6), 3)]).astype(np.int32)
    opts1 = np.stack([opts[d, n_rounds[d] - 1][None] for d in range(3)])   # [D, 1, O, U]: the test split's only option list
    C = lambda name, mode, e, d, **k: GenCase(name, k.get("cap", cap), k.get("ques", ques), k.get("ans", ans), k.get("opts", opts),
                                              k.get("gt", gt), mode, e, d, k.get("T", T), k.get("Ud", Ud), k.get("no", 6),
                                              k.get("p", 0.0), k.get("u"))
    out = [
        C("eval_no6", "eval", enc, dec6),
        C("eval_no4", "eval", enc, dec4, no=4),
        C("eval_noise_row_per_option", "eval", dec6[:2], dec6, p=0.15, u=_noise(72, T, gen)),
        C("test_Ro1", "test", tenc, tdec, opts=opts1, gt=None),
        C("test_RoR_no5", "test", tenc, tdec[:, tdec[2] < 5], gt=None, no=5),
        C("train_a", "train_a", enc, dec0, opts=None, gt=None),
        C("train_q", "train_q", enc, dec0, opts=None, gt=None),
        C("train_q_noise", "train_q", enc, dec0, opts=None, gt=None, p=0.15, u=_noise(12, T, gen)),
        C("eval_enc_only", "eval", enc, None),
        C("eval_dec_only", "eval", None, dec6),
        C("train_a_enc_only", "train_a", enc, None, opts=None, gt=None),
        C("train_q_dec_only", "train_q", None, dec0, opts=None, gt=None),
    ]
    # rows that name nothing (dialog, round, slot out of range; a ground truth outside the options) next to good ones
    bad_gt = gt.copy()
    bad_gt[1, 1], bad_gt[2, 2] = 6, -1
    benc = np.array([[0, 3, -1, 1, 2, 2], [0, 0, 0, 4, -1, 3]], np.int32)
    bdec = np.array([[0, 3, -1, 1, 2, 1, 0, 1, 2, 0, 2], [0, 0, 0, 4, -1, 1, 2, 0, 2, 1, 3], [0, 0, 0, 0, 0, 1, 4, -1, 0, 3, 3]], np.int32)
    out += [C("eval_invalid_rows", "eval", benc, bdec, gt=bad_gt, no=4),
            C("test_invalid_rows", "test", benc, bdec, gt=None, no=4),
            C("train_a_invalid_rows", "train_a", benc, bdec, opts=None, gt=None),
            C("train_q_invalid_rows", "train_q", benc, bdec, opts=None, gt=None)]
    # U = Lc = 64, every row full: Ud = 70 keeps the 64 tokens (and walks the row in two steps), Ud = 25 cuts them to 23
    wide = dict(cap=_full_rows(64, (1,), gen), ques=_full_rows(64, (1, 2), gen), opts=_full_rows(64, (1, 2, 2), gen),
                gt=np.array([[1, 0]], np.int64))
    wide["ans"] = np.stack([np.stack([wide["opts"][0, j, wide["gt"][0, j]] for j in range(2)])])
    out += [C("eval_U64_Ud70", "eval", _grid(1, 2), _grid(1, 2, 2), T=200, Ud=70, no=2, **wide),
            C("train_a_U64_Ud25", "train_a", _grid(1, 2), np.concatenate([_grid(1, 2), np.zeros((1, 2), np.int32)]), T=300, Ud=25,
              **dict(wide, opts=None, gt=None))]
    # R = 12 under S = 25: round 11 has 24 separators (23 for the questioner)
    r12 = dict(cap=np.stack([_row(8, 4, gen)]), ques=np.stack([np.stack([_row(8, int(gen.integers(0, 4)), gen) for _ in range(12)])]),
               opts=np.stack([np.stack([np.stack([_row(8, int(gen.integers(0, 4)), gen) for _ in range(2)]) for _ in range(12)])]),
               gt=gen.integers(0, 2, (1, 12)).astype(np.int64))
    r12["ans"] = np.stack([np.stack([r12["opts"][0, j, r12["gt"][0, j]] for j in range(12)])])
    out += [C("eval_R12", "eval", _grid(1, 12), _grid(1, 12, 2), T=64, no=2, **r12),
            C("train_q_R12", "train_q", _grid(1, 12), np.concatenate([_grid(1, 12), np.zeros((1, 12), np.int32)]), T=64,
              **dict(r12, opts=None, gt=None))]
    # the production shape: every context of two dialogs, 48 sampled option rows, 24 noisy rows with their own draws
    bcap, bques, bans, bopts, bgt = big_pools()
    big = dict(cap=bcap, ques=bques, ans=bans, opts=bopts, gt=bgt, T=256, Ud=25, no=100)
    pick = gen.permutation(2 * 10 * 100)[:48]
    rows = np.stack([pick // 1000, pick // 100 % 10, pick % 100]).astype(np.int32)
    rows[:, 0], rows[:, 1], rows[:, 2] = (0, 0, 99), (0, 1, 99), (1, 9, 71)                          # gt 0 / O - 1 / 70 at the far slots
    out += [C("eval_full", "eval", _grid(2, 10), rows, **big),
            C("eval_full_noise", "eval", rows[:2, :24], rows[:, :24], p=0.15, u=_noise(24, 256, gen), **big),
            C("train_q_full", "train_q", _grid(2, 10), np.concatenate([_grid(2, 10), np.zeros((1, 20), np.int32)]),
              **dict(big, opts=None, gt=None))]
    return out


def rule_of(c):
    return rows_rule(c.cap, c.ques, c.ans, c.opts, c.gt, c.mode, c.enc, c.dec, c.T, c.Ud, c.num_options, c.mask_prob, c.u_tok)


# ------------------------------------------------------------------------------------------------------------------ the harness
def rows_windows(c, device, S=S_MAX):
    """The outputs as windows: POISON inside, canaries around; the [n, T] arrays share one row stride, the [n, Ud] arrays one."""
    w = {}
    if c.enc is not None:
        n = c.enc.shape[1]
        for k, cols, pad in (("tokens", c.T, 3), ("segments", c.T, 3), ("mlm", c.T, 3), ("att", c.T, 3), ("sep_indices", S, 2)):
            w[k] = Window(n, cols, torch.float32 if k == "att" else torch.int64, device, "canary", ld=cols + pad)
        w["hist_len"] = Window(1, n, torch.int64, device, "canary", guard=1)
    if c.dec is not None:
        n = c.dec.shape[1]
        for k in ("dec_ids", "dec_att", "dec_labels"):
            w[k] = Window(n, c.Ud, torch.float32 if k == "dec_att" else torch.int64, device, "canary", ld=c.Ud + 5)
    for v in w.values():
        v.view.fill_(POISON)
    return w


def run_case(be, c, want=None):
    """`be.rows` on case c into poisoned windows with strided pools, against rows_rule (or the recorded `want`); twice: same bits."""
    dev = be.device
    if want is None:
        want = rule_of(c)
    train = c.mode in ("train_a", "train_q")
    capw = _window(c.cap, torch.int64, dev, 3)
    capw.flat[~capw.inside.to(capw.flat.device)] = V1 + 9                   # ids, not canaries, behind every caption row
    big, opts = _strided_opts(c.opts, dev) if c.opts is not None else (None, None)
    ins = dict(cap=capw.view, ques=_t(c.ques, dev, torch.int64), ans=_t(c.ans, dev, torch.int64), opts=opts, gt=_t(c.gt, dev, torch.int64),
               enc=_t(c.enc, dev, torch.int32), dec=_t(c.dec, dev, torch.int32), u_tok=_t(c.u_tok, dev, torch.float32))
    for k in ("enc", "dec"):                                                # the row lists: three dense vectors each
        ins[k] = None if ins[k] is None else ins[k].contiguous()
    keep = {k: v.clone() for k, v in ins.items() if v is not None}
    big0 = None if big is None else big.clone()
    names = out_names(c)
    got = []
    for rep in range(2):
        w = rows_windows(c, dev)
        out = {k: (v.vector() if k == "hist_len" else v.view) for k, v in w.items()}
        if c.dec is not None:
            n_dec = c.dec.shape[1]
            opt_buf, out["dec_option"] = _i32_vec(np.full(n_dec, POISON), dev)
        be.rows(ins["cap"], ins["ques"], ins["ans"], ins["opts"], ins["gt"], c.mode, c.T, c.Ud,
                None if c.enc is None else (ins["enc"][0], ins["enc"][1]),
                None if c.dec is None else (ins["dec"][0], ins["dec"][1], ins["dec"][2]),
                num_options=None if train else c.num_options, mask_prob=c.mask_prob, u_tok=ins["u_tok"], out=out)
        for k in names:
            v = out[k].cpu()
            assert not bool((v == POISON).any()), "%s: %s has elements the launch did not write" % (c.name, k)
            ref = torch.as_tensor(want[k]).reshape(v.shape).to(v.dtype)
            same = torch.equal(v.view(torch.int32), ref.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(v, ref)
            assert same, "%s: %s differs from the rule at %s" % (c.name, k, (v != ref).nonzero()[:6].tolist())
        if c.dec is not None and not train:
            assert bool((out["dec_labels"] == POISON).all()), c.name + ": dec_labels was written outside the train modes"
        for k, win in w.items():
            win.assert_surroundings_untouched("%s %s" % (c.name, k))
        if c.dec is not None:
            _i32_intact(opt_buf, n_dec, c.name + " dec_option")
        got.append({k: out[k].cpu().clone() for k in names})
    for k in names:
        assert torch.equal(got[0][k], got[1][k]), "%s: %s differs between two launches" % (c.name, k)
    for k, v in keep.items():
        assert torch.equal(ins[k], v), "%s: input %s was written" % (c.name, k)
    assert big is None or torch.equal(big, big0), c.name + ": the option pool was written"
    return got[0]


FIXTURE_CASES = ("eval", "eval_noise", "test", "train_a", "train_q")


def fixture_cases(g):
    """The cases of tests/golden/gen_rows.npz (a dict of numpy arrays) as (GenCase, recorded outputs) pairs.  The pools are stored
    once (`pools::`); a case may carry its own opts (the test split's [D, 1, O, U])."""
    out = []
    for n in sorted(set(k.split("::")[0] for k in g) - {"pools"}):
        f = lambda k: np.asarray(g["%s::%s" % (n, k)])
        opt = lambda k: f(k) if ("%s::%s" % (n, k)) in g else None
        pool = lambda k: opt(k) if opt(k) is not None else np.asarray(g["pools::" + k])
        mode = MODES[int(f("mode"))]
        train = mode in ("train_a", "train_q")
        enc, dec = opt("enc"), opt("dec")
        c = GenCase(n, pool("cap"), pool("ques"), pool("ans"), None if train else pool("opts"), pool("gt") if mode == "eval" else None, mode,
                    None if enc is None else enc.astype(np.int32), None if dec is None else dec.astype(np.int32), int(f("T")), int(f("Ud")),
                    int(f("num_options")), float(f("mask_prob")), opt("u_tok"))
        out.append((c, {k: f("out_" + k) for k in ENC_OUT + DEC_OUT if opt("out_" + k) is not None}))
    return out


class NumpyBackend(object):
    """Stand-in backend: the rule itself, written into the caller's tensors (proves the harness without a GPU)."""
    device = "cpu"

    def rows(self, cap, ques, ans, opts, gt, mode, T, Ud, enc_rows=None, dec_rows=None, num_options=None, mask_prob=0.0, u_tok=None, out=None):
        n = lambda x: None if x is None else x.numpy()
        rows = lambda l: None if l is None else np.stack([n(x) for x in l])
        r = rows_rule(n(cap), n(ques), n(ans), n(opts), n(gt), mode, rows(enc_rows), rows(dec_rows), T, Ud, num_options, mask_prob, n(u_tok))
        for k, v in r.items():
            if k != "dec_labels" or mode in ("train_a", "train_q"):
                out[k].copy_(torch.as_tensor(v).reshape(out[k].shape))
        return out
