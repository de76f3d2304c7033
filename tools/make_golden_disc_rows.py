"""Fixture of the discriminative rows: tests/golden/disc_rows.npz, modelled on tools/make_golden_selftrain.py.

Runs in the build container only.  It imports the reference tree (the path of oracle.ref_harness) and copies none of its text: it
drives the reference's own loader, dataloader/dataloader_visdial_disc.py `VisdialDataset.__getitem__`, on an object that was never
constructed (object.__new__: the constructor opens JSON files, an LMDB reader and a tokenizer, none of which exist here) and whose
attributes are stand-ins:

  * the JSON dicts hold keys instead of text, and `tokenizer.encode(key)` returns the recorded ids of that utterance, so the
    token-id pools ARE the loader's inputs;
  * the feature reader returns recorded arrays;
  * the modules the loader imports and that are not installed (pytorch_transformers, h5py / lmdb behind
    utils.image_features_reader) are empty stand-ins, as in oracle/ref_harness.py;
  * the name `random` inside the loader module and inside utils.data_utils is bound, for the duration of a call, to a play-back:
    `choice` walks a recorded permutation of the candidates (the option the loop settles on is therefore its first feasible
    element, or its last one), `random` returns recorded fp32-representable draws in call order, `randint` a recorded region.

Option order, pruneRounds, the negative loop with its running length, encode_input and encode_image_input all run as the reference
wrote them.  What the fixture stores per case (keys `<case>::<name>`): the pools cap, ques, ans, opts, gt; dense (train_dense);
the scalars T, tot_rounds, num_options, train, mask_prob; rows [3, N] (dialog, round, slot); the recorded out_tokens, out_segments,
out_mask, out_sep_indices, out_hist_len, out_nsp_labels, and out_neg_option -- the option each negative settled on, from which the
tests derive u_neg = (rank + 0.5) / |F| (or / |C|); u_tok [N, T]: the draw each utterance token at position p < T received (0.0
at every other position: a draw that would mask if it were looked at); for train cases the image record img_feats, img_image_mask,
img_u_img, img_forced_region and the loader's img_out_feats, img_out_label.  out_att is train_disc.py:97-99 restated (one line).

    python tools/make_golden_disc_rows.py

Cases: train_a (R = 10, O = 6, T = 64, no pruning, 2 negatives), train_b (T = 48, tot_rounds 3, num_options 4 < O, train_dense: late
rounds have few or no feasible negatives), eval_a / eval_b (R = 4, O = 6, T = 32; tot_rounds 11 / 2, num_options 6 / 4), and the
production shape R = 10, O = 100, U = 18, T = 256 as a sample of 24 rows each: full_train, full_eval.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                   # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, GOLDEN                # noqa: E402

CLS, SEP, MASK, PAD, UNK = 101, 102, 103, 0, 100
V0, V1 = 104, 320
REGIONS, FEAT, CLASSES = 37, 8, 6


def reference_loader():
    if RH.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, RH.REFERENCE_ROOT)
    pt = types.ModuleType("pytorch_transformers")
    tb = types.ModuleType("pytorch_transformers.tokenization_bert")
    tb.BertTokenizer = object
    pt.tokenization_bert = tb
    sys.modules.setdefault("pytorch_transformers", pt)
    sys.modules.setdefault("pytorch_transformers.tokenization_bert", tb)
    rd = types.ModuleType("utils.image_features_reader")               # the real one imports h5py and lmdb at the top
    rd.ImageFeaturesH5Reader = object
    import utils                                                        # noqa: F401
    sys.modules.setdefault("utils.image_features_reader", rd)
    import utils.data_utils as DU
    import dataloader.dataloader_visdial_disc as DL
    return DL, DU


class Playback(object):
    """Stands in for the `random` module inside the two reference modules for one __getitem__."""

    def __init__(self, perms, draws, region):
        self.perms, self.draws, self.region = [list(p) for p in perms], [float(x) for x in draws], int(region)
        self.k, self.perm_i, self.pos, self.chosen, self.cur, self.lists = 0, -1, 0, [], None, []

    def choice(self, seq):
        if seq is not self.cur:                                        # a new negative: the loader builds a fresh list for each
            self.perm_i, self.pos, self.cur = self.perm_i + 1, 0, seq
            assert sorted(seq) == sorted(self.perms[self.perm_i]), (seq, self.perms[self.perm_i])
            self.chosen.append(None)
            self.lists.append([seq, 0])
        self.lists[-1][1] += 1
        v = self.perms[self.perm_i][self.pos]
        assert v in seq
        self.pos += 1
        self.chosen[-1] = v
        return v

    def kinds(self):
        """Per negative: 'none' (the loop emptied its list), 'retried' (it met an option that did not fit, then one that did), 'first'."""
        return ["none" if not left else "retried" if calls > 1 else "first" for left, calls in self.lists]

    def random(self):
        self.k += 1
        return self.draws[self.k - 1] if self.k <= len(self.draws) else 0.5

    def randint(self, a, b):
        assert a == 1 and b == REGIONS - 1
        return self.region


class Tokenizer(object):
    def __init__(self, table):
        self.table = table

    def encode(self, key):
        return list(self.table[key])


class Reader(object):
    def __init__(self, items):
        self.items = items

    def __getitem__(self, img_id):
        return self.items[img_id]


def _ids(row):
    row = [int(v) for v in row]
    return row[:row.index(0)] if 0 in row else row


def dataset(DL, pools, params, images, dense, val_dense):
    """A VisdialDataset that was never constructed: its attributes are the stand-ins described above."""
    cap, ques, ans, opts, gt = pools
    D, R, O = opts.shape[:3]
    table, questions, answers, dialogs = {}, [], [], []
    for d in range(D):
        table["c%d" % d] = _ids(cap[d])
        rounds = []
        for j in range(R):
            questions.append("q%d_%d" % (d, j))
            table[questions[-1]] = _ids(ques[d, j])
            first = len(answers)
            for c in range(O):
                answers.append("o%d_%d_%d" % (d, j, c))
                table[answers[-1]] = _ids(opts[d, j, c])
            assert _ids(ans[d, j]) == _ids(opts[d, j, gt[d, j]])
            rounds.append(dict(question=len(questions) - 1, answer=first + int(gt[d, j]), gt_index=int(gt[d, j]),
                               answer_options=list(range(first, first + O))))
        dialogs.append(dict(image_id=d, caption="c%d" % d, dialog=rounds))
    data = dict(data=dict(dialogs=dialogs, questions=questions, answers=answers))
    ds = object.__new__(DL.VisdialDataset)
    ds.numDataPoints = dict(vd_train=D, vd_eval_val=D)
    ds.visdial_data_train = ds.visdial_data_val = data
    ds.visdial_data_train_dense = None if dense is None else [dict(scores=[[float(s) for s in r] for r in dense[d]]) for d in range(D)]
    ds.visdial_data_val_dense = val_dense
    ds.overfit = False
    ds.num_options = params["num_options"]
    ds.subsets = ["vd_train", "vd_eval_val", "vd_eval_test", "vd_gen_val"]
    ds.tokenizer = Tokenizer(table)
    ds.CLS, ds.MASK, ds.SEP, ds.PAD, ds.UNK = CLS, MASK, SEP, PAD, UNK
    ds.params = params
    ds._max_region_num = REGIONS
    ds._image_features_reader = Reader(images)
    return ds


def getitem(DL, DU, ds, mode, index, pb):
    real_l, real_u = DL.random, DU.random
    DL.random = DU.random = pb
    try:
        ds._mode = mode
        return ds[index]
    finally:
        DL.random, DU.random = real_l, real_u


def draws_by_position(sep_indices, hist_len, seq, T):
    """The draws of one row, made in token order, as u_tok[p] for p < T: position 0 is [CLS], the separator positions are skipped."""
    u = np.zeros(T, np.float32)
    seps = set(int(s) for s in sep_indices[:int(hist_len) + 1])
    k = 0
    for p in range(1, int(sep_indices[int(hist_len)])):
        if p in seps:
            continue
        if p < T:
            u[p] = seq[k]
        k += 1
    return u, k


def _row(U, n, gen):
    row = np.zeros(U, np.int64)
    row[:n] = gen.integers(V0, V1, n)
    return row


def make_pools(gen, D, R, O, U, Lc, cap_lens, q_hi, o_hi):
    cap = np.stack([_row(Lc, n, gen) for n in cap_lens])
    ques = np.stack([np.stack([_row(U, int(gen.integers(0, q_hi + 1)), gen) for _ in range(R)]) for _ in range(D)])
    opts = np.stack([np.stack([np.stack([_row(U, int(gen.integers(0, o_hi + 1)), gen) for _ in range(O)]) for _ in range(R)]) for _ in range(D)])
    gt = gen.integers(0, O, (D, R)).astype(np.int64)
    gt[0, 0], gt[0, 1] = 0, O - 1
    ans = np.stack([np.stack([opts[d, j, gt[d, j]] for j in range(R)]) for d in range(D)])
    return cap, ques, ans, opts, gt


def make_images(gen, D, boxes):
    out = []
    for d in range(D):
        n = boxes[d]
        out.append((gen.standard_normal((n, FEAT)).astype(np.float32), n, gen.random((n, 5)).astype(np.float32), None,
                    gen.random((n, CLASSES)).astype(np.float32)))
    return out


def fp32_draws(gen, n):
    u = gen.random(n).astype(np.float32)
    u[1::6], u[2::6] = np.float32(0.15), np.nextafter(np.float32(0.15), np.float32(0))
    return u


def record_train(DL, DU, gen, pools, params, dense, boxes, forced):
    cap, ques, ans, opts, gt = pools
    D, R, O = opts.shape[:3]
    T, nneg, no = params["max_seq_len"], params["num_negative_samples"], params["num_options"]
    images = make_images(gen, D, boxes)
    ds = dataset(DL, pools, params, images, dense, None)
    rec = {k: [] for k in ("rows", "tokens", "segments", "mask", "sep_indices", "hist_len", "nsp_labels", "neg_option", "u_tok", "kinds")}
    img = {k: [] for k in ("feats", "image_mask", "u_img", "forced_region", "out_feats", "out_label")}
    for d in range(D):
        perms = []
        for j in range(R):
            C = [c for c in range(O) if c != gt[d, j]][:no - 1]
            perms += [list(gen.permutation(C)) for _ in range(nneg)]
        seq = fp32_draws(gen, 64 * R * (1 + nneg) * 3)
        pb = Playback(perms, seq, forced[d])
        item = getitem(DL, DU, ds, "vd_train", d, pb)
        assert len(pb.chosen) == R * nneg and item["tokens"].shape == (R, 1 + nneg, T)
        rec["kinds"] += pb.kinds()
        k = 0
        for j in range(R):
            for s in range(1 + nneg):
                u, used = draws_by_position(item["sep_indices"][j, s].numpy(), item["hist_len"][j, s], seq[k:], T)
                k += used
                rec["rows"].append((d, j, s))
                rec["u_tok"].append(u)
                rec["neg_option"].append(-1 if s == 0 else pb.chosen[j * nneg + s - 1])
                for name, key in (("tokens", "tokens"), ("segments", "segments"), ("mask", "mask"), ("sep_indices", "sep_indices"),
                                  ("hist_len", "hist_len"), ("nsp_labels", "next_sentence_labels")):
                    rec[name].append(item[key][j, s].numpy())
        n = min(boxes[d], REGIONS)
        assert pb.k == k + n, (pb.k, k, n)                                # every draw is accounted for: tokens, then real regions
        u_img = np.zeros(REGIONS, np.float64)
        u_img[:n] = seq[k:k + n]
        feats = np.zeros((REGIONS, FEAT), np.float32)
        feats[:n] = images[d][0][:n]
        for key, v in (("feats", feats), ("image_mask", item["image_mask"].numpy()), ("u_img", u_img), ("forced_region", forced[d]),
                       ("out_feats", item["image_feat"].numpy()), ("out_label", item["image_label"].numpy())):
            img[key].append(v)
    return rec, img


def record_eval(DL, DU, gen, pools, params, round_ids):
    cap, ques, ans, opts, gt = pools
    D, R, O = opts.shape[:3]
    rel = gen.random((D, O)).astype(np.float32)
    val_dense = [dict(round_id=int(round_ids[d]), gt_relevance=[float(x) for x in rel[d]]) for d in range(D)]
    ds = dataset(DL, pools, params, make_images(gen, D, [REGIONS] * D), None, val_dense)
    rec = {k: [] for k in ("rows", "tokens", "segments", "mask", "sep_indices", "hist_len", "neg_option")}
    rel_out = []
    for d in range(D):
        item = getitem(DL, DU, ds, "vd_eval_val", d, Playback([], [], 1))
        assert not item["gt_option_inds"].any()
        rel_out.append(item["gt_relevance"].numpy())
        for j in range(R):
            for s in range(params["num_options"]):
                rec["rows"].append((d, j, s))
                rec["neg_option"].append(int(gt[d, j]) if s == 0 else (s - 1 if s - 1 < gt[d, j] else s))   # checked below
                for key in ("tokens", "segments", "mask", "sep_indices", "hist_len"):
                    rec[key].append(item[key][j, s].numpy())
                # the option the loader put at slot s: its tokens sit in front of the row's last separator
                seps, h = item["sep_indices"][j, s].numpy(), int(item["hist_len"][j, s])
                lo, hi = (int(seps[h - 1]) + 1 if h else 1), int(seps[h])
                if hi <= params["max_seq_len"]:
                    assert item["tokens"][j, s, lo:hi].tolist() == _ids(opts[d, j, rec["neg_option"][-1]])
    return rec, dict(gt_relevance=rel, round_id=np.asarray(round_ids, np.int64), out_gt_relevance=np.stack(rel_out))


def pack(name, out, pools, params, train, rec, dense=None, img=None, extra=None, sample=None):
    cap, ques, ans, opts, gt = pools
    idx = np.arange(len(rec["rows"])) if sample is None else np.sort(sample)
    put = lambda k, v: out.__setitem__("%s::%s" % (name, k), np.asarray(v))
    for k, v in (("cap", cap), ("ques", ques), ("ans", ans), ("opts", opts), ("gt", gt), ("T", params["max_seq_len"]),
                 ("tot_rounds", params["visdial_tot_rounds"]), ("num_options", params["num_options"]), ("train", int(train)),
                 ("mask_prob", params["mask_prob"] if train else 0.0)):
        put(k, v)
    if dense is not None:
        put("dense", dense)
    put("rows", np.array(rec["rows"], np.int32)[idx].T)
    for k in ("tokens", "segments", "mask", "sep_indices", "hist_len", "nsp_labels"):
        if k in rec:
            put("out_" + k, np.stack([np.asarray(rec[k][i]) for i in idx]).reshape(len(idx), -1) if k != "hist_len"
                else np.array([int(rec[k][i]) for i in idx], np.int64))
    put("out_neg_option", np.array(rec["neg_option"], np.int32)[idx])
    sep, hist = out["%s::out_sep_indices" % name], out["%s::out_hist_len" % name]
    put("out_att", (np.arange(params["max_seq_len"])[None] < (sep[np.arange(len(idx)), hist] + 1)[:, None]).astype(np.float32))
    if "u_tok" in rec:
        put("u_tok", np.stack([rec["u_tok"][i] for i in idx]))
    for k, v in (img or {}).items():
        put("img_" + k, np.stack([np.asarray(x) for x in v]))
    for k, v in (extra or {}).items():
        put(k, v)
    print("%-11s rows %4d  T %3d  masked %4d  cut rows %3d  negatives %3d" % (
        name, len(idx), params["max_seq_len"], int((out["%s::out_mask" % name] >= 0).sum()),
        int((sep[np.arange(len(idx)), hist] >= params["max_seq_len"]).sum()), int((out["%s::out_neg_option" % name] >= 0).sum() if train else 0)))


def main():
    DL, DU = reference_loader()
    gen = np.random.default_rng(4321)
    out = {}
    base = dict(num_negative_samples=2, train_dense=False, mask_prob=0.15)
    # train_a / train_b: the loader asserts ten rounds
    pools = make_pools(gen, 2, 10, 6, 10, 12, (12, 4), 3, 9)
    p = dict(base, max_seq_len=64, visdial_tot_rounds=11, num_options=6)
    rec, img = record_train(DL, DU, gen, pools, p, None, (REGIONS + 3, 20), (5, 30))     # dialog 1: region 30 is padding and is forced
    assert {"none", "retried", "first"} == set(rec["kinds"]), set(rec["kinds"])  # a round where only some negatives fit is recorded
    pack("train_a", out, pools, p, True, rec, img=img)
    pools = make_pools(gen, 2, 10, 6, 10, 12, (9, 0), 3, 10)
    dense = gen.random((2, 10, 6))
    p = dict(base, max_seq_len=48, visdial_tot_rounds=3, num_options=4, train_dense=True)
    rec, img = record_train(DL, DU, gen, pools, p, dense, (REGIONS, 1), (36, 1))
    pack("train_b", out, pools, p, True, rec, dense=dense, img=img)
    # eval_a / eval_b
    pools = make_pools(gen, 2, 4, 6, 10, 12, (12, 3), 5, 8)
    for name, tr, no in (("eval_a", 11, 6), ("eval_b", 2, 4)):
        p = dict(base, max_seq_len=32, visdial_tot_rounds=tr, num_options=no)
        rec, extra = record_eval(DL, DU, gen, pools, p, (1, 4))
        pack(name, out, pools, p, False, rec, extra=extra)
    # the production shape, 24 sampled rows of each mode
    pools = make_pools(gen, 1, 10, 100, 18, 38, (38,), 17, 18)
    dense = gen.random((1, 10, 100))
    p = dict(base, max_seq_len=256, visdial_tot_rounds=11, num_options=100, num_negative_samples=4, train_dense=True)
    rec, img = record_train(DL, DU, gen, pools, p, dense, (REGIONS,), (7,))
    pack("full_train", out, pools, p, True, rec, dense=dense, img=img, sample=gen.permutation(len(rec["rows"]))[:24])
    rec, extra = record_eval(DL, DU, gen, pools, p, (10,))
    pack("full_eval", out, pools, p, False, rec, extra=extra, sample=gen.permutation(len(rec["rows"]))[:24])
    files = write_npz(os.path.join(GOLDEN, "disc_rows.npz"), out)
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
