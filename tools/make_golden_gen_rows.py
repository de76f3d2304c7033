"""Fixture of the generative rows: tests/golden/gen_rows.npz, modelled on tools/make_golden_disc_rows.py.

Runs in the build container only.  It imports the reference tree (the path of oracle.ref_harness) and copies none of its text: it
drives the reference's own loader, dataloader/dataloader_visdial_gen.py `VisdialDataset.__getitem__`, on an object that was never
constructed (object.__new__: the constructor opens JSON files, a feature reader and a tokenizer, none of which exist here) and whose
attributes are stand-ins:

  * the JSON dicts hold keys instead of text, and `tokenizer.encode(key)` returns the recorded ids of that utterance, so the
    token-id pools ARE the loader's inputs;
  * the feature reader returns recorded arrays;
  * the modules the loader imports and that are not installed are empty stand-ins (tools/make_golden_disc_rows.reference_loader);
  * the name `random` inside the loader module and inside utils.data_utils is bound, for the duration of a call, to a play-back
    that returns recorded fp32-representable draws in call order.

The option order, the context lists of every mode, the cut of the targets, encode_input and the label shift all run as the
reference wrote them, at the production shape R = 10, O = 100, U = 18, T = 256, Ud = 25 (the eval loop is written for ten rounds of a
hundred options), for two dialogs.  The pools are stored once (`pools::cap, ques, ans, opts, gt`); per case (keys `<case>::<name>`):
mode (0 eval, 1 test, 2 train_a, 3 train_q), T, Ud, num_options, mask_prob, the row lists enc [2, n_enc] (dialog, round) and dec
[3, n_dec] (dialog, round, slot), the loader's rows out_tokens, out_segments, out_mlm, out_att, out_sep_indices, out_hist_len,
out_dec_ids, out_dec_att, out_dec_labels (train) and out_dec_option (eval / test: the option the slot rule names, checked against
the tokens the loader put there).  To stay below the size limit of a committed file the rows are sampled:

  eval        every context (option 0's copy; the loader's 100 copies of a round are compared here and found equal), 48 option rows;
              plus gt_relevance [D, O], round_id and the loader's re-ordered out_gt_relevance
  eval_noise  attack = 'random_token', mask_prob 0.15: 16 (dialog, round, option) rows, each with ITS copy of the context and u_tok
              [16, T]: the draw each utterance token at position p < T received (0.0 at every other position: a draw that would
              mask if it were looked at)
  test        dialogs of 10 and 4 rounds, opts [D, 1, O, U] (the last round's list), n_rounds; both contexts, 32 option rows
  train_a     -model enc_dec_a: all 20 context and target rows
  train_q     -model enc_dec_q: the same for the questioner

    python tools/make_golden_gen_rows.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_disc_rows as MD                                     # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, GOLDEN                # noqa: E402

CLS, SEP, MASK, PAD, UNK = MD.CLS, MD.SEP, MD.MASK, MD.PAD, MD.UNK
REGIONS = MD.REGIONS
D, R, O, U, LC, T, UD = 2, 10, 100, 18, 38, 256, 25


def reference_loader():
    _, DU = MD.reference_loader()                                       # installs the stand-in modules and the reference path
    import dataloader.dataloader_visdial_gen as DL
    return DL, DU


def dataset(DL, pools, params, images, val_dense, n_rounds=None):
    """A VisdialDataset that was never constructed.  n_rounds: the test split -- dialog d has that many rounds, the last one
    without an answer and with the option list."""
    cap, ques, ans, opts, gt = pools
    table, questions, answers, dialogs = {}, [], [], []
    for d in range(D):
        table["c%d" % d] = MD._ids(cap[d])
        rounds = []
        for j in range(R if n_rounds is None else int(n_rounds[d])):
            questions.append("q%d_%d" % (d, j))
            table[questions[-1]] = MD._ids(ques[d, j])
            first = len(answers)
            for c in range(O):
                answers.append("o%d_%d_%d" % (d, j, c))
                table[answers[-1]] = MD._ids(opts[d, j, c])
            assert MD._ids(ans[d, j]) == MD._ids(opts[d, j, gt[d, j]])
            rnd = dict(question=len(questions) - 1, answer=first + int(gt[d, j]), gt_index=int(gt[d, j]),
                       answer_options=list(range(first, first + O)))
            if n_rounds is not None:
                if j == int(n_rounds[d]) - 1:
                    del rnd["answer"], rnd["gt_index"]
                else:
                    del rnd["answer_options"], rnd["gt_index"]
            rounds.append(rnd)
        dialogs.append(dict(image_id=d, caption="c%d" % d, dialog=rounds, round_id=len(rounds)))
    data = dict(data=dict(dialogs=dialogs, questions=questions, answers=answers))
    ds = object.__new__(DL.VisdialDataset)
    ds.numDataPoints = dict(vd_train=D, vd_eval_val=D, vd_eval_test=D, vd_gen_val=D)
    ds.visdial_data_train = ds.visdial_data_val = ds.visdial_data_test = data
    ds.visdial_data_val_dense = val_dense
    ds.overfit = False
    ds.num_options = params["num_options"]
    ds.subsets = ["vd_train", "vd_eval_val", "vd_eval_test", "vd_gen_val"]
    ds.tokenizer = MD.Tokenizer(table)
    ds.CLS, ds.MASK, ds.SEP, ds.PAD, ds.UNK = CLS, MASK, SEP, PAD, UNK
    ds.params = params
    ds._max_region_num = REGIONS
    ds._max_seq_len, ds._max_utt_len = params["max_seq_len"], params["max_utt_len"]
    ds._image_features_reader = MD.Reader(images)
    return ds


ENC = (("tokens", "enc_input_ids"), ("segments", "enc_segments"), ("mlm", "enc_mlm_labels"), ("att", "enc_att_mask"),
       ("sep_indices", "enc_sep_indices"))
DEC = (("dec_ids", "dec_input_ids"), ("dec_att", "dec_att_mask"))


def eval_option(gt, slot):
    return gt if slot == 0 else (slot - 1 if slot - 1 < gt else slot)


def check_option(item_ids, x, who):
    """The decoder row the loader wrote holds [CLS], the first Ud - 2 tokens of option x and [SEP]."""
    want = [CLS] + MD._ids(x)[:UD - 2] + [SEP]
    assert item_ids[:len(want)].tolist() == want and not item_ids[len(want):].any(), who


def put_rows(out, name, mode, params, enc, dec, rec, extra=None):
    put = lambda k, v: out.__setitem__("%s::%s" % (name, k), np.asarray(v))
    for k, v in (("mode", mode), ("T", params["max_seq_len"]), ("Ud", params["max_utt_len"]), ("num_options", params["num_options"]),
                 ("mask_prob", params["mask_prob"] if params["attack"] == "random_token" else 0.0),
                 ("enc", np.array(enc, np.int32).T), ("dec", np.array(dec, np.int32).T)):
        put(k, v)
    for k, v in rec.items():
        put(k if k == "u_tok" else "out_" + k, np.stack([np.asarray(x) for x in v]) if np.ndim(v[0]) else
            np.array(v, np.int32 if k == "dec_option" else np.int64))
    for k, v in (extra or {}).items():
        put(k, v)
    print("%-10s enc rows %3d  dec rows %3d  masked %4d  cut rows %3d" % (
        name, len(enc), len(dec), int((out[name + "::out_mlm"] >= 0).sum()),
        int((out[name + "::out_sep_indices"][np.arange(len(enc)), out[name + "::out_hist_len"]] >= params["max_seq_len"]).sum())))


def record_eval(DL, DU, gen, pools, images, out):
    cap, ques, ans, opts, gt = pools
    rel = gen.random((D, O)).astype(np.float32)
    round_ids = (3, 10)
    val_dense = [dict(round_id=round_ids[d], gt_relevance=[float(x) for x in rel[d]]) for d in range(D)]
    base = dict(num_options=O, max_seq_len=T, max_utt_len=UD, vd_version="1.0", model="enc_dec_a", mask_prob=0.15)
    pick = set(int(x) for x in gen.permutation(D * R * O)[:45]) | {99, 199, 1099}   # + the far slot of gt 0, of gt O - 1 and of a round 0
    noisy = set(int(x) for x in gen.permutation(D * R * O)[:16])
    for name, attack in (("eval", None), ("eval_noise", "random_token")):
        params = dict(base, attack=attack)
        ds = dataset(DL, pools, params, images, val_dense)
        rec = {k: [] for k, _ in ENC + DEC}
        rec.update(hist_len=[], dec_option=[])
        enc, dec, rel_out = [], [], []
        if attack:
            rec["u_tok"] = []
        for d in range(D):
            seq = MD.fp32_draws(gen, R * O * T) if attack else []
            pb = MD.Playback([], seq, 1)
            item = MD.getitem(DL, DU, ds, "vd_eval_val", d, pb)
            assert not item["gt_option_inds"].any() and tuple(item["enc_input_ids"].shape) == (R, O, T)
            rel_out.append(item["gt_relevance"].numpy())
            k = 0
            for j in range(R):
                if not attack:                                         # the hundred copies of a round's context are one row
                    for key in ("enc_input_ids", "enc_segments", "enc_mlm_labels", "enc_att_mask", "enc_sep_indices"):
                        assert bool((item[key][j] == item[key][j, :1]).all()), key
                    assert not (item["enc_mlm_labels"][j] >= 0).any()
                    enc.append((d, j))
                    for short, key in ENC:
                        rec[short].append(item[key][j, 0].numpy())
                    rec["hist_len"].append(int(item["enc_hist_len"][j, 0]))
                for s in range(O):
                    flat = (d * R + j) * O + s
                    c = eval_option(int(gt[d, j]), s)
                    check_option(item["dec_input_ids"][j, s].numpy(), opts[d, j, c], (name, d, j, s))
                    if attack:
                        u, used = MD.draws_by_position(item["enc_sep_indices"][j, s].numpy(), item["enc_hist_len"][j, s], seq[k:], T)
                        k += used + min(len(MD._ids(opts[d, j, c])), UD - 2)     # the target's tokens draw too (and mask nothing)
                    if flat in (noisy if attack else pick):
                        dec.append((d, j, s))
                        for short, key in DEC:
                            rec[short].append(item[key][j, s].numpy())
                        rec["dec_option"].append(c)
                        if attack:
                            enc.append((d, j))
                            for short, key in ENC:
                                rec[short].append(item[key][j, s].numpy())
                            rec["hist_len"].append(int(item["enc_hist_len"][j, s]))
                            rec["u_tok"].append(u)
            assert not attack or pb.k == k + REGIONS, (pb.k, k)           # every draw is accounted for: tokens, then the regions
        extra = dict(gt_relevance=rel, round_id=np.asarray(round_ids, np.int64), out_gt_relevance=np.stack(rel_out)) if not attack else None
        put_rows(out, name, 0, params, enc, dec, rec, extra)


def record_test(DL, DU, gen, pools, images, out):
    cap, ques, ans, opts, gt = pools
    n_rounds = np.array([10, 4], np.int64)
    params = dict(num_options=O, max_seq_len=T, max_utt_len=UD, vd_version="1.0", model="enc_dec_a", mask_prob=0.15, attack=None)
    ds = dataset(DL, pools, params, images, None, n_rounds)
    rec = {k: [] for k, _ in ENC + DEC}
    rec.update(hist_len=[], dec_option=[])
    enc, dec = [], []
    pick = set(int(x) for x in gen.permutation(D * O)[:32])
    for d in range(D):
        item = MD.getitem(DL, DU, ds, "vd_eval_test", d, MD.Playback([], [], 1))
        j = int(n_rounds[d]) - 1
        assert tuple(item["enc_input_ids"].shape) == (1, O, T) and int(item["round_id"]) == j + 1
        for key in ("enc_input_ids", "enc_segments", "enc_mlm_labels", "enc_att_mask", "enc_sep_indices"):
            assert bool((item[key][0] == item[key][0, :1]).all()), key
        enc.append((d, j))
        for short, key in ENC:
            rec[short].append(item[key][0, 0].numpy())
        rec["hist_len"].append(int(item["enc_hist_len"][0, 0]))
        for s in range(O):
            check_option(item["dec_input_ids"][0, s].numpy(), opts[d, j, s], ("test", d, s))
            if d * O + s in pick:
                dec.append((d, j, s))
                for short, key in DEC:
                    rec[short].append(item[key][0, s].numpy())
                rec["dec_option"].append(s)
    opts1 = np.stack([opts[d, n_rounds[d] - 1][None] for d in range(D)])
    put_rows(out, "test", 1, params, enc, dec, rec, dict(opts=opts1, n_rounds=n_rounds))


def record_train(DL, DU, gen, pools, images, out):
    for name, model, mode in (("train_a", "enc_dec_a", 2), ("train_q", "enc_dec_q", 3)):
        params = dict(num_options=O, max_seq_len=T, max_utt_len=UD, vd_version="1.0", model=model, mask_prob=0.15, attack=None)
        ds = dataset(DL, pools, params, images, None)
        rec = {k: [] for k, _ in ENC + DEC}
        rec.update(hist_len=[], dec_labels=[])
        enc, dec = [], []
        for d in range(D):
            item = MD.getitem(DL, DU, ds, "vd_train", d, MD.Playback([], [], 1))
            assert tuple(item["enc_input_ids"].shape) == (R, 1, T) and bool((item["enc_next_sentence_labels"] == -1).all())
            for j in range(R):
                enc.append((d, j))
                dec.append((d, j, 0))
                for short, key in ENC + DEC + (("dec_labels", "dec_labels"),):
                    rec[short].append(item[key][j, 0].numpy())
                rec["hist_len"].append(int(item["enc_hist_len"][j, 0]))
        put_rows(out, name, mode, params, enc, dec, rec)


def main():
    DL, DU = reference_loader()
    gen = np.random.default_rng(8642)
    pools = MD.make_pools(gen, D, R, O, U, LC, (38, 9), 17, 18)
    pools[1][0] = gen.integers(MD.V0, MD.V1, (R, U))                   # dialog 0: full-width questions (no 0 in the row); late rounds pass T
    pools[2][1, 3] = 0                                                 # an empty answer in the history (and its option)
    pools[3][1, 3, pools[4][1, 3]] = 0
    images = MD.make_images(gen, D, [REGIONS] * D)
    out = {"pools::" + k: v for k, v in zip(("cap", "ques", "ans", "opts", "gt"), pools)}
    record_eval(DL, DU, gen, pools, images, out)
    record_test(DL, DU, gen, pools, images, out)
    record_train(DL, DU, gen, pools, images, out)
    files = write_npz(os.path.join(GOLDEN, "gen_rows.npz"), out)
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
