"""Fixture of the self-training rows: tests/golden/selftrain_rows.npz, modelled on tools/make_golden_fgsm.py.

Runs in the build container only.  It imports the reference tree (the path of oracle.ref_harness) and copies none of its text: for
every context and every target of every case it CALLS the reference's utils.data_utils.encode_input and records what comes back.
The [MASK] noise of that function reads `random.random()` once per utterance token; for the duration of a call the name `random`
inside the reference module is bound to a stand-in that plays back a recorded sequence of fp32-representable draws (the k-th draw
belongs to the k-th utterance token), and is restored afterwards.  The fixture stores the draws by row position (u_tok[b, j, p]:
the draw of the utterance token at position p < T), which is how the device rule consumes them.

The loader class around encode_input (dataloader/dataloader_cc12m_gen.py:104-248) cannot be constructed here -- the tokenizer and
the LMDB reader are not installed -- so its remaining lines are restated below in this file's own words: the caption cut at 38
tokens, the answer cut at max_utt_len - 2, the label shift, the select_data zeroing and [SEP] -> [PAD].

    python tools/make_golden_selftrain.py

Cases (keys `<case>::<name>`; inputs cap, ques, ans, ppl, valid, u_tok and the scalars T, Ud, select_data, threshold, mask_prob;
outputs out_<name> for the nine arrays of gstvd_dialog_rows):
  cut     T = 32, R = 3, three dialogs whose last context is 32, 33 and 39 tokens long: it fits exactly, loses its final [SEP],
          is cut inside the question; perplexities AT the threshold (zeroed), one fp32 below (kept) and +inf; mask_prob 0
  noise   T = 32, R = 3, mask_prob 0.15, Ud = 6 (answers cut to 4 tokens): an empty question, special ids 100 / 101 / 103 inside
          utterances, an 18-token answer without [SEP], a 38-token caption, draws 0.14 / 0.15 side by side
  r12     R = 12 (24 separators, most of them past the cut at T = 32), U = 6, one invalid dialog (its labels are zeroed)
  full    T = 256, R = 10, U = 18, Ud = 25, mask_prob 0.15: the production shape
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                   # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, GOLDEN                # noqa: E402

CLS, SEP, MASK, PAD = 101, 102, 103, 0
SPECIAL = (0, 100, 101, 102, 103)
V0, V1 = 104, 320
MAX_CAP, S = 38, 25
OUT = ("enc_ids", "enc_seg", "enc_mlm", "enc_att", "enc_sep", "enc_hist_len", "dec_ids", "dec_labels", "dec_att")


def reference_data_utils():
    if RH.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, RH.REFERENCE_ROOT)
    try:
        import tqdm  # noqa: F401
    except ImportError:                                                # the module imports it at the top and never needs it here
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda x, **k: x)
    import utils.data_utils as DU
    return DU


class Playback(object):
    """Stands in for the `random` module inside utils.data_utils for one call: .random() plays the recorded draws back."""

    def __init__(self, draws):
        self.draws, self.k = [float(d) for d in draws], 0

    def random(self):
        self.k += 1
        return self.draws[self.k - 1]


def encode(DU, utts, max_len, mask_prob, draws):
    real = DU.random
    pb = Playback(draws)
    DU.random = pb
    try:
        out = DU.encode_input(utts, 1, CLS, SEP, MASK, PAD, max_seq_len=max_len, max_sep_len=S, mask_prob=mask_prob)
    finally:
        DU.random = real
    assert pb.k == len(pb.draws) == sum(len(u) for u in utts)
    return out


def text(row):
    """What tokenizer.decode(skip_special_tokens=True) keeps of a row of sampled ids (generate.py:20-23)."""
    return [int(v) for v in row if int(v) not in SPECIAL]


def reference_rows(DU, c):
    """The loader's rows of case c: encode_input from the reference, the lines around it restated."""
    B, R, U = c["ques"].shape
    T, Ud = c["T"], c["Ud"]
    o = {k: [] for k in OUT}
    for b in range(B):
        cap = [int(v) for v in c["cap"][b]]
        cap = (cap[:cap.index(0)] if 0 in cap else cap)[:MAX_CAP]
        qs, as_ = [text(r) for r in c["ques"][b]], [text(r) for r in c["ans"][b]]
        for j in range(R):
            ctx = [cap]
            for k in range(j):
                ctx += [qs[k], as_[k]]
            ctx.append(qs[j])
            draws, p = [], 1                                           # the k-th utterance token sits at position p (0 is [CLS])
            for utt in ctx:
                for _ in utt:
                    draws.append(float(c["u_tok"][b, j, p]) if (c["u_tok"] is not None and p < T) else 1.0)
                    p += 1
                p += 1
            ids, seg, sep, mlm, att = encode(DU, ctx, T, c["mask_prob"], draws)
            target = as_[j][:Ud - 2]
            dec, _, _, _, datt = encode(DU, [target], Ud, 0, [1.0] * len(target))
            labels = dec.new_zeros(dec.shape)
            invalid = c["valid"] is not None and int(c["valid"][b]) == 0
            if not (c["select_data"] and float(c["ppl"][b, j]) >= c["threshold"]) and not invalid:
                labels[:, :-1] = dec[:, 1:].clone()
            dec = dec.masked_fill(dec == SEP, PAD)
            for k, v in zip(OUT, (ids, seg, mlm, att, sep, None, dec, labels, datt)):
                o[k].append(np.array([len(ctx) - 1], np.int64) if v is None else v.numpy()[0])
    shape = lambda k, v: np.stack(v).reshape((B, R) + v[0].shape if k != "enc_hist_len" else (B, R))
    return {k: shape(k, v) for k, v in o.items()}


def utt_row(gen, U, n, sep=True, specials=()):
    row = np.zeros(U, np.int64)
    row[:n] = gen.integers(V0, V1, n)
    for pos, tok in specials:
        row[pos] = tok
    if sep and n < U:
        row[n] = SEP
    return row


def dialog(gen, U, Lc, cap_len, q_lens, a_lens, q_special=None, a_special=None):
    cap = np.zeros(Lc, np.int64)
    cap[:cap_len] = gen.integers(V0, V1, cap_len)
    q = np.stack([utt_row(gen, U, n, specials=(q_special or {}).get(k, ())) for k, n in enumerate(q_lens)])
    a = np.stack([utt_row(gen, U, n, specials=(a_special or {}).get(k, ())) for k, n in enumerate(a_lens)])
    return cap, q, a


def stack(dialogs):
    return tuple(np.stack(x) for x in zip(*dialogs))


def make_cases():
    gen = np.random.default_rng(1234)
    thr = np.float32(50.0)
    below = np.nextafter(thr, np.float32(0))
    f32 = lambda x: np.asarray(x, np.float32)
    cases = {}
    # cut: 1 + (8 + 1) + (4 + 1) + (3 + 1) + (5 + 1) + (2 + 1) = 28 tokens in front of q2; q2 of 3 / 4 / 10 tokens
    cap, q, a = stack([dialog(gen, 18, 8, 8, [4, 5, n], [3, 2, 6]) for n in (3, 4, 10)])
    cases["cut"] = dict(cap=cap, ques=q, ans=a, ppl=f32([[thr, below, np.inf], [below, thr, 3.0], [np.inf, 49.0, thr]]), valid=None,
                        u_tok=None, T=32, Ud=25, select_data=1, threshold=float(thr), mask_prob=0.0)
    # noise
    d0 = dialog(gen, 18, 38, 38, [5, 0, 4], [18, 3, 7], q_special={0: [(2, 103)]}, a_special={0: [(4, 100), (9, 101)]})
    d1 = dialog(gen, 18, 38, 5, [0, 6, 17], [2, 18, 1], a_special={1: [(0, 103)]})
    d2 = dialog(gen, 18, 38, 12, [3, 3, 3], [5, 9, 18])
    cap, q, a = stack([d0, d1, d2])
    u = gen.random((3, 3, 32)).astype(np.float32)
    u[:, :, 1::6], u[:, :, 2::6] = np.float32(0.14), np.float32(0.15)
    u[:, :, 4::6] = np.nextafter(np.float32(0.15), np.float32(0))
    cases["noise"] = dict(cap=cap, ques=q, ans=a, ppl=f32([[10, 60, thr], [below, 51, 2], [np.inf, 1.5, 49.99]]), valid=None, u_tok=u,
                          T=32, Ud=6, select_data=1, threshold=float(thr), mask_prob=0.15)
    # r12
    ds = [dialog(gen, 6, 8, c, [int(x) for x in gen.integers(0, 6, 12)], [int(x) for x in gen.integers(0, 7, 12)]) for c in (8, 3, 0)]
    cap, q, a = stack(ds)
    cases["r12"] = dict(cap=cap, ques=q, ans=a, ppl=f32(gen.choice([3.0, float(thr), float(below), 80.0], (3, 12))),
                        valid=np.array([1, 0, 1], np.int32), u_tok=gen.random((3, 12, 32)).astype(np.float32), T=32, Ud=25, select_data=1,
                        threshold=float(thr), mask_prob=0.15)
    # full
    ds = [dialog(gen, 18, 38, c, [int(x) for x in gen.integers(3, 18, 10)], [int(x) for x in gen.integers(1, 19, 10)]) for c in (38, 11)]
    cap, q, a = stack(ds)
    cases["full"] = dict(cap=cap, ques=q, ans=a, ppl=f32(gen.uniform(1.0, 100.0, (2, 10))), valid=None,
                         u_tok=gen.random((2, 10, 256)).astype(np.float32), T=256, Ud=25, select_data=1, threshold=float(thr), mask_prob=0.15)
    return cases


def check_against_reference(DU):
    """What the device rule relies on, asserted on the reference function itself."""
    ids, seg, sep, mlm, att = encode(DU, [[200, 201], [], [202]], 6, 0.15, [np.float32(0.14), np.float32(0.15), 0.9])
    assert ids[0].tolist() == [CLS, MASK, 201, SEP, SEP, 202], ids          # 0.14 masks, 0.15 does not; the empty utterance: a lone [SEP]
    assert mlm[0].tolist() == [-1, 200, -1, -1, -1, -1] and seg[0].tolist() == [1, 1, 1, 1, 0, 1]
    assert sep[0].tolist()[:4] == [3, 4, 6, 0] and att[0].tolist() == [1.0] * 6   # the last [SEP], at position 6, is cut; its position stays listed


def main():
    DU = reference_data_utils()
    check_against_reference(DU)
    out = {}
    for name, c in make_cases().items():
        rows = reference_rows(DU, c)
        for k, v in c.items():
            if v is not None:
                out["%s::%s" % (name, k)] = np.asarray(v)
        for k, v in rows.items():
            out["%s::out_%s" % (name, k)] = v
        n_sep = int((rows["enc_sep"] != 0).sum(-1).max())
        print("%-6s rows %s  masked %d  zeroed label rows %d  separators <= %d (past T: %d)"
              % (name, rows["enc_ids"].shape, int((rows["enc_mlm"] >= 0).sum()), int((rows["dec_labels"].sum(-1) == 0).sum()), n_sep,
                 int((rows["enc_sep"] >= c["T"]).sum())))
    # the coverage the fixture promises
    cut = out["cut::out_enc_ids"]
    assert cut[0, 2, 31] == SEP and cut[1, 2, 31] != SEP and (cut[1, 2] != 0).all() and out["cut::out_enc_sep"][1, 2, 5] == 32
    assert (cut[2, 2] != 0).all() and cut[2, 2, 31] != SEP
    assert (out["r12::out_enc_sep"][:, 11] != 0).sum(-1).max() == 24
    files = write_npz(os.path.join(GOLDEN, "selftrain_rows.npz"), out)
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
