"""gstvd_gen_rows (csrc/gen_rows.hip) on the case table of tests/exact_gen_rows.py and on the fixture recorded from the reference's
loader: torch.equal to the rule (the 0 / 1 floats bit for bit), strided pools, every element written once (no poison left), canaries
intact, the same bits from a second launch; the teacher rows against gstvd_dialog_rows on the same pools; and every refusal of the
library itself."""
import os

import numpy as np
import pytest
import torch

import exact_gen_rows as X
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Hip(object):
    device = DEV

    def rows(self, *a, **k):
        from gst_visdial_amd import ops
        return ops.gen_rows(*a, **k)


CASES = X.cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_gen_rows_case_table(c):
    X.run_case(Hip(), c)


def test_gen_rows_reproduces_the_reference_fixture():
    from gst_visdial_amd.selfcheck import read_npz
    cases = X.fixture_cases(read_npz(os.path.join(GOLDEN, "gen_rows.npz")))
    assert sorted(c.name for c, _ in cases) == sorted(X.FIXTURE_CASES)
    for c, want in cases:
        X.run_case(Hip(), c, dict(X.rule_of(c), **want))           # the recorded arrays, plus dec_option where the loader has none


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", ["train_a", "train_a_U64_Ud25", "train_q_full"])
def test_teacher_rows_equal_dialog_rows_on_the_same_pools(name):
    """TRAIN_A is the student's row rule without the perplexity cut and the noise: gstvd_dialog_rows (select_data off, mask_prob 0)
    writes the same rows from the same pools, compared as bit patterns."""
    from gst_visdial_amd import ops
    c = next(c for c in CASES if c.name == name)
    t = lambda x: torch.as_tensor(np.asarray(x)).to(DEV)
    cap, ques, ans = t(c.cap), t(c.ques), t(c.ans)
    D, R = c.ques.shape[:2]
    rounds = torch.arange(D * R, device=DEV)
    d, j = (rounds // R).to(torch.int32), (rounds % R).to(torch.int32)
    got = ops.gen_rows(cap, ques, ans, None, None, "train_a", c.T, c.Ud, (d, j), (d, j, torch.zeros_like(d)))
    ref = ops.dialog_rows(cap, ques, ans, torch.zeros(D, R, device=DEV), c.T, c.Ud, False, 0.0, 0.0)
    for k, r in (("tokens", "enc_ids"), ("segments", "enc_seg"), ("mlm", "enc_mlm"), ("att", "enc_att"), ("sep_indices", "enc_sep"),
                 ("hist_len", "enc_hist_len"), ("dec_ids", "dec_ids"), ("dec_labels", "dec_labels"), ("dec_att", "dec_att")):
        a, b = got[k], ref[r].reshape(got[k].shape)
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), k
    assert bool((got["dec_option"] == -1).all()) and bool((got["dec_labels"] != 0).any())


def test_gen_rows_default_outputs_and_argument_status():
    """Without `out` the op allocates its outputs (torch.empty: nothing is zeroed in front); the library itself refuses bad
    arguments with a status, not a launch, and writes nothing."""
    import ctypes as C
    from gst_visdial_amd import ops, _lib
    c = next(c for c in CASES if c.name == "eval_no4")
    t = lambda x, d: None if x is None else torch.as_tensor(np.asarray(x)).to(d).to(DEV)
    pools = [t(c.cap, torch.int64), t(c.ques, torch.int64), t(c.ans, torch.int64), t(c.opts, torch.int64), t(c.gt, torch.int64)]
    enc, dec = t(c.enc, torch.int32), t(c.dec, torch.int32)
    got = ops.gen_rows(*pools, "eval", c.T, c.Ud, (enc[0], enc[1]), (dec[0], dec[1], dec[2]), num_options=4)
    want = X.rule_of(c)
    assert set(got) == set(X.out_names(c))
    for k in X.out_names(c):
        assert torch.equal(got[k].cpu(), torch.as_tensor(want[k])), k
    lib = _lib.load()
    assert lib.gstvd_gen_rows(C.byref(_lib.GenRowsDesc()), None) == -4                      # GSTVD_E_NULL
    n_enc, n_dec = c.enc.shape[1], c.dec.shape[1]
    out = {k: torch.full((n, w), X.POISON, dtype=dt, device=DEV) for k, dt, n, w in
           (("tokens", torch.int64, n_enc, c.T), ("segments", torch.int64, n_enc, c.T), ("mlm", torch.int64, n_enc, c.T),
            ("att", torch.float32, n_enc, c.T), ("sep_indices", torch.int64, n_enc, 25), ("dec_ids", torch.int64, n_dec, c.Ud),
            ("dec_att", torch.float32, n_dec, c.Ud), ("dec_labels", torch.int64, n_dec, c.Ud))}
    out["hist_len"] = torch.full((n_enc,), X.POISON, dtype=torch.int64, device=DEV)
    out["dec_option"] = torch.full((n_dec,), X.POISON, dtype=torch.int32, device=DEV)
    p = lambda x: x.data_ptr()

    def desc(mode=_lib.GEN_EVAL):
        d = _lib.GenRowsDesc()
        d.cap, d.ld_cap, d.ques, d.ans, d.ld_utt, d.opts, d.ld_opt, d.gt_index = p(pools[0]), 8, p(pools[1]), p(pools[2]), 8, p(pools[3]), 8, p(pools[4])
        d.enc_dialog, d.enc_round = p(enc[0]), p(enc[1])
        d.tokens, d.segments, d.mlm, d.att, d.ld_row = p(out["tokens"]), p(out["segments"]), p(out["mlm"]), p(out["att"]), c.T
        d.sep_indices, d.ld_sep, d.hist_len = p(out["sep_indices"]), 25, p(out["hist_len"])
        d.dec_dialog, d.dec_round, d.dec_slot = p(dec[0]), p(dec[1]), p(dec[2])
        d.dec_ids, d.dec_att, d.ld_dec, d.dec_option = p(out["dec_ids"]), p(out["dec_att"]), c.Ud, p(out["dec_option"])
        d.cls, d.sep, d.mask_id, d.n_enc, d.n_dec = X.CLS, X.SEP, X.MASK, n_enc, n_dec
        d.D, d.R, d.Ro, d.O, d.U, d.Lc, d.T, d.S, d.Ud, d.num_options, d.mode = 3, 4, 4, 6, 8, 8, c.T, 25, c.Ud, 4, mode
        return d

    E_SHAPE, E_NULL = -2, -4
    refused = []
    for field in ("cap", "ques", "ans", "opts", "gt_index", "enc_dialog", "enc_round", "tokens", "segments", "mlm", "att", "sep_indices",
                  "hist_len", "dec_dialog", "dec_round", "dec_slot", "dec_ids", "dec_att", "dec_option"):
        refused.append((field, None, _lib.GEN_EVAL, E_NULL))
    refused.append(("dec_labels", None, _lib.GEN_TRAIN_A, E_NULL))                          # (it is NULL in desc(): the train modes need it)
    refused.append(("dec_labels", None, _lib.GEN_TRAIN_Q, E_NULL))
    refused.append(("mask_prob", 0.15, _lib.GEN_EVAL, E_NULL))                              # noise without uniforms
    for field, value in (("U", 65), ("U", 0), ("Lc", 65), ("Lc", 0), ("R", 13), ("R", 0), ("S", 65), ("S", 7), ("O", 101), ("O", 1),
                         ("num_options", 7), ("num_options", 1), ("Ro", 2), ("T", 1), ("Ud", 2), ("D", 0), ("mode", 4), ("mode", -1),
                         ("n_enc", -1), ("n_dec", -1), ("n_enc", 2 ** 31), ("ld_cap", 7), ("ld_utt", 7), ("ld_opt", 7),
                         ("ld_row", c.T - 1), ("ld_sep", 24), ("ld_dec", c.Ud - 1)):
        refused.append((field, value, _lib.GEN_EVAL, E_SHAPE))
    for field, value, mode, status in refused:
        d = desc(mode)
        setattr(d, field, value)
        assert lib.gstvd_gen_rows(C.byref(d), None) == status, (field, value, mode)
    d = desc()                                                                               # a null pointer is reported in front of a bad shape
    d.opts, d.U = None, 65
    assert lib.gstvd_gen_rows(C.byref(d), None) == E_NULL
    d = desc()                                                                               # ... and a bad shape in front of a short stride
    d.u_tok, d.ld_u, d.mask_prob = p(out["att"]), c.T - 1, 0.15
    assert lib.gstvd_gen_rows(C.byref(d), None) == E_SHAPE
    torch.cuda.synchronize()
    assert all(bool((v == X.POISON).all()) for v in out.values())                           # a refused call writes nothing
    # what the modes do not read may be NULL; an empty list may have NULL pointers
    stream = torch.cuda.current_stream().cuda_stream
    d = desc(_lib.GEN_TEST)
    d.gt_index, d.n_enc, d.enc_dialog, d.tokens, d.hist_len = None, 0, None, None, None
    assert lib.gstvd_gen_rows(C.byref(d), stream) == 0
    torch.cuda.synchronize()
    tw = X.rows_rule(c.cap, c.ques, c.ans, c.opts, None, "test", None, c.dec, c.T, c.Ud, 4)
    assert torch.equal(out["dec_ids"].cpu(), torch.as_tensor(tw["dec_ids"])) and bool((out["tokens"] == X.POISON).all())
    assert bool((out["dec_labels"] == X.POISON).all())
    d = desc(_lib.GEN_TRAIN_Q)
    d.opts, d.gt_index, d.O, d.num_options, d.Ro, d.n_dec, d.dec_ids, d.dec_slot = None, None, 0, 0, 0, 0, None, None
    assert lib.gstvd_gen_rows(C.byref(d), stream) == 0
    torch.cuda.synchronize()
    qw = X.rows_rule(c.cap, c.ques, c.ans, None, None, "train_q", c.enc, None, c.T, c.Ud)
    assert torch.equal(out["tokens"].cpu(), torch.as_tensor(qw["tokens"])) and torch.equal(out["hist_len"].cpu(), torch.as_tensor(qw["hist_len"]))
    d = desc()
    d.n_enc = d.n_dec = 0                                                                    # nothing to do: accepted, nothing launched
    assert lib.gstvd_gen_rows(C.byref(d), stream) == 0
    assert lib.gstvd_gen_rows(C.byref(desc()), stream) == 0                                  # the same descriptor, unchanged: accepted
    torch.cuda.synchronize()
    for k in X.out_names(c):
        assert torch.equal(out[k].cpu(), torch.as_tensor(want[k])), k
