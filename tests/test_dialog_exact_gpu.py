"""gstvd_context_append and gstvd_dialog_rows (csrc/dialog.hip) on the case tables of tests/exact_dialog.py and on the fixture
recorded from the reference: torch.equal to the rule, canaries intact, no poison left, the same bits from a second launch, and
the same result from the replay of a captured (linear) graph after the inputs' contents changed -- no host synchronisation."""
import os

import numpy as np
import pytest
import torch

import exact_dialog as X
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Hip(object):
    device = DEV

    def append(self, *a, **k):
        from gst_visdial_amd import ops
        return ops.context_append(*a, **k)

    def rows(self, *a, **k):
        from gst_visdial_amd import ops
        return ops.dialog_rows(*a, **k)


@pytest.mark.parametrize("U", [6, 18])
def test_context_append_edge_table(U):
    for c in X.append_edge_cases(T=32, U=U):
        got = X.run_append_case(Hip(), c)
        full = torch.as_tensor(c.ctx_len) >= 32
        assert bool(full.any())
        assert torch.equal(got["ctx_ids"][full], torch.as_tensor(c.ctx_ids)[full])          # the full row is untouched ...
        assert bool((got["full"][full] == 1).all()) and bool((got["abnormal"][full] == 1).all())   # ... and its flags are set
        assert not bool(got["full"][~full].any())


def test_context_append_random_cases_with_full_rows():
    for c in X.append_random_cases(48, T=32, U=18, allow_full=True) + X.append_random_cases(16, T=32, U=6, seed=5) \
            + X.append_random_cases(8, T=200, U=70, seed=9):                                  # U > 64: more than one ballot
        X.run_append_case(Hip(), c)


CASES = X.rows_cases(B=3, T=32)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_dialog_rows_case_table(c):
    X.run_rows_case(Hip(), c)


def test_dialog_rows_reproduces_the_reference_fixture():
    from gst_visdial_amd.selfcheck import read_npz
    cases = X.fixture_cases(read_npz(os.path.join(GOLDEN, "selftrain_rows.npz")))
    assert len(cases) == 4
    for c, want in cases:
        X.run_rows_case(Hip(), c, want)


def test_dialog_rows_default_outputs_and_argument_status():
    """Without `out` the op allocates [B, R, .] tensors (torch.empty: nothing is zeroed in front); the library itself refuses bad
    arguments with a status, not a launch."""
    import ctypes as C
    from gst_visdial_amd import ops, _lib
    c = CASES[4]
    t = lambda x, d: None if x is None else torch.as_tensor(x).to(d).to(DEV)
    got = ops.dialog_rows(t(c.cap, torch.int64), t(c.ques, torch.int64), t(c.ans, torch.int64), t(c.ppl, torch.float32), c.T, c.Ud,
                          c.select_data, c.threshold, c.mask_prob, valid=t(c.valid, torch.int32), u_tok=t(c.u_tok, torch.float32))
    want = X.rows_rule(c.cap, c.ques, c.ans, c.ppl, c.T, c.Ud, c.select_data, c.threshold, c.mask_prob, c.valid, c.u_tok)
    for k in X.ROWS_OUT:
        assert torch.equal(got[k].cpu(), torch.as_tensor(want[k])), k
    lib = _lib.load()
    d = _lib.DialogRowsDesc()
    assert lib.gstvd_dialog_rows(C.byref(d), None) == -4                                     # GSTVD_E_NULL
    a = _lib.ContextAppendDesc()
    assert lib.gstvd_context_append(C.byref(a), None) == -4


def test_both_ops_replay_from_a_captured_graph_after_the_inputs_changed():
    from gst_visdial_amd import ops
    from gst_visdial_amd.graph import capture
    t = lambda x, d: torch.as_tensor(np.asarray(x)).to(d).to(DEV)
    # ---- context_append: capture on one case, replay on another of the same shape
    a0, a1 = X.append_random_cases(16, T=32, U=18, seed=3, allow_full=True)
    assert a1.segments is not None
    a0 = a0._replace(segments=a1.segments[::-1].copy())
    st = dict(ctx=t(a0.ctx_ids, torch.int64), ln=t(a0.ctx_len, torch.int64), new=t(a0.new_ids, torch.int64),
              seg=t(a0.segments, torch.int64), att=t(np.asarray(a0.ctx_ids) != 0, torch.float32),
              ab=torch.zeros(8, dtype=torch.int32, device=DEV), fu=torch.zeros(8, dtype=torch.int32, device=DEV),
              n=torch.zeros(8, dtype=torch.int64, device=DEV))
    call = lambda: ops.context_append(st["ctx"], st["ln"], st["new"], X.SEP, st["ab"], st["fu"], segments=st["seg"], segment_value=1,
                                      att_mask=st["att"], n_out=st["n"])
    call()                                                                                   # eager once: library loaded, nothing lazy left
    g = torch.cuda.CUDAGraph()
    with capture(g):
        call()
    for c in (a1, a0):
        st["ctx"].copy_(t(c.ctx_ids, torch.int64)), st["ln"].copy_(t(c.ctx_len, torch.int64)), st["new"].copy_(t(c.new_ids, torch.int64))
        st["seg"].copy_(t(c.segments, torch.int64)), st["att"].copy_(t(np.asarray(c.ctx_ids) != 0, torch.float32))
        st["ab"].zero_(), st["fu"].zero_(), st["n"].fill_(X.POISON)
        g.replay()
        want = X.append_rule(c.ctx_ids, c.ctx_len, c.new_ids, X.SEP, c.segments, 1, (np.asarray(c.ctx_ids) != 0).astype(np.float32))
        for k, v in (("ctx_ids", st["ctx"]), ("ctx_len", st["ln"]), ("segments", st["seg"]), ("att_mask", st["att"]), ("n_out", st["n"]),
                     ("abnormal", st["ab"]), ("full", st["fu"])):
            assert torch.equal(v.cpu(), torch.as_tensor(want[k]).to(v.dtype)), (c.name, k)
    # ---- dialog_rows: capture on CASES[k], replay on a case of the same shape with other contents
    c0 = next(c for c in CASES if c.name.startswith("U18_Lc38_R3"))
    gen = np.random.default_rng(99)
    c1 = c0._replace(cap=np.roll(c0.cap, 1, 0), ques=X._utt_rows((3, 3), gen, 18), ans=X._utt_rows((3, 3), gen, 18),
                     ppl=np.roll(c0.ppl, 1, 1), u_tok=gen.random((3, 3, 32)).astype(np.float32), valid=np.array([0, 1, 1], np.int32))
    assert c0.u_tok is not None and c0.valid is not None
    ins = dict(cap=t(c0.cap, torch.int64), ques=t(c0.ques, torch.int64), ans=t(c0.ans, torch.int64), ppl=t(c0.ppl, torch.float32),
               valid=t(c0.valid, torch.int32), u=t(c0.u_tok, torch.float32))
    w = X.rows_windows(3, 3, c0.T, c0.Ud, DEV)
    out = {k: (w[k].vector() if k == "enc_hist_len" else w[k].view) for k in X.ROWS_OUT}
    rows = lambda: ops.dialog_rows(ins["cap"], ins["ques"], ins["ans"], ins["ppl"], c0.T, c0.Ud, c0.select_data, c0.threshold, c0.mask_prob,
                                   valid=ins["valid"], u_tok=ins["u"], out=out)
    rows()
    g2 = torch.cuda.CUDAGraph()
    with capture(g2):
        rows()
    for c in (c1, c0):
        for k, src, d in (("cap", c.cap, torch.int64), ("ques", c.ques, torch.int64), ("ans", c.ans, torch.int64), ("ppl", c.ppl, torch.float32),
                          ("valid", c.valid, torch.int32), ("u", c.u_tok, torch.float32)):
            ins[k].copy_(t(src, d))
        for k in X.ROWS_OUT:
            out[k].fill_(X.POISON)
        g2.replay()
        want = X.rows_rule(c.cap, c.ques, c.ans, c.ppl, c.T, c.Ud, c.select_data, c.threshold, c.mask_prob, c.valid, c.u_tok)
        X.check_rows(c.name + " (replay)", w, want, 3, 3)
