"""gstvd_disc_rows (csrc/disc_rows.hip) on the case table of tests/exact_disc_rows.py and on the fixture recorded from the
reference's loader: torch.equal to the rule (label floats bit for bit), strided pools, every element written once (no poison
left), canaries intact, the same bits from a second launch, and the same result from the replay of a captured graph after the
inputs' contents changed."""
import os

import numpy as np
import pytest
import torch

import exact_disc_rows as X
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Hip(object):
    device = DEV

    def rows(self, *a, **k):
        from gst_visdial_amd import ops
        return ops.disc_rows(*a, **k)


CASES = X.cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_disc_rows_case_table(c):
    X.run_case(Hip(), c)


def test_disc_rows_reproduces_the_reference_fixture():
    from gst_visdial_amd.selfcheck import read_npz
    cases = X.fixture_cases(read_npz(os.path.join(GOLDEN, "disc_rows.npz")))
    assert len(cases) == 6
    for c, want, _ in cases:
        X.run_case(Hip(), c, want)


def test_disc_rows_default_outputs_and_argument_status():
    """Without `out` the op allocates its outputs (torch.empty: nothing is zeroed in front); the library itself refuses bad
    arguments with a status, not a launch, and writes nothing."""
    import ctypes as C
    from gst_visdial_amd import ops, _lib
    c = next(c for c in CASES if c.name == "train_tr2_no4_dense")
    t = lambda x, d: None if x is None else torch.as_tensor(np.asarray(x)).to(d).to(DEV)
    args = [t(c.cap, torch.int64), t(c.ques, torch.int64), t(c.ans, torch.int64), t(c.opts, torch.int64), t(c.gt, torch.int64),
            t(c.rows[0], torch.int32), t(c.rows[1], torch.int32), t(c.rows[2], torch.int32)]
    got = ops.disc_rows(*args, c.T, c.tot_rounds, c.num_options, True, u_neg=t(c.u_neg, torch.float32), dense_scores=t(c.dense, torch.float64))
    want = X.rule_of(c)
    for k in X.ROWS_OUT:
        assert torch.equal(got[k].cpu(), torch.as_tensor(want[k])), k
    lib = _lib.load()
    assert lib.gstvd_disc_rows(C.byref(_lib.DiscRowsDesc()), None) == -4                     # GSTVD_E_NULL
    # over-limit shapes through the raw entry: GSTVD_E_SHAPE, and the poisoned outputs stay poisoned
    N = c.rows.shape[1]
    out = {k: torch.full((N, w), X.POISON, dtype=dt, device=DEV) for k, dt, w in
           (("tokens", torch.int64, c.T), ("segments", torch.int64, c.T), ("mask", torch.int64, c.T), ("att", torch.float32, c.T),
            ("sep_indices", torch.int64, 25))}
    hist = torch.full((N,), X.POISON, dtype=torch.int64, device=DEV)
    p = lambda x: x.data_ptr()
    def desc():
        d = _lib.DiscRowsDesc()
        d.cap, d.ld_cap, d.ques, d.ans, d.ld_utt, d.opts, d.ld_opt, d.gt_index = p(args[0]), 8, p(args[1]), p(args[2]), 18, p(args[3]), 18, p(args[4])
        d.row_dialog, d.row_round, d.row_slot = p(args[5]), p(args[6]), p(args[7])
        d.tokens, d.segments, d.mask, d.att, d.ld_row = p(out["tokens"]), p(out["segments"]), p(out["mask"]), p(out["att"]), c.T
        d.sep_indices, d.ld_sep, d.hist_len = p(out["sep_indices"]), 25, p(hist)
        d.cls, d.sep, d.mask_id, d.N = X.CLS, X.SEP, X.MASK, N
        d.D, d.R, d.O, d.U, d.Lc, d.T, d.S, d.tot_rounds, d.num_options, d.train = 3, 3, 5, 18, 8, c.T, 25, 11, 5, 0
        return d

    for field, value in (("U", 65), ("Lc", 65), ("R", 13), ("O", 101), ("num_options", 6), ("num_options", 1), ("tot_rounds", 0), ("T", 1),
                         ("S", 65), ("ld_row", c.T - 1), ("N", -1)):
        d = desc()
        setattr(d, field, value)
        assert lib.gstvd_disc_rows(C.byref(d), None) == -2, field                            # GSTVD_E_SHAPE
    d = desc()
    d.train = 1                                                                              # train mode without u_neg / nsp_labels
    assert lib.gstvd_disc_rows(C.byref(d), None) == -4
    d = desc()
    d.mask_prob = 0.15                                                                       # noise without uniforms
    assert lib.gstvd_disc_rows(C.byref(d), None) == -4
    torch.cuda.synchronize()
    assert all(bool((v == X.POISON).all()) for v in list(out.values()) + [hist])            # a refused call writes nothing
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.gstvd_disc_rows(C.byref(desc()), stream) == 0                                 # the same descriptor, unchanged: accepted
    torch.cuda.synchronize()
    ev = X.rows_rule(c.cap, c.ques, c.ans, c.opts, c.gt, c.rows[0], c.rows[1], c.rows[2], c.T, 11, 5, False)
    assert torch.equal(out["tokens"].cpu(), torch.as_tensor(ev["tokens"])) and torch.equal(hist.cpu(), torch.as_tensor(ev["hist_len"]))


def test_disc_rows_replays_from_a_captured_graph_after_the_inputs_changed():
    from gst_visdial_amd import ops
    from gst_visdial_amd.graph import capture
    t = lambda x, d: torch.as_tensor(np.asarray(x)).to(d).to(DEV)
    c0 = next(c for c in CASES if c.name == "train_tr2_no2_p15_dense")
    gen = np.random.default_rng(5)
    c1 = c0._replace(cap=np.roll(c0.cap, 1, 0), ques=np.roll(c0.ques, 1, 0), gt=c0.gt[::-1].copy(), ans=np.roll(c0.ans, 1, 1),
                     u_tok=X._noise(c0.rows.shape[1], c0.T, gen), u_neg=gen.random(c0.rows.shape[1]).astype(np.float32),
                     rows=c0.rows[:, ::-1].copy())
    names = (("cap", torch.int64), ("ques", torch.int64), ("ans", torch.int64), ("opts", torch.int64), ("gt", torch.int64),
             ("u_tok", torch.float32), ("u_neg", torch.float32), ("dense", torch.float64))
    ins = {k: t(getattr(c0, k), d) for k, d in names}
    rows = t(c0.rows, torch.int32)
    N = c0.rows.shape[1]
    w = X.rows_windows(N, c0.T, DEV)
    out = dict(tokens=w["tokens"].view, segments=w["segments"].view, mask=w["mask"].view, att=w["att"].view,
               sep_indices=w["sep_indices"].view, hist_len=w["hist_len"].vector(), nsp_labels=w["nsp_labels"].vector().view(N, 2),
               neg_option=torch.empty(N, dtype=torch.int32, device=DEV))
    call = lambda: ops.disc_rows(ins["cap"], ins["ques"], ins["ans"], ins["opts"], ins["gt"], rows[0], rows[1], rows[2], c0.T, c0.tot_rounds,
                                 c0.num_options, True, mask_prob=c0.mask_prob, u_tok=ins["u_tok"], u_neg=ins["u_neg"],
                                 dense_scores=ins["dense"], out=out)
    call()                                                                                   # eager once: library loaded, nothing lazy left
    g = torch.cuda.CUDAGraph()
    with capture(g):
        call()
    for c in (c1, c0):
        for k, d in names:
            ins[k].copy_(t(getattr(c, k), d))
        rows.copy_(t(c.rows, torch.int32))
        for v in out.values():
            v.fill_(X.POISON)
        g.replay()
        want = X.rule_of(c)
        for k in X.ROWS_OUT:
            v = out[k].cpu()
            assert torch.equal(v, torch.as_tensor(want[k]).reshape(v.shape).to(v.dtype)), (c.name, k)
        for k, win in w.items():
            win.assert_surroundings_untouched("%s %s (replay)" % (c.name, k))
