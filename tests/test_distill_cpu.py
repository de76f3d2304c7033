"""Soft pseudo-labels, the part that needs no GPU: the three entry points in header, bindings and Makefile; the alignment of the
teacher's positions with the student's rows (selftrain.align_soft_labels) on hand-made tensors; the validation of the forward's
soft-label keywords; step.select_rows / forward_rows carrying the tensors to a stand-in model whose loss has a grad_fn."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gstvd_topk_logp", "gstvd_distill_fwd", "gstvd_distill_bwd")


# ------------------------------------------------------------------------------------------ the entry points
def test_entry_points_are_declared_bound_and_built_without_an_abi_bump():
    from gst_visdial_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gstvd_topk_logp"][1]) == 10 and len(_lib.SIGNATURES["gstvd_distill_fwd"][1]) == 18
    assert len(_lib.SIGNATURES["gstvd_distill_bwd"][1]) == 19
    assert _lib.ABI_VERSION == 9
    mk = open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "Makefile")).read()
    assert "distill.hip" in mk and "ce_row.h" in mk
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%d entry points" % len(_lib.SIGNATURES) in design and "### Soft pseudo-labels" in design
    for doc in ("INTEGRATION.md", "README.md"):
        assert "dec_soft_ids" in open(os.path.join(ROOT, doc)).read(), doc


def test_ops_refuse_bad_arguments_before_loading_anything_onto_a_gpu():
    from gst_visdial_amd import ops
    from gst_visdial_amd._lib import GstvdError
    ids, lp = torch.zeros(6, 4, dtype=torch.int64), torch.zeros(6, 4)
    assert ops._soft_pair("t", ids, lp, 6) == 4 and ops._soft_pair("t", ids.view(2, 3, 4), lp.view(2, 3, 4), 6) == 4
    for bad in ((ids.int(), lp), (ids, lp.double()), (ids[:, :3], lp), (ids.t(), lp.t()), (ids, lp[:5]),
                (torch.zeros(6, 17, dtype=torch.int64), torch.zeros(6, 17))):
        with pytest.raises(GstvdError):
            ops._soft_pair("t", bad[0], bad[1], 6)
    with pytest.raises(GstvdError):
        ops._soft_pair("t", ids, lp, 5)
    assert ops._distill_scalars("t", 0.5, 2.0) == (0.5, 0.5) and ops._distill_scalars("t", 0, 1) == (0.0, 1.0)
    for a, t in ((-0.1, 1.0), (1.1, 1.0), (float("nan"), 1.0), (0.5, 0.0), (0.5, -2.0), (0.5, float("inf")), (0.5, float("nan"))):
        with pytest.raises(GstvdError):
            ops._distill_scalars("t", a, t)


# ------------------------------------------------------------------------------------------ validation of the forward's keywords
def test_soft_label_keywords_are_validated_before_anything_is_launched():
    from gst_visdial_amd.engine import Engine
    from gst_visdial_amd._lib import GstvdError
    dec = torch.zeros(3, 9, dtype=torch.long)
    ids, lp = torch.zeros(3, 9, 4, dtype=torch.long), torch.zeros(3, 9, 4)
    check = lambda soft, red=True: Engine._soft_labels(None, soft, dec, red)           # noqa: E731
    assert check(None) is None and check((None, None, 0.5, 1.0)) is None
    got = check((ids, lp.double(), 1, 2))
    assert got["ids"].shape == got["logp"].shape == (27, 4) and got["logp"].dtype == torch.float32 and got["alpha"] == 1.0 and got["temperature"] == 2.0
    for soft, pat in (((ids, None, 0.5, 1.0), "both or neither"), ((None, lp, 0.5, 1.0), "both or neither"),
                      ((ids, lp, 1.5, 1.0), "alpha"), ((ids, lp, -0.5, 1.0), "alpha"), ((ids, lp, 0.5, 0.0), "temperature"),
                      ((ids, lp, 0.5, float("inf")), "temperature"), ((ids[:, :8], lp[:, :8], 0.5, 1.0), "B = 3, U = 9"),
                      ((ids, lp[..., :3], 0.5, 1.0), "B = 3, U = 9"), ((ids.view(27, 4), lp.view(27, 4), 0.5, 1.0), "B = 3, U = 9"),
                      ((torch.zeros(3, 9, 17, dtype=torch.long), torch.zeros(3, 9, 17), 0.5, 1.0), "K <= 16")):
        with pytest.raises(GstvdError, match=pat):
            check(soft)
    with pytest.raises(GstvdError, match="loss_reduction"):
        check((ids, lp, 0.5, 1.0), red=False)


# ------------------------------------------------------------------------------------------ alignment
def _teacher(B, R, Ut, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(104, 320, (B, R, Ut, K), generator=g), -torch.rand(B, R, Ut, K, generator=g)


def test_alignment_uses_a_row_only_when_every_labelled_position_agrees():
    from gst_visdial_amd.selftrain import align_soft_labels
    B, R, Ut, Ud, K = 2, 3, 4, 6, 2
    sid, slp = _teacher(B, R, Ut, K)
    lab = torch.zeros(B, R, Ud, dtype=torch.long)
    tgt = torch.zeros(B, R, Ut, dtype=torch.long)
    lab[0, 0, :3] = torch.tensor([150, 151, 102]); tgt[0, 0, :3] = torch.tensor([150, 151, 102])      # aligned
    lab[0, 1, :3] = torch.tensor([150, 151, 102]); tgt[0, 1, :3] = torch.tensor([150, 152, 102])      # one position differs
    lab[0, 2, :2] = torch.tensor([150, 102]); tgt[0, 2, :4] = torch.tensor([150, 102, 7, 9])          # teacher labels behind the row's end: ignored
    lab[1, 0, :5] = torch.tensor([1, 2, 3, 4, 102]); tgt[1, 0, :4] = torch.tensor([1, 2, 3, 4])        # a label at a position >= Ut
    tgt[1, 1, :2] = torch.tensor([5, 102])                                                             # a zeroed row: no kept token
    lab[1, 2, :4] = torch.tensor([1, 2, 3, 102]); tgt[1, 2, :4] = torch.tensor([1, 2, 3, 102])        # aligned, full teacher width
    ids, lp = align_soft_labels(sid, slp, tgt, lab)
    assert ids.shape == lp.shape == (B, R, Ud, K) and ids.dtype == torch.int64 and lp.dtype == torch.float32
    use = {(0, 0): True, (0, 1): False, (0, 2): True, (1, 0): False, (1, 1): True, (1, 2): True}
    for (b, r), u in use.items():
        if u:
            assert torch.equal(ids[b, r, :Ut], sid[b, r]) and torch.equal(lp[b, r, :Ut], slp[b, r]), (b, r)
        else:
            assert bool((ids[b, r] == -1).all()) and bool((lp[b, r] == 0).all()), (b, r)
        assert bool((ids[b, r, Ut:] == -1).all()) and bool((lp[b, r, Ut:] == 0).all()), (b, r)
    # a student row shorter than the teacher's: the positions behind it are cut
    ids2, lp2 = align_soft_labels(sid, slp, tgt, lab[..., :3])
    assert ids2.shape == (B, R, 3, K) and torch.equal(ids2[0, 0], sid[0, 0, :3]) and bool((ids2[0, 1] == -1).all())


def test_alignment_refuses_tensors_that_do_not_belong_together():
    from gst_visdial_amd.selftrain import align_soft_labels
    from gst_visdial_amd._lib import GstvdError
    sid, slp = _teacher(2, 3, 4, 2)
    tgt, lab = torch.zeros(2, 3, 4, dtype=torch.long), torch.zeros(2, 3, 6, dtype=torch.long)
    for args in ((sid, slp[..., :1], tgt, lab), (sid, slp, tgt[:, :2], lab), (sid, slp, tgt, lab[:1])):
        with pytest.raises(GstvdError):
            align_soft_labels(*args)


# ------------------------------------------------------------------------------------------ the step driver
class StandInModel(object):
    """Records the keywords of its call; the loss is a tensor with a grad_fn, like the engine's."""

    def __init__(self):
        self.w = torch.ones(1, requires_grad=True)
        self.calls = []

    def __call__(self, **kw):
        self.calls.append(kw)
        return (self.w * 2.0).sum(), kw["dec_input_ids"].float()


def _batch(B=2, R=3, T=5, Ud=4, K=2, soft=True):
    g = torch.Generator().manual_seed(1)
    b = dict(enc_input_ids=torch.randint(1, 9, (B, R, 1, T), generator=g), enc_segments=torch.zeros(B, R, 1, T, dtype=torch.long),
             enc_att_mask=torch.ones(B, R, 1, T), dec_input_ids=torch.randint(1, 9, (B, R, 1, Ud), generator=g),
             dec_att_mask=torch.ones(B, R, 1, Ud), dec_labels=torch.randint(1, 9, (B, R, 1, Ud), generator=g),
             enc_image_feat=torch.rand(B, 3, 4, generator=g), enc_image_loc=torch.rand(B, 3, 5, generator=g), enc_image_mask=torch.ones(B, 3))
    if soft:
        b["dec_soft_ids"] = torch.randint(0, 9, (B, R, 1, Ud, K), generator=g)
        b["dec_soft_logp"] = -torch.rand(B, R, 1, Ud, K, generator=g)
    return b


def test_select_rows_carries_the_soft_labels_like_any_decoder_tensor():
    from gst_visdial_amd import step
    b = _batch()
    idx = torch.tensor([4, 0, 4])
    rows, _ = step.select_rows(b, dict(mode="vd_train", batch_size=3), sample_indices=idx)
    assert rows["dec_soft_ids"].shape == (3, 4, 2) and rows["dec_soft_logp"].shape == (3, 4, 2)
    flat_i, flat_l = b["dec_soft_ids"].reshape(6, 4, 2), b["dec_soft_logp"].reshape(6, 4, 2)
    assert torch.equal(rows["dec_soft_ids"], flat_i[idx]) and torch.equal(rows["dec_soft_logp"], flat_l[idx])
    assert torch.equal(rows["dec_labels"], b["dec_labels"].reshape(6, 4)[idx])
    rows, _ = step.select_rows(_batch(soft=False), dict(mode="vd_train", batch_size=3), sample_indices=idx)
    assert "dec_soft_ids" not in rows and "dec_soft_logp" not in rows


def test_forward_rows_hands_the_soft_labels_and_the_two_scalars_to_the_model():
    from gst_visdial_amd import step
    params = dict(mode="vd_train", batch_size=3, device="cpu")
    idx = torch.tensor([1, 2, 5])
    m = StandInModel()
    loss, _ = step.forward(m, _batch(), params, sample_indices=idx, distill_alpha=0.25, distill_temperature=4.0)
    assert loss.grad_fn is not None
    kw = m.calls[0]
    assert kw["distill_alpha"] == 0.25 and kw["distill_temperature"] == 4.0 and kw["dec_soft_ids"].shape == (3, 4, 2)
    m = StandInModel()
    step.forward(m, _batch(soft=False), params, sample_indices=idx)
    assert not any(k.startswith(("dec_soft", "distill")) for k in m.calls[0])                 # nothing new reaches the plain step
