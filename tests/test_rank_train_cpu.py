"""Listwise candidate training, the parts that need no GPU: rank_train.rank_targets on the eval loader's layout, the C header /
ctypes table / ABI number of the two new entry points, and the invariants of tests/golden/tiny_rank.npz itself."""
import os
import re

import pytest
import torch

from gst_visdial_amd import _lib, rank_train
from gst_visdial_amd._lib import GstvdError
from gst_visdial_amd.selfcheck import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_batch(B=3, R_=4, O=5, T=6, U=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randint(1, 50, (B, R_, 1, T), generator=g)
    b = dict(enc_input_ids=ctx.expand(B, R_, O, T).clone(), enc_segments=(ctx % 2).expand(B, R_, O, T).clone(),
             enc_att_mask=torch.ones(B, R_, O, T), dec_input_ids=torch.randint(1, 50, (B, R_, O, U), generator=g),
             dec_att_mask=torch.ones(B, R_, O, U), enc_image_feat=torch.randn(B, 7, 8, generator=g), enc_image_loc=torch.rand(B, 7, 5, generator=g),
             enc_image_mask=torch.ones(B, 7), gt_option_inds=torch.randint(0, O, (B, R_), generator=g),
             gt_relevance=torch.rand(B, O, generator=g), round_id=torch.tensor([[2], [4], [1]]))
    return b


def test_rank_targets_picks_the_annotated_round_of_every_dialog():
    b = make_batch()
    t = rank_train.rank_targets(b)
    B, R_, O, T = b["enc_input_ids"].shape
    assert t["num_options"] == O and t["relevance"].shape == (B, O) and torch.equal(t["relevance"], b["gt_relevance"])
    for d, r in enumerate((1, 3, 0)):
        assert torch.equal(t["enc_input_ids"][d], b["enc_input_ids"][d, r, 0])
        assert torch.equal(t["enc_segments"][d], b["enc_segments"][d, r, 0])
        assert torch.equal(t["dec_input_ids"][d * O:(d + 1) * O], b["dec_input_ids"][d, r])
        assert torch.equal(t["dec_attention_mask"][d * O:(d + 1) * O], b["dec_att_mask"][d, r])
    assert t["enc_image_features"].shape[0] == B and t["enc_input_ids"].shape == (B, T)


def test_rank_targets_checks_that_the_options_share_one_context():
    b = make_batch()
    b["enc_input_ids"][1, 3, 2, 0] += 1                       # dialog 1's annotated round: option 2 sees another token
    with pytest.raises(GstvdError, match="share one context"):
        rank_train.rank_targets(b)
    b = make_batch()
    b["enc_input_ids"][1, 0, 2, 0] += 1                       # another round of the dialog: not looked at
    rank_train.rank_targets(b)
    b["round_id"][0, 0] = 5
    with pytest.raises(GstvdError, match="round_id"):
        rank_train.rank_targets(b)


def test_rank_targets_falls_back_to_one_hot_sparse_targets():
    b = make_batch()
    for t in (rank_train.rank_targets(b, sparse=True), rank_train.rank_targets({k: v for k, v in b.items() if k != "gt_relevance"})):
        rel = t["relevance"]
        assert torch.equal(rel.sum(1), torch.ones(3)) and bool(((rel == 0) | (rel == 1)).all())
        for d, r in enumerate((1, 3, 0)):
            assert rel[d, b["gt_option_inds"][d, r]] == 1


def test_header_ctypes_table_and_abi_number():
    with open(os.path.join(ROOT, "include", "gstvd_hip.h")) as f:
        h = f.read()
    assert _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "elementwise.hip")) as f:
        assert re.search(r"gstvd_abi_version\(void\) \{ return 9; \}", f.read())
    m = re.search(r"int gstvd_attn_group_bwd\(const gstvd_attn_t\* a, gstvd_stream_t s\);", h)
    assert m and "gstvd_attn_group_bwd" in _lib.SIGNATURES
    assert _lib.SIGNATURES["gstvd_attn_group_bwd"] == _lib.SIGNATURES["gstvd_attn_bwd"]
    m = re.search(r"int gstvd_rank_loss\(([^;]*)\);", h)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["gstvd_rank_loss"][1]) == 16
    with open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "Makefile")) as f:
        assert "attn_group.hip" in f.read()


def test_the_fixture_keeps_its_own_invariants():
    fx = load_npz("tiny_rank.npz")
    rel, scores, lr = fx["relevance"], fx["scores"], fx["loss_round"]
    assert rel.shape == scores.shape == (3, 4) and fx["in::dec_input_ids"].shape == (12, 9) and fx["in::enc_input_ids"].shape == (3, 24)
    assert rel.sum(1).tolist() == pytest.approx([1.7, 0.0, 1.0]) and int(fx["count"]) == 2
    logp = torch.log_softmax(scores.double(), 1)
    assert float(lr[1]) == 0.0
    assert abs(float(lr[2]) + float(logp[2, 1])) < 1e-5                   # the one-hot round: -log p of its target
    t0 = rel[0].double() / rel[0].sum().double()
    assert abs(float(lr[0]) + float((t0 * logp[0]).sum())) < 1e-4
    assert abs(float(fx["loss"]) - float(lr.sum()) / 2) < 1e-5
    assert bool((fx["in::enc_image_mask"][2, -2:] == 0).all()) and float(fx["in::enc_image_mask"].sum()) == 19
    assert bool((fx["d_feats"][2, -2:] == 0).all()) and bool((fx["d_feats"][1] == 0).all()) and fx["d_feats"].abs().max() > 0
    assert sum(1 for k in fx if k.startswith("grad::")) > 200
    for f in os.listdir(os.path.join(ROOT, "tests", "golden")):
        if f.startswith("tiny_rank"):
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < (1 << 20), f
