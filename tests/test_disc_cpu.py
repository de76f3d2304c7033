"""CPU side of the discriminative (enc_only_a) evaluation: module surface, fixture self-check against a plain-torch restatement
of pooler + NSP head on top of the oracle's encoder, the host index work of gst_visdial_amd.evaluate_disc, and the C ABI entry."""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_npz


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def restated_scores(sd, cfg, tokens, segments, att, feat, loc, imask, fusion="mul"):
    """models/vilbert_dialog.py:915-941,1026-1041 in fp32 torch on top of oracle.vd_oracle.encoder_forward: first token of each
    stream -> Linear + ReLU -> mul / sum -> bi_seq_relationship.  `sd`: an enc_only_a state dict (keys bert_pretrained.*)."""
    from oracle import vd_oracle as O
    osd = {"encoder." + k: v for k, v in sd.items()}
    xt, xv = O.encoder_forward(osd, cfg, tokens, segments, att, feat, loc, imask)
    p = "bert_pretrained."
    pt = F.relu(F.linear(xt[:, 0], sd[p + "bert.t_pooler.dense.weight"], sd[p + "bert.t_pooler.dense.bias"]))
    pv = F.relu(F.linear(xv[:, 0], sd[p + "bert.v_pooler.dense.weight"], sd[p + "bert.v_pooler.dense.bias"]))
    f = pt * pv if fusion == "mul" else pt + pv
    return F.linear(f, sd[p + "cls.bi_seq_relationship.weight"], sd[p + "cls.bi_seq_relationship.bias"])


def fixture_rows(fx):
    """The fixture batch flattened to one row per option, image tensors expanded the reference's way (evaluate_disc.py:52-58)."""
    b = sc().disc_batch(fx)
    B, R_, O = b["tokens"].shape[:3]
    n = B * R_ * O
    ex = lambda x: x.unsqueeze(1).unsqueeze(1).expand(B, R_, O, *x.shape[1:]).contiguous().view(n, *x.shape[1:])
    return dict(tokens=b["tokens"].view(n, -1), segments=b["segments"].view(n, -1), sep=b["sep_indices"].view(n, -1),
                hist_len=b["hist_len"].view(n), feat=ex(b["image_feat"]), loc=ex(b["image_loc"]), imask=ex(b["image_mask"])), b


def test_enc_only_a_constructs_loads_the_reference_state_dict_strictly_and_round_trips():
    enc, params, fx = sc().build_tiny_disc_encoder()
    ref = {k[len("state::"):]: v for k, v in fx.items() if k.startswith("state::")}
    assert all(k.startswith("bert_pretrained.") for k in ref) and len(ref) > 100
    got = enc.state_dict()
    assert list(got.keys()) == list(ref.keys())
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


@pytest.mark.parametrize("arch", ["enc_only_b", "enc_only", "disc", ""])
def test_other_model_strings_still_raise(arch, tiny_cfg, tmp_path):
    from gst_visdial_amd.modules import VisualDialogEncoder
    p = tmp_path / "enc.json"
    p.write_text(json.dumps(tiny_cfg[0]))
    with pytest.raises(NotImplementedError):
        VisualDialogEncoder(dict(model_enc_config=str(p), gpu_ids=[0], model=arch, mode="vd_eval_val"))


def test_a_train_mode_or_training_state_raises_before_any_device_work():
    enc, params, fx = sc().build_tiny_disc_encoder()
    rows, _ = fixture_rows(fx)
    args = (rows["tokens"][:2], rows["feat"][:2], rows["loc"][:2])
    params["mode"] = "vd_train"                     # params is re-read on every call
    with pytest.raises(NotImplementedError, match="train_disc.py"):
        enc(*args)
    params["mode"] = "vd_eval_val"
    enc.train()
    with pytest.raises(NotImplementedError, match="train_disc.py"):
        enc(*args)
    assert enc._engine is None                      # nothing was built, let alone launched
    enc.eval()
    from gst_visdial_amd._lib import GstvdError
    with torch.no_grad(), pytest.raises(GstvdError, match="no CPU path"):
        enc(*args)                                  # CPU tensors raise as elsewhere


def test_fixture_agrees_with_the_restatement_scores_1e5_ranks_exact(tiny_cfg):
    from gst_visdial_amd.metrics import scores_to_ranks
    from gst_visdial_amd import evaluate_disc as ED
    fx = load_npz("tiny_disc.npz")
    rows, b = fixture_rows(fx)
    sd = {k[len("state::"):]: v for k, v in fx.items() if k.startswith("state::")}
    att = ED.sequence_mask(ED.sequence_lengths(rows["sep"], rows["hist_len"]), rows["tokens"].shape[1])
    assert torch.equal(att, fx["attention_mask"].bool())
    z = restated_scores(sd, tiny_cfg[0], rows["tokens"], rows["segments"], att, rows["feat"], rows["loc"], rows["imask"])
    err = (z - fx["seq_relationship_score"]).abs().max().item()
    print("restatement vs recorded seq_relationship_score: max err %.3e" % err)
    assert err < 1e-5
    prob0 = torch.softmax(z, 1)[:, 0].view(fx["prob0"].shape)
    assert torch.equal(scores_to_ranks(prob0), fx["ranks"].long())
    assert torch.equal(scores_to_ranks(fx["prob0"]), fx["ranks"].long())


def test_fixture_probabilities_keep_the_stated_gap():
    fx = load_npz("tiny_disc.npz")
    p = fx["prob0"]
    assert p.shape[0] >= 2 and p.shape[1] >= 3 and p.shape[2] >= 10
    srt = p.sort(-1)[0]
    gap = (srt[..., 1:] - srt[..., :-1]).min().item()
    assert float(fx["min_gap"]) >= 0.01 and gap >= float(fx["min_gap"]), gap
    # ragged rows, padded image regions
    assert len(set(fx["attention_mask"].sum(1).tolist())) > 3 and int((fx["in::image_mask"] == 0).sum()) >= 2


def test_host_index_work_is_bit_equal_to_torch_restatements():
    """Sequence mask, per-option image indexing and chunking (a rows_per_call that does not divide the 60 rows)."""
    from gst_visdial_amd import evaluate_disc as ED
    fx = load_npz("tiny_disc.npz")
    rows, b = fixture_rows(fx)
    n = rows["tokens"].shape[0]
    B, R_, O = b["tokens"].shape[:3]
    # train_disc.py:97-99 + utils/data_utils.py:7-18, restated
    lengths = torch.gather(rows["sep"], 1, rows["hist_len"].view(-1, 1)).squeeze(1) + 1
    want = torch.arange(0, rows["tokens"].shape[1]).long().unsqueeze(0).expand(n, -1) < lengths.unsqueeze(1).expand(n, -1)
    assert torch.equal(ED.sequence_lengths(rows["sep"], rows["hist_len"]), lengths)
    assert torch.equal(ED.sequence_mask(lengths, rows["tokens"].shape[1]), want)
    d = ED.option_rows_to_dialog(B, R_, O)
    for key, src in (("feat", "image_feat"), ("loc", "image_loc"), ("imask", "image_mask")):
        assert torch.equal(b[src][d], rows[key])
    bounds = ED.chunk_bounds(n, 17)
    assert bounds[0] == (0, 17) and bounds[-1] == (51, 60) and len(bounds) == 4
    assert [s for s, _ in bounds[1:]] == [e for _, e in bounds[:-1]]
    seen = []
    params = dict(device=torch.device("cpu"), mode="vd_eval_val")
    for s, e in bounds:
        item = ED.chunk_item(b, d, s, e)
        tokens, features, spatials, sep, segments, mask, att, image_mask = ED._prepare(item, params)
        assert torch.equal(tokens, rows["tokens"][s:e]) and torch.equal(segments, rows["segments"][s:e])
        assert torch.equal(features, rows["feat"][s:e]) and torch.equal(spatials, rows["loc"][s:e])
        assert torch.equal(image_mask, rows["imask"][s:e]) and torch.equal(att, want[s:e])
        seen.append(tokens.shape[0])
    assert sum(seen) == n


def test_evaluate_disc_driver_reproduces_reference_metrics_from_recorded_scores():
    """The driver with the device work replaced by the recorded scores: chunk order, reshape, metric calls (evaluate_disc.py:87-95)."""
    from gst_visdial_amd import evaluate_disc as ED
    fx = load_npz("tiny_disc.npz")
    b = sc().disc_batch(fx)
    flat = fx["seq_relationship_score"]

    class Stub(object):
        def __init__(self):
            self.at = 0

        def eval(self):
            return self

        def nsp_scores(self, tokens, *a):
            z = flat[self.at:self.at + tokens.shape[0]]
            self.at += tokens.shape[0]
            return z, torch.softmax(z, 1)[:, 0]

    m = ED.evaluate_disc(Stub(), [b], dict(device=torch.device("cpu"), mode="vd_eval_val"), 2, rows_per_call=17)
    ref = dict(zip(("r@1", "r@5", "r@10", "mean", "mrr"), fx["sparse"].tolist()), ndcg=float(fx["ndcg"]))
    for k, v in ref.items():
        assert m[k] == v, (k, m[k], v)
    b["image_id"] = torch.tensor([7, 9])
    b1 = {k: (v[:, :1] if k in ("tokens", "segments", "sep_indices", "mask", "hist_len") else v) for k, v in b.items()}
    st = Stub()
    st.nsp_scores = lambda tokens, *a: (None, fx["prob0"][:, :1].reshape(-1))
    rj = ED.evaluate_disc(st, [b1], dict(device=torch.device("cpu"), mode="vd_eval_test"), 2, rows_per_call=200)
    assert [r["image_id"] for r in rj] == [7, 9] and rj[0]["ranks"] == fx["ranks"][0, 0].tolist()


def test_header_bindings_and_library_agree_on_gstvd_nsp_head():
    from gst_visdial_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    assert re.search(r"\bint\s+gstvd_nsp_head\s*\(\s*const\s+gstvd_nsp_head_t\s*\*", hdr)
    assert "gstvd_nsp_head" in _lib.SIGNATURES
    # the struct the header declares, field for field, against the ctypes mirror
    body = re.search(r"typedef struct \{([^}]*)\} gstvd_nsp_head_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [x.strip().lstrip("*").strip() for x in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.NspHeadDesc._fields_], names
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    assert hasattr(lib, "gstvd_nsp_head") and lib.gstvd_abi_version() == 9
    assert lib.gstvd_nsp_head(None, None) == -4          # GSTVD_E_NULL: argument checks run before anything touches a device
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"nsp_head_kernel" in blob
    src = open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "pool_head.hip")).read()
    assert "getenv" not in src
