"""Host-side checks of the random-token text attack (no GPU): the text-only encoder configuration, the BertForMaskedLM key
mapping, the fill rule against tests/golden/tiny_mlm_fill.npz (what the reference's TextAttack.random_token_attack returned),
the library's new entry points, and the attack wiring with a fake filler."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import exact_mlm as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    from gst_visdial_amd.selfcheck import load_npz
    return load_npz("tiny_mlm_fill.npz")


def mlm_state(fx):
    return {k[len("mlm_state::"):]: v for k, v in fx.items() if k.startswith("mlm_state::")}


def mlm_config(fx):
    cfg = {k[len("mlm_cfg::"):]: v.item() for k, v in fx.items() if k.startswith("mlm_cfg::")}
    cfg["hidden_act"] = "gelu"
    return cfg


# ------------------------------------------------------------------------------------------ configuration
def test_text_only_config_validates_and_schedules_the_text_layers():
    from gst_visdial_amd.config import BertConfig, encoder_schedule
    from gst_visdial_amd.mlm import text_only_config
    cfg = BertConfig.from_dict(text_only_config(dict(vocab_size=600, hidden_size=64, num_hidden_layers=3, num_attention_heads=2,
                                                     intermediate_size=128, max_position_embeddings=64, type_vocab_size=2)))
    cfg.validate()
    assert cfg.text_only()
    assert encoder_schedule(cfg) == [("t", 0), ("t", 1), ("t", 2)]
    with pytest.raises(NotImplementedError):
        text_only_config(dict(vocab_size=600, hidden_size=64, num_hidden_layers=3, layer_norm_eps=1e-5))
    with pytest.raises(NotImplementedError) as e:                   # head size 16: no attention kernel
        text_only_config(dict(vocab_size=600, hidden_size=64, num_hidden_layers=3, num_attention_heads=4))
    assert "head sizes 32, 64 and 128" in str(e.value)


def test_shipped_and_tiny_configs_validate_as_before():
    import json
    from gst_visdial_amd.config import BertConfig, bert_base_enc_config, encoder_schedule
    shipped = BertConfig.from_dict(bert_base_enc_config())
    shipped.validate()
    assert not shipped.text_only()
    sched = encoder_schedule(shipped)
    assert len(sched) == 12 + 6 + 6 and sched[-1] == ("t", 11) and sched[6] == ("c", 0) and sched.count(("t", 0)) == 1
    with open(os.path.join(ROOT, "tests", "golden", "tiny_cfg.json")) as f:
        tiny = BertConfig.from_dict(json.load(f)["enc"])
    tiny.validate()
    assert not tiny.text_only()
    assert [k for k, _ in encoder_schedule(tiny)] == ["t", "t", "c", "v", "t", "c", "v", "t"]
    # what was refused stays refused: no connection layers but vision layers left over, and lists of different lengths
    with pytest.raises(ValueError):
        BertConfig.from_dict(dict(bert_base_enc_config(), v_biattention_id=[], t_biattention_id=[])).validate()
    with pytest.raises(AssertionError):
        BertConfig.from_dict(dict(bert_base_enc_config(), v_biattention_id=[0], t_biattention_id=[])).validate()
    with pytest.raises(AssertionError):
        BertConfig.from_dict(dict(bert_base_enc_config(), v_biattention_id=[9], t_biattention_id=[3])).validate()


# ------------------------------------------------------------------------------------------ key mapping
def test_state_dict_round_trip(fx):
    from gst_visdial_amd.mlm import MaskedLMFiller
    sd = mlm_state(fx)
    filler = MaskedLMFiller(mlm_config(fx), "cpu", precision="fp32", mask_token_id=int(fx["mask_token_id"]))
    before = {k: v.clone() for k, v in filler.model.state_dict().items()}
    ignored = filler.load_bert_mlm_state_dict(sd)
    assert all(k.endswith("position_ids") for k in ignored), ignored
    own = filler.model.state_dict()
    covered = set()
    for k, v in sd.items():
        if k.endswith("position_ids"):
            continue
        name = "bert_pretrained." + ("cls.predictions.bias" if k == "cls.predictions.decoder.bias" else k)
        assert torch.equal(own[name], v), k
        covered.add(name)
    bert = filler.model.bert_pretrained
    assert bert.cls.predictions.decoder.weight is bert.bert.embeddings.word_embeddings.weight        # still tied
    left = set(own) - covered
    assert left and all(torch.equal(own[k], before[k]) for k in left)                                # the rest keeps its init
    for part in ("token_type_embeddings_extension", "sep_embeddings", "v_embeddings", "t_pooler", "v_pooler", "bi_seq_relationship",
                 "imagePredictions"):
        assert any(part in k for k in left), part
    assert not any(".encoder.layer." in k or "cls.predictions" in k for k in left)


def test_legacy_layer_norm_names_and_refusals(fx):
    from gst_visdial_amd.mlm import map_bert_mlm_state_dict
    sd = mlm_state(fx)
    legacy = {}
    for k, v in sd.items():
        if "LayerNorm.weight" in k:
            legacy[k.replace("LayerNorm.weight", "LayerNorm.gamma")] = v
        elif "LayerNorm.bias" in k:
            legacy[k.replace("LayerNorm.bias", "LayerNorm.beta")] = v
        else:
            legacy[k] = v
    a, _ = map_bert_mlm_state_dict(sd, 3)
    b, ignored = map_bert_mlm_state_dict(legacy, 3)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(k.endswith("position_ids") for k in ignored)

    missing = dict(sd)
    del missing["bert.encoder.layer.1.attention.output.dense.bias"]
    with pytest.raises(KeyError) as e:
        map_bert_mlm_state_dict(missing, 3)
    assert "bert.encoder.layer.1.attention.output.dense.bias" in str(e.value)

    untied = dict(sd)
    untied["cls.predictions.decoder.weight"] = sd["cls.predictions.decoder.weight"].clone()
    untied["cls.predictions.decoder.weight"][5, 7] += 1.0
    with pytest.raises(ValueError) as e:
        map_bert_mlm_state_dict(untied, 3)
    assert "cls.predictions.decoder.weight" in str(e.value)

    if "cls.predictions.decoder.bias" in sd:
        unbias = dict(sd)
    else:
        unbias = dict(sd, **{"cls.predictions.decoder.bias": sd["cls.predictions.bias"].clone()})
        map_bert_mlm_state_dict(unbias, 3)                      # equal: accepted
    unbias["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"] + 0.5
    with pytest.raises(ValueError) as e:
        map_bert_mlm_state_dict(unbias, 3)
    assert "cls.predictions.decoder.bias" in str(e.value)

    without_decoder = {k: v for k, v in sd.items() if not k.startswith("cls.predictions.decoder.")}
    c, _ = map_bert_mlm_state_dict(without_decoder, 3)          # a checkpoint saved without the tied copies
    assert set(c) == set(a)


# ------------------------------------------------------------------------------------------ fill rule against the reference
def test_fill_rule_reproduces_the_reference(fx):
    mask = int(fx["mask_token_id"])
    ids = fx["ids"].numpy()
    keep = ids.copy()
    got = X.fill_rule(ids, mask, logits=fx["logits0"].numpy())
    assert got.dtype == ids.dtype and np.array_equal(got, fx["filled"].numpy())
    assert np.array_equal(ids, keep)
    idx, val = X.argmax_rows(fx["logits0"].numpy(), fx["logits0"].shape[1])
    assert np.array_equal(idx, fx["argmax0"].numpy())
    assert np.array_equal(X.fill_rule(fx["nomask_ids"].numpy(), mask), fx["nomask_filled"].numpy())
    assert np.array_equal(X.fill_rule(fx["full_ids"].numpy(), mask, logits=fx["full_logits"].numpy()), fx["full_filled"].numpy())
    # the multi-row record is consistent with the single-row one: row 0's positions come first
    n0 = fx["logits0"].shape[0]
    assert np.array_equal(fx["argmax_all"].numpy()[:n0], fx["argmax0"].numpy())
    assert np.array_equal(fx["pos_all"].numpy(), np.nonzero(ids.reshape(-1) == mask)[0])


def test_fixture_margins(fx):
    """The generator's own condition, re-checked on the stored logits: no masked position within 1e-3 of a tie."""
    m = float(fx["margin"])
    assert m == 1e-3
    for z, rec in (("logits0", "margin0"), ("logits_all", "margin_all"), ("full_logits", "full_margin"), ("disc::logits", "disc::margin")):
        lg = fx[z].double()
        top = lg.topk(2, -1).values
        rel = (top[:, 0] - top[:, 1]) / lg.abs().max()
        assert bool((rel >= m).all()), z
        assert torch.allclose(rel.float(), fx[rec].float(), rtol=1e-4, atol=1e-7)
    assert fx["logits0"].shape[0] == 7 and int((fx["ids"][0] != 0).sum()) == 21
    pos0 = (fx["ids"][0] == int(fx["mask_token_id"])).nonzero().view(-1).tolist()
    assert pos0[0] == 1 and any(b - a == 1 for a, b in zip(pos0, pos0[1:]))
    assert fx["disc::logits"].shape[0] == 5


def test_argmax_rule_ties_and_padding():
    z = np.array([[1.0, 3.0, 3.0, 2.0, 9.0], [0.0, -1.0, 0.0, 5.0, 5.0], [-2.0, -2.0, -2.0, -2.0, 7.0]])
    idx, val = X.argmax_rows(z, 4)
    assert idx.tolist() == [1, 3, 0] and val.tolist() == [3.0, 5.0, -2.0]
    x, w, b = X.exact_operands(3, 64, 127, 0)
    assert w.shape == (128, 64) and np.abs(w).max() <= 8 and np.all(w == np.round(w)) and np.all(b * 2 == np.round(b * 2))
    ref = X.exact_logits(x, w, b, 127)
    assert ref.shape == (3, 127) and np.array_equal(ref, (x.astype(np.float32) @ w[:127].T.astype(np.float32) + b[:127]).astype(np.float64))


# ------------------------------------------------------------------------------------------ library
def test_library_exports_the_argmax_entry_points():
    from gst_visdial_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    want = {"gstvd_rows_argmax": 8, "gstvd_vocab_argmax_ws_bytes": 2, "gstvd_vocab_argmax": 14}
    for name, nargs in want.items():
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert _lib.SIGNATURES["gstvd_vocab_argmax_ws_bytes"][0] is C.c_int64
    assert _lib.ABI_VERSION == 9 and lib.gstvd_abi_version() == 9          # entries added, no signature changed
    # the workspace helper is host arithmetic: one 8-byte pair per row and 64-column tile
    assert lib.gstvd_vocab_argmax_ws_bytes(38, 30522) == 38 * 477 * 8
    assert lib.gstvd_vocab_argmax_ws_bytes(1, 1) == 8 and lib.gstvd_vocab_argmax_ws_bytes(0, 5) == 0
    # argument checks run before any launch (no GPU here)
    assert lib.gstvd_rows_argmax(None, 8, 1, 8, _lib.F32, None, None, None) == -4
    assert lib.gstvd_vocab_argmax(None, 64, None, 64, None, 1, 8, 64, _lib.BF16, None, 0, None, None, None) == -4
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    p += (-p) % 16
    assert lib.gstvd_vocab_argmax(p, 64, p, 64, p, 1, 8, 64, _lib.F32, p, 4096, p, p, None) == -5       # fp32: the GEMM route
    assert lib.gstvd_vocab_argmax(p, 48, p, 48, p, 1, 8, 48, _lib.BF16, p, 4096, p, p, None) == -5      # H % 32 != 0
    assert lib.gstvd_vocab_argmax(p, 64, p, 64, p, 1, 8, 64, _lib.BF16, p, 4, p, p, None) == -2         # workspace too small
    assert lib.gstvd_rows_argmax(p, 4, 1, 8, _lib.F32, p, p, None) == -2                                # ld < V


def test_ops_refuse_cpu_tensors():
    from gst_visdial_amd import ops, _lib
    z = torch.zeros(2, 8)
    with pytest.raises(_lib.GstvdError):
        ops.rows_argmax(z, 8)
    assert ops.rows_argmax(z, 8, n=0)[0].numel() == 0                      # n == 0: nothing launched, nothing checked
    assert ops.vocab_argmax(z, z, torch.zeros(8), 8, n=0)[1].numel() == 0


# ------------------------------------------------------------------------------------------ attack wiring (host logic)
class FakeFiller(object):
    """Stands in for mlm.MaskedLMFiller: fills with a fixed token, records what it was handed."""
    mask_token_id = 103

    def __init__(self):
        self.calls = []

    def host_rows(self, ids):
        assert not ids.is_cuda
        return (ids.reshape(-1) == self.mask_token_id).nonzero().view(-1)

    def fill(self, ids, seg, att, rows=None):
        self.calls.append(dict(ids=ids.clone(), rows=rows.clone()))
        row = ids[:1].clone()
        row.view(-1)[rows] = 250
        return row.repeat(ids.shape[0], 1)


class FakeModel(object):
    def __init__(self):
        self.seen = []

    def __call__(self, **kw):
        self.seen.append(kw)
        return None, "lm_scores"


def chunk(fx):
    b = {k[len("atk::in::"):]: v.clone() for k, v in fx.items() if k.startswith("atk::in::")}
    b["round_id"] = torch.tensor([1])
    b["gt_relevance"] = torch.zeros(b["dec_input_ids"].shape[0])
    return b


def test_forward_attack_passes_filled_ids_on(fx):
    from gst_visdial_amd import attack
    b = chunk(fx)
    ids0 = b["enc_input_ids"].clone()
    filler, model = FakeFiller(), FakeModel()
    params = dict(attack="random_token", device=torch.device("cpu"))
    out = attack.forward_attack(model, b, params, textattack=filler)
    assert out == "lm_scores" and len(model.seen) == 1 and len(filler.calls) == 1
    want = torch.from_numpy(X.fill_rule(ids0.numpy(), 103, argmax=[250] * int((ids0[0] == 103).sum())))
    assert torch.equal(model.seen[0]["enc_input_ids"], want) and int((want == 103).sum()) == 0
    assert torch.equal(b["enc_input_ids"], ids0)                           # the loader's tensor is left alone
    assert torch.equal(filler.calls[0]["rows"], (ids0[0] == 103).nonzero().view(-1))
    assert torch.equal(model.seen[0]["enc_segments"], b["enc_segments"]) and model.seen[0]["dec_labels"] is None
    assert torch.equal(model.seen[0]["enc_image_features"], b["enc_image_feat"])          # no FGSM step on this branch
    # the filler may also come through params; the refusal without one still names what is missing and how to supply it
    model2 = FakeModel()
    attack.forward_attack(model2, b, dict(params, textattack=filler))
    assert torch.equal(model2.seen[0]["enc_input_ids"], want)
    with pytest.raises(NotImplementedError) as e:
        attack.forward_attack(model, b, params)
    for word in ("random_token", "BertForMaskedLM", "counter-fitted", "MaskedLMFiller"):
        assert word in str(e.value)
    with pytest.raises(NotImplementedError):
        attack.forward_attack(model, b, dict(params, attack="coreference"), textattack=filler)
    with pytest.raises(NotImplementedError):
        attack.evaluate_attack(model, [], params)


def test_score_chunk_scores_the_filled_row_in_one_pass(fx):
    from gst_visdial_amd import attack
    b = chunk(fx)
    filler = FakeFiller()
    seen = {}

    def score_candidates(feat, loc, vmask, ids, seg, att, dec_ids, dec_att, group):
        seen.update(ids=ids.clone(), seg=seg.clone(), group=group, rows=dec_ids.shape[0])
        return torch.arange(dec_ids.shape[0], dtype=torch.float32)

    model = types.SimpleNamespace(score_candidates=score_candidates)
    params = dict(attack="random_token", device=torch.device("cpu"), textattack=filler)
    scores = attack.score_chunk(model, b, params, 1.0)
    n = b["dec_input_ids"].shape[0]
    assert scores.tolist() == list(range(n)) and seen["group"] == n and seen["rows"] == n
    assert seen["ids"].shape == (1, b["enc_input_ids"].shape[1]) and int((seen["ids"] == 103).sum()) == 0
    assert int((seen["ids"] == 250).sum()) == int((b["enc_input_ids"][0] == 103).sum())
    assert int((b["enc_input_ids"] == 103).sum()) > 0                       # the chunk itself still carries its masks
