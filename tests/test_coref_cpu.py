"""Host logic of the coreference text attack (no GPU): the substitution plan and its skip counts, the attack wiring with a fake
model and a fake substituter, the dependency indexing of evaluate_attack, and the refusals that stay."""
import types

import numpy as np
import pytest
import torch

CLS, SEP, PAD = 101, 102, 0


def make_table(threshold=0.5):
    from gst_visdial_amd.synonyms import SynonymTable
    words = ["dog", "puppy", "cat", "kitten", "lonely", "dog", "zebra"]           # "dog" twice: the first occurrence wins
    idx = torch.tensor([[1, 3], [0, -1], [3, -1], [2, 0], [-1, -1], [6, -1], [5, -1]], dtype=torch.int32)
    val = torch.tensor([[0.9, 0.6], [0.9, 0.0], [0.8, 0.0], [0.8, 0.6], [0.0, 0.0], [0.7, 0.0], [0.7, 0.0]])
    return SynonymTable(words, idx, val, 2, threshold)


WORD_IDS = {"dog": [11], "puppy": [12, 13], "cat": [14], "kitten": [15, 16, 17], "lonely": [18]}


def test_table_lookups_and_round_trip(tmp_path):
    from gst_visdial_amd.synonyms import SynonymTable, unit_rows, first_occurrence
    t = make_table()
    assert t.word2idx["dog"] == 0 and t.nearest("dog") == "puppy" and t.nearest("kitten") == "cat"
    assert t.nearest("lonely") is None and t.nearest("unicorn") is None
    with pytest.raises(RuntimeError):
        t.neighbours([0])                                                         # no unit rows: nothing to look up on
    t.save(str(tmp_path / "t.npz"))
    u = SynonymTable.load(str(tmp_path / "t.npz"))
    assert u.words == t.words and torch.equal(u.idx_host, t.idx_host) and torch.equal(u.val_host, t.val_host)
    assert u.K == 2 and u.threshold == 0.5 and u.nearest("cat") == "kitten"
    assert first_occurrence(["a", "b", "a"]) == {"a": 0, "b": 1}
    e = np.array([[3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0]], np.float32)
    h = unit_rows(torch.from_numpy(e))
    assert h.dtype == torch.float32 and torch.equal(h, torch.tensor([[0.6, 0.8, 0, 0], [0, 0, 1.0, 0]]))
    assert np.array_equal(h.numpy(), np.asarray(e.astype(np.float64) / np.linalg.norm(e.astype(np.float64), axis=1, keepdims=True), "float32"))


def test_plan_order_and_skip_reasons():
    from gst_visdial_amd.synonyms import CorefSubstituter, SKIP_REASONS
    sub = CorefSubstituter(make_table(), WORD_IDS, device="cpu")
    dep = {"2": "kitten", "0": "dog", "1": "unicorn", "3": "lonely", "4": "zebra", "5": "cat"}
    plan = sub.plan(dep)
    assert plan == [(3, [15, 16, 17], [14]), (4, [15, 16, 17], [14]),             # keys in the dict's order; round 2: utterances 3, 4
                    (0, [11], [12, 13]),                                          # round 0: the caption
                    (9, [14], [15, 16, 17]), (10, [14], [15, 16, 17])]
    assert dict(sub.skipped) == {"not_in_table": 1, "no_neighbour": 1, "no_word_ids": 1} and sub.planned == 3
    assert set(sub.skipped) <= set(SKIP_REASONS)
    assert sub.plan({}) == [] and sub.plan(None) == []
    sub2 = CorefSubstituter(make_table(), {"dog": [11]}, device="cpu")            # the synonym has no wordpieces either
    assert sub2.plan({"1": "dog"}) == [] and sub2.skipped["no_word_ids"] == 1


class FakeSubstituter(object):
    """Stands in for synonyms.CorefSubstituter: replaces token 5 by 77 in row 0, records what it was handed."""

    def __init__(self, refresh=False):
        self.calls, self.refresh = [], refresh

    def attack_row(self, ids, dep, refresh=False, segments=None):
        self.calls.append(dict(ids=ids.clone(), dep=dict(dep), refresh=refresh))
        row = ids[:1].clone()
        row[row == 5] = 77
        if refresh:
            return row, segments[:1] + 10, torch.full((1, 6), 3), torch.full((1, ids.shape[1]), 0.5)
        return row


class FakeModel(object):
    def __init__(self):
        self.seen = []

    def __call__(self, **kw):
        self.seen.append(kw)
        return None, "lm_scores"


def context(round_no, T=16):
    """[CLS] caption [SEP] (q [SEP] a [SEP]) x (round_no - 1) q [SEP]: 2 * round_no separators."""
    row = [CLS, 5, 6, SEP]
    for r in range(round_no - 1):
        row += [7, SEP, 5, SEP]
    row += [8, SEP]
    ids = torch.tensor(row + [PAD] * (T - len(row)))
    sep = (ids == SEP).nonzero().view(-1)
    seg, cur = torch.zeros(T, dtype=torch.long), 0
    for q in range(len(row)):
        seg[q] = cur
        cur ^= int(ids[q] == SEP)
    return ids, seg, torch.cat([sep, torch.zeros(6 - sep.numel(), dtype=torch.long)])


def chunk(round_no, round_id, rows=4, dep=None):
    ids, seg, sep = context(round_no)
    b = dict(enc_input_ids=ids.repeat(rows, 1), enc_segments=seg.repeat(rows, 1), enc_sep_indices=sep.repeat(rows, 1),
             enc_mlm_labels=torch.full((rows, ids.numel()), -1), enc_att_mask=(ids != PAD).float().repeat(rows, 1),
             dec_input_ids=torch.arange(rows * 5).view(rows, 5) + 1, dec_att_mask=torch.ones(rows, 5),
             enc_image_feat=torch.randn(rows, 3, 8), enc_image_loc=torch.rand(rows, 3, 5), enc_image_mask=torch.ones(rows, 3),
             round_id=torch.tensor([round_id]), gt_relevance=torch.zeros(rows))
    if dep is not None:
        b["coref_dependency"] = dep
    return b


PARAMS = dict(attack="coreference", device=torch.device("cpu"))


def test_only_the_relevance_round_is_attacked_and_row_0_is_repeated():
    from gst_visdial_amd import attack
    sub, model = FakeSubstituter(), FakeModel()
    b = chunk(2, 2, dep={"1": "dog"})
    b["enc_input_ids"][1, 1] = 9                                                  # row 1 differs: the result is row 0 repeated
    keep = {k: v.clone() for k, v in b.items() if isinstance(v, torch.Tensor)}
    out = attack.forward_attack(model, b, PARAMS, coref=sub)
    assert out == "lm_scores" and len(sub.calls) == 1 and sub.calls[0]["dep"] == {"1": "dog"} and not sub.calls[0]["refresh"]
    got = model.seen[0]["enc_input_ids"]
    want = keep["enc_input_ids"][:1].clone()
    want[want == 5] = 77
    assert torch.equal(got, want.repeat(4, 1)) and int((got == 77).sum()) == 8
    for k, v in keep.items():
        assert torch.equal(b[k], v), k                                            # the loader's tensors are never written
    assert torch.equal(model.seen[0]["enc_segments"], keep["enc_segments"])       # only the ids change by default
    assert torch.equal(model.seen[0]["enc_sep_indices"], keep["enc_sep_indices"])
    assert torch.equal(model.seen[0]["enc_attention_mask"], keep["enc_att_mask"])
    assert torch.equal(model.seen[0]["enc_image_features"], keep["enc_image_feat"])          # no FGSM step on this branch
    # another round of the same dialog: not attacked, the substituter is not asked
    attack.forward_attack(model, chunk(1, 2, dep={"0": "dog"}), PARAMS, coref=sub)
    assert len(sub.calls) == 1 and int((model.seen[1]["enc_input_ids"] == 77).sum()) == 0
    # no dependencies: the ids are unchanged, every row as loaded
    b = chunk(2, 2, dep={})
    b["enc_input_ids"][1, 1] = 9
    attack.forward_attack(model, b, PARAMS, coref=sub)
    assert len(sub.calls) == 1 and torch.equal(model.seen[2]["enc_input_ids"], b["enc_input_ids"])
    # the substituter may come through params
    attack.forward_attack(model, chunk(2, 2, dep={"1": "dog"}), dict(PARAMS, coref=sub))
    assert len(sub.calls) == 2 and int((model.seen[3]["enc_input_ids"] == 77).sum()) == 8


def test_refresh_substituter_replaces_segments_separators_and_mask():
    from gst_visdial_amd import attack
    sub, model = FakeSubstituter(refresh=True), FakeModel()
    b = chunk(2, 2, dep={"1": "dog"})
    attack.forward_attack(model, b, PARAMS, coref=sub)
    kw = model.seen[0]
    assert sub.calls[0]["refresh"]
    assert torch.equal(kw["enc_segments"], (b["enc_segments"][:1] + 10).repeat(4, 1))
    assert torch.equal(kw["enc_sep_indices"], torch.full((4, 6), 3)) and torch.equal(kw["enc_attention_mask"], torch.full((4, 16), 0.5))


def scoring_model(seen):
    def score_candidates(feat, loc, vmask, ids, seg, att, dec_ids, dec_att, group):
        seen.append(dict(ids=ids.clone(), seg=seg.clone(), att=att.clone(), rows=dec_ids.shape[0]))
        return torch.arange(dec_ids.shape[0], dtype=torch.float32)
    return types.SimpleNamespace(score_candidates=score_candidates, eval=lambda: None)


def test_score_chunk_takes_the_one_pass_route():
    from gst_visdial_amd import attack
    seen, sub = [], FakeSubstituter()
    model = scoring_model(seen)
    s = attack.score_chunk(model, chunk(2, 2, dep={"1": "dog"}), PARAMS, 1.0, coref=sub)
    assert s.tolist() == [0.0, 1.0, 2.0, 3.0] and seen[0]["ids"].shape == (1, 16) and int((seen[0]["ids"] == 77).sum()) == 2
    attack.score_chunk(model, chunk(1, 2, dep={"0": "dog"}), dict(PARAMS, coref=sub), 1.0)          # not the attacked round
    assert len(sub.calls) == 1 and int((seen[1]["ids"] == 77).sum()) == 0
    attack.score_chunk(model, chunk(2, 2, dep={}), PARAMS, 1.0, coref=sub)                          # nothing to substitute
    assert len(sub.calls) == 1 and int((seen[2]["ids"] == 77).sum()) == 0
    rsub = FakeSubstituter(refresh=True)
    attack.score_chunk(model, chunk(2, 2, dep={"1": "dog"}), PARAMS, 1.0, coref=rsub)
    assert int(seen[3]["seg"].min()) >= 10 and float(seen[3]["att"][0, 0]) == 0.5


def test_evaluate_attack_indexes_the_dependencies_by_dialog_and_chunk():
    from gst_visdial_amd import attack
    rounds, options, Bd = 2, 100, 2

    def dialog(round_id):
        per_round = [chunk(r + 1, round_id, rows=options) for r in range(rounds)]
        d = {k: torch.stack([c[k] for c in per_round]) for k in ("enc_input_ids", "enc_segments", "enc_sep_indices", "enc_mlm_labels",
                                                                 "enc_att_mask", "dec_input_ids", "dec_att_mask")}
        d.update(enc_image_feat=per_round[0]["enc_image_feat"][0], enc_image_loc=per_round[0]["enc_image_loc"][0],
                 enc_image_mask=per_round[0]["enc_image_mask"][0], round_id=torch.tensor([round_id]), gt_relevance=torch.zeros(options),
                 gt_option_inds=torch.zeros(rounds, dtype=torch.long))
        return d

    def batch(round_ids):
        ds = [dialog(r) for r in round_ids]
        return {k: torch.stack([d[k] for d in ds]) for k in ds[0]}

    loader = [batch([2, 1]), batch([1, 2])]
    deps = [{"coreference": [{"0": "a"}, {"1": "b"}]}, {"coreference": [{"0": "c"}, {}]},
            {"coreference": [{}, {"1": "never"}]}, {"coreference": [{"0": "no"}, {"1": "d", "0": "e"}]}]
    seen, sub = [], FakeSubstituter()
    params = dict(PARAMS, vd_version="0.9")
    _, metrics = attack.evaluate_attack(scoring_model(seen), loader, params, coref=sub, coref_dependency=deps)
    assert [c["dep"] for c in sub.calls] == [{"1": "b"}, {"0": "c"}, {"1": "d", "0": "e"}]           # dialog 2's attacked chunk is empty
    assert len(seen) == Bd * rounds * len(loader) and "r@1" in metrics
    with pytest.raises(ValueError):
        attack.evaluate_attack(scoring_model([]), loader, params, coref=sub)                        # no dependencies handed in


def test_refusals_are_unchanged():
    from gst_visdial_amd import attack
    model = FakeModel()
    b = chunk(2, 2, dep={"1": "dog"})
    with pytest.raises(NotImplementedError) as e:
        attack.forward_attack(model, b, PARAMS)
    for word in ("coreference", "coreference dependencies", "counter-fitted", "BertForMaskedLM", "CorefSubstituter"):
        assert word in str(e.value)
    filler = types.SimpleNamespace(fill=None, host_rows=None)
    with pytest.raises(NotImplementedError):
        attack.forward_attack(model, b, PARAMS, textattack=filler)                # a masked-LM filler is not a substituter
    with pytest.raises(NotImplementedError):
        attack.score_chunk(model, b, PARAMS, 1.0)
    with pytest.raises(NotImplementedError):
        attack.evaluate_attack(model, [], PARAMS)
    with pytest.raises(NotImplementedError):
        attack.evaluate_attack(model, [], dict(PARAMS, attack="random_token"))
    with pytest.raises(NotImplementedError):
        attack.forward_attack(model, b, dict(PARAMS, attack="typo"), coref=FakeSubstituter())
    assert not model.seen


def test_library_entry_points_check_their_arguments():
    import ctypes as C
    from gst_visdial_amd import _lib, ops
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.gstvd_abi_version() == 9                  # entries added, no signature changed
    assert lib.gstvd_cos_topk_route(8, 65713) == _lib.COS_TOPK_FEW and lib.gstvd_cos_topk_route(65713, 65713) == _lib.COS_TOPK_MANY
    assert lib.gstvd_cos_topk_ws_bytes(0, 5, 10) == 0 and lib.gstvd_cos_topk_ws_bytes(8, 65713, 17) == 0
    assert lib.gstvd_cos_topk_ws_bytes(8, 65713, 10) % (8 * 10 * 8) == 0
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    p += (-p) % 16
    assert lib.gstvd_cos_topk(None, 4, 1, 4, None, 1, 1, 0.5, 0, None, 0, None, None, None) == -4
    assert lib.gstvd_cos_topk(p, 300, 8, 300, None, 8, 17, 0.5, 0, p, 4096, p, p, None) == -2       # K > 16
    assert lib.gstvd_cos_topk(p, 300, 8, 300, None, 5, 10, 0.5, 0, p, 4096, p, p, None) == -2       # src NULL with n != V
    assert lib.gstvd_cos_topk(p, 302, 8, 300, None, 8, 10, 0.5, 0, p, 4096, p, p, None) == -3       # ld % 4
    assert lib.gstvd_cos_topk(p + 4, 300, 8, 300, None, 8, 10, 0.5, 0, p, 4096, p, p, None) == -3   # base not 16-byte aligned
    assert lib.gstvd_cos_topk(p, 516, 8, 516, None, 8, 10, 0.5, 0, p, 4096, p, p, None) == -5       # a D the kernel cannot hold
    assert lib.gstvd_cos_topk(p, 300, 8, 300, None, 8, 10, 0.5, _lib.COS_TOPK_FEW, p, 8, p, p, None) == -2   # workspace too small
    assert lib.gstvd_cos_topk(p, 300, 8, 300, None, 8, 10, 0.5, 7, p, 4096, p, p, None) == -2       # unknown route
    d = _lib.SubseqReplaceDesc()
    assert lib.gstvd_subseq_replace(C.byref(d), None) == -4
    d.ids, d.out_ids, d.n_replaced, d.row_ptr = p, p + 2048, p, p
    d.n, d.T, d.ld_ids, d.ld_out = 1, 2000, 2000, 2000
    assert lib.gstvd_subseq_replace(C.byref(d), None) == -5                       # T > 1024
    d.T, d.ld_ids = 8, 4
    assert lib.gstvd_subseq_replace(C.byref(d), None) == -2                       # a row stride below its row
    with pytest.raises(_lib.GstvdError):
        ops.cos_topk(torch.zeros(4, 8), None, K=2)                                # CPU tensors: there is no CPU path
    with pytest.raises(_lib.GstvdError):
        ops.subseq_replace(torch.zeros(2, 8, dtype=torch.int64), [[], []])
    with pytest.raises(_lib.GstvdError):
        ops.pack_substitutions([[(0, [1] * 17, [2])]], "cpu")
    rp, subs, pieces = ops.pack_substitutions([[(1, [5, 6], [7])], [], [(0, [8], [9, 10])]], "cpu")
    assert rp.tolist() == [0, 1, 1, 2] and subs.tolist() == [[1, 0, 2, 1], [0, 3, 1, 2]] and pieces.tolist() == [5, 6, 7, 8, 9, 10]
