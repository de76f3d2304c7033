"""The coreference text attack end to end on a real MI355X: the tiny golden model on rows of tests/golden/tiny_evalset100.npz, a
SynonymTable built from tests/golden/tiny_synonym.npz, the substitution checked against tests/exact_synonym.py's rule."""
import numpy as np
import pytest
import torch

import exact_synonym as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLS, SEP, PAD = 101, 102, 0
DIALOG, ROUND = 0, 2                    # the third round of dialog 0: six separators, so it is round 3 that is attacked


@pytest.fixture(scope="module")
def table():
    from gst_visdial_amd.synonyms import SynonymTable
    fx = X.load_fixture()
    return SynonymTable.build(fx["emb"], fx["words"].tolist(), K=int(fx["K"]), threshold=float(fx["threshold"]), device=DEV), fx


@pytest.fixture(scope="module")
def model():
    from gst_visdial_amd.selfcheck import build_tiny_model
    m, params, _ = build_tiny_model("fp32", DEV, mode="vd_eval_val", state_file="tiny_state_trained.npz")
    m.eval()
    return m, dict(params, attack="coreference", device=torch.device(DEV))


def chunk(dep):
    from gst_visdial_amd.selfcheck import load_npz
    ev = load_npz("tiny_evalset100.npz")
    ids = ev["in::enc_input_ids"][DIALOG, ROUND].long()
    seg = ev["in::enc_segments"][DIALOG, ROUND].long()
    dec = ev["in::dec_input_ids"][DIALOG, ROUND].long()
    rows, T = dec.shape[0], ids.numel()
    sep = (ids == SEP).nonzero().view(-1)
    assert sep.numel() == 2 * (ROUND + 1)
    return dict(enc_input_ids=ids.repeat(rows, 1), enc_segments=seg.repeat(rows, 1),
                enc_sep_indices=torch.cat([sep, torch.zeros(25 - sep.numel(), dtype=torch.long)]).repeat(rows, 1),
                enc_mlm_labels=torch.full((rows, T), -1), enc_att_mask=(ids != PAD).float().repeat(rows, 1),
                dec_input_ids=dec, dec_att_mask=ev["in::dec_att_mask"][DIALOG, ROUND],
                enc_image_feat=ev["in::enc_image_feat"][DIALOG:DIALOG + 1].expand(rows, -1, -1),
                enc_image_loc=ev["in::enc_image_loc"][DIALOG:DIALOG + 1].expand(rows, -1, -1),
                enc_image_mask=ev["in::enc_image_mask"][DIALOG:DIALOG + 1].expand(rows, -1),
                round_id=torch.tensor([ROUND + 1]), gt_relevance=torch.zeros(rows), coref_dependency=dep)


def substituter(tab, refresh=False):
    """Three words of the fixture's vocabulary stand for wordpieces of the chunk's context; their nearest neighbours get new
    pieces.  Caption (round 0), round 2 (utterances 3 and 4), round 1 (utterances 1 and 2)."""
    from gst_visdial_amd.synonyms import CorefSubstituter
    wa, wb, wc = "w0005", "w0100", "w0300"
    word_ids = {wa: [241], tab.nearest(wa): [250, 251], wb: [230, 203], tab.nearest(wb): [252], wc: [171], tab.nearest(wc): [253, 254, 255]}
    assert len(word_ids) == 6
    dep = {"0": wa, "2": wb, "1": wc, "3": "w0007"}                                # the last has no wordpieces: skipped
    plan = [(0, [241], [250, 251]), (3, [230, 203], [252]), (4, [230, 203], [252]), (1, [171], [253, 254, 255]), (2, [171], [253, 254, 255])]
    return CorefSubstituter(tab, word_ids, device=DEV, refresh=refresh), dep, plan


class RuleSubstituter(object):
    """Hands forward_attack the ids tests/exact_synonym.py's rule gives."""
    refresh = False

    def __init__(self, plan):
        self.plan = plan

    def attack_row(self, ids, dep, refresh=False, segments=None):
        out, _ = X.replace_rule(ids[:1].numpy(), [self.plan], SEP, PAD)
        return torch.from_numpy(out).to(DEV)


def test_table_build_equals_neighbours_and_the_reference(table):
    tab, fx = table
    V = len(tab.words)
    idx, val = tab.neighbours(torch.arange(V))
    assert torch.equal(idx, tab.idx) and val.cpu().numpy().tobytes() == tab.val.cpu().numpy().tobytes()
    src = [5, 100, 5, 511, 0]
    idx, val = tab.neighbours(src)
    assert torch.equal(idx.cpu(), tab.idx_host[src]) and torch.equal(val.cpu(), tab.val_host[src])
    chk = fx["checked"]
    assert np.array_equal(tab.idx_host.numpy()[chk], fx["ref_idx"][chk])
    assert tab.nearest("w0005") == fx["words"][fx["ref_idx"][5, 0]] and tab.nearest("nope") is None


def test_scores_equal_the_rule_fed_model_bit_for_bit(table, model):
    from gst_visdial_amd import attack
    m, params = model
    sub, dep, plan = substituter(table[0])
    assert sub.plan(dep) == plan and dict(sub.skipped) == {"no_word_ids": 1}
    b = chunk(dep)
    keep = {k: v.clone() for k, v in b.items() if isinstance(v, torch.Tensor)}
    want_ids, n = X.replace_rule(b["enc_input_ids"][:1].numpy(), [plan], SEP, PAD)
    assert n[0] == 3 and not np.array_equal(want_ids, b["enc_input_ids"][:1].numpy())
    got_ids = sub.attack_row(b["enc_input_ids"], dep)
    assert np.array_equal(got_ids.cpu().numpy(), want_ids)
    with torch.no_grad():
        a = attack.forward_attack(m, b, params, coref=sub).float().cpu()
        r = attack.forward_attack(m, b, params, coref=RuleSubstituter(plan)).float().cpu()
        plain = attack.forward_attack(m, dict(b, coref_dependency={}), params, coref=sub).float().cpu()
    assert torch.equal(a, r) and not torch.equal(a, plain)
    for k, v in keep.items():
        assert torch.equal(b[k], v), k                                            # the loader's tensors are never written
    # the consistent form: segments, separators and mask recomputed from the new ids
    rsub, _, _ = substituter(table[0], refresh=True)
    ids2, seg, sepi, att = rsub.attack_row(b["enc_input_ids"], dep, refresh=True, segments=b["enc_segments"])
    ws, wi, wa = X.refresh_rule(want_ids, SEP, PAD, 25, [int(b["enc_segments"][0, 0])])
    assert np.array_equal(ids2.cpu().numpy(), want_ids) and np.array_equal(seg.cpu().numpy(), ws)
    assert np.array_equal(sepi.cpu().numpy(), wi) and np.array_equal(att.cpu().numpy(), wa)


def test_one_pass_route_agrees_with_the_hundred_row_route(table, model):
    from oracle import vd_oracle as O
    from gst_visdial_amd import attack
    m, params = model
    sub, dep, _ = substituter(table[0])
    b = chunk(dep)
    with torch.no_grad():
        logits = attack.forward_attack(m, b, params, coref=sub).float().cpu()
        sc = O.answer_scores(logits, b["dec_input_ids"])
        one = attack.score_chunk(m, b, params, 1.0, coref=sub).cpu()
        b2 = chunk(dep)
        b2["enc_segments"][1, 2] ^= 1                                             # rows differ: the multi-row forward
        many = attack.score_chunk(m, b2, dict(params, coref=sub), 1.0).cpu()
    print("one-pass scores vs the 100-row forward %.3e" % (one - sc).abs().max().item())
    assert (one - sc).abs().max().item() <= 1e-3                                  # the bar of tests/test_mlm_fill_gpu.py for this pair
    assert abs(many[0].item() - sc[0].item()) <= 1e-3
    with pytest.raises(NotImplementedError):
        attack.score_chunk(m, b, params, 1.0)
