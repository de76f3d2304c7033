"""The session cache that `sample`, `beam_search` and `sample_ranked` share (Engine._decode, Engine._decode_sessions) on the tiny
golden model: the clear-at-four eviction, the three modes side by side in one cache with the decode state each leaves behind, and
the eager torch-filter form of `sample` that never captures.  Every result is compared with a model that issues eagerly."""
import pytest
import torch

from conftest import load_npz
from test_sample_ranked_gpu import ARGS, DEV, LOGIT_BAR, STEPS, batch, build, uniforms

pytestmark = [pytest.mark.gpu, pytest.mark.isolated]           # (stream captures: each test in a child process)


def lib_calls():
    from gst_visdial_amd import _lib
    return _lib.N_CALLS[0]


def test_the_fifth_session_clears_the_cache_and_every_call_equals_eager_issue():
    g = load_npz("tiny_train.npz")
    kw, u = batch(g), uniforms(21, 3)
    model, ref = build(graph=True), build(graph=False)
    counts, first = [], None
    for k in (1, 2, 3, 4, 5):
        args = dict(ARGS, top_k=k)
        n0 = lib_calls()
        got = model(uniforms=u, **args, **kw).clone()                          # eager issue, then the capture
        first = lib_calls() - n0
        assert torch.equal(got, ref(uniforms=u, **args, **kw)), k
        counts.append(len(model.engine._decode_sessions))
    assert counts == [1, 2, 3, 4, 1] and len(ref.engine._decode_sessions) == 0
    n0 = lib_calls()
    again = model(uniforms=u, **args, **kw)                                    # the fifth setting again: a replay
    assert lib_calls() - n0 < first and len(model.engine._decode_sessions) == 1
    assert torch.equal(again, ref(uniforms=u, **args, **kw))
    model.engine.close()


def test_three_modes_share_one_cache_and_leave_the_decode_state_they_promise():
    from gst_visdial_amd._lib import GstvdError
    g = load_npz("tiny_train.npz")
    kw, u, u2 = batch(g), uniforms(22, 3), uniforms(23, 6)
    args = dict(ARGS, ngram_blocking_size=2)

    def rescore(m, ids):
        loss, logits = m.engine.rescore_sampled(ids.clone())
        assert logits.numel() == 3 * STEPS * m.decoder.config.vocab_size and bool(torch.isfinite(logits).all())
        return logits

    def run(m):
        out = []
        a = m(uniforms=u, **args, **kw).clone()
        out += [a, rescore(m, a)]
        seqs, scores = m.beam_search(num_beams=2, **kw)
        out += [seqs.clone(), scores.clone()]
        with pytest.raises(GstvdError, match="no decode state"):
            m.engine.rescore_sampled(seqs[:, 0].contiguous())
        seqs, scores, tl = m.sample_ranked(num_samples=2, uniforms=u2, **args, **kw)
        out += [seqs.clone(), scores.clone(), tl.clone(), rescore(m, seqs[:, 0].contiguous())]
        out.append(m(uniforms=u, **args, **kw).clone())
        return out

    model, ref = build(graph=True), build(graph=False)
    want = run(ref)
    one = run(model)                                                           # eager issue, three captures, one replay
    assert len(model.engine._decode_sessions) == 3
    two = run(model)                                                           # replays only
    assert len(model.engine._decode_sessions) == 3 and len(ref.engine._decode_sessions) == 0
    for i, (w, a, b) in enumerate(zip(want, one, two)):
        if i in (1, 7):                                                        # rescored logits: the project's fp32 parity bar
            assert (a - w).abs().max().item() < LOGIT_BAR and (b - w).abs().max().item() < LOGIT_BAR, i
        else:
            assert torch.equal(a, w) and torch.equal(b, a), i
    assert torch.equal(one[0], one[8])
    model.engine.close()


def test_the_torch_filter_form_of_sample_issues_eagerly_and_captures_nothing():
    """top_k = 1: the kept set is the arg-max alone in both forms of the filters -- on this fixture's logits (the CPU oracle's greedy
    path, temperature 1.3) `decoding.batch_top_k_top_p_sampling` keeps exactly one token at all 18 steps of all 3 rows, and the
    runner-up is never closer than 2.5e-3, 25 times the fp32 logit bar -- so no tie decides between the two forms."""
    from gst_visdial_amd.engine import Engine
    g = load_npz("tiny_train.npz")
    kw, u = batch(g), uniforms(24, 3)
    args = dict(ARGS, top_k=1)
    want = build(graph=False)(uniforms=u, **args, **kw).clone()                # the fused sampling launch, eagerly
    model = build(graph=True)
    keep = Engine.__dict__["_fused_sampling"]                                  # (the staticmethod object itself)
    try:
        Engine._fused_sampling = staticmethod(lambda P, vocab: False)
        got = [model(uniforms=u, **args, **kw).clone() for _ in range(2)]
    finally:
        Engine._fused_sampling = keep
    assert len(model.engine._decode_sessions) == 0
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    model.engine.close()
