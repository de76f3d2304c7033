"""Sample-and-rank decoding (Engine.sample_ranked, model(num_samples=S)) on the tiny golden model: the sampling path is untouched,
S = 1 is `sample`, the reported token log-probabilities are the model's own (teacher-forced), the S rows of a dialog are independent
and read their dialog's encoder row, graph replay equals eager issue, the ranking follows the stated rule, the decode state serves
the perplexity re-score, and the module surface returns the best sample.

Fixtures: the golden batch (3 dialogs: 24 / 17 / 11 context tokens, 7 / 7 / 5 image regions -- ragged and image-padded) with the
golden weights, and the trained tiny checkpoint (peaked distributions: answers end with [SEP]) where the ranking needs ends."""
import pytest
import torch

from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS, PAD, CLS, STEPS = 102, 0, 101, 18
TRAINED = "tiny_state_trained.npz"
ARGS = dict(temperature=1.3, top_k=40, top_p=0.0, ngram_blocking_size=0)
LOGIT_BAR = 1e-4                      # the project's fp32 logit parity bar; a log-probability of fp32 logits is held to it as well
# max |teacher-forced fp32 loss + bf16 token_logp| over the 2 x 3 x 18 sampled positions of test_bf16_..., as measured on the MI355X
# (DESIGN.md section 8); the test asserts twice this value
BF16_MEASURED = 3.123e-3


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def batch(g, dev=DEV, rows=None, shift=0):
    kw = sc().golden_batch(g, dev)
    kw["dec_input_ids"] = torch.full((kw["enc_input_ids"].shape[0], 1), CLS, dtype=torch.long, device=dev)
    kw.pop("dec_attention_mask"), kw.pop("dec_labels")
    if shift:
        ids = kw["enc_input_ids"]
        kw["enc_input_ids"] = torch.where(ids > 110, (ids - 111 + shift) % 200 + 111, ids)
    if rows is not None:
        kw = {k: v[rows].contiguous() for k, v in kw.items()}
    return kw


def uniforms(seed, cols):
    return torch.rand(STEPS, cols, generator=torch.Generator().manual_seed(seed)).clamp_(1e-6, 1 - 1e-6).to(DEV)


def build(precision="fp32", graph=True, state=None, mode="vd_gen_val"):
    model, params, _ = sc().build_tiny_model(precision, DEV, mode=mode, **({"state_file": state} if state else {}))
    params["amd_decode_graph"] = graph
    return model.eval()


@pytest.fixture(scope="module")
def eager_model():
    """fp32, golden weights, no captured graphs: every call issues eagerly."""
    return build(graph=False)


def inside_of(seqs):
    eq = (seqs == EOS).long()
    return (eq.cumsum(-1) - eq) == 0


def teacher_forced(model, kw, seqs):
    """Per-token losses [B, S, STEPS] of every sample from the teacher-forced eval forward (loss_reduction=False): [CLS] + the sampled
    ids against the dialog's own encoder inputs, one decoder row per sample.  That forward ignores [PAD] labels (loss 0); where a
    [PAD] was SAMPLED the loss is taken from the same forward's logits instead (float64 log_softmax)."""
    B, S, L = seqs.shape
    dec = torch.cat((torch.full((B * S, 1), CLS, dtype=torch.long, device=seqs.device), seqs.reshape(B * S, L)), 1)
    enc = {k: v.repeat_interleave(S, 0) for k, v in kw.items() if k.startswith("enc_")}
    params = model.params
    mode = params["mode"]
    params["mode"] = "vd_eval_val"
    try:
        loss, logits = model(dec_input_ids=dec, dec_attention_mask=torch.ones_like(dec).float(), loss_reduction=False, **enc)
        loss = loss.float().reshape(B, S, L + 1)[:, :, :L].clone()
        logits = logits.double().reshape(B, S, L + 1, -1)[:, :, :L]
    finally:
        params["mode"] = mode
    own = -torch.log_softmax(logits, -1).gather(3, seqs[..., None])[..., 0].float()
    return torch.where(seqs == PAD, own, loss)


# ------------------------------------------------------------------------------------------------ sample() is untouched
def test_sample_before_and_after_a_ranked_call_returns_the_same_ids():
    g = load_npz("tiny_train.npz")
    kw, u, u3 = batch(g), uniforms(1, 3), uniforms(2, 9)
    args = dict(ARGS, ngram_blocking_size=2)
    for graph in (False, True):
        model = build(graph=graph)
        a0 = model(uniforms=u, **args, **kw).clone()                           # eager (graph: then captured)
        a1 = model(uniforms=u, **args, **kw).clone()                           # graph: replay
        r0 = model.sample_ranked(num_samples=3, uniforms=u3, **args, **kw)
        a2 = model(uniforms=u, **args, **kw).clone()
        r1 = model.sample_ranked(num_samples=3, uniforms=u3, **args, **kw)     # graph: replay
        a3 = model(uniforms=u, **args, **kw).clone()
        assert torch.equal(a0, a1) and torch.equal(a0, a2) and torch.equal(a0, a3), graph
        assert torch.equal(r0[0], r1[0]) and torch.equal(r0[2], r1[2]), graph
        assert len(model.engine._decode_sessions) == (2 if graph else 0)
        model.engine.close()


@pytest.mark.parametrize("ngram", [0, 2])
def test_one_sample_is_sample(eager_model, ngram):
    g = load_npz("tiny_train.npz")
    kw, u = batch(g), uniforms(3, 3)
    args = dict(ARGS, ngram_blocking_size=ngram)
    want = eager_model(uniforms=u, **args, **kw)
    calls = eager_model.engine.decode_lib_calls_per_token
    seqs, scores, tl = eager_model.sample_ranked(num_samples=1, uniforms=u, **args, **kw)
    assert tuple(seqs.shape) == (3, 1, STEPS) and seqs.dtype == torch.long and torch.equal(seqs[:, 0], want)
    assert tuple(scores.shape) == (3, 1) and tuple(tl.shape) == (3, 1, STEPS) and scores.dtype == tl.dtype == torch.float32
    assert eager_model.engine.decode_lib_calls_per_token == calls              # one launch per token for draw AND score


# ------------------------------------------------------------------------------------------------ the log-probabilities
def test_token_logp_is_the_teacher_forced_log_likelihood_fp32(eager_model):
    """S = 3 rows over B = 2 dialogs of different context length and region count: a wrong cache row, or a cross-attention that read
    another dialog's encoder row (kv_group), changes the logits by far more than the bar."""
    g = load_npz("tiny_train.npz")
    kw = batch(g, rows=slice(1, 3))
    assert kw["enc_attention_mask"].sum(1).tolist() == [17.0, 11.0] and kw["enc_image_mask"].sum(1).tolist() == [7.0, 5.0]
    seqs, scores, tl = eager_model.sample_ranked(num_samples=3, uniforms=uniforms(4, 6), **ARGS, **kw)
    inside = inside_of(seqs)
    loss = teacher_forced(eager_model, kw, seqs)
    err = ((loss + tl).abs() * inside).max().item()
    print("fp32: max |teacher-forced loss + token_logp| = %.3e over %d positions" % (err, int(inside.sum())))
    assert err < LOGIT_BAR
    assert bool((tl[~inside] == 0).all()) and bool((tl[inside] < 0).all())


def test_token_logp_bf16_within_twice_the_measured_error(eager_model):
    g = load_npz("tiny_train.npz")
    kw = batch(g, rows=slice(1, 3))
    model = build("bf16", graph=False)
    seqs, scores, tl = model.sample_ranked(num_samples=3, uniforms=uniforms(4, 6), **ARGS, **kw)
    inside = inside_of(seqs)
    loss = teacher_forced(eager_model, kw, seqs)                               # the fp32 model on the bf16 run's ids
    err = ((loss + tl).abs() * inside).max().item()
    print("bf16: max |fp32 teacher-forced loss + bf16 token_logp| = %.3e over %d positions" % (err, int(inside.sum())))
    assert err <= 2 * BF16_MEASURED
    model.engine.close()


# ------------------------------------------------------------------------------------------------ rows and groups
def test_rows_are_independent_and_grouped_by_dialog(eager_model):
    g = load_npz("tiny_train.npz")
    kw = batch(g)
    B, S = 3, 3
    ARGS = dict(globals()["ARGS"], ngram_blocking_size=1)                      # (every ordinary token of the dialog's OWN context is banned)
    # the S columns of a dialog share their uniforms: S identical samples, bit-identical log-probabilities, order 0, 1, 2 (a tie)
    u1 = uniforms(5, B)
    same = u1[:, :, None].expand(STEPS, B, S).reshape(STEPS, B * S).contiguous()
    seqs, scores, tl = eager_model.sample_ranked(num_samples=S, uniforms=same, **ARGS, **kw)
    for j in range(1, S):
        assert torch.equal(seqs[:, j], seqs[:, 0]) and torch.equal(tl[:, j].view(torch.int32), tl[:, 0].view(torch.int32))
        assert torch.equal(scores[:, j], scores[:, 0])
    assert eager_model.engine.last["sample_order"].tolist() == [[0, 1, 2]] * B
    plain = eager_model(uniforms=u1, **ARGS, **kw)
    assert torch.equal(seqs[:, 0], plain)                                      # ... and each is `sample` under those uniforms
    assert not torch.equal(plain, eager_model(uniforms=u1, **dict(ARGS, ngram_blocking_size=0), **kw))     # (the filter acts here)
    # different uniforms: the samples of a dialog differ (fixture and seed chosen so; asserted)
    u = uniforms(6, B * S)
    seqs, scores, tl = eager_model.sample_ranked(num_samples=S, uniforms=u, **ARGS, **kw)
    assert any(not torch.equal(seqs[b, 0], seqs[b, 1]) for b in range(B))
    assert len(set(tuple(r) for r in seqs.reshape(B * S, STEPS).tolist())) > B
    # permuting the dialogs (and their uniform columns) permutes the outputs
    perm = torch.tensor([2, 0, 1], device=DEV)
    kwp = {k: v[perm].contiguous() for k, v in kw.items()}
    up = u.view(STEPS, B, S)[:, perm].reshape(STEPS, B * S).contiguous()
    seqs_p, scores_p, tl_p = eager_model.sample_ranked(num_samples=S, uniforms=up, **ARGS, **kwp)
    assert torch.equal(seqs_p, seqs[perm])
    assert (tl_p - tl[perm]).abs().max().item() < LOGIT_BAR and (scores_p - scores[perm]).abs().max().item() < LOGIT_BAR


# ------------------------------------------------------------------------------------------------ replay
def test_graph_replay_reproduces_the_eager_call():
    g = load_npz("tiny_train.npz")
    kw, u, u2 = batch(g), uniforms(7, 12), uniforms(8, 12)
    args = dict(ARGS, ngram_blocking_size=2)
    model = build(graph=True)
    first = model.sample_ranked(num_samples=4, uniforms=u, **args, **kw)       # eager, then captures
    assert len(model.engine._decode_sessions) == 1
    for _ in range(2):                                                         # replays
        again = model.sample_ranked(num_samples=4, uniforms=u, **args, **kw)
        assert torch.equal(again[0], first[0]) and torch.equal(again[2].view(torch.int32), first[2].view(torch.int32))
        assert torch.equal(again[1], first[1])
    other = model.sample_ranked(num_samples=4, uniforms=u2, **args, **kw)      # new uniforms through `refresh`
    assert not torch.equal(other[0], first[0]) and not torch.equal(other[2], first[2])
    moved = model.sample_ranked(num_samples=4, uniforms=u, **args, **batch(g, shift=17))   # new inputs through `refresh`
    assert not torch.equal(moved[2], first[2])
    ref = build(graph=False)
    want = ref.sample_ranked(num_samples=4, uniforms=u2, **args, **kw)
    assert torch.equal(other[0], want[0]) and torch.equal(other[2].view(torch.int32), want[2].view(torch.int32))
    assert len(model.engine._decode_sessions) == 1
    model.sample_ranked(num_samples=2, uniforms=u[:, :6].contiguous(), **args, **kw)      # another S: another session
    assert len(model.engine._decode_sessions) == 2
    model.engine.close()


# ------------------------------------------------------------------------------------------------ ranking
def test_scores_order_and_padding_follow_the_rule():
    g = load_npz("tiny_train.npz")
    kw, u = batch(g), uniforms(9, 15)
    model = build(graph=False, state=TRAINED)
    args = dict(temperature=1.0, top_k=10, top_p=0.0, ngram_blocking_size=0)
    by_lp = {}
    for lp in (0.0, 1.0, 2.0):
        seqs, scores, tl = model.sample_ranked(num_samples=5, length_penalty=lp, uniforms=u, **args, **kw)
        order = model.engine.last["sample_order"]
        inside = inside_of(seqs)
        length = inside.sum(2)
        assert bool((seqs[~inside] == PAD).all()) and bool((tl[~inside] == 0).all())       # PAD follows EOS, token_logp 0 there
        want = tl.sum(2) / length.float().pow(lp)
        assert torch.allclose(scores, want, rtol=1e-6, atol=0), lp
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())                                # best first
        tie = scores[:, :-1] == scores[:, 1:]
        assert bool((order[:, :-1] < order[:, 1:])[tie].all())                              # ties to the smaller sample index
        assert sorted(order[0].tolist()) == list(range(5))
        by_lp[lp] = (seqs, order, length)
    seqs0, order0, length0 = by_lp[0.0]
    assert bool((seqs0 == EOS).any()) and len(set(length0.reshape(-1).tolist())) > 1      # answers end, at different lengths
    for lp in (1.0, 2.0):                                                                   # the same samples, re-ranked
        seqs, order, _ = by_lp[lp]
        back0 = torch.empty_like(seqs0).scatter_(1, order0[:, :, None].expand_as(seqs0), seqs0)
        back = torch.empty_like(seqs).scatter_(1, order[:, :, None].expand_as(seqs), seqs)
        assert torch.equal(back0, back)
    model.engine.close()


# ------------------------------------------------------------------------------------------------ decode state
def test_decode_state_serves_the_perplexity_rescore_of_the_best_answers():
    from gst_visdial_amd._lib import GstvdError
    from gst_visdial_amd.generate import answer_perplexity
    g = load_npz("tiny_train.npz")
    kw, u = batch(g), uniforms(10, 9)
    enc_kw = {k: v for k, v in kw.items() if k.startswith("enc_")}
    for graph in (False, True):
        model = build(graph=graph, mode="cc12m_gen")
        if graph:
            model.sample_ranked(num_samples=3, uniforms=u, **ARGS, **kw)       # first call captures
        best = model.sample_ranked(num_samples=3, uniforms=u, **ARGS, **kw)[0][:, 0].contiguous()
        ans = best.clone()
        ppl_fast, len_fast = answer_perplexity(model, enc_kw, ans, reuse_decode_state=True)
        ans2 = best.clone()
        ppl_full, len_full = answer_perplexity(model, enc_kw, ans2, reuse_decode_state=False)
        assert torch.equal(ans, ans2) and torch.equal(len_fast, len_full)
        assert (ppl_fast - ppl_full).abs().max().item() <= 1e-4 * ppl_full.max().item()    # (the bar of the same check after sample())
        model.sample_ranked(num_samples=3, uniforms=u, **ARGS, **kw)
        model.engine.rescore_sampled(best.clone())
        with pytest.raises(GstvdError, match="no decode state"):               # the state is single use, as after sample()
            model.engine.rescore_sampled(best.clone())
        model.engine.close()


# ------------------------------------------------------------------------------------------------ module surface
def test_forward_with_num_samples_returns_the_best_sample(eager_model):
    g = load_npz("tiny_train.npz")
    kw, u = batch(g), uniforms(11, 9)
    out = eager_model(num_samples=3, uniforms=u, **ARGS, **kw)
    seqs, _, _ = eager_model.sample_ranked(num_samples=3, uniforms=u, **ARGS, **kw)
    assert out.dtype == torch.long and tuple(out.shape) == (3, STEPS) and torch.equal(out, seqs[:, 0])
    one = eager_model(num_samples=1, uniforms=u[:, :3].contiguous(), **ARGS, **kw)                  # S = 1: the sampling branch
    assert torch.equal(one, eager_model(uniforms=u[:, :3].contiguous(), **ARGS, **kw))
    # greedy under the n-gram filter: every sample of a dialog is the S = 1 answer (the filter of row b*S + j reads dialog b's history)
    greedy = dict(temperature=0.7, top_k=1, top_p=0.0, ngram_blocking_size=4)
    q1 = eager_model(**greedy, **kw)
    q2 = eager_model(num_samples=2, **greedy, **kw)
    assert torch.equal(q1, q2)
    both = eager_model.sample_ranked(num_samples=2, **greedy, **kw)[0]
    assert torch.equal(both[:, 0], q1) and torch.equal(both[:, 1], q1)


def test_dialog_round_runs_with_num_samples():
    from gst_visdial_amd.generate import dialog_round
    g = load_npz("tiny_train.npz")
    model = build(graph=True, mode="cc12m_gen")
    kw = sc().golden_batch(g, DEV)
    B, T = kw["enc_input_ids"].shape

    def fresh_state():
        ids = kw["enc_input_ids"].clone()
        ids[:, T // 2:] = 0
        seg = kw["enc_segments"].clone() * (ids != 0)
        return dict(enc_image_features=kw["enc_image_features"], enc_image_spatials=kw["enc_image_spatials"],
                    enc_image_mask=kw["enc_image_mask"], enc_input_ids=ids, enc_segments=seg, enc_input_len=(ids != 0).sum(-1),
                    dec_input_ids=torch.full((B, 1), CLS, dtype=torch.long, device=DEV), dec_attention_mask=torch.ones(B, 1, device=DEV))

    q_kwargs = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=4, num_samples=2)
    a_kwargs = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=0, num_samples=3)
    for _ in range(2):                                                         # eager, then replayed
        state = fresh_state()
        len0 = state["enc_input_len"].clone()
        torch.manual_seed(0)
        ques, ans, ppl, bad = dialog_round(model, model, state, q_kwargs=q_kwargs, a_kwargs=a_kwargs)
        assert ques.shape == ans.shape == (B, STEPS) and ques.dtype == ans.dtype == torch.long
        assert ppl.shape == (B,) and torch.isfinite(ppl).all() and (ppl > 1).all()
        assert (state["enc_input_len"] > len0).all()
    model.engine.close()
