"""gst_visdial_amd.selftrain on the tiny fp32 model of tests/golden: whole-dialog generation against a loop of `dialog_round`,
graph replay, the context-full error after the loop, and the generated batch through the existing step driver."""
import pytest
import torch

from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, ROUNDS, MAXLEN = 40, 3, 4
# the last row is nearly full: 21 free slots for six utterances of up to 4 tokens, the least that can never run into "context
# already full".  (Under the uniforms below it ends at exactly T = 40; the lone-[SEP] and full rows are pinned by the exact tests.)
LENS = (10, 14, 19)


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def gen_model(graph):
    model, params, cfg = sc().build_tiny_model("fp32", DEV, mode="cc12m_gen")
    model.eval()
    params["amd_decode_graph"] = graph
    return model, params


def fresh_state(lens=LENS, seed=0):
    g = load_npz("tiny_train.npz")
    kw = sc().golden_batch(g, DEV)
    B = kw["enc_input_ids"].shape[0]
    gen = torch.Generator().manual_seed(seed)
    ids = torch.zeros(B, T, dtype=torch.long)
    seg = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(104, 320, (n,), generator=gen)
        ids[b, 0], ids[b, n - 1], seg[b, :n] = 101, 102, 1
    return dict(enc_image_features=kw["enc_image_features"], enc_image_spatials=kw["enc_image_spatials"],
                enc_image_mask=kw["enc_image_mask"], enc_input_ids=ids.to(DEV), enc_segments=seg.to(DEV),
                enc_input_len=(ids != 0).sum(-1).to(DEV), dec_input_ids=torch.full((B, 1), 101, dtype=torch.long, device=DEV),
                dec_attention_mask=torch.ones(B, 1, device=DEV))


def uniforms(B=3, seed=5):
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(2, ROUNDS, MAXLEN, B, generator=gen).clamp_(1e-6, 1 - 1e-6).to(DEV)
    return u[0], u[1]


QK = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=4, max_seq_len=MAXLEN)
AK = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=0, max_seq_len=MAXLEN)


def generate(model, state, rounds=ROUNDS):
    from gst_visdial_amd.selftrain import generate_dialogs
    qu, au = uniforms()
    return generate_dialogs(model, model, state, num_rounds=rounds, q_kwargs=QK, a_kwargs=AK, q_uniforms=qu, a_uniforms=au)


@pytest.mark.isolated
def test_generate_dialogs_equals_a_loop_of_dialog_round():
    from gst_visdial_amd.generate import dialog_round
    model, params = gen_model(graph=False)
    state = fresh_state()
    out = generate(model, state)
    ref = fresh_state()
    qu, au = uniforms()
    qs, as_, ppls, bad = [], [], [], set()
    for r in range(ROUNDS):
        q, a, p, b = dialog_round(model, model, ref, q_kwargs=dict(QK, uniforms=qu[r]), a_kwargs=dict(AK, uniforms=au[r]))
        qs.append(q), as_.append(a), ppls.append(p), bad.update(b.tolist())
    B = ref["enc_input_ids"].shape[0]
    assert out["questions"].shape == out["answers"].shape == (B, ROUNDS, MAXLEN) and out["ppl"].shape == (B, ROUNDS)
    assert torch.equal(out["questions"], torch.stack(qs, 1)) and torch.equal(out["answers"], torch.stack(as_, 1))
    assert not bool((out["answers"] == 102).any())                         # as the perplexity pass left them: [SEP] -> [PAD]
    for k in ("enc_input_ids", "enc_segments", "enc_input_len"):
        assert torch.equal(out[k], ref[k]) and out[k] is state[k], k        # the caller's tensors, updated in place
    want_bad = torch.zeros(B, dtype=torch.bool)
    want_bad[sorted(bad)] = True
    print("context lengths %s, abnormal rows %s" % (out["enc_input_len"].tolist(), sorted(bad)))
    assert out["abnormal"].dtype == torch.bool and torch.equal(out["abnormal"].cpu(), want_bad)
    ref_ppl = torch.stack(ppls, 1)
    assert torch.isfinite(out["ppl"]).all() and out["ppl"].dtype == torch.float32
    assert (out["ppl"] - ref_ppl).abs().max().item() <= 1e-3 * ref_ppl.max().item()
    assert torch.equal((out["enc_input_ids"] != 0).sum(-1), out["enc_input_len"]) and bool((out["enc_input_len"] <= T).all())


@pytest.mark.isolated
def test_generate_dialogs_replays_captured_decode_graphs():
    from gst_visdial_amd import _lib
    model, params = gen_model(graph=True)
    n0 = _lib.N_CALLS[0]
    first = generate(model, fresh_state())
    n1 = _lib.N_CALLS[0]
    sessions = set(model.engine._decode_sessions)
    assert len(sessions) == 2                                               # the questioner's and the answerer's sampling settings
    state = fresh_state()
    out = generate(model, state)
    n2 = _lib.N_CALLS[0]
    assert set(model.engine._decode_sessions) == sessions and (n2 - n1) < (n1 - n0)      # nothing captured anew: every decode replayed
    B = state["enc_input_ids"].shape[0]
    assert out["questions"].shape == out["answers"].shape == (B, ROUNDS, MAXLEN) and out["ppl"].shape == (B, ROUNDS)
    assert torch.isfinite(out["ppl"]).all() and out["abnormal"].shape == (B,)
    assert torch.equal(out["enc_input_len"], (out["enc_input_ids"] != 0).sum(-1))
    for k in ("questions", "answers", "enc_input_ids", "enc_segments", "enc_input_len", "abnormal"):
        assert torch.equal(out[k], first[k]), k                            # same inputs, same uniforms: eager and replay agree


@pytest.mark.isolated
def test_generate_dialogs_raises_after_the_loop_when_a_context_is_full():
    model, params = gen_model(graph=False)
    state = fresh_state(lens=(10, T, 14))
    with pytest.raises(RuntimeError, match="context already full"):
        generate(model, state, rounds=2)
    assert int(state["enc_input_len"][1]) == T                             # the full row was left alone; the loop ran to its end
    assert int(state["enc_input_len"][0]) > 10 and int(state["enc_input_len"][2]) > 14


@pytest.mark.isolated
def test_generated_batch_goes_through_the_step_driver():
    from gst_visdial_amd import step
    from gst_visdial_amd.selftrain import dialog_train_batch
    model, params = gen_model(graph=False)
    state = fresh_state()
    dialogs = generate(model, state)
    B = state["enc_input_ids"].shape[0]
    gen = torch.Generator().manual_seed(3)
    cap = torch.zeros(B, 12, dtype=torch.long)
    for b, n in enumerate((12, 5, 8)):
        cap[b, :n] = torch.randint(104, 320, (n,), generator=gen)
    tp = dict(select_data=1, threshold=float(dialogs["ppl"].median()), mask_prob=0.15, max_seq_len=T, max_utt_len=8)
    batch = dialog_train_batch(dialogs, cap.to(DEV), state, tp)
    regions = state["enc_image_mask"].shape[1]
    assert batch["enc_input_ids"].shape == (B, ROUNDS, 1, T) and batch["dec_labels"].shape == (B, ROUNDS, 1, 8)
    assert batch["enc_image_feat"].shape[:2] == (B, regions) and all(v.is_cuda for v in batch.values())
    assert bool((batch["enc_input_ids"] == 103).any()) and bool((batch["enc_mlm_labels"] >= 0).any())
    zeroed = batch["dec_labels"].reshape(B * ROUNDS, -1).sum(-1) == 0
    assert torch.equal(zeroed.cpu(), (dialogs["ppl"].reshape(-1) >= tp["threshold"]).cpu() | dialogs["abnormal"].cpu().repeat_interleave(ROUNDS))
    student, sp, _ = sc().build_tiny_model("fp32", DEV, mode="vd_train", seed=1)
    # train mode, row candidates and torch.multinomial on the device, then given indices
    student.train()
    loss, _ = step.forward(student, batch, sp)
    assert torch.isfinite(loss)
    idx = torch.nonzero(~zeroed.cpu()).flatten()[:3]
    idx = idx[torch.arange(3) % idx.numel()]
    loss, _ = step.forward(student, batch, sp, sample_indices=idx)
    assert torch.isfinite(loss)
    # eval(): the same rows reach the same launches from the device batch and from its copy on the host
    student.eval()
    with torch.no_grad():
        dev_loss, dev_scores = step.forward(student, batch, sp, sample_indices=idx)
        dev_loss, dev_scores = dev_loss.clone(), dev_scores.clone()
        host_loss, host_scores = step.forward(student, {k: v.cpu() for k, v in batch.items()}, sp, sample_indices=idx)
    assert torch.equal(dev_loss, host_loss) and torch.equal(dev_scores, host_scores)
