"""Soft pseudo-labels through the self-training plumbing on the tiny fp32 model ("Soft pseudo-labels"):
generate_dialogs(soft_top_k=4) -> dialog_train_batch -> step.forward.  The alignment rule is restated here in plain Python loops
over host copies and compared with what the device decided."""
import pytest
import torch

from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, ROUNDS, MAXLEN, UD, K = 40, 3, 4, 8, 4
LENS = (10, 14, 19)
QK = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=4, max_seq_len=MAXLEN)
AK = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=0, max_seq_len=MAXLEN)
CLS, SEP, UNK = 101, 102, 100


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def fresh_state(seed=0):
    g = load_npz("tiny_train.npz")
    kw = sc().golden_batch(g, DEV)
    B = kw["enc_input_ids"].shape[0]
    gen = torch.Generator().manual_seed(seed)
    ids = torch.zeros(B, T, dtype=torch.long)
    seg = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(LENS):
        ids[b, :n] = torch.randint(104, 320, (n,), generator=gen)
        ids[b, 0], ids[b, n - 1], seg[b, :n] = CLS, SEP, 1
    return dict(enc_image_features=kw["enc_image_features"], enc_image_spatials=kw["enc_image_spatials"],
                enc_image_mask=kw["enc_image_mask"], enc_input_ids=ids.to(DEV), enc_segments=seg.to(DEV),
                enc_input_len=(ids != 0).sum(-1).to(DEV), dec_input_ids=torch.full((B, 1), CLS, dtype=torch.long, device=DEV),
                dec_attention_mask=torch.ones(B, 1, device=DEV))


def generate(model, state, soft_top_k):
    from gst_visdial_amd.selftrain import generate_dialogs
    gen = torch.Generator().manual_seed(5)
    u = torch.rand(2, ROUNDS, MAXLEN, 3, generator=gen).clamp_(1e-6, 1 - 1e-6).to(DEV)
    return generate_dialogs(model, model, state, num_rounds=ROUNDS, q_kwargs=QK, a_kwargs=AK, q_uniforms=u[0], a_uniforms=u[1],
                            soft_top_k=soft_top_k)


@pytest.fixture(scope="module")
def generated():
    model, params, cfg = sc().build_tiny_model("fp32", DEV, mode="cc12m_gen", state_file="tiny_state_trained.npz")
    model.eval()
    params["amd_decode_graph"] = False
    state = fresh_state()
    soft = generate(model, state, K)
    plain = generate(model, fresh_state(), None)
    model.engine.close()
    return state, soft, plain


def caption():
    gen = torch.Generator().manual_seed(3)
    cap = torch.zeros(3, 12, dtype=torch.long)
    for b, n in enumerate((12, 5, 8)):
        cap[b, :n] = torch.randint(104, 320, (n,), generator=gen)
    return cap.to(DEV)


TP = dict(select_data=0, threshold=0.0, mask_prob=0.0, max_seq_len=T, max_utt_len=UD)


def expected_use(soft_tgt, dec_labels):
    """The alignment rule in loops: [B, R] bool."""
    B, R, Ud = dec_labels.shape
    Ut = soft_tgt.shape[-1]
    use = torch.zeros(B, R, dtype=torch.bool)
    for b in range(B):
        for r in range(R):
            ok = True
            for i in range(Ud):
                lab = int(dec_labels[b, r, i])
                if lab != 0 and (i >= Ut or int(soft_tgt[b, r, i]) != lab):
                    ok = False
            use[b, r] = ok
    return use


def check_batch(dialogs, batch):
    """dec_soft_* of `batch` against the rule -> the [B, R] bool of rows that carry soft labels."""
    lab = batch["dec_labels"][:, :, 0].cpu()
    sid, slp = batch["dec_soft_ids"][:, :, 0].cpu(), batch["dec_soft_logp"][:, :, 0].cpu()
    assert sid.shape == slp.shape == (3, ROUNDS, UD, K) and sid.dtype == torch.int64 and slp.dtype == torch.float32
    use = expected_use(dialogs["soft_tgt"].cpu(), lab)
    tid, tlp = dialogs["soft_ids"].cpu(), dialogs["soft_logp"].cpu()
    for b in range(3):
        for r in range(ROUNDS):
            if use[b, r]:
                assert torch.equal(sid[b, r, :MAXLEN], tid[b, r]) and torch.equal(slp[b, r, :MAXLEN], tlp[b, r]), (b, r)
            else:
                assert bool((sid[b, r, :MAXLEN] == -1).all()) and bool((slp[b, r, :MAXLEN] == 0).all()), (b, r)
            assert bool((sid[b, r, MAXLEN:] == -1).all()) and bool((slp[b, r, MAXLEN:] == 0).all()), (b, r)
    return use


def test_generation_with_soft_top_k_adds_the_teachers_distributions_and_changes_nothing_else(generated):
    state, soft, plain = generated
    for k in plain:
        assert torch.equal(soft[k], plain[k]), k
    assert set(soft) - set(plain) == {"soft_ids", "soft_logp", "soft_tgt"}
    assert soft["soft_ids"].shape == soft["soft_logp"].shape == (3, ROUNDS, MAXLEN, K) and soft["soft_tgt"].shape == (3, ROUNDS, MAXLEN)
    assert bool(((soft["soft_ids"] >= 0) & (soft["soft_ids"] < 320)).all())
    lp = soft["soft_logp"]
    assert bool((lp <= 0).all()) and bool((lp[..., :-1] >= lp[..., 1:]).all())           # log-probabilities, best first
    # the labels of the scoring pass: the answer's tokens behind [CLS], then the [SEP] the pass replaced by [PAD]
    ans = soft["answers"]
    assert torch.equal(torch.where(soft["soft_tgt"][..., :-1] == SEP, torch.zeros_like(ans[..., 1:]), soft["soft_tgt"][..., :-1]), ans[..., 1:])


def test_used_rows_satisfy_the_alignment_rule(generated):
    from gst_visdial_amd.selftrain import dialog_train_batch
    state, soft, plain = generated
    batch = dialog_train_batch(soft, caption(), state, TP)
    use = check_batch(soft, batch)
    # (measured: 0 of 9 -- no answer of the tiny models ends in a sampled [SEP] within 4 tokens, so every row fails the rule at the
    # student's [SEP]; rows that pass it are made by hand in the next test)
    print("rows with soft labels: %d of %d" % (int(use.sum()), use.numel()))
    assert "dec_soft_ids" not in dialog_train_batch(plain, caption(), state, TP)


def test_a_forced_special_id_costs_exactly_its_row_and_the_batch_trains(generated):
    from gst_visdial_amd import step
    from gst_visdial_amd.selftrain import dialog_train_batch
    state, soft, plain = generated
    d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in soft.items()}
    # two hand-aligned rows: the answer "[CLS] t [PAD] [PAD]" as the scoring pass leaves it, scored against "t [SEP]"
    for b, r, t in ((0, 1, 150), (2, 0, 200)):
        d["answers"][b, r] = torch.tensor([CLS, t, 0, 0], device=DEV)
        d["soft_tgt"][b, r] = torch.tensor([t, SEP, 0, 0], device=DEV)
    d["abnormal"] = torch.zeros_like(d["abnormal"])
    base = check_batch(d, dialog_train_batch(d, caption(), state, TP))
    assert bool(base[0, 1]) and bool(base[2, 0])
    d["answers"][0, 1] = torch.tensor([CLS, UNK, 150, 0], device=DEV)         # a special id inside the answer: the target drops it
    d["soft_tgt"][0, 1] = torch.tensor([UNK, 150, SEP, 0], device=DEV)
    batch = dialog_train_batch(d, caption(), state, TP)
    forced = check_batch(d, batch)
    want = base.clone()
    want[0, 1] = False
    assert torch.equal(forced, want)                                          # that row lost its soft labels, and nothing else did
    student, sp, _ = sc().build_tiny_model("fp32", DEV, mode="vd_train", seed=1)
    student.eval()                                                            # (no dropout: the two losses below differ by the soft labels alone)
    idx = torch.tensor([1, 6, 2])                                             # rows (0, 1), (2, 0), (0, 2)
    loss, _ = step.forward(student, batch, sp, sample_indices=idx, distill_alpha=0.5, distill_temperature=2.0)
    assert torch.isfinite(loss)
    loss.backward()
    hard, _ = step.forward(student, {k: v for k, v in batch.items() if not k.startswith("dec_soft")}, sp, sample_indices=idx)
    assert torch.isfinite(hard) and hard.item() != loss.item()                # row (2, 0) carries a soft label: another loss
    student.train()
    loss2, _ = step.forward(student, batch, sp)                               # rows drawn on the device
    assert torch.isfinite(loss2)
