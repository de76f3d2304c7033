"""Soft pseudo-labels at model level on a real MI355X ("Soft pseudo-labels"): the tiny fixture model against
tests/golden/tiny_distill.npz (tools/make_golden_distill.py: the reference model's logits, the distillation loss formed in float64,
autograd's gradients) under the project's fp32 bars -- loss 1e-5, every recorded gradient 2e-4 of its tensor's maximum --, alpha = 0
against the plain step bit for bit, the teacher's side (Engine.rescore_sampled / soft_labels with top_k) against torch.topk of the
float64 log_softmax of the logits the call returns, and a step with an attached one-GPU BackwardPipeline."""
import pytest
import torch

from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# bf16 engine against the fp32 fixture, measured on an MI355X (DESIGN.md section 8 records both); the test allows twice that
BF16_LOSS_ERR = 5.4654e-05
BF16_GRAD_ERR = 1.4615e-02


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def maxerr(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().max().item()


def soft_kw(d, dev=DEV, alpha=None, tau=None):
    return dict(dec_soft_ids=d["soft_ids"].to(dev), dec_soft_logp=d["soft_logp"].to(dev),
                distill_alpha=float(d["alpha"]) if alpha is None else alpha, distill_temperature=float(d["tau"]) if tau is None else tau)


def run_step(precision, extra, seed=0, train=False):
    s = sc()
    model, params, cfg = s.build_tiny_model(precision, DEV, seed=seed)
    model.train() if train else model.eval()
    g = load_npz("tiny_train.npz")
    feats = g["in::enc_image_features"].clone().to(DEV).requires_grad_(True)
    kw = s.golden_batch(g, DEV)
    kw["enc_image_features"] = feats
    loss, logits = model(**kw, **extra)
    loss.backward()
    torch.cuda.synchronize()
    return model, loss, logits, feats


@pytest.fixture(scope="module")
def fixture():
    return load_npz("tiny_distill.npz")


@pytest.fixture(scope="module")
def fp32_run(fixture):
    return run_step("fp32", soft_kw(fixture))


def grad_errors(model, d):
    named = dict(model.named_parameters())
    out = {}
    for k in [k for k in d if k.startswith("grad::")]:
        p = named[k[6:]]
        assert p.grad is not None, k
        out[k[6:]] = maxerr(p.grad, d[k]) / max(d[k].abs().max().item(), 1e-3)
    return out


def test_fp32_loss_matches_the_float64_rule_on_the_reference_logits(fp32_run, fixture):
    model, loss, logits, feats = fp32_run
    e = abs(loss.item() - fixture["loss"].item())
    print("distillation loss %.8f, fixture %.8f, error %.3e" % (loss.item(), fixture["loss"].item(), e))
    assert e <= 1e-5
    assert maxerr(logits, load_npz("tiny_train.npz")["logits"]) < 1e-4            # the logits are the plain step's


def test_fp32_gradients_match_autograd_of_the_reference(fp32_run, fixture):
    model, loss, logits, feats = fp32_run
    errs = grad_errors(model, fixture)
    worst = max(errs, key=errs.get)
    print("worst gradient error %.3e of the tensor maximum (%s)" % (errs[worst], worst))
    for k, e in errs.items():
        assert e <= 2e-4, (k, e)
    assert maxerr(feats.grad, fixture["d_feats"]) <= 1e-5 + 2e-4 * fixture["d_feats"].abs().max().item()


# gradients that the backward accumulates with float atomics (csrc/layernorm.hip: the embedding scatters of word, position and
# token-type rows, gstvd_locgrad): the order of their additions is not fixed, so not even two runs of the PLAIN step agree there
ATOMIC = ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
          "token_type_embeddings_extension.weight", "image_location_embeddings.weight")


def test_alpha_zero_is_the_plain_step_bit_for_bit(fixture):
    """Loss, logits, d loss / d image features and every `.grad` whose additions have a fixed order, bit for bit.  The ATOMIC
    tensors are held to 1e-6 of their maximum: a few fp32 roundings of a sum of at most B * T terms taken in another order."""
    plain, l0, lg0, f0 = run_step("fp32", {})
    soft, l1, lg1, f1 = run_step("fp32", soft_kw(fixture, alpha=0.0))
    assert torch.equal(l0.detach().view(torch.int32), l1.detach().view(torch.int32))
    assert torch.equal(lg0, lg1) and torch.equal(f0.grad, f1.grad)
    exact = loose = 0
    for (ka, pa), (kb, pb) in zip(plain.named_parameters(), soft.named_parameters()):
        assert ka == kb and (pa.grad is None) == (pb.grad is None), ka
        if pa.grad is None:
            continue
        if ka.endswith(ATOMIC):
            assert maxerr(pa.grad, pb.grad) <= 1e-6 * pa.grad.abs().max().item(), ka
            loose += 1
        else:
            assert torch.equal(pa.grad.view(torch.int32), pb.grad.view(torch.int32)), ka
            exact += 1
    assert exact > 100 and 1 <= loose <= len(ATOMIC)


def test_a_row_without_soft_labels_and_validation(fixture):
    from gst_visdial_amd._lib import GstvdError
    s = sc()
    model, params, cfg = s.build_tiny_model("fp32", DEV)
    model.eval()
    g = load_npz("tiny_train.npz")
    kw = s.golden_batch(g, DEV)
    sk = soft_kw(fixture)
    with pytest.raises(GstvdError, match="both or neither"):
        model(**kw, dec_soft_ids=sk["dec_soft_ids"])
    with pytest.raises(GstvdError, match="alpha"):
        model(**kw, **dict(sk, distill_alpha=1.5))
    with pytest.raises(GstvdError, match="temperature"):
        model(**kw, **dict(sk, distill_temperature=0.0))
    with pytest.raises(GstvdError, match=r"\[B = 3, U = 9"):
        model(**kw, **dict(sk, dec_soft_ids=sk["dec_soft_ids"][:, :5], dec_soft_logp=sk["dec_soft_logp"][:, :5]))
    with pytest.raises(GstvdError, match="loss_reduction"):
        model(**kw, loss_reduction=False, **sk)
    # no soft label anywhere: the plain loss, bit for bit
    none = dict(sk, dec_soft_ids=torch.full_like(sk["dec_soft_ids"], -1))
    with torch.no_grad():
        l_none, _ = model(**s.golden_batch(g, DEV), **none)
        l_plain, _ = model(**s.golden_batch(g, DEV))
    assert torch.equal(l_none.view(torch.int32), l_plain.view(torch.int32))
    with pytest.raises(GstvdError, match="eval"):                               # the teacher's side refuses a 'train' mode
        model.soft_labels(**s.golden_batch(g, DEV), top_k=4)


def _topk_check(logits, ids, logp, K):
    """ids / logp of the call against torch.topk of float64 log_softmax of the logits it returned: logp within 1e-4; ids equal
    wherever the reference's neighbouring top values are separated by more than that."""
    lp = torch.log_softmax(logits.double(), -1)
    rv, ri = torch.topk(lp, K + 1, dim=-1)
    assert maxerr(logp, rv[..., :K]) <= 1e-4
    sep = (rv[..., :-1] - rv[..., 1:]) > 1e-4                                    # entry k is clear of entry k + 1
    clear = sep.clone()
    clear[..., 1:] &= sep[..., :-1]                                              # ... and of entry k - 1
    assert bool(clear.float().mean() > 0.9)
    assert torch.equal(ids[clear], ri[..., :K][clear])


def test_rescore_sampled_returns_the_top_k_of_its_own_logits():
    s = sc()
    g = load_npz("tiny_train.npz")
    model, params, cfg = s.build_tiny_model("fp32", DEV, mode="cc12m_gen")
    model.eval()
    kw = s.golden_batch(g, DEV)
    kw["dec_input_ids"] = torch.full((3, 1), 101, dtype=torch.long, device=DEV)
    kw["dec_labels"] = None
    torch.manual_seed(5)
    ans = model(temperature=0.7, top_k=7, **kw)
    plain_ids = ans.clone()
    loss, logits, (ids, logp, labels) = model.engine.rescore_sampled(ans, (ans != 0).float(), soft_top_k=4)
    assert ids.shape == (3, ans.shape[1], 4) and ids.dtype == torch.int64 and logp.dtype == torch.float32
    _topk_check(logits, ids, logp, 4)
    want = plain_ids.new_zeros(plain_ids.shape)
    want[:, :-1] = plain_ids[:, 1:]
    assert torch.equal(labels, want)                                            # the labels of the pass: the ids shifted left
    # the same pass without soft_top_k returns exactly what it returned before
    torch.manual_seed(5)
    ans2 = model(temperature=0.7, top_k=7, **kw)
    out = model.engine.rescore_sampled(ans2, (ans2 != 0).float())
    assert len(out) == 2 and torch.equal(out[0], loss) and torch.equal(out[1], logits)
    model.engine.close()


def test_soft_labels_of_teacher_forced_rows():
    s = sc()
    g = load_npz("tiny_train.npz")
    model, params, cfg = s.build_tiny_model("fp32", DEV, mode="vd_eval_val")
    model.eval()
    loss, logits, (ids, logp, labels) = model.soft_labels(**s.golden_batch(g, DEV), top_k=16)
    _topk_check(logits, ids, logp, 16)
    assert torch.equal(labels.cpu(), g["in::dec_labels"]) and maxerr(logits, g["logits"]) < 1e-4
    assert not loss.requires_grad


def test_one_gpu_backward_pipeline_takes_the_same_step(fixture):
    """As tests/test_model_gpu.py compares the pipeline with the two-launch route: three steps, losses and parameters."""
    from gst_visdial_amd.optim import FusedAdamW
    from gst_visdial_amd.pipeline import BackwardPipeline
    s = sc()
    g = load_npz("tiny_train.npz")

    def run(pipelined):
        model, params, cfg = s.build_tiny_model("fp32", DEV, seed=11)
        model.train()
        kw = dict(s.golden_batch(g, DEV), **soft_kw(fixture))
        opt = FusedAdamW(model, lr=1e-3)
        pipe = BackwardPipeline(model.engine, optimizer=opt, chunk_elems=100000) if pipelined else None
        losses = []
        for _ in range(3):
            loss, _ = model(**kw)
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.item())
        assert pipe is None or len(pipe.slices) >= 3
        torch.cuda.synchronize()
        return losses, model.engine.flat.P.clone()

    l0, p0 = run(False)
    l1, p1 = run(True)
    for a, b in zip(l0, l1):
        assert abs(a - b) < 1e-4 * max(1.0, abs(a)), (l0, l1)
    assert maxerr(p0, p1) < 1e-5


def test_inputs_only_returns_the_feature_gradient_of_the_full_replay(fp32_run, fixture):
    s = sc()
    model, params, cfg = s.build_tiny_model("fp32", DEV)
    model.eval()
    g = load_npz("tiny_train.npz")
    feats = g["in::enc_image_features"].clone().to(DEV).requires_grad_(True)
    kw = s.golden_batch(g, DEV)
    kw["enc_image_features"] = feats
    with model.inputs_only():
        loss, _ = model(**kw, **soft_kw(fixture))
        loss.backward()
    assert torch.equal(feats.grad, fp32_run[3].grad)
    assert all(p.grad is None for p in model.parameters())


def test_bf16_engine_against_the_fp32_fixture(fixture):
    model, loss, logits, feats = run_step("bf16", soft_kw(fixture))
    le = abs(loss.item() - fixture["loss"].item())
    errs = grad_errors(model, fixture)
    worst = max(errs, key=errs.get)
    print("bf16: loss error %.4e, worst gradient error %.4e of the tensor maximum (%s)" % (le, errs[worst], worst))
    assert le <= 2 * BF16_LOSS_ERR and errs[worst] <= 2 * BF16_GRAD_ERR
