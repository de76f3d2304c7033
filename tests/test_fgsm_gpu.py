"""FGSM attack evaluation on a real MI355X: the two kernels against PyTorch, the per-token backward and the inputs-only replay
against tests/golden/tiny_fgsm.npz (what the reference's evaluate_gen_attack.py:101-148 computes on the tiny model), and the
public functions of gst_visdial_amd/attack.py.  Gates: fp32 gradients 2e-4 of the tensor maximum, logits 1e-4, scores 1e-3, ranks
exact; bf16 gradients 3e-2 of the tensor maximum (the project's gates)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.autograd import Variable

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ops():
    from gst_visdial_amd import ops as o
    return o


def op_tol(dtype):
    return (2e-5 if dtype == torch.float32 else 1.2e-2) * 2.0         # tests/test_ops_gpu.py: check("ce_dlogits", ..., dtype, 2.0)


# ------------------------------------------------------------------------------------------ kernels
def _ce_case(V, dtype, seed):
    M, Vp = 7, (V + 63) // 64 * 64
    g = torch.Generator().manual_seed(seed)
    logits = torch.zeros(M, Vp, dtype=dtype, device=DEV)
    logits[:, :V] = (torch.randn(M, V, generator=g) * 2.0).to(DEV).to(dtype)
    labels = torch.randint(1, V, (M,), generator=g)
    labels[3] = 0                                                      # an ignored row with a non-zero upstream gradient
    return M, Vp, logits, labels.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [600, 37])
def test_ce_bwd_rows(V, dtype):
    """gstvd_ce_bwd_rows against autograd of F.cross_entropy(reduction='none'); rows with g == 0 or label 0 and the columns
    V..Vp exactly zero; nothing written past the buffer; with g = 1 / count the mean form of gstvd_ce_bwd to the last bit (the two
    kernels share one row routine and hence the arithmetic order)."""
    o = ops()
    M, Vp, logits, labels = _ce_case(V, dtype, 5 + V)
    upstream = torch.tensor([0.0, -1.5, 1.0e4, 0.7, 0.0, 1.0, 0.25], device=DEV)
    logits[4, 1] = float("inf")              # a g == 0 row whose softmax is inf - inf: it must be stored as zeros, not multiplied
    row_loss, lse, stats = torch.empty(M, device=DEV), torch.empty(M, device=DEV), torch.empty(4, device=DEV)
    o.ce_fwd(logits, labels, M, V, row_loss, lse, stats)
    canary = 64
    store = torch.full((M * Vp + canary,), 7.0, dtype=dtype, device=DEV)
    dl = store[:M * Vp].view(M, Vp)
    dl.fill_(float("nan"))
    o.ce_bwd_rows(logits, labels, lse, upstream, M, V, dl)
    torch.cuda.synchronize()
    assert bool((store[M * Vp:] == 7.0).all()), "write past the buffer"
    assert bool((dl[:, V:] == 0).all())
    for r in (0, 3, 4):
        assert bool((dl[r] == 0).all()), "row %d (g == 0 or label 0) is not exactly zero" % r
    ok = [1, 2, 5, 6]
    lr = logits[ok, :V].float().requires_grad_(True)
    F.cross_entropy(lr, labels[ok], ignore_index=0, reduction="none").backward(upstream[ok])
    for i, r in enumerate(ok):
        scale = lr.grad[i].abs().max().item()
        err = (dl[r, :V].float() - lr.grad[i]).abs().max().item() / scale
        print("ce_bwd_rows V=%d %s row %d: error %.3e of the row maximum %.3e" % (V, dtype, r, err, scale))
        assert torch.isfinite(dl[r]).all() and err <= op_tol(dtype), (r, err)
    # the mean form
    logits[4, 1] = 0.0
    o.ce_fwd(logits, labels, M, V, row_loss, lse, stats)
    count = int((labels != 0).sum())
    assert stats[1].item() == count
    gmean = torch.full((M,), float(np.float32(1.0) / np.float32(count)), device=DEV)
    a, b = torch.full((M, Vp), float("nan"), dtype=dtype, device=DEV), torch.full((M, Vp), float("nan"), dtype=dtype, device=DEV)
    o.ce_bwd_rows(logits, labels, lse, gmean, M, V, a)
    o.ce_bwd(logits, labels, lse, stats, None, True, M, V, b)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("n", [1, 1027])
def test_fgsm_step(n):
    """gstvd_fgsm_step bit-equal to x + eps * torch.sign(g) (computed on the host: IEEE fp32, no denormal flushing), with +0, -0,
    denormals of both signs and +-inf among the gradients; also with out aliased to x."""
    o = ops()
    gen = torch.Generator().manual_seed(n)
    x, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    special = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, float("inf"), float("-inf")]
    if n >= len(special):
        g[3:3 + len(special)] = torch.tensor(special)
        g[n - 1] = -0.0
        x[3] = -0.0
        assert g[5] != 0 and g[5].abs() < 1.2e-38                       # really denormal
    else:
        g[0] = -1e-45
    for eps in (1.0, 0.1):
        want = x + eps * torch.sign(g)
        xd, gd = x.to(DEV), g.to(DEV)
        got = o.fgsm_step(xd, gd, eps)
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
        assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))
        assert o.fgsm_step(xd, gd, eps, out=xd) is xd
        assert torch.equal(xd.cpu().view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------ engine + attack.py
@pytest.fixture(scope="module")
def fx():
    from gst_visdial_amd.selfcheck import load_npz
    return load_npz("tiny_fgsm.npz")


def build(precision, **kw):
    from gst_visdial_amd.selfcheck import build_tiny_model
    model, params, _ = build_tiny_model(precision, DEV, mode="vd_eval_val", **kw)
    model.eval()
    return model, params


@pytest.fixture(scope="module")
def fp32_model():
    return build("fp32")[0]


def kwargs_of(fx, device=DEV):
    from gst_visdial_amd.attack import _MODEL_KEYS
    kw = dict.fromkeys(_MODEL_KEYS)
    kw.update({k[4:]: v.clone().to(device) for k, v in fx.items() if k.startswith("in::")})
    return kw


def reference_lines(model, kw, gt_relevance):
    """evaluate_gen_attack.py:101-130 as the script has them, on the drop-in model -> (per-token losses, d loss / d features)."""
    enc_image_features, dec_input_ids = kw["enc_image_features"], kw["dec_input_ids"]
    batch_size, seq_len = dec_input_ids.size()
    enc_image_variables = Variable(enc_image_features.data, requires_grad=True)
    with torch.enable_grad():
        lm_loss, lm_scores = model(**dict(kw, enc_image_features=enc_image_variables), loss_reduction=False)
        per_token = lm_loss.detach().clone()
        lm_loss = lm_loss.view(batch_size, seq_len)
        lm_loss = lm_loss.mean(dim=1)
        lm_loss = torch.sum(lm_loss * gt_relevance)
    lm_loss.backward()
    return per_token, enc_image_variables.grad.data.clone()


_FULL = {}


def full_run(model, fx):
    if "d" not in _FULL:
        for p in model.parameters():
            p.grad = None
        kw = kwargs_of(fx)
        _FULL["loss"], _FULL["d"] = reference_lines(model, kw, fx["gt_relevance"].to(DEV))
        _FULL["ids_after"] = kw["dec_input_ids"].cpu()
    return _FULL


def outside_margin(fx):
    g = fx["d_feats"]
    return (g.abs() >= fx["sign_margin"].item() * g.abs().max()) | (g == 0)


def ranks_per_round(scores):
    return torch.argsort(torch.argsort(scores.view(2, 4), dim=1, descending=True), dim=1)


def test_reference_lines_run_on_the_drop_in_model(fp32_model, fx):
    """The backward through loss_reduction=False that Engine.backward used to refuse: d_feats within 2e-4 of the golden's maximum,
    zero-relevance rows and padded regions exactly zero, parameter gradients written as the reference writes them."""
    r = full_run(fp32_model, fx)
    ref = fx["d_feats"]
    d = r["d"].cpu()
    err_loss = (r["loss"].cpu() - fx["loss_none"]).abs().max().item()
    err = (d - ref).abs().max().item() / ref.abs().max().item()
    print("fp32: per-token loss error %.3e; d_feats error %.3e of the maximum %.3e" % (err_loss, err, ref.abs().max().item()))
    assert err_loss <= 1e-5
    assert torch.isfinite(d).all() and err <= 2e-4
    for b in range(8):
        if fx["gt_relevance"][b] == 0:
            assert bool((d[b] == 0).all()), b
    assert bool((d[2, -2:] == 0).all())
    assert torch.equal(r["ids_after"], fx["dec_input_ids_after"])
    eng = fp32_model.engine
    assert all(p.grad is not None for p in eng.flat.live) and float(fp32_model.vlfusion.fc_v.weight.grad.abs().max()) > 0


class _Untouchable(object):
    def __getattr__(self, name):
        raise AssertionError("the inputs-only replay touched the attached pipeline: ." + name)


def test_inputs_only_replay_is_bit_identical_and_writes_no_parameter_gradient(fp32_model, fx):
    r = full_run(fp32_model, fx)
    eng = fp32_model.engine
    grads = [p.grad for p in eng.flat.live]
    flat_before = eng.flat.G.clone()
    written, accumulate = set(eng.written), eng.accumulate
    eng.pipe = _Untouchable()
    try:
        with fp32_model.inputs_only():
            loss, d = reference_lines(fp32_model, kwargs_of(fx), fx["gt_relevance"].to(DEV))
    finally:
        eng.pipe = None
    assert torch.equal(d.view(torch.int32), r["d"].view(torch.int32))
    assert torch.equal(loss, r["loss"])
    assert all(p.grad is g for p, g in zip(eng.flat.live, grads))
    assert torch.equal(eng.flat.G.view(torch.int32), flat_before.view(torch.int32))
    assert eng.written == written and eng.accumulate == accumulate
    assert not eng._inputs_only and not eng._io
    # the mode is for calls that ask for the image-feature gradient
    from gst_visdial_amd._lib import GstvdError
    with pytest.raises(GstvdError), fp32_model.inputs_only(), torch.enable_grad():
        fp32_model(**kwargs_of(fx), loss_reduction=False)


@pytest.mark.parametrize("inputs_only", [True, False])
def test_fgsm_features(fp32_model, fx, inputs_only):
    from gst_visdial_amd import attack
    ok = outside_margin(fx)
    hit = fx["sign_margin_rows"].tolist()
    for i, b in enumerate(hit):
        share = (~ok[b]).float().mean().item()
        assert share <= 0.05, (b, share)                     # the fixture's own condition, on the fixture
    for tag in ("e1", "e01"):
        kw = kwargs_of(fx)
        feats0 = kw["enc_image_features"].clone()
        adv = attack.fgsm_features(fp32_model, kw, fx["gt_relevance"], fx["epsilon::" + tag].item(), inputs_only=inputs_only).cpu()
        want = fx["adv_feats::" + tag]
        flips = int((adv != want).sum())
        print("fgsm_features %s inputs_only=%s: %d of %d elements differ from the golden (all inside the sign margin: %s)"
              % (tag, inputs_only, flips, adv.numel(), bool((adv == want)[ok].all())))
        assert torch.equal(adv[ok], want[ok])
        for b in range(8):
            if b not in hit:
                assert torch.equal(adv[b].view(torch.int32), feats0[b].cpu().view(torch.int32))
        assert torch.equal(kw["dec_input_ids"].cpu(), fx["dec_input_ids_after"])
        assert torch.equal(kw["enc_image_features"], feats0)


def test_second_forward(fp32_model, fx):
    """On the golden's perturbed features: logits within 1e-4, ranks exact.  On its own perturbed features: the score deviation is
    measured and printed (profiles/fgsm.txt records it); the bound is 1e-3, the project's fp32 score gate, when no sign differs
    from the golden's, and otherwise that plus the largest change the WHOLE attack makes to a score in the fixture -- the own
    features differ from the golden's in at most the 5 % of elements inside the sign margin."""
    from gst_visdial_amd import attack
    from oracle import vd_oracle as O
    for tag in ("e1", "e01"):
        kw = kwargs_of(fx)
        kw["enc_image_features"] = fx["adv_feats::" + tag].to(DEV)
        kw["dec_input_ids"] = fx["dec_input_ids_after"].clone().to(DEV)
        with torch.no_grad():
            _, logits = fp32_model(**kw)
        logits = logits.cpu()
        err = (logits - fx["logits::" + tag]).abs().max().item()
        sc = O.answer_scores(logits, fx["in::dec_input_ids"])
        gold = fx["answer_scores::" + tag]
        print("second forward %s on the golden's features: logits error %.3e, score error %.3e" % (tag, err, (sc - gold).abs().max().item()))
        assert err <= 1e-4
        assert torch.equal(ranks_per_round(sc), ranks_per_round(gold))
        # own features, through the public function
        batch = {"enc_input_ids": fx["in::enc_input_ids"], "enc_segments": fx["in::enc_segments"],
                 "enc_sep_indices": torch.tensor([[3, 7, 0, 0, 0]]).repeat(8, 1), "enc_mlm_labels": fx["in::enc_mlm_labels"],
                 "enc_att_mask": fx["in::enc_attention_mask"], "dec_input_ids": fx["in::dec_input_ids"].clone(),
                 "dec_att_mask": fx["in::dec_attention_mask"], "enc_image_feat": fx["in::enc_image_features"],
                 "enc_image_loc": fx["in::enc_image_spatials"], "enc_image_mask": fx["in::enc_image_mask"],
                 "round_id": torch.tensor([[1]]), "gt_relevance": fx["gt_relevance"][None]}
        params = dict(attack="fgsm", device=torch.device(DEV))
        with torch.no_grad():
            own = attack.forward_attack(fp32_model, batch, params, epsilon=fx["epsilon::" + tag].item()).cpu()
        assert torch.equal(batch["dec_input_ids"], fx["in::dec_input_ids"])           # the loader's tensor is not written
        sc_own = O.answer_scores(own, fx["in::dec_input_ids"])
        dev = (sc_own - gold).abs().max().item()
        adv = attack.fgsm_features(fp32_model, kwargs_of(fx), fx["gt_relevance"], fx["epsilon::" + tag].item()).cpu()
        same = torch.equal(adv, fx["adv_feats::" + tag])
        effect = (gold - fx["answer_scores::clean"]).abs().max().item()
        print("second forward %s on its own features: score deviation from the golden %.3e (whole attack moves a score by <= %.3e)"
              % (tag, dev, effect))
        assert dev <= 1e-3 + (0.0 if same else effect)
        assert torch.equal(ranks_per_round(sc_own), ranks_per_round(gold))
        # a round that is not the annotated one is scored on the clean features
        batch["round_id"] = torch.tensor([[2]])
        with torch.no_grad():
            clean = attack.forward_attack(fp32_model, batch, params).cpu()
        assert (O.answer_scores(clean, fx["in::dec_input_ids"]) - fx["answer_scores::clean"]).abs().max().item() <= 1e-3


def test_bf16_gradient(fx):
    model, _ = build("bf16")
    with model.inputs_only():
        _, d = reference_lines(model, kwargs_of(fx), fx["gt_relevance"].to(DEV))
    d, ref = d.cpu(), fx["d_feats"]
    gmax = ref.abs().max().item()
    err = (d - ref).abs().max().item() / gmax
    big = ref.abs() >= 3e-2 * gmax
    agree = (torch.sign(d)[big] == torch.sign(ref)[big]).float().mean().item()
    print("bf16: d_feats error %.3e of the maximum; sign agreement %.4f over the %d elements with |g| >= 3e-2 max (reported, not gated)"
          % (err, agree, int(big.sum())))
    assert torch.isfinite(d).all() and err <= 3e-2
    for b in range(8):
        if fx["gt_relevance"][b] == 0:
            assert bool((d[b] == 0).all())


def test_train_step_after_an_attack_call_is_unchanged(fx):
    """One ordinary train step (dropout on) after an inputs-only attack call on the same engine: the loss and every gradient the
    backward produces in a fixed order equal, to the bit, those of a model that never ran the attack -- arena, tape, `written` /
    `accumulate` are left clean.  The embedding tables and the image-location projection are accumulated with fp32 atomic adds
    (csrc/layernorm.hip), whose order differs from launch to launch with or without an attack call: for those "the same gradient"
    is the project's fp32 gradient gate, 2e-4 of the tensor's maximum."""
    from gst_visdial_amd import attack
    from gst_visdial_amd.selfcheck import build_tiny_model, golden_batch, load_npz
    tr = load_npz("tiny_train.npz")

    def train_step(model):
        model.train()
        loss, _ = model(**golden_batch(tr, DEV))
        loss.backward()
        names = {id(p): n for n, p in model.named_parameters()}
        return loss.detach().clone(), [(names.get(id(p), "?"), p.grad.clone()) for p in model.engine.flat.live]

    a = build_tiny_model("fp32", DEV, seed=3, cfg_file="tiny_cfg_dropout.json")[0]
    loss_a, grads_a = train_step(a)
    b = build_tiny_model("fp32", DEV, seed=3, cfg_file="tiny_cfg_dropout.json")[0]
    b.eval()
    attack.fgsm_features(b, kwargs_of(fx), fx["gt_relevance"], 1.0)
    assert all(p.grad is None for p in b.parameters())
    loss_b, grads_b = train_step(b)
    assert torch.equal(loss_a, loss_b)
    assert [n for n, _ in grads_a] == [n for n, _ in grads_b]
    atomic = ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
              "token_type_embeddings_extension.weight", "image_location_embeddings.weight")
    for (name, x), (_, y) in zip(grads_a, grads_b):
        if name.endswith(atomic):
            assert (x - y).abs().max().item() <= 2e-4 * x.abs().max().item(), name
        else:
            assert torch.equal(x, y), name
