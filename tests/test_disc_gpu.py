"""GPU side of the discriminative (enc_only_a) evaluation on a real MI355X: parity with the reference fixture in both precisions,
the exact layer of the head kernel (gstvd_nsp_head: integer operands, float64 reference), its gather / write windows, invariances,
and the proof that the enc_dec path is undisturbed."""
import pytest
import torch

from conftest import load_npz, batch_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("r@1", "r@5", "r@10", "mean", "mrr", "ndcg")
# max |z_bf16 - z_reference| over the fixture's 60 rows as measured on the MI355X (kernel table row
# "NSP head"); the test asserts twice this value (accumulation order differs between the two precisions' kernels, nothing else)
BF16_Z_MEASURED = 9.526396e-02


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


def _ref_metrics(fx):
    return dict(zip(KEYS[:5], fx["sparse"].tolist()), ndcg=float(fx["ndcg"]))


def _rows(fx, dev=DEV):
    from gst_visdial_amd import evaluate_disc as ED
    b = sc().disc_batch(fx)
    B, R_, O = b["tokens"].shape[:3]
    n = B * R_ * O
    d = ED.option_rows_to_dialog(B, R_, O)
    sep, hl = b["sep_indices"].view(n, -1), b["hist_len"].view(n)
    att = ED.sequence_mask(ED.sequence_lengths(sep, hl), b["tokens"].shape[-1])
    r = dict(tokens=b["tokens"].view(n, -1), segments=b["segments"].view(n, -1), att=att, feat=b["image_feat"][d],
             loc=b["image_loc"][d], imask=b["image_mask"][d])
    return {k: v.to(dev) for k, v in r.items()}, b


def _forward(enc, r):
    with torch.no_grad():
        out = enc(r["tokens"], r["feat"], r["loc"], token_type_ids=r["segments"], attention_mask=r["att"],
                  image_attention_mask=r["imask"])
    assert len(out) == 7 and all(o is None for i, o in enumerate(out) if i != 3)
    return out[3]


def _through_both(precision):
    """seq_relationship_score through VisualDialogEncoder.forward (one call), prob0 / metrics through evaluate_disc (chunks of 17)."""
    from gst_visdial_amd import evaluate_disc as ED
    enc, params, fx = sc().build_tiny_disc_encoder(precision, DEV)
    r, b = _rows(fx)
    z = _forward(enc, r).cpu()
    assert z.dtype == torch.float32 and tuple(z.shape) == (60, 2)
    prob0 = ED.score_batch(enc, b, params, rows_per_call=17).cpu()
    metrics = ED.evaluate_disc(enc, [b], params, 2, rows_per_call=17)
    item = ED.chunk_item(b, ED.option_rows_to_dialog(2, 3, 10), 0, 60)
    z2 = ED.forward_disc(torch.nn.DataParallel(enc, [0]), item, params)[4].cpu()
    assert torch.equal(z, z2)
    return fx, z, prob0, metrics


def test_fp32_parity_scores_1e4_prob_1e5_ranks_and_metrics_bit_equal():
    from gst_visdial_amd.metrics import scores_to_ranks
    fx, z, prob0, metrics = _through_both("fp32")
    zerr = (z - fx["seq_relationship_score"]).abs().max().item()
    perr = (prob0 - fx["prob0"]).abs().max().item()
    print("\nfp32: max |z - ref| %.3e, max |prob0 - ref| %.3e" % (zerr, perr))
    assert zerr < 1e-4 and perr < 1e-5
    assert torch.equal(scores_to_ranks(prob0), fx["ranks"].long())
    assert torch.equal(scores_to_ranks(torch.softmax(z, 1)[:, 0].view(2, 3, 10)), fx["ranks"].long())
    ref = _ref_metrics(fx)
    for k in KEYS:
        assert metrics[k] == ref[k], (k, metrics[k], ref[k])


def test_bf16_metrics_within_a_tenth_of_a_point_and_logits_within_twice_the_measured_error():
    from gst_visdial_amd.metrics import scores_to_ranks
    fx, z, prob0, metrics = _through_both("bf16")
    ref = _ref_metrics(fx)
    zerr = (z - fx["seq_relationship_score"]).abs().max().item()
    moved = (scores_to_ranks(prob0) != fx["ranks"].long()).float().mean().item()
    pts = lambda m: {k: (m[k] if k == "mean" else 100.0 * m[k]) for k in KEYS}
    d = {k: pts(metrics)[k] - pts(ref)[k] for k in KEYS}
    print("\nbf16 vs the reference (2 x 3 x 10): max |z - ref| %.5f, max |prob0 - ref| %.5f | candidates whose rank moved %.4f | "
          "metric deltas (points) %s" % (zerr, (prob0 - fx["prob0"]).abs().max().item(), moved, {k: round(v, 4) for k, v in d.items()}))
    for k in KEYS:
        assert abs(d[k]) <= 0.1 + 1e-9, (k, d[k], metrics[k], ref[k])
    assert BF16_Z_MEASURED is not None and zerr <= 2 * BF16_Z_MEASURED, (zerr, BF16_Z_MEASURED)


# ---------------------------------------------------------------------------------------------- exact layer of the head kernel
SHAPES = [(64, 96, 128), (768, 1024, 1024)]
POISON = 0x7FC0ABCD                                    # a quiet NaN as fp32 bits; its upper half is a bf16 NaN too


def _canary(numel, dtype):
    t = torch.full((numel,), POISON, dtype=torch.int32, device=DEV)
    return t.view(torch.float32) if dtype == torch.float32 else t.view(torch.bfloat16)


def _window(values, rows_per_batch, pad, dtype):
    """values [B, K] -> a [B * rows_per_batch, K + pad] buffer of NaN whose row 0 of every batch row holds the values, + its view."""
    Bn, K = values.shape
    buf = _canary(Bn * rows_per_batch * (K + pad) * (2 if dtype == torch.bfloat16 else 1), dtype)[:Bn * rows_per_batch * (K + pad)]
    buf = buf.view(Bn * rows_per_batch, K + pad)
    buf[::rows_per_batch, :K] = values.to(DEV, dtype)
    return buf, buf[:, :K]


def _weights(values, pad, dtype):
    N, K = values.shape
    buf = _canary(N * (K + pad) * (2 if dtype == torch.bfloat16 else 1), dtype)[:N * (K + pad)].view(N, K + pad)
    buf[:, :K] = values.to(DEV, dtype)
    return buf[:, :K]


def _exact_problem(Bn, H, Hv, Hb, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    sparse = lambda n, k, keep: ri(-2, 2, n, k) * (torch.rand(n, k, generator=g) < keep / k).double()
    P = dict(xt=ri(-1, 1, Bn, H), xv=ri(-1, 1, Bn, Hv), wt=sparse(Hb, H, 24.0), wv=sparse(Hb, Hv, 24.0),
             bt=ri(-8, 8, Hb), bv=ri(-8, 8, Hb), bn=ri(-8, 8, 2))
    w0 = ri(-1, 1, Hb)
    P["wn"] = torch.stack([w0, w0 + ri(-1, 1, Hb) * (torch.rand(Hb, generator=g) < 8.0 / Hb).double()])
    return P


def _exact_reference(P, fusion):
    """float64 reference + the guard: every partial sum of the poolers, the fused value and z stay below 2^24 in magnitude."""
    bt_ = P["xt"].abs() @ P["wt"].abs().t() + P["bt"].abs()
    bv_ = P["xv"].abs() @ P["wv"].abs().t() + P["bv"].abs()
    fb = bt_ * bv_ if fusion == "mul" else bt_ + bv_
    zb = fb @ P["wn"].abs().t() + P["bn"].abs()
    peak = max(bt_.max().item(), bv_.max().item(), fb.max().item(), zb.max().item())
    assert peak < 2 ** 24, "exact case out of the fp32 integer range: peak %g" % peak
    pt = torch.relu(P["xt"] @ P["wt"].t() + P["bt"])
    pv = torch.relu(P["xv"] @ P["wv"].t() + P["bv"])
    f = pt * pv if fusion == "mul" else pt + pv
    z = f @ P["wn"].t() + P["bn"]
    m = z.max(1, keepdim=True)[0]
    e = torch.exp(z - m)
    return z, e[:, 0] / e.sum(1)


def _run_head(P, fusion, dtype, rows_t=3, rows_v=2, pad=8):
    from gst_visdial_amd import ops
    Bn = P["xt"].shape[0]
    tbuf, xt = _window(P["xt"], rows_t, pad, dtype)
    vbuf, xv = _window(P["xv"], rows_v, pad, dtype)
    wt, wv = _weights(P["wt"], pad, dtype), _weights(P["wv"], pad, dtype)
    f32 = lambda v: v.to(DEV, torch.float32).contiguous()
    zbuf, pbuf = _canary((Bn + 2) * 4, torch.float32).view(Bn + 2, 4), _canary(Bn + 8, torch.float32)
    z, prob0 = zbuf[1:Bn + 1, :2], pbuf[4:Bn + 4]
    ops.set_device(torch.device(DEV))
    ops.nsp_head(xt, rows_t, xv, rows_v, wt, f32(P["bt"]), wv, f32(P["bv"]), f32(P["wn"]), f32(P["bn"]), Bn, fusion, z, prob0)
    torch.cuda.synchronize()
    # write windows: everything around z / prob0 still carries the fill pattern
    zi, pi = zbuf.view(torch.int32), pbuf.view(torch.int32)
    assert bool((zi[0] == POISON).all()) and bool((zi[Bn + 1] == POISON).all()) and bool((zi[:, 2:] == POISON).all())
    assert bool((pi[:4] == POISON).all()) and bool((pi[Bn + 4:] == POISON).all())
    return z.clone().cpu(), prob0.clone().cpu(), (tbuf, vbuf)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fusion", ["mul", "sum"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Bn", [1, 15, 16, 17, 200, 500])
def test_head_kernel_is_exact_on_integer_operands(Bn, shape, fusion, dtype):
    """z bit-equal to the float64 reference rounded to fp32, prob0 within 2 fp32 ulp of the float64 value; the activation buffers
    hold NaN in every row but row 0 of each batch row and in the row padding (only row 0 is read), z / prob0 are windows inside
    pattern-filled allocations (nothing else is written), a second run is bit-identical."""
    H, Hv, Hb = shape
    P = _exact_problem(Bn, H, Hv, Hb, seed=1000 * Bn + Hb + (fusion == "sum"))
    zr, pr = _exact_reference(P, fusion)
    z, p, _ = _run_head(P, fusion, dtype)
    assert torch.isfinite(z).all() and torch.isfinite(p).all()
    assert torch.equal(z, zr.float()), (z.double() - zr).abs().max().item()
    p32 = pr.float()
    ulp = (torch.nextafter(p32, torch.full_like(p32, float("inf"))) - p32).double()
    assert bool(((p.double() - pr).abs() <= 2 * ulp).all()), ((p.double() - pr).abs() / ulp).max().item()

    z2, p2, _ = _run_head(P, fusion, dtype)
    assert torch.equal(z, z2) and torch.equal(p.view(torch.int32), p2.view(torch.int32))


def test_head_kernel_reads_row_zero_only_clean_buffers_give_the_same_bits():
    """The same problem with clean (zero-filled) activation buffers instead of NaN-filled ones: identical results."""
    from gst_visdial_amd import ops
    P = _exact_problem(37, 64, 96, 128, seed=5)
    z, p, _ = _run_head(P, "mul", torch.bfloat16)
    dt_ = torch.bfloat16
    xt = torch.zeros(37 * 3, 64, device=DEV, dtype=dt_); xt[::3] = P["xt"].to(DEV, dt_)
    xv = torch.zeros(37 * 2, 96, device=DEV, dtype=dt_); xv[::2] = P["xv"].to(DEV, dt_)
    f32 = lambda v: v.to(DEV, torch.float32).contiguous()
    zc, pc = torch.empty(37, 2, device=DEV), torch.empty(37, device=DEV)
    ops.nsp_head(xt, 3, xv, 2, P["wt"].to(DEV, dt_), f32(P["bt"]), P["wv"].to(DEV, dt_), f32(P["bv"]), f32(P["wn"]), f32(P["bn"]),
                 37, "mul", zc, pc)
    assert torch.equal(zc.cpu(), z) and torch.equal(pc.cpu(), p)


def test_head_entry_refuses_what_it_does_not_support():
    from gst_visdial_amd import ops, _lib
    P = _exact_problem(4, 64, 96, 128, seed=6)
    f32 = lambda v: v.to(DEV, torch.float32).contiguous()
    a = lambda k: P[k].to(DEV, torch.float32).contiguous()
    z, p = torch.empty(4, 2, device=DEV), torch.empty(4, device=DEV)
    with pytest.raises(_lib.GstvdError):
        ops.nsp_head(a("xt"), 1, a("xv"), 1, a("wt"), f32(P["bt"]), a("wv"), f32(P["bv"]), f32(P["wn"]), f32(P["bn"]), 4, "max", z, p)
    with pytest.raises(_lib.GstvdError):          # H = 72 is not a multiple of 16
        ops.nsp_head(a("xt")[:, :8].repeat(1, 9), 1, a("xv"), 1, a("wt")[:, :8].repeat(1, 9), f32(P["bt"]), a("wv"), f32(P["bv"]),
                     f32(P["wn"]), f32(P["bn"]), 4, "mul", z, p)


# ---------------------------------------------------------------------------------------------- engine level
def test_launched_kernel_is_the_head_kernel_and_no_torch_matmul_follows_the_encoder():
    from torch.utils._python_dispatch import TorchDispatchMode
    from gst_visdial_amd import ops
    enc, params, fx = sc().build_tiny_disc_encoder("bf16", DEV)
    r, _ = _rows(fx)
    _forward(enc, r)                                            # first call: flat buffers, arena

    class Log(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    log, prof = Log(), ops.Profiler()
    with prof, log:
        z, p = enc.engine.nsp_scores(r["feat"], r["loc"], r["imask"], r["tokens"], r["segments"], r["att"])
    tags = [rec[0] for rec in prof.records]
    heads = [t for t in tags if t.startswith("nsp_head:")]
    assert len(heads) == 1 and tags[-1] == heads[0] and "nsp_head_kernel" in heads[0] and "DF16b" in heads[0], tags[-3:]
    assert sum(t.startswith("gemm:") for t in tags) > 20          # the encoder ran through the library's GEMMs
    bad = [n for n in log.names if any(s in n for s in ("mm", "matmul", "linear", "softmax", "relu", "einsum"))]
    assert not bad, bad
    assert torch.isfinite(z).all() and bool(((p > 0) & (p < 1)).all())


def test_batch_permutation_and_masked_contents_do_not_change_fp32_scores():
    enc, params, fx = sc().build_tiny_disc_encoder("fp32", DEV)
    r, _ = _rows(fx)
    z = _forward(enc, r).clone()
    assert torch.equal(_forward(enc, r), z)                     # run to run
    perm = torch.randperm(60, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(_forward(enc, {k: v[perm] for k, v in r.items()}), z[perm])
    g = torch.Generator().manual_seed(4)
    r2 = {k: v.clone() for k, v in r.items()}
    junk = torch.randint(110, 320, r["tokens"].shape, generator=g).to(DEV)
    r2["tokens"] = torch.where(r["att"], r["tokens"], junk)     # masked text positions (all beyond the first token)
    r2["segments"] = torch.where(r["att"], r["segments"], torch.ones_like(r["segments"]))
    dead = (r["imask"] == 0)
    assert not bool(dead[:, 0].any()) and bool(dead.any()) and not bool(r["att"].all())
    r2["feat"] = torch.where(dead[..., None], torch.randn(r["feat"].shape, generator=g).to(DEV) * 3, r["feat"])
    r2["loc"] = torch.where(dead[..., None], torch.rand(r["loc"].shape, generator=g).to(DEV), r["loc"])
    assert torch.equal(_forward(enc, r2), z)


def test_enc_dec_path_is_undisturbed_by_an_enc_only_encoder_in_the_same_process(tiny_train):
    s = sc()
    model, mparams, _ = s.build_tiny_model("fp32", DEV, mode="vd_eval_val")
    model.eval()
    kw = s.golden_batch(tiny_train, DEV)
    with torch.no_grad():
        loss0, logits0 = model(**{k: (v.clone() if v is not None else None) for k, v in kw.items()})
        loss0, logits0 = loss0.clone(), logits0.clone()
    enc, params, fx = s.build_tiny_disc_encoder("fp32", DEV)
    enc.load_state_dict(model.encoder.state_dict(), strict=True)            # the same encoder weights, the head stays the fixture's
    assert enc.engine is not model.engine
    ids, seg, att = kw["enc_input_ids"], kw["enc_segments"], kw["enc_attention_mask"]
    feat, loc, im = kw["enc_image_features"], kw["enc_image_spatials"], kw["enc_image_mask"]
    z, p = enc.nsp_scores(ids, feat, loc, seg, att, im)
    B = ids.shape[0]
    ht = enc.engine.last["enc_t"].t.view(B, ids.shape[1], -1).float().clone()
    hv = enc.engine.last["enc_v"].t.view(B, feat.shape[1], -1).float().clone()
    assert enc.engine.flat.G is None and enc.engine.flat.S is None          # inference only, fp32: no gradient, no shadow buffer
    assert not any(n.startswith(("dec.", "d0.", "lm.", "vlf.")) for n in enc.engine.flat.slots)
    with torch.no_grad():
        out = model.encoder(ids, feat, loc, token_type_ids=seg, attention_mask=att, image_attention_mask=im)
    assert torch.equal(out[5], ht) and torch.equal(out[6], hv)
    with torch.no_grad():
        loss1, logits1 = model(**{k: (v.clone() if v is not None else None) for k, v in kw.items()})
    assert torch.equal(loss0, loss1) and torch.equal(logits0, logits1)
    assert torch.isfinite(z).all()
