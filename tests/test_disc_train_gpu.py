"""GPU side of the discriminative (enc_only_a) training step on a real MI355X: parity of losses and gradients with the reference
fixture in both precisions, three optimizer steps, the exact / canaried layer of the new kernels (row gather / scatter, the
masked-region KL loss, the NSP head in training form), the empty-mask edges, and the proof that ranking and the enc_dec path are
undisturbed."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = "bert_pretrained."
POISON = 0x7FC0ABCD                                    # a quiet NaN as fp32 bits; its upper half is a bf16 NaN too


def sc():
    from gst_visdial_amd import selfcheck
    return selfcheck


@pytest.fixture(scope="module")
def fx():
    return load_npz("tiny_disc_train.npz")


def _enc(precision, **coeffs):
    kw = dict(lm_loss_coeff=1.0, nsp_loss_coeff=1.0, img_loss_coeff=1.0, batch_size=12)     # all 12 rows of the fixture, permuted
    kw.update(coeffs)
    enc, params, _ = sc().build_tiny_disc_encoder(precision, DEV, mode="vd_train", fixture="tiny_disc_train.npz", **kw)
    return enc, params                                  # eval(): no dropout draws, as the fixture was recorded


def _rows(fx, dev=DEV):
    return {k[len("row::"):]: v.clone().to(dev) for k, v in fx.items() if k.startswith("row::")}


def _call(enc, r, feat=None, **extra):
    out = enc(r["tokens"], r["image_feat"] if feat is None else feat, r["image_loc"], sep_indices=r["sep_indices"],
              token_type_ids=r["segments"], masked_lm_labels=r["mask"], attention_mask=r["attention_mask"].bool(),
              next_sentence_label=r["next_sentence_labels"], image_attention_mask=r["image_mask"], image_label=r["image_label"],
              image_target=r["image_target"], **extra)
    assert len(out) == 7 and out[4] is None and out[5] is None and out[6] is None
    lm, img, nsp, z = out[:4]
    assert tuple(lm.shape) == tuple(img.shape) == tuple(nsp.shape) == (1,) and z.dtype == torch.float32
    return lm, img, nsp, z


def _grads(enc):
    return {k: (p.grad.detach().float().cpu().clone() if p.grad is not None else None) for k, p in enc.named_parameters()}


def _step(precision, fx):
    enc, params = _enc(precision)
    r = _rows(fx)
    feat = r["image_feat"].clone().requires_grad_(True)
    lm, img, nsp, z = _call(enc, r, feat)
    (lm.mean() + nsp.mean() + img.mean()).backward()
    torch.cuda.synchronize()
    return enc, params, r, (lm.detach().cpu(), img.detach().cpu(), nsp.detach().cpu(), z.cpu()), _grads(enc), feat.grad.cpu()


def test_fp32_parity_losses_1e5_scores_1e4_gradients_2e4_of_max_and_both_entry_points_bit_equal(fx):
    from gst_visdial_amd import evaluate_disc as ED
    enc, params, r, (lm, img, nsp, z), grads, dfeat = _step("fp32", fx)
    c2 = fx["coeffs2"].tolist()
    errs = dict(lm=abs(lm.item() - fx["lm_loss"].item()), img=abs(img.item() - fx["img_loss"].item()),
                nsp=abs(nsp.item() - fx["nsp_loss"].item()), z=(z - fx["seq_relationship_score"]).abs().max().item(),
                total=abs((lm + nsp + img).item() - fx["total"].item()),
                total2=abs((c2[0] * lm + c2[1] * nsp + c2[2] * img).item() - fx["total2"].item()))
    print("\nfp32 vs the reference:", {k: "%.3e" % v for k, v in errs.items()})
    assert max(errs["lm"], errs["img"], errs["nsp"], errs["total"], errs["total2"]) < 1e-5 and errs["z"] < 1e-4
    recorded = {k[len("grad::"):]: v for k, v in fx.items() if k.startswith("grad::")}
    assert len(recorded) == 12
    for k, ref in recorded.items():
        got = dfeat if k == "image_feat" else grads[k]
        rel = (got - ref).abs().max().item() / ref.abs().max().item()
        print("  grad %-66s max err / max %.3e" % (k, rel))
        assert rel < 2e-4, (k, rel)
    dead = sorted(k for k, g in grads.items() if g is None)
    assert dead == sorted(bytes(fx["no_grad_names"].tolist()).decode().split("\n"))
    assert all(torch.isfinite(g).all() for g in grads.values() if g is not None)

    # the same step through forward_disc(nn.DataParallel(enc, [0]), ...): per-dialog image tensors, host-side row indices
    batch = {k[4:]: v.clone() for k, v in fx.items() if k.startswith("in::")}
    enc.zero_grad(set_to_none=True)
    torch.manual_seed(int(fx["sample_seed"]))
    loss, lm2, nsp2, img2, z2, lms = ED.forward_disc(torch.nn.DataParallel(enc, [0]), batch, params)
    assert lms is None
    assert torch.equal(lm2.cpu(), lm.mean()) and torch.equal(img2.cpu(), img.mean()) and torch.equal(nsp2.cpu(), nsp.mean())
    assert torch.equal(z2.cpu(), z) and torch.equal(loss.cpu(), lm.mean() + nsp.mean() + img.mean())
    loss.backward()
    torch.cuda.synchronize()
    g2 = _grads(enc)
    for k, g in grads.items():          # (not bit for bit: the embedding tables' backward adds rows with atomics)
        assert (g is None) == (g2[k] is None) and (g is None or (g - g2[k]).abs().max().item() <= 1e-5 * g.abs().max().item()), k
    # the second coefficient triple, through params (re-read on every call)
    params.update(lm_loss_coeff=c2[0], nsp_loss_coeff=c2[1], img_loss_coeff=c2[2])
    torch.manual_seed(int(fx["sample_seed"]))
    with torch.no_grad():
        loss2 = ED.forward_disc(enc, batch, params)[0]
    assert abs(loss2.item() - fx["total2"].item()) < 1e-5


def test_bf16_parity_losses_and_gradients_within_3e2(fx):
    """The project's bf16 gate: losses within 3e-2, every recorded gradient within 3e-2 of its norm; the measured maxima are
    printed.  (The fixture keeps every pooler pre-activation 2^-5 away from zero, tools/make_golden_disc_train.py: which way a
    ReLU decides is then not left to the rounding of the encoder's bf16 output.)"""
    enc, params, r, (lm, img, nsp, z), grads, dfeat = _step("bf16", fx)
    errs = dict(lm=abs(lm.item() - fx["lm_loss"].item()), img=abs(img.item() - fx["img_loss"].item()),
                nsp=abs(nsp.item() - fx["nsp_loss"].item()))
    worst = {}
    for k, ref in {k[len("grad::"):]: v for k, v in fx.items() if k.startswith("grad::")}.items():
        got = dfeat if k == "image_feat" else grads[k]
        worst[k] = ((got - ref).norm() / ref.norm()).item()
    print("\nbf16 vs the reference: losses", {k: "%.3e" % v for k, v in errs.items()}, "| max |z - ref| %.3e" %
          (z - fx["seq_relationship_score"]).abs().max().item())
    for k, v in worst.items():
        print("  grad %-66s norm-relative %.3e" % (k, v))
    assert max(errs.values()) < 3e-2
    assert max(worst.values()) < 3e-2, worst


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_three_sgd_steps_follow_the_reference_and_refresh_the_shadow(fx, precision):
    enc, params = _enc(precision)
    r = _rows(fx)
    opt = torch.optim.SGD(enc.parameters(), lr=float(fx["sgd_lr"]))
    ref = fx["sgd_losses"]
    traj = []
    for step in range(4):
        opt.zero_grad(set_to_none=True)
        lm, img, nsp, _ = _call(enc, r)
        flat = enc.engine.flat
        if precision == "bf16":           # the forward that just ran read shadow weights cast from the CURRENT fp32 parameters
            assert torch.equal(flat.S.view(torch.int16), flat.P.to(torch.bfloat16).view(torch.int16)), step
        traj.append([lm.item(), img.item(), nsp.item()])
        if step == 3:
            break
        (lm.mean() + nsp.mean() + img.mean()).backward()
        opt.step()
    traj = torch.tensor(traj, dtype=torch.float64)
    print("\n%s trajectory (lm, img, nsp):\n%s\nreference:\n%s" % (precision, traj, ref))
    if precision == "fp32":
        assert (traj - ref).abs().max().item() < 2e-4
    else:
        assert traj[3].sum().item() < traj[0].sum().item()


# ---------------------------------------------------------------------------------------------- kernel layer
def _canary(numel, dtype):
    if dtype == torch.float32:
        return torch.full((numel,), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((numel,), POISON >> 16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _poison_bits(dtype):
    return POISON if dtype == torch.float32 else POISON >> 16


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_rows_gather_and_scatter_are_bit_exact_and_write_only_their_windows(n, H, dtype):
    from gst_visdial_amd import ops
    ops.set_device(torch.device(DEV))
    g = torch.Generator().manual_seed(n * 1000 + H)
    M, pad = 131, 8
    pb = _poison_bits(dtype)
    idx = torch.randperm(M, generator=g)[:n].to(DEV)
    vals = torch.randn(M, H, generator=g).to(DEV, dtype)
    src = _canary(M * (H + pad), dtype).view(M, H + pad)          # strided source, poisoned padding
    src[:, :H] = vals
    for _ in range(2):                                              # a second run is bit-identical
        out = _canary((n + 2) * (H + pad), dtype).view(n + 2, H + pad)
        ops.rows_gather(src[:, :H], idx, out[1:n + 1, :H])
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[1:n + 1, :H]), _bits(vals[idx]))
        ob = _bits(out)
        assert bool((ob[0] == pb).all()) and bool((ob[n + 1] == pb).all()) and bool((ob[:, H:] == pb).all())
    # scatter, first writer: named rows = the source rows, every other row of [0, M) zero, padding and neighbours untouched
    upd = torch.randn(n, H, generator=g).to(DEV, dtype)
    dst = _canary((M + 2) * (H + pad), dtype).view(M + 2, H + pad)
    ops.rows_scatter(upd, idx, dst[1:M + 1, :H], accumulate=False)
    torch.cuda.synchronize()
    want = torch.zeros(M, H, device=DEV, dtype=dtype)
    want[idx] = upd
    assert torch.equal(_bits(dst[1:M + 1, :H]), _bits(want))
    db = _bits(dst)
    assert bool((db[0] == pb).all()) and bool((db[M + 1] == pb).all()) and bool((db[:, H:] == pb).all())
    # accumulate: adds to the named rows only (one rounding of the fp32 sum), every other row keeps its bits
    base = torch.randn(M, H, generator=g).to(DEV, dtype)
    dst[1:M + 1, :H] = base
    ops.rows_scatter(upd, idx, dst[1:M + 1, :H], accumulate=True)
    torch.cuda.synchronize()
    want = base.clone()
    want[idx] = (base[idx].float() + upd.float()).to(dtype)
    assert torch.equal(_bits(dst[1:M + 1, :H]), _bits(want))
    db = _bits(dst)
    assert bool((db[0] == pb).all()) and bool((db[M + 1] == pb).all()) and bool((db[:, H:] == pb).all())


def _kl_reference(scores, target, gscale):
    """float64: per-row KL(target || softmax(scores)) with torch's xlogy convention, and d(gscale * mean over rows) / d scores."""
    s = scores.double().clone().requires_grad_(True)
    row = F.kl_div(F.log_softmax(s, 1), target.double(), reduction="none").sum(1)
    (gscale * row.sum() / row.shape[0]).backward()
    return row.detach(), s.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [11, 1601])
@pytest.mark.parametrize("rows", [1, 17])
def test_kl_loss_forward_and_backward_against_float64(rows, C, dtype):
    from gst_visdial_amd import ops
    ops.set_device(torch.device(DEV))
    g = torch.Generator().manual_seed(rows * 10000 + C)
    Cp = (C + 63) // 64 * 64
    nt = rows + 3                                                   # the target has more rows than the scores: picked by index
    target = torch.rand(nt, C, generator=g) * (torch.rand(nt, C, generator=g) < 0.5).float()
    target[:, 0] += 0.01
    target = target / target.sum(1, keepdim=True) * (0.5 + torch.rand(nt, 1, generator=g))      # row sums are NOT 1
    trow = torch.randperm(nt, generator=g)[:rows]
    if rows > 2:
        target[trow[1]] = 0.0                                       # an all-zero target row: loss 0, gradient 0, exactly
        target[trow[2]] = 0.0
        target[trow[2], C // 2] = 1.0                               # a single 1: the row's loss is the cross entropy of that class
    scores = (torch.randn(rows, C, generator=g) * 2.0).to(dtype)
    sbuf = _canary(rows * (Cp + 8), dtype).view(rows, Cp + 8)       # poisoned padding behind the C classes
    sbuf[:, :C] = scores.to(DEV)
    gscale = torch.tensor([0.7], device=DEV)
    tdev, tr = target.to(DEV), trow.to(DEV)
    outs = []
    for _ in range(2):
        f = _canary(2 * rows + 8 + 12, torch.float32)
        row_loss, lse, stats = f[2:rows + 2], f[rows + 6:2 * rows + 6], f[2 * rows + 10:2 * rows + 14]
        dbuf = _canary((rows + 2) * Cp, dtype).view(rows + 2, Cp)      # (the backward zero-fills up to the leading dimension)
        ops.kl_fwd(sbuf[:, :Cp], tdev, rows, C, row_loss, lse, stats, target_row=tr)
        ops.kl_bwd(sbuf[:, :Cp], tdev, lse, stats, gscale, True, rows, C, dbuf[1:rows + 1, :Cp], target_row=tr)
        torch.cuda.synchronize()
        fb, db, pb = _bits(f), _bits(dbuf), _poison_bits(dtype)
        assert bool((fb[:2] == POISON).all()) and bool((fb[rows + 2:rows + 6] == POISON).all()) and bool((fb[2 * rows + 6:2 * rows + 10] == POISON).all())
        assert bool((fb[2 * rows + 13:] == POISON).all())           # stats[3] is not written either
        assert bool((db[0] == pb).all()) and bool((db[rows + 1] == pb).all())
        assert bool((dbuf[1:rows + 1, C:Cp] == 0).all())            # the columns between C and the leading dimension: zero filled
        outs.append((row_loss.clone().cpu(), stats[:3].clone().cpu(), dbuf[1:rows + 1, :C].clone().float().cpu()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    row_loss, stats, d = outs[0]
    ref_row, ref_d = _kl_reference(scores, target[trow], 0.7)
    nz = ref_row.abs() > 0
    rel = ((row_loss.double() - ref_row).abs()[nz] / ref_row.abs()[nz]).max().item() if bool(nz.any()) else 0.0
    derr = (d.double() - ref_d).abs().max().item()
    print("\nKL rows %d C %d %s: row loss max rel err %.3e, gradient max abs err %.3e" % (rows, C, dtype, rel, derr))
    assert rel < 1e-5
    # fp32 gradient: 1e-6 absolute.  bf16: the gradient is STORED in bf16 -- half an ulp of its largest element (2^-9 relative)
    assert derr < (1e-6 if dtype == torch.float32 else ref_d.abs().max().item() * 2.0 ** -8)
    assert abs(stats[0].item() - ref_row.sum().item()) < 1e-5 * max(1.0, ref_row.sum().item()) and stats[1].item() == rows
    assert abs(stats[2].item() - ref_row.mean().item()) < 1e-5 * max(1.0, ref_row.mean().item())
    if rows > 2:
        assert row_loss[1].item() == 0.0 and bool((d[1] == 0).all())
        ce = F.cross_entropy(scores[2:3].double(), torch.tensor([C // 2])).item()
        assert abs(row_loss[2].item() - ce) < 1e-5 * ce


SHAPES = [(64, 96, 128), (768, 1024, 1024)]


def _window(values, rows_per_batch, pad, dtype):
    Bn, K = values.shape
    buf = _canary(Bn * rows_per_batch * (K + pad), dtype).view(Bn * rows_per_batch, K + pad)
    buf[::rows_per_batch, :K] = values.to(DEV, dtype)
    return buf[:, :K]


def _weights(values, pad, dtype):
    N, K = values.shape
    buf = _canary(N * (K + pad), dtype).view(N, K + pad)
    buf[:, :K] = values.to(DEV, dtype)
    return buf[:, :K]


def _exact_problem(Bn, H, Hv, Hb, seed, backward=False):
    """The integer-operand construction of the NSP head's exact test (tests/test_disc_gpu.py), restated.  `backward`: the
    classifier rows are +-64 * w0 and the two biases equal, so z0 - z1 is a multiple of 128: softmax(z) is exactly (1/2, 1/2),
    (1, 0) or (0, 1) in fp32 (exp(-128) is 0) and every gradient is a sum of small integers and halves."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    sparse = lambda n, k, keep: ri(-2, 2, n, k) * (torch.rand(n, k, generator=g) < keep / k).double()
    Pm = dict(xt=ri(-1, 1, Bn, H), xv=ri(-1, 1, Bn, Hv), wt=sparse(Hb, H, 24.0), wv=sparse(Hb, Hv, 24.0),
              bt=ri(-8, 8, Hb), bv=ri(-8, 8, Hb), bn=ri(-8, 8, 2))
    w0 = ri(-1, 1, Hb)
    Pm["wn"] = torch.stack([w0, w0 + ri(-1, 1, Hb) * (torch.rand(Hb, generator=g) < 8.0 / Hb).double()])
    if backward:
        w0 = 64.0 * ri(-1, 1, Hb) * (torch.rand(Hb, generator=g) < 12.0 / Hb).double()
        Pm["wn"] = torch.stack([w0, -w0])
        Pm["bn"] = Pm["bn"][:1].repeat(2)
    Pm["labels"] = ri(0, 3, Bn, 2)
    return Pm


def _head_reference(Pm, fusion, keep=None, p=0.0, gscale=1.0):
    """float64 forward + backward of the training head under the given keep flags."""
    t = {k: v.clone().double() for k, v in Pm.items()}
    for k in ("xt", "xv", "wt", "wv", "bt", "bv", "wn", "bn"):
        t[k].requires_grad_(True)
    at, av = t["xt"] @ t["wt"].t() + t["bt"], t["xv"] @ t["wv"].t() + t["bv"]
    at.retain_grad(); av.retain_grad()
    pt, pv = torch.relu(at), torch.relu(av)
    f = pt * pv if fusion == "mul" else pt + pv
    if keep is not None:
        f = f * keep.double() / (1.0 - p)
    z = f @ t["wn"].t() + t["bn"]
    row = -(t["labels"] * F.log_softmax(z, 1)).sum(1)
    loss = row.sum() / row.shape[0]
    (gscale * loss).backward()
    return dict(z=z.detach(), row=row.detach(), loss=loss.detach(), pt=pt.detach(), pv=pv.detach(), dwn=t["wn"].grad, dbn=t["bn"].grad,
                dpt=at.grad, dpv=av.grad, f=f.detach())


def _run_train_head(Pm, fusion, dtype, p=0.0, rng=None, gscale=1.0, rows_t=3, rows_v=2, pad=8, acc=False):
    from gst_visdial_amd import ops
    ops.set_device(torch.device(DEV))
    Bn, Hb = Pm["xt"].shape[0], Pm["wt"].shape[0]
    xt, xv = _window(Pm["xt"], rows_t, pad, dtype), _window(Pm["xv"], rows_v, pad, dtype)
    wt, wv = _weights(Pm["wt"], pad, dtype), _weights(Pm["wv"], pad, dtype)
    f32 = lambda v: v.to(DEV, torch.float32).contiguous()
    zbuf = _canary((Bn + 2) * 4, torch.float32).view(Bn + 2, 4)
    z = zbuf[1:Bn + 1, :2]
    sav = _canary((2 * Bn + 2) * Hb, torch.float32).view(2 * Bn + 2, Hb)
    pt, pv = sav[1:Bn + 1], sav[Bn + 1:2 * Bn + 1]
    kbuf = torch.full(((Bn + 2) * Hb,), 0xAB, dtype=torch.uint8, device=DEV).view(Bn + 2, Hb)
    keep = kbuf[1:Bn + 1]
    sbuf = _canary(Bn + 16, torch.float32)
    row_loss, stats = sbuf[4:Bn + 4], sbuf[Bn + 8:Bn + 12]
    d = ops.nsp_train_desc(xt, rows_t, xv, rows_v, wt, f32(Pm["bt"]), wv, f32(Pm["bv"]), f32(Pm["wn"]), f32(Pm["bn"]), f32(Pm["labels"]),
                           Bn, fusion, z, pt, pv, keep, row_loss, stats, p=p, site=5, rng=rng)
    ops.nsp_train_fwd(d)
    gbuf = _canary(4 * (Hb + 8) + 16, torch.float32)
    dwn, dbn = gbuf[8:8 + 2 * (Hb + 8)].view(2, Hb + 8)[:, :Hb], gbuf[8 + 2 * (Hb + 8) + 4:8 + 2 * (Hb + 8) + 6]
    if acc:
        dwn.fill_(1.0); dbn.fill_(2.0)
    dbuf = _canary((2 * Bn + 2) * (Hb + pad), dtype).view(2 * Bn + 2, Hb + pad)
    dpt, dpv = dbuf[1:Bn + 1, :Hb], dbuf[Bn + 1:2 * Bn + 1, :Hb]
    ops.nsp_train_bwd(d, torch.tensor([gscale], device=DEV), dwn, dbn, dpt, dpv, acc_w=acc, acc_b=acc)
    torch.cuda.synchronize()
    # write windows
    zi, si, sv, gi, di, pb = _bits(zbuf), _bits(sbuf), _bits(sav), _bits(gbuf), _bits(dbuf), _poison_bits(dtype)
    assert bool((zi[0] == POISON).all()) and bool((zi[Bn + 1] == POISON).all()) and bool((zi[:, 2:] == POISON).all())
    assert bool((si[:4] == POISON).all()) and bool((si[Bn + 4:Bn + 8] == POISON).all()) and bool((si[Bn + 11:] == POISON).all())
    assert bool((sv[0] == POISON).all()) and bool((sv[2 * Bn + 1] == POISON).all())
    assert bool((kbuf[0] == 0xAB).all()) and bool((kbuf[Bn + 1] == 0xAB).all())
    assert bool((gi[:8] == POISON).all()) and bool((gi[8 + 2 * (Hb + 8):8 + 2 * (Hb + 8) + 4] == POISON).all()) and bool((gi[8 + 2 * (Hb + 8) + 6:] == POISON).all())
    assert bool((gi[8:8 + 2 * (Hb + 8)].view(2, Hb + 8)[:, Hb:] == POISON).all())
    assert bool((di[0] == pb).all()) and bool((di[2 * Bn + 1] == pb).all()) and bool((di[:, Hb:] == pb).all())
    assert bool(((keep == 0) | (keep == 1)).all())
    out = dict(z=z, pt=pt, pv=pv, keep=keep, row=row_loss, stats=stats[:3], dwn=dwn, dbn=dbn, dpt=dpt, dpv=dpv)
    return {k: v.clone().cpu() for k, v in out.items()}, (xt, xv, wt, wv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fusion", ["mul", "sum"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Bn", [1, 15, 16, 17])
def test_nsp_train_head_without_dropout_is_exact_on_integer_operands(Bn, shape, fusion, dtype):
    from gst_visdial_amd import ops
    H, Hv, Hb = shape
    # forward: z bit-equal to gstvd_nsp_head on the same problem, pt / pv exact, every keep flag set, the loss against float64
    Pm = _exact_problem(Bn, H, Hv, Hb, seed=1000 * Bn + Hb + (fusion == "sum"))
    out, (xt, xv, wt, wv) = _run_train_head(Pm, fusion, dtype)
    f32 = lambda v: v.to(DEV, torch.float32).contiguous()
    zh, ph = torch.empty(Bn, 2, device=DEV), torch.empty(Bn, device=DEV)
    ops.nsp_head(xt, 3, xv, 2, wt, f32(Pm["bt"]), wv, f32(Pm["bv"]), f32(Pm["wn"]), f32(Pm["bn"]), Bn, fusion, zh, ph)
    ref = _head_reference(Pm, fusion)
    assert torch.equal(out["z"], zh.cpu()) and torch.equal(out["z"], ref["z"].float())
    assert torch.equal(out["pt"], ref["pt"].float()) and torch.equal(out["pv"], ref["pv"].float()) and bool((out["keep"] == 1).all())
    tol = 4e-7 * ref["row"].abs().clamp(min=1.0)
    assert bool(((out["row"].double() - ref["row"]).abs() <= tol).all())
    assert abs(out["stats"][0].item() - ref["row"].sum().item()) <= 4e-7 * Bn * max(1.0, ref["row"].abs().max().item())
    assert out["stats"][1].item() == Bn
    out2, _ = _run_train_head(Pm, fusion, dtype)
    assert all(torch.equal(_bits(out[k]), _bits(out2[k])) for k in out)

    # backward: bit-exact against float64 where every partial sum is an integer or a half below 2^23
    Pb = _exact_problem(Bn, H, Hv, Hb, seed=7000 * Bn + Hb + (fusion == "sum"), backward=True)
    rb = _head_reference(Pb, fusion, gscale=float(Bn))              # gscale = B: the 1 / B of the mean cancels exactly
    dz = (rb["z"][:, 0] - rb["z"][:, 1]).abs()
    assert bool(((dz == 0) | (dz >= 128)).all())
    sl = Pb["labels"].sum(1, keepdim=True)
    dzb = (0.5 * sl + Pb["labels"]).abs()                           # bound of |dz|: softmax <= 1 (here in {0, 1/2, 1})
    fb = rb["f"].abs()
    peak = max((dzb.t() @ fb).max().item(), (dzb @ Pb["wn"].abs()).max().item() * max(1.0, rb["pt"].max().item(), rb["pv"].max().item()),
               rb["z"].abs().max().item(), fb.max().item())
    assert peak < 2 ** 23, "exact backward case out of the fp32 integer range: peak %g" % peak
    ob, _ = _run_train_head(Pb, fusion, dtype, gscale=float(Bn))
    assert torch.equal(ob["z"], rb["z"].float())
    assert torch.equal(ob["dwn"], rb["dwn"].float()) and torch.equal(ob["dbn"], rb["dbn"].float())
    if dtype == torch.float32:
        assert torch.equal(ob["dpt"], rb["dpt"].float()) and torch.equal(ob["dpv"], rb["dpv"].float())
    else:                                                           # stored in bf16: the float64 value rounded once
        assert torch.equal(ob["dpt"], rb["dpt"].to(torch.bfloat16)) and torch.equal(ob["dpv"], rb["dpv"].to(torch.bfloat16))
    oa, _ = _run_train_head(Pb, fusion, dtype, gscale=float(Bn), acc=True)      # accumulate form: adds to what the slots hold
    assert torch.equal(oa["dwn"], (rb["dwn"] + 1.0).float()) and torch.equal(oa["dbn"], (rb["dbn"] + 2.0).float())


@pytest.mark.parametrize("fusion", ["mul", "sum"])
def test_nsp_train_head_with_dropout_matches_float64_under_its_own_keep_flags(fusion):
    from gst_visdial_amd import ops
    H, Hv, Hb = SHAPES[1]
    Bn, p = 200, 0.1
    g = torch.Generator().manual_seed(77)
    Pm = dict(xt=torch.randn(Bn, H, generator=g), xv=torch.randn(Bn, Hv, generator=g), wt=torch.randn(Hb, H, generator=g) * 0.03,
              wv=torch.randn(Hb, Hv, generator=g) * 0.03, bt=torch.randn(Hb, generator=g) * 0.1, bv=torch.randn(Hb, generator=g) * 0.1,
              wn=torch.randn(2, Hb, generator=g) * 0.05, bn=torch.randn(2, generator=g) * 0.1, labels=torch.rand(Bn, 2, generator=g))
    rng = ops.Rng(torch.device(DEV), seed=9)
    rng.advance()
    out, _ = _run_train_head(Pm, fusion, torch.float32, p=p, rng=rng, gscale=1.3)
    frac = 1.0 - out["keep"].float().mean().item()
    print("\ndropped fraction over %d x %d: %.4f" % (Bn, Hb, frac))
    assert abs(frac - p) <= 0.01
    ref = _head_reference(Pm, fusion, keep=out["keep"], p=p, gscale=1.3)
    # fp32 arithmetic with fp32 accumulation over K <= 1024 terms against float64: 1e-5 of each tensor's largest element
    for k in ("z", "pt", "pv", "dwn", "dbn", "dpt", "dpv"):
        err = (out[k].double() - ref[k]).abs().max().item() / ref[k].abs().max().item()
        assert err < 1e-5, (k, err)
    assert abs(out["stats"][2].item() - ref["loss"].item()) < 1e-5 * ref["loss"].item()
    out2, _ = _run_train_head(Pm, fusion, torch.float32, p=p, rng=rng, gscale=1.3)
    assert all(torch.equal(_bits(out[k]), _bits(out2[k])) for k in out)


def _random_problem(Bn, H, Hv, Hb, seed):
    """Non-integer operands: every partial sum is rounded, so z depends on the order of the additions."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(xt=rn(Bn, H), xv=rn(Bn, Hv), wt=rn(Hb, H) * 0.1, wv=rn(Hb, Hv) * 0.1, bt=rn(Hb) * 0.1, bv=rn(Hb) * 0.1,
                wn=rn(2, Hb) * 0.1, bn=rn(2) * 0.1, labels=torch.rand(Bn, 2, generator=g))


# H = 272: one full 256-wide bf16 k step plus a 16-element tail; Hb = 144: wave 0 owns two column tiles, the other waves one;
# Bn = 17, 33: a partly filled last workgroup
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fusion", ["mul", "sum"])
@pytest.mark.parametrize("shape", [(64, 96, 128), (272, 48, 144)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Bn", [1, 17, 33])
def test_nsp_head_and_the_training_forward_with_p_0_give_the_same_z_bits_on_random_operands(Bn, shape, fusion, dtype):
    from gst_visdial_amd import ops
    H, Hv, Hb = shape
    Pm = _random_problem(Bn, H, Hv, Hb, seed=31 * Bn + Hb + (fusion == "sum"))
    out, (xt, xv, wt, wv) = _run_train_head(Pm, fusion, dtype)      # p = 0; padded row strides, canaried write windows
    f32 = lambda v: v.to(DEV, torch.float32).contiguous()
    zbuf = _canary((Bn + 2) * 4, torch.float32).view(Bn + 2, 4)
    pbuf = _canary(Bn + 8, torch.float32)
    zh, ph = zbuf[1:Bn + 1, :2], pbuf[4:Bn + 4]
    ops.nsp_head(xt, 3, xv, 2, wt, f32(Pm["bt"]), wv, f32(Pm["bv"]), f32(Pm["wn"]), f32(Pm["bn"]), Bn, fusion, zh, ph)
    torch.cuda.synchronize()
    zi, pi = _bits(zbuf), _bits(pbuf)
    assert bool((zi[0] == POISON).all()) and bool((zi[Bn + 1] == POISON).all()) and bool((zi[:, 2:] == POISON).all())
    assert bool((pi[:4] == POISON).all()) and bool((pi[Bn + 4:] == POISON).all())
    z = zh.clone().cpu()
    assert torch.isfinite(z).all() and bool((z != z.round()).all()) and bool((out["keep"] == 1).all())
    assert torch.equal(_bits(out["z"]), _bits(z))


@pytest.mark.parametrize("rows", [1, 64, 65, 257])
def test_the_shared_row_loss_reduction_counts_exactly_and_sums_within_the_fp32_worst_case(rows):
    """stats = (sum, count, quotient) of the one reduction kernel behind gstvd_ce_fwd (rows whose label is not ignore_index
    count), gstvd_kl_fwd (rows with label 1; no labels: all) and gstvd_nsp_train_fwd (all).  The sum's bound is the worst case
    of ANY order of rows - 1 fp32 additions, (rows - 1) * 2^-24 * sum |row_loss|; 257 is more than one stride of a 256-thread
    block.  (rows = 1: the one row counts -- an all-ignored call has the quotient 0 / 0.)"""
    from gst_visdial_amd import ops
    ops.set_device(torch.device(DEV))
    g = torch.Generator().manual_seed(500 + rows)
    idx = torch.arange(rows)
    skip = (idx % 3 == 0) & (idx < rows - 1)                        # some rows out; the last row always counts
    cases = []

    V, ignore = 37, -1
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[skip] = ignore
    logits = torch.zeros(rows, 40, device=DEV)
    logits[:, :V] = (torch.randn(rows, V, generator=g) * 2.0).to(DEV)
    row_loss, lse, stats = (torch.zeros(n, device=DEV) for n in (rows, rows, 4))
    ops.ce_fwd(logits[:, :V], lab.to(DEV), rows, V, row_loss, lse, stats, ignore_index=ignore)
    cases.append(("ce", row_loss, stats, int((~skip).sum())))

    C = 11
    target = torch.rand(rows, C, generator=g).to(DEV)
    scores = (torch.randn(rows, C, generator=g) * 2.0).to(DEV)
    for name, labels in (("kl, no labels", None), ("kl, 0/1 labels", (~skip).to(torch.int64).to(DEV))):
        row_loss, lse, stats = (torch.zeros(n, device=DEV) for n in (rows, rows, 4))
        ops.kl_fwd(scores, target, rows, C, row_loss, lse, stats, labels=labels)
        cases.append((name, row_loss, stats, rows if labels is None else int((~skip).sum())))

    out, _ = _run_train_head(_random_problem(rows, 64, 96, 128, seed=900 + rows), "mul", torch.float32)
    cases.append(("nsp", out["row"], out["stats"], rows))
    torch.cuda.synchronize()

    for name, row_loss, stats, count in cases:
        row_loss, stats = row_loss.cpu(), stats.cpu()
        s64, a64 = row_loss.double().sum().item(), row_loss.double().abs().sum().item()
        err, bound = abs(stats[0].double().item() - s64), (rows - 1) * 2.0 ** -24 * a64
        print("\n%-15s rows %3d: count %3d, sum %.9g, |sum - sum64| %.3e (bound %.3e)" % (name, rows, stats[1].item(), stats[0].item(), err, bound))
        assert a64 > 0 and torch.isfinite(row_loss).all(), name
        assert stats[1].item() == count, (name, stats[1].item(), count)
        assert torch.equal(_bits(stats[2:3]), _bits(stats[0:1] / stats[1:2])), (name, stats)
        assert err <= bound, (name, err, bound)


# ---------------------------------------------------------------------------------------------- engine level
def _profiled(enc, r, backward=True):
    from gst_visdial_amd import ops
    prof = ops.Profiler()
    with prof:
        lm, img, nsp, z = _call(enc, r)
        if backward:
            sum(x.mean() for x in (lm, img, nsp) if torch.isfinite(x).all()).backward()      # a dropped loss: zero seed
        torch.cuda.synchronize()
    return (lm.detach().cpu(), img.detach().cpu(), nsp.detach().cpu()), [(rec[0], rec[6]) for rec in prof.records]


def test_a_batch_without_masked_regions_or_tokens_gives_nan_for_that_loss_and_launches_nothing_for_the_head(fx):
    enc, params = _enc("fp32")
    r = _rows(fx)
    base, tags = _profiled(enc, r)
    assert {"head.mlm", "head.img", "head.nsp"} <= set(s for _, s in tags)
    word = P + "bert.embeddings.word_embeddings.weight"
    g_full = _grads(enc)
    for key, fill, scope, names in (("image_label", -1, "head.img", ("cls.imagePredictions.",)),
                                    ("mask", -1, "head.mlm", ("cls.predictions.",))):
        r2 = dict(r)
        r2[key] = torch.full_like(r[key], fill)
        enc.zero_grad(set_to_none=True)
        got, tags = _profiled(enc, r2)
        i = 1 if key == "image_label" else 0
        assert torch.isnan(got[i]).all()
        for j in range(3):
            if j != i:
                assert torch.isfinite(got[j]).all() and torch.equal(got[j], base[j]), (key, j)
        assert not [t for t, s in tags if s == scope], [t for t, s in tags if s == scope]
        g = _grads(enc)
        for k, v in g.items():
            if any(n in k for n in names):
                assert v is not None and bool((v == 0).all()), k
        assert g[word] is not None and torch.isfinite(g[word]).all() and (key != "mask" or not torch.equal(g[word], g_full[word]))


def test_ranking_and_the_enc_dec_path_are_bit_equal_before_and_after_a_training_call(fx, tiny_train):
    s = sc()
    enc, params, dfx = s.build_tiny_disc_encoder("fp32", DEV)
    rows = {k[4:]: v.clone() for k, v in dfx.items() if k.startswith("in::")}
    from gst_visdial_amd import evaluate_disc as ED
    model, _, _ = s.build_tiny_model("fp32", DEV, mode="vd_eval_val")
    model.eval()
    kw = s.golden_batch(tiny_train, DEV)
    run = lambda: model(**{k: (v.clone() if v is not None else None) for k, v in kw.items()})
    with torch.no_grad():
        p0 = ED.score_batch(enc, rows, params, rows_per_call=17).clone()
        loss0, logits0 = [x.clone() for x in run()]
    assert enc.engine.flat.G is None
    # a training call on the SAME encoder (weights of the evaluation fixture), then back to ranking
    params["mode"] = "vd_train"
    lm, img, nsp, z = _call(enc, _rows(fx))
    (lm + img + nsp).sum().backward()
    assert enc.engine.flat.G is not None and enc.bert_pretrained.cls.predictions.bias.grad is not None
    params["mode"] = "vd_eval_val"
    with torch.no_grad():
        p1 = ED.score_batch(enc, rows, params, rows_per_call=17)
        loss1, logits1 = run()
    assert torch.equal(p0, p1) and torch.equal(loss0, loss1) and torch.equal(logits0, logits1)


def test_no_torch_math_between_the_encoder_and_the_losses_nor_in_backward(fx):
    from torch.utils._python_dispatch import TorchDispatchMode
    enc, params = _enc("bf16")
    r = _rows(fx)
    lm, img, nsp, _ = _call(enc, r)                                 # first call: flat buffers, arena, gradient buffer
    (lm + img + nsp).sum().backward()

    class Log(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    enc.zero_grad(set_to_none=True)
    log = Log()
    with log:
        lm, img, nsp, _ = _call(enc, r)
        n_fwd = len(log.names)
        (lm + img + nsp).sum().backward()
    torch.cuda.synchronize()
    banned = ("mm", "matmul", "linear", "softmax", "kl_div", "cross_entropy", "nll_loss", "relu", "gelu", "einsum", "layer_norm")
    bad = [n for n in log.names if any(s in n for s in banned)]
    assert not bad, bad
    assert n_fwd > 0 and len(log.names) > n_fwd
    assert torch.isfinite(lm).all() and enc.bert_pretrained.cls.bi_seq_relationship.weight.grad is not None
