"""gstvd_sample_topk_scored on a real MI355X: the draw of gstvd_sample_topk plus, in the same launch, the drawn id's log-probability
under the row's RAW logits.  Rows and windows come from tests/exact_sample.py (logits with ld > V and NaN padding, `out` a strided
column of a canary-filled buffer); `logp` is a strided column of a canary-filled fp32 buffer of its own.  Every launch is repeated
and must return the same bits.

Same ids.      A spread of the exact table's cases runs through the scored entry point: the ids pass the float64 reference of that
               table AND equal those of gstvd_sample_topk on the same windows (torch.equal).
Pointer rows.  Every value is a bf16 number: one hot column holds an integer L, every other column L - 112 - 8k (k in 0..31) or -inf.
               expf(x) adds nothing to 1 for x <= -112, so the normaliser is L bit for bit: the hot token's logp is exactly 0, a cold
               token's exactly -(112 + 8k).  The cold token is drawn at temperature 64 (weights exp(-(112 + 8k) / 64), no underflow)
               with u at the float64 midpoint of its CDF interval: a kernel that normalised the scaled logits, or read another
               column's logit, cannot return -(112 + 8k).  The drawn token carries the smallest k of the row, so it is the likeliest
               cold token; from V = 1023 on top_k = 2 keeps {hot, drawn} (exact_sample's reference requires every kept token to have
               probability >= 2^-10: a midpoint among a thousand kept tokens would sit inside the CDF's own rounding).
               test_premises asserts what these rows rest on, through this kernel itself: a full row of 30521 columns at max - 112
               leaves the sum at 1 and logf(1) == 0, and expf(0) == 1 (V = 1).  (The sum always holds the maximum's 1, so this kernel
               cannot show expf(-112) == 0 on its own; what the rows need is that the cold columns vanish against 1.)
Filters.       Four tokens tied at the maximum, the rest 112 or more below; three of the four are removed -- by `banned`, by the n-gram
               filter, and by both at once -- with top_k = 1 set throughout, so the survivor is the only kept token.  logp is -log 4,
               not 0: neither bans nor top-k enter the normaliser.
Noise rows.    Gaussian logits at scale 2 with offset +60 and at scale 20 (tests/exact_loss.py's noise_logits), logp against float64
               log_softmax of the stored values under that module's row_loss tolerance, tol(F32) * 5 relative to the reference
               maximum (the same arithmetic: a logit minus a log-sum-exp), at that module's vocabulary sizes.  (Not at V = 5: there
               a scale-20 row puts nearly all mass on one token, every |logp| drawn is below 1e-4 and fp32's own rounding of
               1 + 1e-4 is 1e-3 of it -- "relative to the reference maximum" measures nothing; V = 5 is covered exactly above.)
Beam's bits.   "The definition `beam_step` uses": on a gaussian row with a unique maximum, beam_step (one beam, score 0, K = 1) and top_k = 1
               here pick the same token, and score and logp are the same 32 bits (both call csrc/select.h's normaliser)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import exact_loss as EL
import exact_sample as X
from exact_gemm import BF16, F32, Window

pytestmark = pytest.mark.gpu

DEV = "cuda"
NOISE_TOL = EL.tol(F32) * 5


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    """Backend of exact_sample: scored=True sends every launch through ops.sample_topk_scored with a fresh canary-filled logp
    column (kept as self.lp, every result cloned into self.logps)."""

    def __init__(self, scored=True):
        self.device = torch.device(DEV, torch.cuda.current_device())
        self.scored, self.lp, self.logps = scored, None, []

    def sample(self, logits, T, k, u, out, banned=None, ngram=None, top_p=0.0):
        if not self.scored:
            return ops().sample_topk(logits, T, k, u, out, banned, ngram=ngram, top_p=top_p)
        self.lp = Window(logits.shape[0], 1, F32, self.device, "canary", ld=5)
        ops().sample_topk_scored(logits, T, k, u, out, self.lp.view[:, 0], banned, ngram=ngram, top_p=top_p)
        self.lp.assert_surroundings_untouched("logp")
        self.logps.append(self.lp.view[:, 0].clone())


def bits(t):
    return t.contiguous().view(torch.int32)


def ref_logp(row, ids):
    """float64 log_softmax of the row's stored raw logits at `ids`."""
    lp = torch.log_softmax(row.logits.double(), -1)
    return lp[ids]


def launch_twice(be, row, u):
    """Two launches on the same windows -> (ids, logp) of the first, with the second's bits, every window and the canaries checked."""
    L = X.Launch(be, row, u)
    ids = L.run(be)
    again = L.run(be)
    L.assert_windows(row.name)
    a, b = be.logps[-2], be.logps[-1]
    assert torch.equal(ids, again) and torch.equal(bits(a), bits(b)), row.name + ": a second launch returned other bits"
    return ids, a.cpu()


# ---------------------------------------------------------------------------------------------- same ids
SPREAD = ["tie-v1-mid", "tie-v1023-k16-T2-step", "tie-v1024-k1000-mid", "tie-v1025-k17-maxbanned-step", "tie-v30522-k64-mid",
          "iter-v1025-bf16-k7-T0.5-step", "iter-v30522-bf16-k16-T1-mid", "iter-v1024-few-finite-k16-mid", "bis-v1024-k65-T0.5-step",
          "bis-v30522-k1000-mid", "bis-v1025-c-ge-k64-mid", "p-v1025-alone-step", "p-v30522-narrow-k7-mid", "p-v1023-kth-inf-mid",
          "noise-v30522-f32-k40-T0.7-mid", "noise-v30522-bf16-k7-T1.3-step", "noise-v1025-bf16-k17-T1.3-mid",
          "ngram-n2-v1025-f32-k7-mid", "ngram-n4-v30522-f32-k17-step", "ngram-n4-v3073-with-mask-mid", "ngram-n4-v1024-short-prefix-mid"]


@pytest.mark.parametrize("cid", SPREAD)
def test_scored_entry_draws_the_ids_of_sample_topk(cid):
    c = X.BY_ID[cid]
    be = Gpu()
    got = X.run_case(be, c)                                            # the float64 reference, both launches, every window
    a, b = be.logps[-2], be.logps[-1]
    assert torch.equal(bits(a), bits(b)), cid + ": logp of a second launch differs"
    plain = Gpu(scored=False)
    want = X.Launch(plain, c.row, X.probes(c.row, c.kind)[0]).run(plain)
    assert torch.equal(got, want), cid
    ref = ref_logp(c.row, got)
    err = EL.rel_to_max(a.cpu(), ref)
    print("%s: logp rel-to-max error %.3e" % (cid, err))
    assert err <= NOISE_TOL, "%s: logp %.3e (tol %.1e)" % (cid, err, NOISE_TOL)


# ---------------------------------------------------------------------------------------------- pointer rows
def pointer_row(V, dtype, hot, drawn, kc, L):
    """hot column L; column `drawn` L - 112 - 8 kc (the only one at kc); every other column k in kc + 1 .. 31, a few -inf."""
    j = torch.arange(V)
    k = kc + 1 + (j * 7) % (31 - kc)
    lg = (L - 112.0 - 8.0 * k).float()
    for i in (5, 77, 1000, V - 2):
        if 0 <= i < V and i not in (hot, drawn):
            lg[i] = X.NEG
    lg[hot] = float(L)
    if drawn is not None:
        lg[drawn] = L - 112.0 - 8.0 * kc
    assert bool((lg.to(BF16).float() == lg).all())                     # every value is a bf16 number, whatever `dtype`
    name = "pointer-v%d-%s-hot%d-drawn%s-k%d-L%d" % (V, dtype, hot, drawn, kc, L)
    return X.Row(name, V, dtype, lg, 1.0, 1, 0.0, None, None, False, None)


POINTER = [(1, 0, None, 0, 40), (5, 0, 4, 0, 40), (5, 4, 0, 9, -24), (1023, 0, 1022, 5, 0), (1023, 1022, 0, 17, 96),
           (1024, 1023, 0, 30, 40), (1024, 0, 1023, 0, -24), (1025, 1024, 1023, 9, 40), (1025, 1023, 1024, 17, 0), (1025, 0, 1024, 5, 96),
           (30522, 0, 30521, 30, 40), (30522, 30521, 1024, 0, 96), (30522, 1023, 0, 17, -24), (30522, 1024, 1023, 9, 0)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V,hot,drawn,kc,L", POINTER)
def test_pointer_rows_are_exact(V, hot, drawn, kc, L, dtype):
    be = Gpu()
    row = pointer_row(V, dtype, hot, drawn, kc, L)
    # top_k = 1: the hot column, at any u; its log-probability is exactly 0
    ids, lp = launch_twice(be, row, torch.tensor([X.U_FIRST, 0.5, X.U_LAST], dtype=torch.float32))
    assert ids.tolist() == [hot] * 3 and bool((lp == 0).all()), (row.name, ids.tolist(), lp.tolist())
    if drawn is None:
        return
    # temperature 64: u at the float64 midpoints of the hot and of the drawn cold token's CDF intervals
    warm = row._replace(name=row.name + "-T64", T=64.0, k=0 if V <= 5 else 2)
    r = X.reference(warm)
    kept = [int(i) for i in r.kept]
    assert hot in kept and drawn in kept and (V <= 5 or len(kept) == 2)
    start = r.cdf - r.prob
    u = [np.float32((start[kept.index(t)] + r.cdf[kept.index(t)]) / 2) for t in (hot, drawn)]
    ids, lp = launch_twice(be, warm, torch.tensor(np.array(u, dtype=np.float32)))
    assert ids.tolist() == [hot, drawn], (warm.name, ids.tolist())
    assert lp.tolist() == [0.0, -(112.0 + 8 * kc)], (warm.name, lp.tolist())


def test_premises():
    """What the pointer rows rest on, for the functions THIS kernel uses (expf, logf): 30521 columns at max - 112 leave the sum at 1
    and logf(1) == 0 (logp of the maximum is +0 or -0 ... by value 0, and not a single ulp off), and expf(0) == 1 on a row of one."""
    be = Gpu()
    for dtype in ("f32", "bf16"):
        lg = torch.full((30522,), 40.0 - 112.0)
        lg[17] = 40.0
        row = X.Row("premise-cold-%s" % dtype, 30522, dtype, lg, 1.0, 1, 0.0, None, None, False, None)
        ids, lp = launch_twice(be, row, torch.tensor([0.5], dtype=torch.float32))
        assert ids.tolist() == [17] and lp.tolist() == [0.0], "premise: expf(x <= -112) vanishes against 1, logf(1) == 0; got %r" % lp.tolist()
        one = X.Row("premise-one-%s" % dtype, 1, dtype, torch.tensor([-3.0]), 1.0, 0, 0.0, None, None, False, None)
        ids, lp = launch_twice(be, one, torch.tensor([0.5], dtype=torch.float32))
        assert ids.tolist() == [0] and lp.tolist() == [0.0], "premise: logf(expf(0)) == 0; got %r" % lp.tolist()


# ---------------------------------------------------------------------------------------------- filters stay out of the normaliser
TIED = (7, 500, 1023, 1024)                                            # the survivor is the last one


def tied_row(V, dtype, how):
    j = torch.arange(V)
    lg = (2.0 - 112.0 - 8.0 * (j % 5)).float()
    lg[torch.tensor(TIED)] = 2.0
    ban = torch.zeros(V, dtype=torch.bool)
    ngram = None
    p, q = 300, 301                                                    # the generated prefix: ordinary tokens, not among the tied
    by_mask = {"banned": TIED[:3], "ngram": (), "both": TIED[:1]}[how]
    by_ngram = {"banned": (), "ngram": TIED[:3], "both": TIED[1:3]}[how]
    for t in by_mask:
        ban[t] = True
    if by_ngram:
        ngram = X.ng(2, [q, p], [(p, t) for t in by_ngram], end=(p,))
    return X.Row("tied4-v%d-%s-%s" % (V, dtype, how), V, dtype, lg, 0.7, 1, 0.0, ban if by_mask else None, ngram, False, None)


@pytest.mark.parametrize("how", ["banned", "ngram", "both"])
@pytest.mark.parametrize("V,dtype", [(1025, "f32"), (30522, "bf16")])
def test_bans_and_top_k_do_not_enter_the_normaliser(V, dtype, how):
    be = Gpu()
    row = tied_row(V, dtype, how)
    assert [int(i) for i in X.reference(row).kept] == [TIED[3]]
    ids, lp = launch_twice(be, row, torch.tensor([X.U_FIRST, 0.3, 0.9, X.U_LAST], dtype=torch.float32))
    assert ids.tolist() == [TIED[3]] * 4, ids.tolist()
    err = (lp.double() + math.log(4.0)).abs().max().item() / math.log(4.0)
    print("%s: logp %r, -log 4 = %.9g, rel error %.3e" % (row.name, lp.tolist(), -math.log(4.0), err))
    assert err <= NOISE_TOL, (row.name, lp.tolist())


# ---------------------------------------------------------------------------------------------- noise rows
@pytest.mark.parametrize("kind", ["offset", "scaled"])
@pytest.mark.parametrize("V,B", [(1025, 64), (2049, 7), (30522, 16)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_noise_rows_follow_float64_log_softmax(dtype, V, B, kind):
    be = Gpu()
    dt = X.DT[dtype]
    gen = EL.generator(9100 + V, be.device)
    x = EL.noise_logits(B, V, kind, dt, gen, be.device)                # float64 image of the STORED values
    logits = Window(B, V, dt, be.device, "poison", ld=V + (8 if dt == BF16 else 4)).set(x.to(dt))
    u = Window(1, B, F32, be.device, "poison").set(torch.rand(B, generator=gen, device=be.device).clamp_(2.0 ** -20, 1 - 2.0 ** -20))
    got = []
    for rep in range(2):
        out = Window(B, 1, torch.int64, be.device, "canary", ld=3)
        be.sample(logits.view, 0.7, 7, u.vector(), out.view[:, 0], None)
        out.assert_surroundings_untouched("noise: out")
        got.append((out.view[:, 0].clone(), be.logps[-1]))
    logits.assert_surroundings_untouched("noise: logits")
    u.assert_surroundings_untouched("noise: u")
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(bits(got[0][1]), bits(got[1][1]))
    ids, lp = got[0]
    plain = torch.empty(B, dtype=torch.int64, device=be.device)
    ops().sample_topk(logits.view, 0.7, 7, u.vector(), plain, None)
    assert torch.equal(ids, plain)
    ref = torch.log_softmax(x, -1).gather(1, ids.view(-1, 1))[:, 0]
    err = EL.rel_to_max(lp, ref)
    print("noise-%s-v%d-%s: logp rel-to-max error %.3e (largest |logp| %.3f)" % (dtype, V, kind, err, ref.abs().max().item()))
    assert err <= NOISE_TOL, "noise-%s-v%d-%s: logp %.3e (tol %.1e)" % (dtype, V, kind, err, NOISE_TOL)


# ---------------------------------------------------------------------------------------------- the definition beam_step uses
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [600, 1025, 30522])
def test_logp_has_the_bits_of_the_beam_steps_score(V, dtype):
    """ops.sample_topk_scored promises "the definition `beam_step` uses": on a gaussian row with a unique maximum, one beam with
    score 0 and K = 1 scores its best token 0 + ((z - max) - lse); top_k = 1 draws that token, and its logp holds the same 32 bits."""
    o, dev = ops(), torch.device(DEV, torch.cuda.current_device())
    x = torch.randn(1, V, generator=torch.Generator().manual_seed(77 + V)) * 2.5
    x[0, V - 3] = x.max() + 1.5
    x = x.to(X.DT[dtype]).to(dev)
    assert int((x == x.max()).sum()) == 1
    zero, live = torch.zeros(1, 1, device=dev), torch.zeros(1, 1, dtype=torch.int32, device=dev)
    score, done, parent = torch.full_like(zero, 7.0), torch.zeros_like(live), torch.zeros_like(live)
    ids = torch.full((1, 1), -1, dtype=torch.int64, device=dev)
    o.beam_step(x, zero, live, score, done, parent, ids, 0, o.beam_workspace(1, 1, dev), eos=V, pad=0)
    out, lp = torch.full((1,), -1, dtype=torch.int64, device=dev), torch.full((1,), 7.0, device=dev)
    o.sample_topk_scored(x, 1.0, 1, torch.full((1,), 0.5, device=dev), out, lp)
    assert ids.item() == out.item() == V - 3
    print("V=%d %s: beam score %r, sampler logp %r" % (V, dtype, score.item(), lp.item()))
    assert torch.equal(bits(score.view(1)), bits(lp)), (score.item(), lp.item())


# ---------------------------------------------------------------------------------------------- other cases
def test_an_all_banned_row_draws_id_zero_and_reports_its_log_probability():
    be = Gpu()
    X.all_banned_case(be)                                              # zeros: id 0, logp -log V
    assert EL.rel_to_max(be.logps[-1].cpu(), torch.full((4,), -math.log(1025.0), dtype=torch.float64)) <= NOISE_TOL
    for hot, want in ((0, 0.0), (1024, -(112.0 + 8 * 3))):             # pointer rows: exact
        row = pointer_row(1025, "bf16", hot, 0 if hot else None, 3, 40)._replace(name="all-banned-hot%d" % hot, k=7, p=0.5,
                                                                                   ban=torch.ones(1025, dtype=torch.bool))
        ids, lp = launch_twice(be, row, torch.tensor([X.U_FIRST, 0.5, X.U_LAST], dtype=torch.float32))
        assert ids.tolist() == [0] * 3 and lp.tolist() == [want] * 3, (hot, ids.tolist(), lp.tolist())


def _launch():
    be = Gpu()
    row = X.BY_ID["iter-v97-f32-k7-T1-mid"].row
    return be, X.Launch(be, row, X.probes(row, "mid")[0])


def test_refusals_of_the_wrapper_come_before_any_launch():
    be, L = _launch()
    o, B = ops(), L.B
    out, u, lg = L.out.view[:, 0], L.u.vector(), L.logits.view
    lpw = Window(B, 1, F32, be.device, "canary", ld=3)
    lp = lpw.view[:, 0]
    for kw in (dict(u=u.double()), dict(u=u[:B - 1]), dict(out=out.int()), dict(out=out[:B - 1]), dict(logp=lp.double()), dict(logp=lp[:B - 1]),
               dict(logp=lp.cpu()), dict(logp=None), dict(logp=lpw.view), dict(banned=torch.zeros(B, 96, dtype=torch.bool, device=be.device))):
        a = dict(u=u, out=out, logp=lp, banned=None)
        a.update(kw)
        with pytest.raises(Exception, match="sample_topk_scored|GPU tensors"):
            o.sample_topk_scored(lg, 1.0, 7, a["u"], a["out"], a["logp"], a["banned"])
    L.assert_windows("refusals")
    lpw.assert_surroundings_untouched("refusals: logp")
    assert bool((out == X.CANARY[torch.int64]).all()) and bool((bits(lp) == X.CANARY[F32]).all())          # nothing was launched


def test_refusals_of_the_entry_point():
    be, L = _launch()
    o = ops()
    out, u, lg = L.out.view[:, 0], L.u.vector(), L.logits.view
    lpw = Window(L.B, 1, F32, be.device, "canary", ld=3)
    lp = lpw.view[:, 0]
    for (T, k, p) in ((0.0, 7, 0.0), (-1.0, 7, 0.0), (float("nan"), 7, 0.0), (1.0, -1, 0.0), (1.0, 7, -0.25), (1.0, 7, float("nan"))):
        with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
            o.sample_topk_scored(lg, T, k, u, out, lp, None, top_p=p)
    wide = torch.zeros(2, 31745, device=be.device)
    with pytest.raises(Exception, match="GSTVD_E_UNSUPPORTED"):
        o.sample_topk_scored(wide, 1.0, 7, u[:2].contiguous(), torch.zeros(2, dtype=torch.int64, device=be.device), torch.zeros(2, device=be.device))
    from gst_visdial_amd import _lib as Lb
    lib = Lb.load()

    def desc(**over):
        d = Lb.SampleDesc()
        d.logits, d.ld, d.dtype, d.B, d.V, d.top_k, d.temperature = lg.data_ptr(), lg.stride(0), o.dt(lg), L.B, 97, 7, 1.0
        d.u, d.out, d.out_stride = u.data_ptr(), out.data_ptr(), out.stride(0)
        for k_, v in over.items():
            setattr(d, k_, v)
        return d

    def rc(d, logp=lp.data_ptr(), stride=lp.stride(0)):
        return Lb.status_name(lib.gstvd_sample_topk_scored(C.byref(d) if d is not None else None, logp, stride, None))

    assert rc(None) == "GSTVD_E_NULL"
    assert rc(desc(ld=96)) == "GSTVD_E_SHAPE"
    for name in ("logits", "u", "out"):
        assert rc(desc(**{name: None})) == "GSTVD_E_NULL"
    assert rc(desc(ngram=2, hist=None, ids_tm=None)) == "GSTVD_E_NULL"
    assert rc(desc(dtype=7)) == "GSTVD_E_DTYPE"
    assert rc(desc(), logp=None) == "GSTVD_E_NULL"
    for s in (0, -1, -3):
        assert rc(desc(), stride=s) == "GSTVD_E_SHAPE"
    torch.cuda.synchronize()
    L.assert_windows("refusals")
    lpw.assert_surroundings_untouched("refusals: logp")
    assert bool((out == X.CANARY[torch.int64]).all())
    assert bool((bits(lp) == X.CANARY[F32]).all())                     # nothing was launched
