"""The listwise loss head (gstvd_rank_loss, csrc/loss.hip) on a real MI355X, through ops.rank_loss only.  Scores are compared bit
for bit with ops.answer_scores; the loss of every round, the probabilities and the per-token upstream gradients with a float64
torch restatement (formed from those scores) at exact_loss.tol(fp32), the tolerance of an fp32 op; the cases the formulas single
out -- a round without relevance, no round with relevance, a candidate of probability zero, [PAD] targets -- exactly.  Every
output sits in a canary window."""
import pytest
import torch

import exact_loss as XL

pytestmark = pytest.mark.gpu

V = 37
CASES = [(dt, E, G, T) for dt in ("f32", "bf16") for E in (1, 5) for G in (1, 3, 100, 130) for T in (1.0, 0.5)]


def ops():
    from gst_visdial_amd import ops as o
    return o


def reference(scores, rel, ids, inv_t):
    """float64: (round_loss [E], p [E, G], g_tok [E, G, U], stats [3]) of the formulas in include/gstvd_hip.h."""
    E, G = rel.shape
    z = scores.double().view(E, G) * inv_t
    logp = torch.log_softmax(z, 1)
    rs = rel.double().sum(1, keepdim=True)
    counts = rs[:, 0] > 0
    t = torch.where(counts[:, None], rel.double() / rs.clamp_min(1e-300), torch.zeros_like(z))
    loss = -torch.where(t > 0, t * logp, torch.zeros_like(z)).sum(1) * counts
    n = float(counts.sum())
    tgt = torch.zeros_like(ids)
    tgt[:, :-1] = ids[:, 1:]
    w = -(logp.exp() - t) * inv_t / max(n, 1.0) * counts[:, None]
    g = w.reshape(-1, 1) * (tgt != 0)
    stats = torch.tensor([float(loss.sum()), n, float(loss.sum()) / n if n else 0.0], dtype=torch.float64)
    return loss, logp.exp(), g.view(E, G, -1), stats


def run(dtype, E, G, U, inv_t, rel, seed, ninf=()):
    """One launch on fresh windows -> dict of outputs (+ the inputs the reference needs); canaries checked."""
    o = ops()
    dev = torch.device("cuda", torch.cuda.current_device())
    dt = XL.DT[dtype]
    gen = XL.generator(9000 + seed, dev)
    rows = E * G
    x = (torch.randn(rows * U, V, generator=gen, device=dev) * 1.5).to(dt).double()
    ids = torch.randint(1, V, (rows, U), generator=gen, device=dev)
    if U > 2:
        ids[::2, U // 2] = 0                                       # [PAD] in the middle of every other row
        ids[1::3, U - 1] = 0
    for (i, u) in ninf:                                            # target logit -inf: the candidate's probability is exactly 0
        x[i * U + u, ids[i, u + 1]] = XL.NEG
    L = torch.logsumexp(x, 1).float()
    pad = (-V) % 4 + 4
    logits, lse, idw = XL.win_in(x, dt, dev, pad=pad), XL.win_in(L.double(), XL.F32, dev), XL.win_in(ids, XL.I64, dev)
    relw = XL.win_in(rel.reshape(-1).double(), XL.F32, dev)
    outs = dict(scores=XL.win_out(1, rows, XL.F32, dev), p=XL.win_out(1, rows, XL.F32, dev), round_loss=XL.win_out(1, E, XL.F32, dev),
                g_tok=XL.win_out(1, rows * U, XL.F32, dev), stats=XL.win_out(1, 3, XL.F32, dev))
    ref_sc = XL.win_out(1, rows, XL.F32, dev)
    o.answer_scores(logits.view, XL.vec(lse), idw.view, rows, U, XL.vec(ref_sc))
    o.rank_loss(logits.view, XL.vec(lse), idw.view, XL.vec(relw), E, G, U, inv_t, *(XL.vec(outs[k]) for k in ("scores", "p", "round_loss", "g_tok", "stats")))
    name = "rank_loss-%s-e%d-g%d-u%d" % (dtype, E, G, U)
    XL.surroundings(list(outs.items()) + [("logits", logits), ("lse", lse), ("ids", idw), ("relevance", relw)], name)
    r = {k: XL.vec(w).clone() for k, w in outs.items()}
    for k, v in r.items():
        assert not bool((XL.bits(v) == XL._canary(XL.F32)).any()), "%s: %s has elements that were never written" % (name, k)
    XL.assert_same_bits(r["scores"], XL.vec(ref_sc), name + ": scores vs answer_scores")
    r.update(ids=ids, name=name)
    return r


def close(got, ref, name, out=print):
    err = XL.rel_to_max(got, ref)
    out("%s: rel-to-max error %.3e (tol %.1e)" % (name, err, XL.tol(XL.F32)))
    assert bool(torch.isfinite(got).all()) and err <= XL.tol(XL.F32), "%s: rel-to-max error %.3e" % (name, err)


def relevance(E, G, seed, dev="cuda"):
    gen = XL.generator(9500 + seed, dev)
    rel = torch.randint(0, 5, (E, G), generator=gen, device=dev).float() * 0.25
    rel = rel * (torch.rand(E, G, generator=gen, device=dev) < 0.4)       # dense annotations are mostly zero
    rel[:, 0] = 1.0                                                     # every round counts ...
    if E > 1:
        rel[1] = 0.0                                                   # ... but the second: no relevance at all
    return rel


@pytest.mark.parametrize("dtype,E,G,T", CASES, ids=["%s-e%d-g%d-t%g" % c for c in CASES])
def test_loss_probabilities_and_token_gradients_match_float64(dtype, E, G, T):
    U = 5 if G < 100 else 3
    rel = relevance(E, G, E * 1000 + G)
    r = run(dtype, E, G, U, 1.0 / T, rel, E * 1000 + G)
    loss, p, g, stats = reference(r["scores"], rel, r["ids"], 1.0 / T)
    close(r["round_loss"], loss, r["name"] + ": round loss")
    close(r["p"], p, r["name"] + ": p")
    close(r["g_tok"], g, r["name"] + ": g_tok")
    close(r["stats"][[0, 2]], stats[[0, 2]].to(r["stats"].device), r["name"] + ": stats")
    assert float(r["stats"][1]) == float(stats[1]) == (E - 1 if E > 1 else 1)
    # [PAD] targets (and the last position) get exactly zero; so does every token of the round without relevance
    tgt = torch.zeros_like(r["ids"])
    tgt[:, :-1] = r["ids"][:, 1:]
    gt = r["g_tok"].view(E * G, U)
    assert int((gt[tgt == 0] != 0).sum()) == 0 and bool((XL.bits(gt[tgt == 0]) == 0).all())
    if E > 1:
        assert bool((XL.bits(gt.view(E, G * U)[1]) == 0).all()) and float(r["round_loss"][1]) == 0.0
        assert G == 1 or bool((gt.view(E, G * U)[0] != 0).any())      # (one candidate: p = t = 1, no gradient)
    r2 = run(dtype, E, G, U, 1.0 / T, rel, E * 1000 + G)
    for k in ("scores", "p", "round_loss", "g_tok", "stats"):
        XL.assert_same_bits(r[k], r2[k], r["name"] + ": repeated launch: " + k)


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_no_round_with_relevance_gives_zero_loss_zero_count_and_no_nan(dtype):
    E, G, U = 3, 7, 4
    r = run(dtype, E, G, U, 1.0, torch.zeros(E, G, device="cuda"), 1)
    assert r["stats"].tolist() == [0.0, 0.0, 0.0] and r["round_loss"].tolist() == [0.0] * E
    assert bool((XL.bits(r["g_tok"]) == 0).all()) and bool(torch.isfinite(r["p"]).all())


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_a_candidate_of_probability_zero_without_relevance_does_not_poison_the_loss(dtype):
    E, G, U = 2, 5, 4
    rel = torch.tensor([[1.0, 0.0, 0.5, 0.0, 0.0], [0.0, 0.0, 0.0, 2.0, 0.0]], device="cuda")
    r = run(dtype, E, G, U, 1.0, rel, 2, ninf=((1, 0), (9, 2)))      # candidates 1 of round 0 and 4 of round 1: t = 0, logp = -inf
    assert float(r["scores"][1]) == XL.NEG and float(r["scores"][9]) == XL.NEG and float(r["p"][1]) == 0.0 and float(r["p"][9]) == 0.0
    loss, p, g, stats = reference(r["scores"], rel, r["ids"], 1.0)
    assert bool(torch.isfinite(loss).all())
    close(r["round_loss"], loss, r["name"] + ": round loss")
    close(r["g_tok"], g, r["name"] + ": g_tok")
    close(r["stats"], stats.to(r["stats"].device), r["name"] + ": stats")
    assert bool((r["g_tok"].view(E * G, U)[[1, 9]] == 0).all())
