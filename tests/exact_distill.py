"""Exact layer of the soft pseudo-label tests ("Soft pseudo-labels"): csrc/distill.hip -- gstvd_topk_logp,
gstvd_distill_fwd, gstvd_distill_bwd -- on inputs whose answer is known, in the manner of tests/exact_loss.py, whose pointer rows,
noise rows, windows and tolerances it reuses unchanged.

Top-K.  Rows of integers (exact in bf16) with the winners on the borders of the kernel's loops: the first vectors, both sides of
the 1024-column and of the 4096-column stride (a thread's next vector), the last vector, the start of the scalar tail, the last
column.  A row of distinct winners, a row whose winners are all tied (the smaller id first), a row with fewer than K finite values
(it ends in -inf entries, smaller id first), a constant row (ids 0 .. K - 1), a random row with -inf holes.  lse is an integer, so
logp = x[id] - lse is exact: ids and logp are compared bit for bit with a stable descending sort in float64.

Backward, exact.  exact_loss's pointer rows: softmax is exactly one-hot at tau = 1 and lse_tau == lse == L.  K = 2 equal soft_logp
give q = (1/2, 1/2) exactly; alpha and gs are powers of two, the counted rows 4.  A kept row with a soft label is then
  gs / 4 * ((1 - a) * ([v == hot] - [v == label]) + a * ([v == hot] - ([v == id_0] + [v == id_1]) / 2))
to the last bit, zeros elsewhere and in the padding; the rows without a soft label (soft_ids[m, 0] == -1; an id outside [0, V)) are
the cross entropy's, the ignored row is zero.  Hot column, label and ids rotate over the borders; one row has both ids on one
column (duplicates add up), one has an id on the hot column.  alpha == 0 is compared with gstvd_ce_bwd on noise rows bit for bit.

Forward and tau != 1.  Noise rows (exact_loss.noise_logits) against float64 torch of the STORED values, soft labels from the top-4 of
a second noise row, one row without a soft label: row_loss, row_kd, lse_tau under tol(fp32) x 5 and dlogits under tol(dtype) x 2,
relative to the reference maximum -- exact_loss.check_ce_noise's bars for the cross entropy's row_loss and dlogits.

Every output is a window inside a canary-filled allocation, every input a window inside a NaN-poisoned one (integers: canary),
ldl != ldd, every launch is repeated and must return the same bits.

Plain helper module: every check takes a backend `be` (be.device, be.ce_fwd, be.ce_bwd, be.topk_logp, be.distill_fwd,
be.distill_bwd), so tests/test_exact_distill_harness_cpu.py proves it on the CPU against a stand-in written in torch and
tests/test_distill_exact_gpu.py runs it on the HIP kernels.
"""
import torch

import exact_gemm as E
import exact_loss as X
from exact_loss import DT, F32, I64, NEG, assert_same_bits, assert_equal_values, rel_to_max, surroundings, tol, vec, win_in, win_out

IGNORE = 0                 # the noise rows: [PAD], as the engine has it
IGNORE_EXACT = -1          # the pointer rows: every border column can be a label


def borders(V):
    """exact_loss.border_columns' borders plus both sides of the 4096-column stride of the top-K kernel's threads."""
    V4 = V & ~3
    c = [0, 3, 4, 1023, 1024, 4095, 4096, V4 - 1, V4, V - 1]
    return sorted(set(x for x in c if 0 <= x < V))


def _dims(V):
    V4 = -(-V // 4) * 4
    return V4 + 4, V4 + 8            # ldl, ldd


# ============================================================================================== top-K
TOPK_V = (5, 1023, 1025, 4099, 30522)
TOPK_K = (1, 4, 16)
TOPK_CASES = [(dtype, V, K) for dtype in ("f32", "bf16") for V in TOPK_V for K in TOPK_K if K <= V]


def topk_rows(V, K, gen, dev):
    """[5, V] float64 integer rows (see the module text) and the integer lse handed in."""
    b = borders(V)
    M = 5
    x = torch.randint(-120, -19, (M, V), generator=gen, device=dev).double()
    order = torch.randperm(len(b), generator=E.generator(V + K, "cpu")).tolist()
    for r, j in enumerate(order):                          # row 0: distinct winners, best first in a shuffled column order
        x[0, b[j]] = 100 - r
    x[1, b] = 50                                           # row 1: every border tied
    x[2, :] = NEG                                          # row 2: fewer than K finite values, at the LAST borders
    for r, c in enumerate(b[::-1][:min(K - 1, len(b))]):
        x[2, c] = -3 - (r // 2)                            # (pairs of them tied)
    x[3, :] = -7                                           # row 3: constant
    hole = torch.rand(V, generator=gen, device=dev) < 0.125
    x[4] = torch.where(hole, torch.full_like(x[4], NEG), x[4])
    lse = torch.tensor([7.0, -3.0, 0.0, 12.0, -20.0], dtype=torch.float64, device=dev)
    return x, lse


def check_topk(be, dtype, V, K):
    dev, dt = be.device, DT[dtype]
    name = "topk-%s-v%d-k%d" % (dtype, V, K)
    x, lse = topk_rows(V, K, E.generator(9100 + V + K, dev), dev)
    M = x.shape[0]
    vals, idx = torch.sort(x, dim=1, descending=True, stable=True)       # value descending, then smaller id
    ref_ids, ref_logp = idx[:, :K].contiguous(), vals[:, :K] - lse[:, None]
    if K > 1:
        assert bool(torch.isinf(ref_logp[2, -1])) and bool(torch.isfinite(ref_logp[0]).all())
    logits, lw = win_in(x, dt, dev, pad=_dims(V)[0] - V), win_in(lse, F32, dev)
    got = []
    for rep in range(2):
        ids, logp = win_out(M, K, I64, dev), win_out(M, K, F32, dev)
        be.topk_logp(logits.view, vec(lw), M, V, K, ids.view, logp.view)
        assert torch.equal(ids.view, ref_ids), "%s: ids %r against %r" % (name, ids.view.tolist(), ref_ids.tolist())
        E.assert_bit_equal(logp.view, ref_logp, name + ": logp = x[id] - lse")
        surroundings((("ids", ids), ("logp", logp)), name)
        got.append((ids.view.clone(), logp.view.clone()))
    assert torch.equal(got[0][0], got[1][0])
    assert_same_bits(got[0][1], got[1][1], name + ": logp of the repeated launch")
    surroundings((("logits", logits), ("lse", lw)), name)
    assert torch.equal(logits.view.double(), x), name + ": the logits were written"


# ============================================================================================== backward, exact
BWD_V = (5, 1025, 4099, 30522)
BWD_PARAMS = ((0.5, 1.0), (0.25, -2.0), (0.5, 0.5))          # (alpha, gs): powers of two
BWD_CASES = [(dtype, V, rot) for dtype in ("f32", "bf16") for V in BWD_V for rot in range(3)]
PLAN = ("soft", "dup", "none", "oor", "ignored")           # counted rows: 4


class ExactProblem(object):
    """Five pointer rows: a soft row, a soft row whose two ids coincide (on the hot column when rot is odd), a row with
    soft_ids[m, 0] == -1, a row with an id outside [0, V), an ignored row with a valid soft label."""

    def __init__(self, be, dtype, V, rot):
        dev = be.device
        self.be, self.dev, self.dt, self.V, self.rot = be, dev, DT[dtype], V, rot
        self.alpha, self.gs = BWD_PARAMS[rot % len(BWD_PARAMS)]
        b = borders(V)
        n = len(b)
        pick = lambda i: b[(i + 2 * rot) % n]
        M = len(PLAN)
        hot = [pick(3 * m) for m in range(M)]
        lab = [pick(3 * m + 1 + (m % 2)) for m in range(M)]
        ids = [[pick(3 * m + 2), pick(3 * m + 4)] for m in range(M)]
        ids[1] = [hot[1], hot[1]] if rot % 2 else [pick(5), pick(5)]
        ids[2] = [-1, pick(1)]
        ids[3] = [pick(2), V + (0, 3, 1 << 40)[rot % 3]]
        lab[4] = IGNORE_EXACT
        self.hot, self.lab, self.ids, self.M = hot, lab, ids, M
        avoid = [tuple([lab[m]] + [i for i in ids[m] if 0 <= i < V]) for m in range(M)]
        gen = E.generator(9300 + V + rot, dev)
        self.x, self.L = X.pointer_rows(M, V, hot, avoid, gen, dev)
        self.ldl, self.ldd = _dims(V)
        self.logits = win_in(self.x, self.dt, dev, pad=self.ldl - V)
        self.labels = win_in(torch.tensor(lab, dtype=I64, device=dev), I64, dev)
        self.sid = win_in(torch.tensor(ids, dtype=I64, device=dev), I64, dev)
        self.slp = win_in(torch.full((M, 2), -1.0, dtype=torch.float64, device=dev), F32, dev)
        self.gsw = win_in(torch.tensor([self.gs], dtype=torch.float64, device=dev), F32, dev)
        self.soft = [True, True, False, False, False]
        self.kept = [True, True, True, True, False]
        count = 4.0
        a, gsn = self.alpha, self.gs / count
        d = torch.zeros(M, self.ldd, dtype=torch.float64, device=dev)
        kd = torch.zeros(M, dtype=torch.float64, device=dev)
        ce = torch.zeros(M, dtype=torch.float64, device=dev)
        for m in range(M):
            if not self.kept[m]:
                continue
            ce[m] = self.L[m] - self.x[m, lab[m]]
            if self.soft[m]:
                d[m, hot[m]] += gsn
                d[m, lab[m]] -= gsn * (1 - a)
                for i in ids[m]:
                    d[m, i] -= gsn * a * 0.5
                    kd[m] += 0.5 * (-torch.log(torch.tensor(2.0, dtype=torch.float64)) - (self.x[m, i] - self.L[m]))
            else:
                d[m, hot[m]] += gsn
                d[m, lab[m]] -= gsn
        self.d_ref, self.kd_ref, self.ce_ref = d, kd, ce
        am = torch.tensor([a if s else 0.0 for s in self.soft], dtype=torch.float64, device=dev)
        self.loss_ref = (1 - am) * ce + am * kd
        assert bool(torch.isfinite(self.loss_ref).all())

    def forward(self, name):
        be, M, V, dev = self.be, self.M, self.V, self.dev
        rl, lse, st = (win_out(1, n, F32, dev) for n in (M, M, 3))
        be.ce_fwd(self.logits.view, vec(self.labels), M, V, vec(rl), vec(lse), vec(st), IGNORE_EXACT)
        E.assert_bit_equal(vec(lse), self.L, name + ": lse == L")
        dl_, kd, lt, so = (win_out(1, n, F32, dev) for n in (M, M, M, 3))
        be.distill_fwd(self.logits.view, vec(self.labels), self.sid.view, self.slp.view, M, V, self.alpha, 1.0, vec(rl), vec(dl_), vec(kd),
                       vec(lt), vec(so), IGNORE_EXACT)
        want_lt = torch.where(torch.tensor(self.soft, device=dev), self.L, torch.zeros_like(self.L))
        E.assert_bit_equal(vec(lt), want_lt, name + ": lse_tau == L at tau = 1 on the rows with a soft label, 0 elsewhere")
        for m in range(M):
            if not self.soft[m]:
                assert X.bits(vec(kd))[m] == 0, "%s: row_kd of row %d (%s) must be +0" % (name, m, PLAN[m])
                assert X.bits(vec(dl_))[m] == X.bits(vec(rl))[m], "%s: row_loss of row %d (%s) is the cross entropy's" % (name, m, PLAN[m])
        e_kd, e_l = rel_to_max(vec(kd), self.kd_ref), rel_to_max(vec(dl_), self.loss_ref)
        assert e_kd <= tol(F32) * 5 and e_l <= tol(F32) * 5, "%s: row_kd %.3e row_loss %.3e (tol %.1e)" % (name, e_kd, e_l, tol(F32) * 5)
        s = vec(so)
        assert s[1].item() == 4.0 and abs(s[0].item() - self.loss_ref.sum().item()) <= tol(F32) * 5 * self.loss_ref.abs().max().item() * M
        assert X.bits((s[0] / s[1]).reshape(1))[0] == X.bits(s[2].reshape(1))[0], name + ": stats[2] is the quotient"
        surroundings((("row_loss", dl_), ("row_kd", kd), ("lse_tau", lt), ("stats", so), ("ce row_loss", rl)), name)
        return lse, lt, so, (dl_, kd)

    def backward(self, lse, lt, so, name):
        be, M, V = self.be, self.M, self.V
        dl = win_out(M, self.ldd, self.dt, self.dev)
        be.distill_bwd(self.logits.view, vec(self.labels), self.sid.view, self.slp.view, vec(lse), vec(lt), vec(so), vec(self.gsw), M, V,
                       self.alpha, 1.0, dl.view, IGNORE_EXACT)
        assert_equal_values(dl.view, self.d_ref, name + ": dlogits (hot column, label, the two soft ids; zeros elsewhere and in the padding)")
        surroundings((("dlogits", dl),), name)
        return dl

    def inputs_untouched(self, name):
        surroundings((("logits", self.logits), ("labels", self.labels), ("soft_ids", self.sid), ("soft_logp", self.slp), ("gscale", self.gsw)), name)
        assert torch.equal(self.logits.view.double(), self.x), name + ": the logits were written"


def check_bwd_exact(be, dtype, V, rot):
    p = ExactProblem(be, dtype, V, rot)
    name = "distill_exact-%s-v%d-rot%d-a%g-gs%g" % (dtype, V, rot, p.alpha, p.gs)
    lse, lt, so, f1 = p.forward(name)
    lse2, lt2, so2, f2 = p.forward(name + " (repeated)")
    for tag, a, b in (("lse_tau", lt, lt2), ("stats", so, so2), ("row_loss", f1[0], f2[0]), ("row_kd", f1[1], f2[1])):
        assert_same_bits(a.view, b.view, "%s: %s of the repeated launch" % (name, tag))
    dl = p.backward(lse, lt, so, name)
    dl2 = p.backward(lse, lt, so, name + " (repeated)")
    assert_same_bits(dl.view, dl2.view, name + ": dlogits of the repeated launch")
    # the rows without a soft label against the cross entropy's own backward (mean form), bit for bit
    rl, lse_c, st = (win_out(1, n, F32, p.dev) for n in (p.M, p.M, 3))
    be.ce_fwd(p.logits.view, vec(p.labels), p.M, V, vec(rl), vec(lse_c), vec(st), IGNORE_EXACT)
    dc = win_out(p.M, p.ldd, p.dt, p.dev)
    be.ce_bwd(p.logits.view, vec(p.labels), vec(lse_c), vec(st), vec(p.gsw), True, p.M, V, dc.view, IGNORE_EXACT)
    for m in (2, 3, 4):
        assert_same_bits(dl.view[m], dc.view[m], "%s: row %d (%s) against gstvd_ce_bwd" % (name, m, PLAN[m]))
    p.inputs_untouched(name)


# ============================================================================================== noise rows
NOISE_V = (1025, 30522)
TAUS = (0.5, 2.0)
NOISE_CASES = [(dtype, V, kind, tau) for dtype in ("f32", "bf16") for V in NOISE_V for kind in ("gauss", "offset", "scaled") for tau in TAUS]
ALPHA0_CASES = [(dtype, V) for dtype in ("f32", "bf16") for V in (1030, 30522)]
MEASURED = {}


def noise_problem(be, dtype, V, kind, seed, K=4, M=4):
    """Student noise rows, labels, and soft labels from the top-K of a teacher noise row (fp32 log-probabilities as stored); row 1
    has no soft label, row 2 is ignored."""
    dev, dt = be.device, DT[dtype]
    gen = E.generator(seed, dev)
    x = X.noise_logits(M, V, kind, dt, gen, dev)
    t = X.noise_logits(M, V, "gauss", F32, gen, dev)
    lab = torch.randint(1, V, (M,), generator=gen, device=dev)
    lab[0] = V - 1
    lab[2] = IGNORE
    tl, ti = torch.topk(torch.log_softmax(t, -1), K, dim=-1)
    ti[0, 1] = V - 1                                          # a soft id in the scalar tail, one on column 0
    ti[3, 2] = 0
    ti[1, 0] = -1
    tl = tl.float().double()
    return x, lab, ti, tl


def noise_reference(x, lab, sid, slp, alpha, tau, gs=1.0):
    """float64: (row_loss, row_kd, lse_tau, dlogits [M, V]) of the rule in include/gstvd_hip.h."""
    M, V = x.shape
    keep = lab != IGNORE
    soft = keep & (sid[:, 0] >= 0) & ((sid >= 0) & (sid < V)).all(-1)
    lp = torch.log_softmax(x, -1)
    ce = torch.where(keep, -torch.gather(lp, 1, lab.clamp(0, V - 1).view(-1, 1))[:, 0], torch.zeros(M, dtype=torch.float64, device=x.device))
    lpt = torch.log_softmax(x / tau, -1)
    lq = torch.log_softmax(slp / tau, -1)
    q = lq.exp()
    at = torch.gather(lpt, 1, sid.clamp(0, V - 1))
    kd = torch.where(soft, (q * (lq - at)).sum(-1), torch.zeros_like(ce))
    lt = torch.where(soft, torch.logsumexp(x / tau, -1), torch.zeros_like(ce))
    a = torch.where(soft, torch.full_like(ce, alpha), torch.zeros_like(ce))
    loss = (1 - a) * ce + a * tau * tau * kd
    qd = torch.zeros_like(x)
    qd.scatter_add_(1, sid.clamp(0, V - 1), q * soft[:, None])
    d = (1 - a)[:, None] * (lp.exp() - torch.nn.functional.one_hot(lab, V).double()) + (a * tau)[:, None] * (lpt.exp() - qd)
    d = d * keep[:, None] * (gs / float(keep.sum()))
    return loss, kd, lt, d


def _run_noise(be, dt, x, lab, sid, slp, alpha, tau, name):
    dev = be.device
    M, V = x.shape
    ldl, ldd = _dims(V)
    logits, labels = win_in(x, dt, dev, pad=ldl - V), win_in(lab, I64, dev)
    sw, lw = win_in(sid, I64, dev), win_in(slp, F32, dev)
    gs = win_in(torch.ones(1, dtype=torch.float64, device=dev), F32, dev)
    out = []
    for rep in range(2):
        rl, lse, st = (win_out(1, n, F32, dev) for n in (M, M, 3))
        be.ce_fwd(logits.view, vec(labels), M, V, vec(rl), vec(lse), vec(st), IGNORE)
        l, kd, lt, so = (win_out(1, n, F32, dev) for n in (M, M, M, 3))
        be.distill_fwd(logits.view, vec(labels), sw.view, lw.view, M, V, alpha, tau, vec(rl), vec(l), vec(kd), vec(lt), vec(so), IGNORE)
        dl = win_out(M, ldd, dt, dev)
        be.distill_bwd(logits.view, vec(labels), sw.view, lw.view, vec(lse), vec(lt), vec(so), vec(gs), M, V, alpha, tau, dl.view, IGNORE)
        surroundings((("row_loss", l), ("row_kd", kd), ("lse_tau", lt), ("stats", so), ("dlogits", dl), ("ce row_loss", rl), ("lse", lse), ("ce stats", st)), name)
        out.append(dict(row_loss=vec(l).clone(), row_kd=vec(kd).clone(), lse_tau=vec(lt).clone(), stats=vec(so).clone(), dlogits=dl.view.clone(),
                        ce_row_loss=vec(rl).clone(), ce_stats=vec(st).clone(), lse=vec(lse).clone(), st=st, labels=labels, logits=logits, gs=gs))
    for k in ("row_loss", "row_kd", "lse_tau", "stats", "dlogits"):
        assert_same_bits(out[0][k], out[1][k], "%s: %s of the repeated launch" % (name, k))
    surroundings((("logits", logits), ("labels", labels), ("soft_ids", sw), ("soft_logp", lw), ("gscale", gs)), name)
    assert torch.equal(logits.view.double(), x), name + ": the logits were written"
    return out[0]


def check_noise(be, dtype, V, kind, tau):
    dt = DT[dtype]
    name = "distill_noise-%s-v%d-%s-tau%g" % (dtype, V, kind, tau)
    x, lab, sid, slp = noise_problem(be, dtype, V, kind, 9500 + V)
    alpha = 0.5
    got = _run_noise(be, dt, x, lab, sid, slp, alpha, tau, name)
    loss, kd, lt, d = noise_reference(x, lab, sid, slp, alpha, tau)
    e = dict(row_loss=rel_to_max(got["row_loss"], loss), row_kd=rel_to_max(got["row_kd"], kd), lse_tau=rel_to_max(got["lse_tau"], lt),
             dlogits=rel_to_max(got["dlogits"][:, :V], d), mean=abs(got["stats"][2].item() - loss.sum().item() / 3.0) / (loss.sum().item() / 3.0))
    MEASURED[name] = e
    print("%s: rel-to-max errors %s" % (name, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    for k in ("row_loss", "row_kd", "lse_tau"):
        assert e[k] <= tol(F32) * 5, "%s: %s %.3e (tol %.1e)" % (name, k, e[k], tol(F32) * 5)
    assert e["dlogits"] <= tol(dt) * 2, "%s: dlogits %.3e (tol %.1e)" % (name, e["dlogits"], tol(dt) * 2)
    assert e["mean"] < 1e-4 and got["stats"][1].item() == 3.0, name + ": stats"
    assert bool((got["dlogits"][:, V:] == 0).all()) and bool((got["dlogits"][2] == 0).all()), name + ": padding columns and the ignored row"
    assert got["row_kd"][1].item() == 0 and got["row_kd"][2].item() == 0 and got["lse_tau"][1].item() == 0
    assert X.bits(got["row_loss"])[1] == X.bits(got["ce_row_loss"])[1], name + ": the row without a soft label keeps the cross entropy's loss"


def check_alpha_zero(be, dtype, V):
    """alpha == 0 with valid soft labels: loss, stats and every dlogits row are the cross entropy's, bit for bit."""
    dt, dev = DT[dtype], be.device
    name = "distill_alpha0-%s-v%d" % (dtype, V)
    x, lab, sid, slp = noise_problem(be, dtype, V, "gauss", 9700 + V)
    got = _run_noise(be, dt, x, lab, sid, slp, 0.0, 2.0, name)
    M = x.shape[0]
    dc = win_out(M, _dims(V)[1], dt, dev)
    be.ce_bwd(got["logits"].view, vec(got["labels"]), got["lse"], got["ce_stats"], vec(got["gs"]), True, M, V, dc.view, IGNORE)
    assert_same_bits(got["dlogits"], dc.view, name + ": dlogits against gstvd_ce_bwd")
    assert_same_bits(got["row_loss"], got["ce_row_loss"], name + ": row_loss against gstvd_ce_fwd")
    assert_same_bits(got["stats"], got["ce_stats"], name + ": stats against gstvd_ce_fwd")
    surroundings((("dlogits of ce_bwd", dc),), name)


# ============================================================================================== one row log-sum-exp
LSE1_V = (1, 3, 4, 5, 1025, 30522)      # no vector body, tail only, exactly one vector, vector plus tail, the workload's size
LSE1_CASES = [(dtype, V) for dtype in ("f32", "bf16") for V in LSE1_V]


def check_lse_tau_one(be, dtype, V):
    """tau = 1 on rows that count and carry a soft label: gstvd_distill_fwd's lse_tau is gstvd_ce_fwd's lse as 32-bit patterns.  The
    two kernels run ONE row log-sum-exp (csrc/ce_row.h), the student's with v * inv_tau in front, and v * 1.0f - mx, fused or not,
    rounds once to v - mx; gstvd_distill_bwd mixes the two normalisers on one row, so they must stay in step."""
    dev, dt, M = be.device, DT[dtype], 5
    name = "distill_lse_tau1-%s-v%d" % (dtype, V)
    gen = E.generator(9900 + V, dev)
    x = X.noise_logits(M, V, "gauss", dt, gen, dev)
    lab = torch.randint(0, V, (M,), generator=gen, device=dev)
    sid = (torch.arange(M, device=dev) % V).view(M, 1)
    logits, labels = win_in(x, dt, dev, pad=_dims(V)[0] - V), win_in(lab, I64, dev)
    sw, lw = win_in(sid, I64, dev), win_in(torch.full((M, 1), -1.0, dtype=torch.float64, device=dev), F32, dev)
    rl, lse, st = (win_out(1, n, F32, dev) for n in (M, M, 3))
    be.ce_fwd(logits.view, vec(labels), M, V, vec(rl), vec(lse), vec(st), IGNORE_EXACT)
    l, kd, lt, so = (win_out(1, n, F32, dev) for n in (M, M, M, 3))
    be.distill_fwd(logits.view, vec(labels), sw.view, lw.view, M, V, 0.5, 1.0, vec(rl), vec(l), vec(kd), vec(lt), vec(so), IGNORE_EXACT)
    assert bool(torch.isfinite(vec(lse)).all()) and st.view.reshape(-1)[1].item() == float(M), name + ": every row counts"
    assert_same_bits(vec(lt), vec(lse), name + ": lse_tau at tau = 1 against gstvd_ce_fwd's lse")
    e = rel_to_max(vec(lse), torch.logsumexp(x, -1))
    assert e <= tol(F32) * 5, "%s: lse %.3e (tol %.1e)" % (name, e, tol(F32) * 5)
    surroundings((("row_loss", l), ("row_kd", kd), ("lse_tau", lt), ("stats", so), ("ce row_loss", rl), ("lse", lse), ("ce stats", st),
                  ("logits", logits), ("labels", labels), ("soft_ids", sw), ("soft_logp", lw)), name)


def case_count():
    return {"top-k": len(TOPK_CASES), "backward exact": len(BWD_CASES), "noise": len(NOISE_CASES), "alpha 0": len(ALPHA0_CASES),
            "lse at tau 1": len(LSE1_CASES)}
