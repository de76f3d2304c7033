"""Exact layer of the grouped cross-attention backward (gstvd_attn_group_bwd, csrc/attn_group.hip): kv_group = G consecutive
query rows share the K, V and key mask of one row; dQ and delta are per query row, dK and dV are the sums over each group,
written once.  Built on tests/exact_attn.py (windows, float64 reference, assertions) without changing it.

Plain helper module: no fixtures, no hooks.  Every check takes a *backend* with
    device
    run(p)        the grouped forward and gstvd_attn_group_bwd on the windows of problem p
    run_plain(p)  the forward and gstvd_attn_bwd (kv_group == 1 only): the two-part kernel the new one is compared with
    keep(p)       the dropout keep mask [B, nh, Lq, Lk] of the launch, indexed by the QUERY row
    refuse(p, **change)   the descriptor of p with `change` applied must be refused
so tests/test_exact_attn_group_harness_cpu.py proves each check on the CPU against a torch stand-in, and against deliberately
wrong stand-ins, before tests/test_attn_group_exact_gpu.py points them at the HIP kernels."""
import re

import torch

import exact_attn as A
from exact_attn import BF16, F32, Window, generator, integers

E = A.E
SHAPES = [(4, 2, 3, 19, 19), (6, 3, 2, 9, 70), (4, 4, 2, 70, 37), (2, 1, 2, 25, 293), (3, 3, 1, 1, 5)]      # (B, G, nh, Lq, Lk)
GROUP_KERNEL_RE = re.compile(rb"_Z\d+xgroup_bwd\w*")
_TY = {"bf16": "DF16b", "f32": "f"}


def case(dtype, d, shape, p=0.0, neg=-10000.0):
    B, G, nh, Lq, Lk = shape
    return A.case(dtype, d, Lq, Lk, "tiled", A.two(Lq, Lk), B=B, nh=nh, p=p, neg=neg, kv_group=G)


def build_cases():
    """dtype x d, the five shapes dealt round-robin so that every (dtype, d) meets every shape once with and once without
    dropout (p = 0.1)."""
    c = []
    for dt in ("bf16", "f32"):
        for i, d in enumerate((32, 64, 128)):
            for j, shp in enumerate(SHAPES):
                c.append(case(dt, d, shp, p=0.1 if (i + j) % 2 == 0 else 0.0))
                c.append(case(dt, d, shp, p=0.0 if (i + j) % 2 == 0 else 0.1))
    return c


CASES = build_cases()


def kernel_of(c):
    return "xgroup_bwdI%sLi%dEE" % (_TY[c.dtype], c.d)


def cid(c):
    return c.id


# ---------------------------------------------------------------------------------------------- windows
class GroupProblem(A.Problem):
    """exact_attn.Problem for a grouped case (K, V, key mask, dK, dV with B / G batch rows).  `wide`: K and V are column slices
    of ONE poisoned [B / G * Lk, 4 * nh * d (+ pad)] buffer -- the cross-attention K/V projection of two decoder layers, the
    second layer's slices are used -- and dK, dV the two halves of one canary [B / G * Lk, 2 * nh * d (+ pad)] buffer."""

    def __init__(self, c, device, seed=0, key_mask=True, wide=False, scale=None):
        A.Problem.__init__(self, c, device, seed, key_mask, scale)
        self.wide = wide
        if not wide:
            return
        dt, H = A.DT[c.dtype], c.nh * c.d
        pad = 8 if seed % 2 == 0 else 16
        for n in ("K", "V", "dK", "dV"):
            del self.wins[n]
        kv = self.wins["KV"] = Window(c.Lk, 4 * H, dt, device, "poison", ld=4 * H + pad, batch=self.Bkv, stride=c.Lk * (4 * H + pad))
        g = self.wins["dKV"] = Window(c.Lk, 2 * H, dt, device, "canary", ld=2 * H + pad, batch=self.Bkv, stride=c.Lk * (2 * H + pad))
        self.ld_kv, self.ld_dkv = kv.ld, g.ld
        self._K, self._V = kv.view3[..., 2 * H:3 * H], kv.view3[..., 3 * H:4 * H]
        self._dK, self._dV = g.view3[..., :H], g.view3[..., H:]


def launch(be, c, inp, seed=0, name=None, wide=False, plain=False, scale=None):
    """One forward + backward of case c on backend be: windows built (dK, dV NaN before the launch: a row that is not written
    shows), backend run, windows checked.  -> (outputs, keep mask or None)."""
    name = name or c.id
    km = inp.get("key_mask")
    p = GroupProblem(c, be.device, seed, key_mask=km is not None, wide=wide, scale=scale)
    p.set(**{k: v for k, v in inp.items() if v is not None})
    p.t("dK").fill_(float("nan"))
    p.t("dV").fill_(float("nan"))
    (be.run_plain if plain else be.run)(p)
    p.assert_windows(name)
    keep = be.keep(p) if c.p > 0 else None
    return p.outputs(), keep


def replicated(c, inp):
    """The same launch without the group: K, V and the mask repeated G times."""
    G = c.kv_group
    rep = dict(inp, K=inp["K"].repeat_interleave(G, 0), V=inp["V"].repeat_interleave(G, 0))
    if inp.get("key_mask") is not None:
        rep["key_mask"] = inp["key_mask"].repeat_interleave(G, 0)
    return c._replace(kv_group=1), rep


def group_sum(x, G):
    """[B, Lk, nh, d] per query row -> [B / G, Lk, nh, d], the sums over each group."""
    return x.reshape(x.shape[0] // G, G, *x.shape[1:]).sum(1)


def _inputs(c, seed, dev, mask):
    gen = generator(5000 + seed, dev)
    km = A.make_mask(c, gen, dev) if mask else None
    return A.random_inputs(c, gen, dev, km)


# ---------------------------------------------------------------------------------------------- G = 1
def check_group_of_one(be, c, seed=0):
    """kv_group = 1: dQ, dK, dV, delta (and O, LSE) are those of gstvd_attn_bwd's two-part kernel, bit for bit."""
    assert c.kv_group == 1
    inp = _inputs(c, seed, be.device, seed % 2 == 0)
    a, _ = launch(be, c, inp, seed, c.id + ": group of one", wide=seed % 3 == 0)
    b, _ = launch(be, c, inp, seed + 1, c.id + ": two-part backward", plain=True)
    for n in ("O", "LSE", "dQ", "dK", "dV", "delta"):
        A.assert_same(a[n], b[n], "%s: group of one vs gstvd_attn_bwd: %s" % (c.id, n))


# ---------------------------------------------------------------------------------------------- any G: dQ and delta
def check_dq_matches_replicated(be, c, seed=0):
    """dQ and delta (and the forward's O, LSE) equal those of gstvd_attn_bwd on K, V and the mask repeated G times, bit for bit:
    per query row nothing but the address of its keys changed."""
    inp = _inputs(c, seed, be.device, seed % 2 == 0)
    a, _ = launch(be, c, inp, seed, c.id + ": grouped", wide=seed % 3 == 0)
    c1, rep = replicated(c, inp)
    b, _ = launch(be, c1, rep, seed + 1, c.id + ": replicated", plain=True)
    for n in ("O", "LSE", "dQ", "delta"):
        A.assert_same(a[n], b[n], "%s: grouped vs replicated K / V: %s" % (c.id, n))


# ---------------------------------------------------------------------------------------------- any G: dK and dV
def check_dkv(be, c, seed=0, out=None):
    """dK, dV against the float64 reference summed over each group, at 4 x exact_attn.TOL (the project's attention gate);
    bit-identical between two runs; and a group member whose dO rows are exactly zero contributes exactly nothing (dropout off:
    the draws are indexed by the query row, which removing a member renumbers)."""
    dev, dt, G = be.device, A.DT[c.dtype], c.kv_group
    inp = _inputs(c, seed, dev, seed % 2 == 1)
    wide = seed % 3 != 0
    a, keep = launch(be, c, inp, seed, c.id + ": first run", wide=wide)
    b, _ = launch(be, c, inp, seed, c.id + ": second run", wide=wide)
    for n in ("dQ", "dK", "dV", "delta"):
        A.assert_same(a[n], b[n], "%s: two runs: %s" % (c.id, n))
    ref = A.reference(c, inp, keep)
    for n in ("dK", "dV"):
        A.assert_close(a[n], group_sum(ref[n], G), 4 * A.TOL[dt], "%s: %s vs float64" % (c.id, n), out)
    A.assert_close(a["dQ"], ref["dQ"], 4 * A.TOL[dt], "%s: dQ vs float64" % c.id, out)
    if G == 1:
        return
    # the last member of every group with dO = 0, against the group without that member
    c0 = c._replace(p=0.0)
    member = torch.arange(c.B, device=dev) % G
    dO0 = inp["dO"] * (member != G - 1)[:, None, None, None]
    z, _ = launch(be, c0, dict(inp, dO=dO0), seed, c.id + ": last member's dO zero", wide=wide)
    cs = c0._replace(B=c.B // G * (G - 1), kv_group=G - 1)
    rows = member != G - 1
    sub = dict(inp, Q=inp["Q"][rows], dO=inp["dO"][rows])
    s, _ = launch(be, cs, sub, seed, c.id + ": without the last member", wide=wide)
    for n in ("dK", "dV"):
        A.assert_bit_equal(z[n], s[n].double(), "%s: a member with dO = 0 changed %s" % (c.id, n))
    A.assert_all_zero(z["dQ"][~rows], c.id + ": dQ of the member with dO = 0")


# ---------------------------------------------------------------------------------------------- exact families
def check_onehot(be, c, seed=0):
    """exact_attn family C across a group: P exactly one-hot, integer V and dO -> dV[e, k] is the exact sum of fac * keep * dO
    over ALL queries of ALL members of group e that selected k; dQ = dK = 0 exactly."""
    dev, G = be.device, c.kv_group
    assert 1.0 / (1.0 - c.p) in (1.0, 2.0)
    gen = generator(1000 + seed, dev)
    km = A.make_mask(c, gen, dev) if seed % 3 != 2 else None
    nb = max(1, (c.Lk - 1).bit_length())
    reps = c.d // nb
    assert reps >= 1 and 2 * 256 * reps * A.scale32(c.d) > 104
    k = torch.arange(c.Lk, device=dev)
    code = torch.zeros(c.Lk, c.d, device=dev)
    code[:, :nb * reps] = (((k[:, None] >> torch.arange(nb, device=dev)[None, :]) & 1) * 32.0 - 16.0).repeat(1, reps)
    Bkv = c.B // G
    sign = torch.randint(0, 2, (Bkv, 1, c.nh, c.d), generator=gen, device=dev).float() * 2 - 1
    K = code[None, :, None, :] * sign
    al = A.allowed_keys(c, km, dev).expand(c.B, c.nh, c.Lq, c.Lk)
    sel = torch.multinomial(al.reshape(-1, c.Lk).float(), 1, generator=gen).view(c.B, c.nh, c.Lq)
    bidx = torch.arange(c.B, device=dev)[:, None, None]
    hidx = torch.arange(c.nh, device=dev)[None, :, None]
    Q = K.repeat_interleave(G, 0)[bidx, sel, hidx].permute(0, 2, 1, 3)
    V = integers((Bkv, c.Lk, c.nh, c.d), 64, gen, torch.float32, dev)
    dO = integers((c.B, c.Lq, c.nh, c.d), 3, gen, torch.float32, dev)
    got, keep = launch(be, c, dict(Q=Q, K=K, V=V, dO=dO, key_mask=km), seed, c.id + ": one-hot", wide=seed % 2 == 0)
    w = torch.full((c.B, c.nh, c.Lq), 1.0 / (1.0 - c.p), device=dev, dtype=torch.float64)
    if keep is not None:
        w = w * keep.gather(-1, sel[..., None]).squeeze(-1).double()
    want = torch.zeros(Bkv * c.nh * c.Lk, c.d, dtype=torch.float64, device=dev)
    rows = (((bidx // G) * c.nh + hidx) * c.Lk + sel).reshape(-1)
    want.index_add_(0, rows, (w[..., None] * dO.double().permute(0, 2, 1, 3)).reshape(-1, c.d))
    A.assert_bit_equal(got["dV"], want.view(Bkv, c.nh, c.Lk, c.d).permute(0, 2, 1, 3), c.id + ": one-hot dV")
    A.assert_all_zero(got["dQ"], c.id + ": one-hot dQ")
    A.assert_all_zero(got["dK"], c.id + ": one-hot dK")


def check_uniform(be, c, seed=0):
    """exact_attn family D across a group: Q = 0 and a power-of-two number n of allowed keys -> P = 1 / n; V in {-1, 0, 1}, dO =
    +-1 in one column per row.  P * fac (fac 1 or 2) and dO are exact in bf16, every term of dV is a multiple of 1 / n below 2 and
    their sum over the group's queries stays exact in fp32: dV is bit-equal to the float64 reference summed over the group;
    dK = dS^T Q = 0 exactly."""
    dev, G = be.device, c.kv_group
    assert 1.0 / (1.0 - c.p) in (1.0, 2.0)
    gen = generator(2000 + seed, dev)
    pow2 = 1 << (c.Lk.bit_length() - 1)
    if pow2 == c.Lk and c.Lk > 1 and seed % 2:
        pow2 //= 2
    km = A.make_mask(c, gen, dev, allowed=pow2) if (pow2 < c.Lk or seed % 3 == 0) else None
    Bkv = c.B // G
    Q = torch.zeros(c.B, c.Lq, c.nh, c.d, device=dev)
    K = integers((Bkv, c.Lk, c.nh, c.d), 3, gen, torch.float32, dev)
    V = integers((Bkv, c.Lk, c.nh, c.d), 1, gen, torch.float32, dev)
    col = torch.randint(0, c.d, (c.B, c.Lq, c.nh, 1), generator=gen, device=dev)
    dO = torch.zeros(c.B, c.Lq, c.nh, c.d, device=dev).scatter_(-1, col, torch.randint(0, 2, col.shape, generator=gen, device=dev).float() * 2 - 1)
    inp = dict(Q=Q, K=K, V=V, dO=dO, key_mask=km)
    got, keep = launch(be, c, inp, seed, c.id + ": uniform", wide=seed % 2 == 1)
    ref = A.reference(c, inp, keep)
    n = A.allowed_keys(c, km, dev).sum(-1)
    assert bool(((n & (n - 1)) == 0).all()) and int(n.min()) >= 1
    A.assert_bit_equal(got["dV"], group_sum(ref["dV"], G), c.id + ": uniform dV")
    A.assert_all_zero(got["dK"], c.id + ": uniform dK")


def disjoint_must_be_exact(c):
    """exact_attn.disjoint_must_be_exact for the grouped cases (no causal mask here): fp32 always, bf16 without dropout below
    256 keys; None: the data decide."""
    return "exact" if c.dtype == "f32" or (c.p == 0 and c.Lk < 256) else None


def check_uniform_dk(be, c, seed=0, out=None):
    """exact_attn family H across a group: Q on the upper half of the columns, K on the lower, explicit scale 2^-3 -- every score
    is exactly 0 and P = 1 / n as in check_uniform, but dK = dS^T Q is nonzero: the sum over ALL queries of ALL members of the
    group.  Where the float64 guards of exact_attn.check_uniform_dk hold (bf16 operands exact, every partial sum below 2^24 units,
    taken over the WHOLE group) dK and dV are bit-equal to the float64 reference summed over the group, whatever the order of
    the additions, and dQ and delta to the reference per query row; elsewhere 4 x TOL.  Returns the mode."""
    dev, dt, G = be.device, A.DT[c.dtype], c.kv_group
    assert 1.0 / (1.0 - c.p) in (1.0, 2.0)
    gen = generator(6000 + seed, dev)
    km = A.pow2_mask(c, gen, dev, seed)
    inp = dict(A.disjoint_inputs(c, gen, dev), key_mask=km)
    got, keep = launch(be, c, inp, seed, c.id + ": uniform, disjoint columns", wide=seed % 2 == 1, scale=A.H_SCALE)
    ref = A.reference(c, inp, keep, scale=A.H_SCALE)
    n = A.allowed_keys(c, km, dev).sum(-1)
    assert bool(((n & (n - 1)) == 0).all()) and int(n.min()) >= 1
    A.assert_bit_equal(got["O"], ref["O"], c.id + ": disjoint O")
    Kx, Vx = (inp[t].double().repeat_interleave(G, 0) for t in ("K", "V"))
    # the group's sum runs over (member, query): fold the members into the query axis for the guard
    fold = lambda x: x.reshape(c.B // G, G, *x.shape[1:])
    dSg = fold(ref["dS"]).permute(0, 2, 1, 3, 4).reshape(c.B // G, c.nh, G * c.Lq, c.Lk)
    Pdg = fold(ref["Pd"]).permute(0, 2, 1, 3, 4).reshape(c.B // G, c.nh, G * c.Lq, c.Lk)
    Qg, dOg = (fold(inp[t].double()).reshape(c.B // G, G * c.Lq, c.nh, c.d) for t in ("Q", "dO"))
    exact = (A.sum_is_exact("bhqk,bqhd->bkhd", dSg, Qg) and A.sum_is_exact("bhqk,bqhd->bkhd", Pdg, dOg)
             and A.sum_is_exact("bhqk,bkhd->bqhd", ref["dS"], Kx) and A.sum_is_exact("bhqk,bkhd->bqhd", ref["Pd"], Vx)
             and (dt == F32 or (A.fits(ref["Pd"], BF16) and A.fits(ref["O"], BF16) and A.fits(ref["dS"], BF16))))
    want = dict(dK=group_sum(ref["dK"], G), dV=group_sum(ref["dV"], G), dQ=ref["dQ"], delta=ref["delta"])
    if exact:
        for nme in ("delta", "dV", "dQ", "dK"):
            A.assert_bit_equal(got[nme], want[nme], "%s: disjoint %s" % (c.id, nme))
        assert int((got["dK"] != 0).sum()) > 0 or int(n.max()) < 4, c.id + ": the construction gave dK = 0"
    else:
        A.assert_bit_equal(got["dV"], want["dV"], c.id + ": disjoint dV")              # (as check_uniform: P * fac is exact whatever dS holds)
        for nme in ("dQ", "dK"):
            A.assert_close(got[nme], want[nme], 4 * A.TOL[dt], "%s: disjoint %s" % (c.id, nme))
    mode = "exact" if exact else "tol"
    must = disjoint_must_be_exact(c)
    assert must is None or mode == must, "%s: disjoint-column backward was checked as %r, the construction promises %r" % (c.id, mode, must)
    if out:
        out("%s: disjoint-column backward checked as %s" % (c.id, mode))
    return mode


def check_all_masked_row(be, c, seed=0, out=None):
    """exact_attn family G: K / V row 0 has every key masked (mask_neg = -10000 cancels in the softmax); its group's gradients are
    held to exact_attn.G_BOUND + 4 x TOL, the others to 4 x TOL; everything is finite."""
    dev, dt, G = be.device, A.DT[c.dtype], c.kv_group
    assert c.B // G >= 2 and c.neg == -10000.0
    gen = generator(4000 + seed, dev)
    km = A.make_mask(c, gen, dev)
    km[0] = 0
    inp = A.random_inputs(c, gen, dev, km)
    got, keep = launch(be, c, inp, seed, c.id + ": a fully masked K / V row", wide=True)
    ref = A.reference(c, inp, keep)
    for n in ("dK", "dV"):
        r = group_sum(ref[n], G)
        A.assert_close(got[n][1:], r[1:], 4 * A.TOL[dt], "%s: other rows %s" % (c.id, n), out)
        A.assert_close(got[n][0], r[0], A.G_BOUND + 4 * A.TOL[dt], "%s: masked row %s" % (c.id, n), out)
    A.assert_close(got["dQ"][G:], ref["dQ"][G:], 4 * A.TOL[dt], c.id + ": other rows dQ", out)
    A.assert_close(got["dQ"][:G], ref["dQ"][:G], A.G_BOUND + 4 * A.TOL[dt], c.id + ": masked row dQ", out)


# ---------------------------------------------------------------------------------------------- the dropout masks applied
def check_dropout_masks(be, c, seed=0):
    """exact_attn family F for a grouped launch (Q = 0, p = 0.5, no key mask, indicator operands):
      forward:  V[k, col] = [k in block j, k mod d == col]                        -> O[b, q, col]  = (2 / Lk) keep[b, q, k_col]
      dK / dV:  dO[b, q, col] = [b is member m of its group, q in block i, ...]   -> dV[e, k, col] = (2 / Lk) keep[e G + m, q_col, k]
    one launch per key block and per (member, query block): the mask the key-owning backward applied to every (query row, head, q,
    k) equals the mask the grouped forward applied, and both equal the mask probe."""
    assert c.p == 0.5
    dev, d, G = be.device, c.d, c.kv_group
    Bkv = c.B // G
    zq = torch.zeros(c.B, c.Lq, c.nh, d, device=dev)
    zk = torch.zeros(Bkv, c.Lk, c.nh, d, device=dev)
    kk, qq = torch.arange(c.Lk, device=dev), torch.arange(c.Lq, device=dev)
    rec_f = torch.zeros(c.B, c.nh, c.Lq, c.Lk, dtype=torch.bool, device=dev)
    rec_kv = rec_f.clone()
    hi = torch.tensor(2.0 / c.Lk, dtype=torch.float64, device=dev)
    probe = None
    for blk in range(-(-c.Lk // d)):
        V = zk.clone()
        ks = kk[(kk // d) == blk]
        V[:, ks, :, ks % d] = 1.0
        got, keep = launch(be, c, dict(Q=zq, K=zk, V=V, dO=zq, key_mask=None), seed, "%s: forward draws, block %d" % (c.id, blk))
        probe = keep if probe is None else probe
        assert torch.equal(probe, keep)
        rec_f[..., ks] = A._decode_levels(got["O"].permute(0, 2, 1, 3)[..., ks % d], hi, c.id + ": forward draws")
    member = torch.arange(c.B, device=dev) % G
    for m in range(G):
        for blk in range(-(-c.Lq // d)):
            dO = zq.clone()
            qs = qq[(qq // d) == blk]
            dO[:, qs, :, qs % d] = 1.0
            dO = dO * (member == m)[:, None, None, None]
            got, keep = launch(be, c, dict(Q=zq, K=zk, V=zk, dO=dO, key_mask=None), seed, "%s: dK / dV draws, member %d block %d" % (c.id, m, blk))
            assert torch.equal(probe, keep)
            dv = got["dV"].permute(0, 2, 1, 3)[..., qs % d].transpose(-1, -2)      # [Bkv, nh, |qs|, Lk]
            rec = A._decode_levels(dv, hi, c.id + ": dK / dV draws")
            rec_kv[m::G][:, :, qs] = rec
    A.assert_same(rec_f, probe, c.id + ": the draws the grouped forward applied vs the mask probe")
    A.assert_same(rec_kv, rec_f, c.id + ": the draws the key-owning backward applied vs the grouped forward's")


# ---------------------------------------------------------------------------------------------- refusals
REFUSALS = (dict(causal=1), dict(q_bstride=64), dict(kv_bstride=512), dict(B_minus=1), dict(null="dO"), dict(null="dK"), dict(null="delta"))


def check_refusals(be, c, seed=0):
    """Every descriptor gstvd_attn_group_bwd does not take is answered with an error code and nothing is written: every output
    window of the backward still holds its canaries."""
    inp = _inputs(c, seed, be.device, True)
    for change in REFUSALS:
        p = GroupProblem(c, be.device, seed, key_mask=True)
        p.set(**inp)
        be.refuse(p, **change)
        for tag in ("dQ", "dK", "dV", "delta"):
            w = p.wins[tag]
            w.assert_surroundings_untouched("%s refused (%r): %s" % (c.id, change, tag))
            inner = w.flat[w.inside].view(E._INT[w.dtype])
            assert bool((inner == E.CANARY[w.dtype]).all()), "%s refused (%r): %s was written" % (c.id, change, tag)
