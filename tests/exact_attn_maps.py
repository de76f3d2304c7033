"""Exact layer of the attention-map tests (gstvd_attn_probs, csrc/attn_maps.hip), in the manner of tests/exact_attn.py, whose
constructions it reuses: P in a canary window whose inside is NaN before the launch, Q / K / key mask in NaN-poisoned windows with
padded leading dimensions, and input families whose probabilities are known exactly.

Plain helper module: no fixtures, no hooks.  Every check takes a *backend* with `device` and `run(problem, **changes)`, which
launches the map of the problem's descriptor into the problem's P window; tests/test_attn_maps_cpu.py proves the checks against a
stand-in written in torch before tests/test_attn_maps_exact_gpu.py points them at the HIP kernel.
"""
import collections
import math

import torch

import exact_attn as A
import exact_gemm as E
from exact_gemm import BF16, F32, Window, generator, integers

DT = A.DT

_Case = collections.namedtuple("MapCase", "dtype d B nh Lq Lk causal neg fused kv_group mean mask")


class Case(_Case):
    """One descriptor.  fused: Q and K are column slices of ONE [B * L, 3 * nh * d] buffer with a padded leading dimension;
    mean: head_mean; mask: the key-mask variant -- "none", "ones", "prefix" (ragged prefixes), "holes", "rowzero" (holes, and the
    keys of the LAST key-side batch row all masked)."""
    __slots__ = ()

    @property
    def id(self):
        s = "%s-d%d-%dx%d-q%d-k%d-%s" % (self.dtype, self.d, self.B, self.nh, self.Lq, self.Lk, self.mask)
        if self.causal: s += "-causal"
        if self.neg != -10000.0: s += "-neg1e9"
        if self.fused: s += "-fused"
        if self.kv_group > 1: s += "-g%d" % self.kv_group
        if self.mean: s += "-mean"
        return s


def case(dtype, d, Lq, Lk, B=2, nh=2, causal=False, neg=-10000.0, fused=False, kv_group=1, mean=False, mask="holes"):
    return Case(dtype, d, B, 4 if mean and nh == 2 else nh, Lq, Lk, bool(causal), float(neg), bool(fused), kv_group, bool(mean), mask)


KEYS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 293, 549]
QUERIES = [1, 15, 16, 17, 63, 64, 65, 256]
MASKS = ["none", "ones", "prefix", "holes", "rowzero"]


def build_cases():
    c = []
    for dt in ("bf16", "f32"):
        for d in (32, 64, 128):
            # every key count; query counts, mask variants and the two mask values dealt round-robin; the head mean on every third
            for i, Lk in enumerate(KEYS):
                c.append(case(dt, d, QUERIES[i % 8], Lk, neg=-1e9 if i % 2 else -10000.0, mask=MASKS[i % 5], mean=i % 3 == 2))
            # the causal mask at Lq == Lk and at Lq != Lk (both ways)
            c += [case(dt, d, 17, 17, causal=True, mask="none"), case(dt, d, 25, 25, causal=True, mask="prefix", fused=True),
                  case(dt, d, 17, 70, causal=True, mask="holes", neg=-1e9), case(dt, d, 70, 17, causal=True, mask="rowzero", mean=True)]
            # Q and K as column slices of one fused buffer (Lq == Lk); shared keys
            c += [case(dt, d, 65, 65, fused=True, mask="holes"), case(dt, d, 16, 16, fused=True, mask="ones", mean=True),
                  case(dt, d, 5, 70, B=4, kv_group=2, mask="rowzero"), case(dt, d, 3, 19, B=6, kv_group=3, mask="prefix", mean=True)]
    # the product shapes (head of csrc/attention.hip) at two batch rows: text, vision, both co-attention directions, decoder self and cross
    for dt in ("bf16", "f32"):
        c += [case(dt, 64, 256, 256, nh=12, fused=True, mask="prefix"), case(dt, 128, 37, 37, nh=8, fused=True, mask="holes"),
              case(dt, 128, 256, 37, nh=8, mask="holes"), case(dt, 128, 37, 256, nh=8, mask="prefix", mean=True),
              case(dt, 64, 25, 25, nh=12, causal=True, fused=True, mask="prefix"), case(dt, 64, 25, 293, nh=12, neg=-1e9, mask="prefix"),
              case(dt, 64, 25, 293, nh=12, neg=-1e9, mask="holes", mean=True)]
    return c


CASES = build_cases()


def make_mask(c, gen, device, variant=None):
    """The key mask [B / kv_group, Lk] of the case's variant, or None."""
    v = c.mask if variant is None else variant
    Bkv = c.B // c.kv_group
    if v == "none":
        return None
    km = torch.ones(Bkv, c.Lk, device=device)
    if v == "prefix":
        for b in range(Bkv):
            km[b, max(1, (c.Lk * (b + 2)) // (Bkv + 2)):] = 0
    elif v in ("holes", "rowzero"):
        km = A.make_mask(c, gen, device)
        if v == "rowzero":
            km[Bkv - 1] = 0
    return km


# ---------------------------------------------------------------------------------------------- the windows of one launch
class Problem(object):
    """Q, K and the key mask inside NaN-poisoned allocations (leading dimension nh * d + 8 or + 16, guard rows), P inside a canary
    allocation -- its inside NaN before the launch, its base 16-byte aligned or, for odd seeds, one float past that."""

    def __init__(self, c, device, seed=0, key_mask=True):
        self.c, self.device = c, device
        dt, H = DT[c.dtype], c.nh * c.d
        pad = 8 if seed % 2 == 0 else 16
        self.Bkv = c.B // c.kv_group
        assert self.Bkv * c.kv_group == c.B and (not c.fused or (c.Lq == c.Lk and c.kv_group == 1))
        self.wins = {}
        if c.fused:
            w = self.wins["QKV"] = Window(c.Lq, 3 * H, dt, device, "poison", ld=3 * H + pad, batch=c.B)
            self.Q, self.K = w.view3[..., :H], w.view3[..., H:2 * H]
            self.ldq = self.ldk = w.ld
        else:
            q = self.wins["Q"] = Window(c.Lq, H, dt, device, "poison", ld=H + pad, batch=c.B)
            k = self.wins["K"] = Window(c.Lk, H, dt, device, "poison", ld=H + pad, batch=self.Bkv)
            self.Q, self.K, self.ldq, self.ldk = q.view3, k.view3, q.ld, k.ld
        self.km = None
        if key_mask:
            self.wins["key_mask"] = Window(1, self.Bkv * c.Lk, F32, device, "poison")
            self.km = self.wins["key_mask"].vector().view(self.Bkv, c.Lk)
        self.shape = (c.B, c.Lq, c.Lk) if c.mean else (c.B, c.nh, c.Lq, c.Lk)
        n = 1
        for s in self.shape:
            n *= s
        pw = self.wins["P"] = Window(1, n, F32, device, "canary", misalign=seed % 2)
        self.P = pw.vector()
        self.P.fill_(float("nan"))

    def set(self, Q, K, key_mask=None):
        c = self.c
        self.Q.unflatten(-1, (c.nh, c.d)).copy_(Q)
        self.K.unflatten(-1, (c.nh, c.d)).copy_(K)
        if key_mask is not None:
            self.km.copy_(key_mask)
        return self

    def assert_windows(self, name, written=True):
        for tag, w in self.wins.items():
            w.assert_surroundings_untouched("%s: %s" % (name, tag))
        nn = int(torch.isnan(self.P).sum().item())
        if written:
            assert nn == 0, "%s: %d of %d elements of P are NaN (never written, or something outside an operand was read)" % (name, nn, self.P.numel())
        else:
            assert nn == self.P.numel(), "%s: a refused call wrote %d element(s) of P" % (name, self.P.numel() - nn)


def launch(be, c, inp, seed=0, name=None, **changes):
    """One launch of case `c` with inputs `inp` (Q [B, Lq, nh, d], K [B / kv_group, Lk, nh, d], key_mask or None); windows built,
    backend run, windows checked.  -> P [B, nh, Lq, Lk] (or [B, Lq, Lk]) as a copy."""
    name = name or c.id
    km = inp.get("key_mask")
    p = Problem(c, be.device, seed, key_mask=km is not None)
    p.set(inp["Q"], inp["K"], km)
    be.run(p, **changes)
    p.assert_windows(name)
    return p.P.view(p.shape).clone()


# ---------------------------------------------------------------------------------------------- reference
def additive_mask(c, km, device):
    """[B, 1, Lq, Lk] fp32: 0 where the key mask and the causal mask allow the key, mask_neg elsewhere (added once)."""
    al = A.allowed_keys(c, km, device)
    return al, torch.where(al, torch.zeros((), device=device), torch.full((), c.neg, device=device)).float()


def reference(c, inp, scale):
    """float64 softmax of the scores as the formula gives them in fp32: fl32(s * scale + mask) with ONE rounding (the operands of
    the families below make s * scale exact).  -> P [B, nh, Lq, Lk] float64, allowed [B, 1, Lq, Lk]."""
    dev = inp["Q"].device
    Q, K = inp["Q"].double(), inp["K"].double().repeat_interleave(c.kv_group, 0)
    al, add = additive_mask(c, inp.get("key_mask"), dev)
    s = (torch.einsum("bqhd,bkhd->bhqk", Q, K) * scale + add.double()).float().double()
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True), al


def head_mean_rule(P, nh):
    """(p_0 + p_1 + ... + p_{nh-1}) * (1.0f / nh) in fp32, heads in ascending order -- the rule of gstvd_attn_probs."""
    acc = P[:, 0].clone()
    for h in range(1, nh):
        acc = acc + P[:, h]
    return acc * (torch.ones((), dtype=torch.float32, device=P.device) / nh)


def per_head(c):
    return c._replace(mean=False)


def expect(be, c, inp, seed, name, **changes):
    """The launch of `c`, and for a head-mean case the per-head launch next to it: -> (what the case's own launch wrote, per-head P).
    A head-mean result is first held to the rule, bit for bit."""
    got = launch(be, c, inp, seed, name, **changes)
    if not c.mean:
        return got, got
    ph = launch(be, per_head(c), inp, seed + 1, name + " (per head)", **changes)
    A.assert_same(got, head_mean_rule(ph, c.nh), name + ": head mean vs (p_0 + ... + p_nh-1) * (1 / nh) of the per-head launch")
    return got, ph


# ---------------------------------------------------------------------------------------------- C. one-hot
def check_onehot(be, c, seed=0):
    """exact_attn family C: K[k] is a +-16 code of k, Q[q] = K[sel(q)] with sel random over the allowed keys (rows with no allowed
    key: over all keys): the selected score is at least 181 above every other, so P is exactly one-hot, bit for bit -- every other
    entry, the masked ones among them, is +0.0."""
    dev = be.device
    gen = generator(1000 + seed, dev)
    km = make_mask(c, gen, dev)
    nb = max(1, (c.Lk - 1).bit_length())
    reps = c.d // nb
    assert reps >= 1 and 2 * 256 * reps * A.scale32(c.d) > 104
    k = torch.arange(c.Lk, device=dev)
    code = torch.zeros(c.Lk, c.d, device=dev)
    code[:, :nb * reps] = (((k[:, None] >> torch.arange(nb, device=dev)[None, :]) & 1) * 32.0 - 16.0).repeat(1, reps)
    Bkv = c.B // c.kv_group
    sign = torch.randint(0, 2, (Bkv, 1, c.nh, c.d), generator=gen, device=dev).float() * 2 - 1
    K = code[None, :, None, :] * sign
    al = A.allowed_keys(c, km, dev).expand(c.B, c.nh, c.Lq, c.Lk)
    al = al | ~al.any(-1, keepdim=True)                       # a fully masked row: the mask cancels, any key can be selected
    sel = torch.multinomial(al.reshape(-1, c.Lk).float(), 1, generator=gen).view(c.B, c.nh, c.Lq)
    bidx = torch.arange(c.B, device=dev)[:, None, None]
    hidx = torch.arange(c.nh, device=dev)[None, :, None]
    Q = K.repeat_interleave(c.kv_group, 0)[bidx, sel, hidx].permute(0, 2, 1, 3)
    _, ph = expect(be, c, dict(Q=Q, K=K, key_mask=km), seed, c.id + ": one-hot")
    want = torch.zeros(c.B, c.nh, c.Lq, c.Lk, device=dev).scatter_(-1, sel[..., None], 1.0)
    E.assert_bit_equal(ph, want, c.id + ": one-hot P")


# ---------------------------------------------------------------------------------------------- D. uniform
def check_uniform(be, c, seed=0):
    """Q = 0: the allowed entries of a row are bit-identical and 1 / n within two roundings, the others exactly 0.0f; a row whose
    keys are all masked is uniform over ALL Lk keys (the mask term cancels)."""
    dev = be.device
    gen = generator(2000 + seed, dev)
    km = make_mask(c, gen, dev)
    Bkv = c.B // c.kv_group
    Q = torch.zeros(c.B, c.Lq, c.nh, c.d, device=dev)
    K = integers((Bkv, c.Lk, c.nh, c.d), 3, gen, torch.float32, dev)
    _, ph = expect(be, c, dict(Q=Q, K=K, key_mask=km), seed, c.id + ": uniform")
    al = A.allowed_keys(c, km, dev).expand(c.B, c.nh, c.Lq, c.Lk)
    none = ~al.any(-1, keepdim=True)
    al = al | none
    n = al.sum(-1, keepdim=True)
    A.assert_all_zero(ph[~al], c.id + ": uniform: masked entries")
    first = (ph * al).max(-1, keepdim=True).values
    bad = int(((ph != first) & al).sum().item())
    assert bad == 0, "%s: uniform: %d allowed entries differ from the others of their row" % (c.id, bad)
    err = ((first.double() * n.double()) - 1).abs().max().item()
    assert err <= 2 * 2.0 ** -24 * 2, "%s: uniform: n * p = 1 + %.3e" % (c.id, err)
    if c.mask == "rowzero":
        assert bool(none[c.B - c.kv_group:].all()) and int(n[c.B - 1].min()) == c.Lk


# ---------------------------------------------------------------------------------------------- exact scores
def integer_scale(c):
    """A power of two near 1 / (4 sqrt(d)): with operands in [-4, 4] every score s * scale is exact in fp32 in any summation order,
    and the scores of a row spread with a standard deviation of about 2 (a row keeps several probabilities of weight)."""
    return 2.0 ** -(int(math.log2(c.d)) // 2 + 2)


def check_integer_scores(be, c, seed=0, out=None):
    """Integer operands in [-4, 4] and an explicit power-of-two scale: the scores are exact, so P is the float64 softmax up to one
    rounding per term of the row sum plus expf and the division: (Lk + 8) * 2^-24 of the row's reference maximum."""
    dev, dt = be.device, DT[c.dtype]
    gen = generator(3000 + seed, dev)
    km = make_mask(c, gen, dev)
    Bkv = c.B // c.kv_group
    Q = integers((c.B, c.Lq, c.nh, c.d), 4, gen, torch.float32, dev)
    K = integers((Bkv, c.Lk, c.nh, c.d), 4, gen, torch.float32, dev)
    scale = integer_scale(c)
    inp = dict(Q=Q, K=K, key_mask=km)
    _, ph = expect(be, c, inp, seed, c.id + ": integer scores", scale=scale)
    ref, al = reference(c, inp, scale)
    tol = (c.Lk + 8) * 2.0 ** -24
    err = ((ph.double() - ref).abs() / ref.max(-1, keepdim=True).values).max().item()
    if out:
        out("%s: integer scores: largest |P - ref| / row max %.3e (tol %.3e)" % (c.id, err, tol))
    assert torch.isfinite(ph).all()
    assert err <= tol, "%s: integer scores: largest |P - ref| / row max %.3e (tol %.3e)" % (c.id, err, tol)
    al = al.expand_as(ph)
    A.assert_all_zero(ph[(~al) & al.any(-1, keepdim=True)], c.id + ": integer scores: masked entries of rows with an allowed key")
    rs = (ph.double().sum(-1) - 1).abs().max().item()
    assert rs <= tol, "%s: integer scores: row sums off by %.3e" % (c.id, rs)


# ---------------------------------------------------------------------------------------------- E. invariances
def random_inputs(c, gen, dev, km):
    dt, Bkv = DT[c.dtype], c.B // c.kv_group

    def rn(*shape):
        return (torch.randn(*shape, generator=gen, device=dev) * 0.5).to(dt).float()
    return dict(Q=rn(c.B, c.Lq, c.nh, c.d), K=rn(Bkv, c.Lk, c.nh, c.d), key_mask=km)


def check_invariances(be, c, seed=0):
    """Bit for bit: two runs agree; the key mask None equals a key mask of ones; the contents of masked keys, and of the keys
    after the last query under the causal mask, do not change P (rows with an allowed key); a head-mean launch obeys the rule."""
    dev = be.device
    gen = generator(4000 + seed, dev)
    km = make_mask(c, gen, dev, "holes" if c.mask in ("none", "ones", "rowzero") else c.mask)
    inp = random_inputs(c, gen, dev, km)
    a, _ = expect(be, c, inp, seed, c.id + ": random")
    b = launch(be, c, inp, seed + 2, c.id + ": random, again")
    A.assert_same(a, b, c.id + ": two runs")
    dead = (km == 0)
    if c.causal and c.Lk > c.Lq:
        dead = dead | (torch.arange(c.Lk, device=dev) >= c.Lq)[None, :]
    K2 = torch.where(dead[:, :, None, None], (torch.randn(inp["K"].shape, generator=gen, device=dev) * 3).to(DT[c.dtype]).float(), inp["K"])
    assert bool(dead.any()) and not torch.equal(K2, inp["K"])
    d = launch(be, c, dict(inp, K=K2), seed + 3, c.id + ": other contents in masked / later keys")
    A.assert_same(a, d, c.id + ": contents of masked / later keys")
    ones = torch.ones(c.B // c.kv_group, c.Lk, device=dev)
    e = launch(be, c, dict(inp, key_mask=None), seed, c.id + ": no key mask")
    f = launch(be, c, dict(inp, key_mask=ones), seed + 1, c.id + ": key mask of ones")
    A.assert_same(e, f, c.id + ": key mask None vs ones")
    assert not torch.equal(a, e)


# ---------------------------------------------------------------------------------------------- refusals
def check_refusals(be, c, refused):
    """dropout_p != 0, q_bstride != 0 and kv_bstride != 0 answer GSTVD_E_UNSUPPORTED and write nothing.  `refused(fn)`: asserts
    that fn() raises that status."""
    dev = be.device
    gen = generator(5000, dev)
    inp = random_inputs(c, gen, dev, make_mask(c, gen, dev, "holes"))
    for change in (dict(drop_p=0.1), dict(q_bstride=c.Lq + 3), dict(kv_bstride=c.Lk + 5)):
        p = Problem(c, dev, 0, key_mask=True)
        p.set(inp["Q"], inp["K"], inp["key_mask"])
        refused(lambda: be.run(p, **change))
        p.assert_windows("%s: refused %r" % (c.id, change), written=False)
