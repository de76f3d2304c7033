"""Exact layer of the attention tests: a route table, canary / poison windows and eight families of
inputs whose results are known exactly (J: to a derived rounding bound), so that ONE mis-handled key, dropout draw, mask term,
address, dK term or softmax rescale shows.

  A  route table: every case names the forward and the backward kernel it expects (the library is asked, ops.attn_kernel_symbol)
  B  windows: outputs in canary allocations, inputs in NaN-poisoned ones, padded leading dimensions (exact_gemm.Window)
  C  one-hot ("pointer") attention: K[k] is a +-16 code of k, Q[q] = K[sel(q)] -> P is exactly one-hot, O[q] = V[sel(q)]
  D  uniform attention: Q = 0 -> P = 1 / n(q) over the allowed keys, O[q] = mean of the allowed V rows
  E  invariances, bit for bit (mask None vs ones, contents of masked / later keys, appended masked keys, permutations, keep bits)
  F  the dropout mask each consumer applied, recovered element by element from its own outputs with indicator operands
  G  a batch row whose keys are ALL masked (the additive mask then cancels in the softmax: softmax of the raw scores)
  H  uniform attention with Q and K on disjoint columns: every score still 0, but dK = dS^T Q is nonzero and bit-exact
  I  subset attention: C with j bits of the code left out -> 2^j keys tie at score 0, P = 2^-j there; O, dV, dQ and dK bit-exact
  J  graded ("tent") rows: running maxima that move by 0.5 per tile, different rows of a wave at different updates -- the
     online-softmax rescale with factors between 0 and 1, every element judged against float64 within a first-order rounding bound
H, I, J run on an explicit power-of-two softmax scale (Problem(scale=)), so integer operands give exact scores at every head size.

Plain helper module: no fixtures, no hooks.  Every check takes a *backend* -- an object with `device`, `run(problem)` (forward,
and backward when the case has one, on the problem's windows) and `keep(problem)` (the dropout keep mask [B, nh, Lq, Lk] of that
launch, None without dropout) -- so tests/test_exact_attn_harness_cpu.py proves each check on the CPU against a stand-in written
in torch, and against deliberately wrong stand-ins, before tests/test_attn_exact_gpu.py points them at the HIP kernels.
"""
import collections
import math
import re

import torch

import exact_gemm as E
from exact_gemm import BF16, F32, Window, generator, integers

DT = {"bf16": BF16, "f32": F32}
TOL = {F32: 2e-5, BF16: 1.2e-2}          # tests/test_ops_gpu.py: tol(dtype), unchanged; its attention test takes 2 x (O, LSE), 4 x (dQ, dK, dV)
ATTN_KERNEL_RE = re.compile(rb"_Z\d+attn_\w*kernel\w*")

# ---------------------------------------------------------------------------------------------- A. the route table
_TY = {"bf16": "DF16b", "f32": "f"}
FWD_ROUTES = {
    "decode": lambda c: "attn_decode_kernelI%sLi%dEE" % (_TY[c.dtype], c.d),
    "tiled": lambda c: "attn_fwd_kernelI%sLi%dEE" % (_TY[c.dtype], c.d),
}
BWD_ROUTES = {
    "two0": lambda c: "attn_bwd_kernelI%sLi%dEE" % (_TY[c.dtype], c.d),       # two-part, dK/dV blocks first
    "two1": lambda c: "attn_bwd_kernelI%sLi%dEE" % (_TY[c.dtype], c.d),       # two-part, dQ blocks first
    "onepass": lambda c: "attn_bwd_onepass_kernelILb1ELb0EE",                  # one pass, hashed draws, 32-bit indices
    "onepass_bits": lambda c: "attn_bwd_onepass_kernelILb1ELb1EE",             # one pass, forward's keep bits
}
# Kernel instantiations no case names, each with its reason.  (The bf16 `E32 = false` BODIES of attn_fwd_kernel / attn_bwd_kernel are
# not symbols of their own: the kernel picks the body on the device by the same index-space test.)
EXEMPT = {
    "attn_bwd_onepass_kernelILb0ELb0EE":
        "64-bit draw indices: needs B * nh * Lq * round4(Lk) >= 2^33 score elements (more than 10 000 batch rows at the text "
        "shape); the same template text runs with 64-bit indices as the float instantiations of attn_bwd_kernel / attn_fwd_kernel",
}

_Case = collections.namedtuple("AttnCase", "dtype d B nh Lq Lk causal neg p bits fused kv_group kv_bstride fwd bwd")


class Case(_Case):
    """One descriptor.  bits: forward writes / backward reads the keep-bit buffer; fused: Q, K, V (and dQ, dK, dV) are column
    slices of ONE [B * L, 3 * nh * d] buffer; bwd: a key of BWD_ROUTES, None (forward only) or "refuse" (the backward must answer
    GSTVD_E_UNSUPPORTED)."""
    __slots__ = ()

    @property
    def fwd_kernel(self):
        return FWD_ROUTES[self.fwd](self)

    @property
    def bwd_kernel(self):
        return BWD_ROUTES[self.bwd](self) if self.bwd in BWD_ROUTES else None

    @property
    def dq_first(self):
        return {"two0": 0, "two1": 1}.get(self.bwd)

    @property
    def has_bwd(self):
        return self.bwd in BWD_ROUTES

    @property
    def id(self):
        s = "%s-d%d-%dx%d-q%d-k%d-%s" % (self.dtype, self.d, self.B, self.nh, self.Lq, self.Lk, self.fwd)
        s += "-" + (self.bwd or "fwdonly")
        if self.causal: s += "-causal"
        if self.neg != -10000.0: s += "-neg1e9"
        if self.p: s += "-drop"
        if self.bits: s += "-bits"
        if self.fused: s += "-fused"
        if self.kv_group > 1: s += "-g%d" % self.kv_group
        if self.kv_bstride: s += "-kvs%d" % self.kv_bstride
        return s


def two(Lq, Lk):
    """The two-part backward's block order as the table states it: the class of blocks that walks more 64-row chunks goes first,
    the key-owning (dK / dV) blocks at a tie."""
    return "two1" if -(-Lk // 64) > -(-Lq // 64) else "two0"


def case(dtype, d, Lq, Lk, fwd, bwd, B=2, nh=2, causal=False, neg=-10000.0, p=0.0, bits=False, fused=False, kv_group=1, kv_bstride=0):
    return Case(dtype, d, B, nh, Lq, Lk, bool(causal), float(neg), float(p), bool(bits), bool(fused), kv_group, kv_bstride, fwd, bwd)


KEYS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 293]
QUERIES = [15, 17, 63, 64, 65, 256, 1024, 1025]


def build_cases():
    c = []
    for dt in ("bf16", "f32"):
        for d in (32, 64, 128):
            one = dt == "bf16" and d == 64          # the one-pass backward's type and head size

            def bwd_of(Lq, Lk, causal, p=0.0, bits=False):
                if one and not causal and 64 < Lk <= 256 and 64 <= Lq <= 1024:
                    return "onepass_bits" if bits and p > 0 else "onepass"
                return two(Lq, Lk)
            # -- the tiled forward and the two-part backward over every key count; query counts dealt round-robin (Lq != Lk under
            #    the causal mask), dropout on every other case, both mask values
            for i, Lk in enumerate(KEYS):
                Lq = [17, 65, 15, 63, 64, 256][i % 6]
                causal = i % 4 == 1
                p = 0.5 if i % 2 == 0 else 0.0
                c.append(case(dt, d, Lq, Lk, "tiled", bwd_of(Lq, Lk, causal), causal=causal, p=p, neg=-1e9 if i % 3 == 2 else -10000.0))
            # -- every query count (1024 / 1025: one batch row); both block orders and the tie nkb == nqb
            for i, Lq in enumerate(QUERIES):
                Lk = [37, 300, 64, 130, 65, 16, 64, 40][i]
                causal = i in (2, 5)
                c.append(case(dt, d, Lq, Lk, "tiled", bwd_of(Lq, Lk, causal), B=1 if Lq >= 1024 else 2, causal=causal, p=0.5 if i % 2 else 0.0))
            # -- one query: the decode kernel at every key count (no dropout, no causal mask) ...
            for i, Lk in enumerate(KEYS):
                c.append(case(dt, d, 1, Lk, "decode", two(1, Lk), B=3, neg=-1e9 if i % 2 else -10000.0))
            # ... and the tiled kernel once dropout or the causal mask is on
            c += [case(dt, d, 1, 293, "tiled", "two1", p=0.5), case(dt, d, 1, 17, "tiled", "two0", causal=True),
                  case(dt, d, 1, 65, "tiled", "two1", causal=True, p=0.5)]
            # -- shared keys / values (kv_group) and a KV-cache batch stride: forward only, both forward kernels; the backward refuses
            c += [case(dt, d, 1, 77, "decode", None, B=6, kv_group=3, kv_bstride=90), case(dt, d, 5, 70, "tiled", None, B=4, kv_group=2, kv_bstride=80),
                  case(dt, d, 3, 19, "tiled", "refuse", B=4, kv_group=2)]
            # -- the fused QKV layout (Lq == Lk; the neighbours of an operand are data)
            c += [case(dt, d, 65, 65, "tiled", bwd_of(65, 65, False), fused=True, p=0.5), case(dt, d, 25, 25, "tiled", "two0", fused=True, causal=True)]
    # -- the one-pass backward (bf16, d = 64, no causal mask): every key count of its range, with hashed draws, with forward's keep
    #    bits and without dropout; both sides of each border of the range (keys 64 | 65 and 256 | 257, queries 63 | 64 and 1024 | 1025)
    for i, Lk in enumerate([65, 127, 128, 129, 255, 256]):
        Lq = [64, 65, 256, 127, 64, 1024][i]
        c += [case("bf16", 64, Lq, Lk, "tiled", "onepass_bits", B=1 if Lq == 1024 else 2, p=0.5, bits=True),
              case("bf16", 64, Lq, Lk, "tiled", "onepass", B=1 if Lq == 1024 else 2, p=0.5 if i % 2 else 0.0)]
    c += [case("bf16", 64, 64, 64, "tiled", "two0", p=0.5), case("bf16", 64, 64, 65, "tiled", "onepass", p=0.5),
          case("bf16", 64, 100, 256, "tiled", "onepass", p=0.5), case("bf16", 64, 100, 257, "tiled", "two1", p=0.5),
          case("bf16", 64, 63, 200, "tiled", "two1", p=0.5), case("bf16", 64, 64, 200, "tiled", "onepass_bits", p=0.5, bits=True),
          case("bf16", 64, 1024, 200, "tiled", "onepass_bits", B=1, p=0.5, bits=True), case("bf16", 64, 1025, 200, "tiled", "two0", B=1, p=0.5),
          case("bf16", 64, 100, 200, "tiled", "two1", causal=True, p=0.5),           # the causal mask keeps a one-pass shape on the two-part kernel
          case("f32", 64, 100, 200, "tiled", "two1", p=0.5), case("bf16", 128, 100, 200, "tiled", "two1", p=0.5)]
    # -- the production shapes (head of csrc/attention.hip), both types
    for dt in ("bf16", "f32"):
        one = dt == "bf16"
        c += [case(dt, 64, 256, 256, "tiled", "onepass_bits" if one else "two0", nh=12, p=0.5, bits=one, fused=True),       # text self-attention
              case(dt, 128, 37, 37, "tiled", "two0", nh=8, p=0.5, fused=True),                                            # vision self-attention
              case(dt, 128, 256, 37, "tiled", "two0", nh=8, p=0.5), case(dt, 128, 37, 256, "tiled", "two1", nh=8, p=0.5),  # co-attention, both ways
              case(dt, 64, 25, 25, "tiled", "two0", nh=12, causal=True, p=0.5, fused=True),                               # decoder self-attention
              case(dt, 64, 25, 293, "tiled", "two1", nh=12, neg=-1e9, p=0.5),                                             # decoder cross-attention
              case(dt, 64, 1, 293, "decode", "two1", nh=12, neg=-1e9)]                                                    # ... its decode step
    return c


CASES = build_cases()


def kernels_named(cases=None):
    """(forward symbols, backward symbols) the table names."""
    cs = CASES if cases is None else cases
    return sorted(set(c.fwd_kernel for c in cs)), sorted(set(c.bwd_kernel for c in cs if c.has_bwd))


def check_census(symbols, cases=None, out=print):
    """Every attention kernel instantiation of the built library is named by a case of the table or exempt, and every kernel the
    table names exists."""
    cs = CASES if cases is None else cases
    fwd, bwd = kernels_named(cs)
    named = sorted(set(fwd) | set(bwd))
    reached = set()
    for s in symbols:
        hits = [n for n in named if n in s]
        ex = [e for e in EXEMPT if e in s]
        assert len(hits) + len(ex) == 1, "%s: named by %r, exempt as %r" % (s, hits, ex)
        reached.update(hits)
        users = [c for c in cs if hits and hits[0] in (c.fwd_kernel, c.bwd_kernel)]
        extra = ""
        if hits and "attn_bwd_kernel" in hits[0]:
            extra = ", dq_first 0: %d, 1: %d" % (sum(1 for c in users if c.bwd == "two0"), sum(1 for c in users if c.bwd == "two1"))
        out("%-62s %s" % (s, ("%d case(s)%s, e.g. %s" % (len(users), extra, users[0].id)) if hits else "EXEMPT: " + EXEMPT[ex[0]]))
    assert reached == set(named), "kernels named by a case but absent from the library: %r" % sorted(set(named) - reached)
    # both block orders and the tie for every instantiation of the two-part backward
    for n in bwd:
        if "attn_bwd_kernel" in n:
            us = [c for c in cs if c.bwd_kernel == n]
            assert any(c.bwd == "two0" for c in us) and any(c.bwd == "two1" for c in us), n
            assert any(-(-c.Lk // 64) == -(-c.Lq // 64) for c in us), n + ": no case with nkb == nqb"


# ---------------------------------------------------------------------------------------------- B. the windows of one launch
def round4(x):
    return (x + 3) & ~3


class Problem(object):
    """The windows of one launch of case `c`: Q, K, V, dO and the key mask inside NaN-poisoned allocations, O, LSE, dQ, dK, dV,
    delta and the keep bits inside canary allocations; leading dimensions nh * d + 8 or + 16 (by `seed`), guard rows around
    every operand.  Tensors are addressed as [B, L, nh, d] (statistics [B, nh, Lq], key mask [B / kv_group, Lk])."""

    def __init__(self, c, device, seed=0, key_mask=True, scale=None):
        self.c, self.device, self.seed = c, device, seed
        self.scale_arg, self.scale = scale, scale32(c.d) if scale is None else float(scale)    # None: the descriptor's default, fl32(1 / sqrt(d))
        dt, H = DT[c.dtype], c.nh * c.d
        pad = 8 if seed % 2 == 0 else 16
        self.Bkv = c.B // c.kv_group
        assert self.Bkv * c.kv_group == c.B and (not c.fused or c.Lq == c.Lk)
        kbs = c.kv_bstride or c.Lk

        def win(L, fill, batch, cols=H, rows_stride=None):
            ld = cols + pad
            return Window(L, cols, dt, device, fill, ld=ld, batch=batch, stride=(rows_stride or L) * ld)
        self.wins = {}
        if c.fused:
            qkv = self.wins["QKV"] = win(c.Lq, "poison", c.B, cols=3 * H)
            self.ld_in = self.ld_kv = qkv.ld
            self._Q, self._K, self._V = (qkv.view3[..., i * H:(i + 1) * H] for i in range(3))
        else:
            q, k, v = win(c.Lq, "poison", c.B), win(c.Lk, "poison", self.Bkv, rows_stride=kbs), win(c.Lk, "poison", self.Bkv, rows_stride=kbs)
            self.wins.update(Q=q, K=k, V=v)
            self.ld_in, self.ld_kv = q.ld, k.ld
            self._Q, self._K, self._V = q.view3, k.view3, v.view3
        o = self.wins["O"] = win(c.Lq, "canary", c.B)
        self._O, self.ld_o = o.view3, o.ld
        nstat = c.B * c.nh * c.Lq
        self.wins["LSE"] = Window(1, nstat, F32, device, "canary")
        self.km = None
        if key_mask:
            self.wins["key_mask"] = Window(1, self.Bkv * c.Lk, F32, device, "poison")
            self.km = self.wins["key_mask"].vector().view(self.Bkv, c.Lk)
        self.bits = None
        if c.bits:
            n = c.B * c.nh * ((c.Lq + 15) // 16) * ((c.Lk + 15) // 16) * 4
            self.wins["drop_bits"] = Window(1, n, torch.int64, device, "canary")
            self.bits = self.wins["drop_bits"].vector()
        if c.has_bwd or c.bwd == "refuse":
            do = self.wins["dO"] = win(c.Lq, "poison", c.B)
            self._dO, self.ld_do = do.view3, do.ld
            self.wins["delta"] = Window(1, nstat, F32, device, "canary")
            if c.fused:
                g = self.wins["dQKV"] = win(c.Lq, "canary", c.B, cols=3 * H)
                self.ld_dq = self.ld_dkv = g.ld
                self._dQ, self._dK, self._dV = (g.view3[..., i * H:(i + 1) * H] for i in range(3))
            else:
                dq, dk, dv = win(c.Lq, "canary", c.B), win(c.Lk, "canary", self.Bkv), win(c.Lk, "canary", self.Bkv)
                self.wins.update(dQ=dq, dK=dk, dV=dv)
                self.ld_dq, self.ld_dkv = dq.ld, dk.ld
                self._dQ, self._dK, self._dV = dq.view3, dk.view3, dv.view3

    def t(self, name):
        """The operand `name` as a [B, L, nh, d] view of its window (LSE, delta: [B, nh, Lq])."""
        c = self.c
        if name in ("LSE", "delta"):
            return self.wins[name].vector().view(c.B, c.nh, c.Lq)
        return getattr(self, "_" + name).unflatten(-1, (c.nh, c.d))

    def set(self, **kw):
        for name, val in kw.items():
            if name == "key_mask":
                self.km.copy_(val)
            else:
                self.t(name).copy_(val)
        return self

    OUTPUTS = ("O", "LSE", "dQ", "dK", "dV", "delta")

    def outputs(self):
        r = {}
        for n in self.OUTPUTS:
            if n in ("O", "LSE") or self.c.has_bwd:
                r[n] = self.t(n).clone()
        return r

    def assert_windows(self, name):
        """Nothing outside a window changed, no canary is left inside an output window, no NaN reached a result."""
        for tag, w in self.wins.items():
            w.assert_surroundings_untouched("%s: %s" % (name, tag))
            if w.fill == "canary" and (self.c.has_bwd or tag in ("O", "LSE", "drop_bits")):
                inner = w.flat[w.inside]
                left = int((inner.view(E._INT[w.dtype]) == E.CANARY[w.dtype]).sum().item())
                assert left == 0, "%s: %s: %d element(s) inside the window were never written" % (name, tag, left)
                if w.dtype.is_floating_point:
                    nn = int(torch.isnan(inner).sum().item())
                    assert nn == 0, "%s: %s: %d NaN(s) in the result (something outside an operand was read)" % (name, tag, nn)


def launch(be, c, inp, seed=0, name=None, scale=None):
    """One launch of case `c` on backend `be` with the inputs `inp` (Q, K, V, dO as [B, L, nh, d] float tensors, key_mask or
    None) and the softmax scale `scale` (None: the descriptor's default): windows built, backend run, windows checked.  Returns
    (outputs, keep mask or None)."""
    name = name or c.id
    km = inp.get("key_mask")
    p = Problem(c, be.device, seed, key_mask=km is not None, scale=scale)
    p.set(**{k: v for k, v in inp.items() if v is not None and (k != "dO" or c.has_bwd or c.bwd == "refuse")})
    be.run(p)
    p.assert_windows(name)
    keep = be.keep(p) if c.p > 0 else None
    out = p.outputs()
    if p.bits is not None:
        out["drop_bits"] = p.bits.clone()
    return out, keep


# ---------------------------------------------------------------------------------------------- float64 reference
def scale32(d):
    """The scale the descriptor carries: fl32(1 / sqrt(d))."""
    return float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32))


def allowed_keys(c, km, device):
    """[B, 1, Lq, Lk] bool: the keys the key mask and the causal mask allow each query."""
    a = torch.ones(c.B, 1, c.Lq, c.Lk, dtype=torch.bool, device=device)
    if km is not None:
        a = a & (km != 0).repeat_interleave(c.kv_group, 0)[:, None, None, :]
    if c.causal:
        a = a & (torch.arange(c.Lk, device=device)[None, :] <= torch.arange(c.Lq, device=device)[:, None])[None, None]
    return a


def reference(c, inp, keep, scale=None, P=None, O_stored=None):
    """float64 attention with the kernels' conventions: the additive mask term is added ONCE (key mask or causal mask or both),
    dropout keeps with factor 1 / (1 - p), delta = rowsum(dO * O) with O as stored (rounded to the operand type; `O_stored`: the
    O a launch wrote).  `scale`: the softmax scale (None: scale32(d)).  `P`: the probabilities [B, nh, Lq, Lk], where a
    construction knows them exactly (no softmax is formed then, and no LSE returned)."""
    dev = inp["Q"].device
    Q, K, V = inp["Q"].double(), inp["K"].double().repeat_interleave(c.kv_group, 0), inp["V"].double().repeat_interleave(c.kv_group, 0)
    sc = scale32(c.d) if scale is None else float(scale)
    if P is None:
        al = allowed_keys(c, inp.get("key_mask"), dev)
        s = torch.einsum("bqhd,bkhd->bhqk", Q, K) * sc + torch.where(al, 0.0, c.neg).double()
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        P = e / l
        r = dict(P=P, S=s, LSE=(m + torch.log(l)).squeeze(-1))
    else:
        r = dict(P=P)
    r["scale"] = sc
    f = (keep.double() / (1.0 - c.p)) if keep is not None else torch.ones_like(P)
    Pd = r["Pd"] = P * f
    r["O"] = torch.einsum("bhqk,bkhd->bqhd", Pd, V)
    if inp.get("dO") is not None and c.has_bwd:
        dO = inp["dO"].double()
        Os = r["O"].float().to(DT[c.dtype]).double() if O_stored is None else O_stored.double()
        r["delta"] = (dO * Os).sum(-1).permute(0, 2, 1)
        dP = torch.einsum("bqhd,bkhd->bhqk", dO, V)
        dS = r["dS"] = P * (dP * f - r["delta"][..., None]) * sc
        r["dV"] = torch.einsum("bhqk,bqhd->bkhd", Pd, dO)
        r["dQ"] = torch.einsum("bhqk,bkhd->bqhd", dS, K)
        r["dK"] = torch.einsum("bhqk,bqhd->bkhd", dS, Q)
    return r


# ---------------------------------------------------------------------------------------------- assertions
def assert_bit_equal(got, ref, name):
    """exact_gemm.assert_bit_equal with the sign of a zero left out of it (0 * -x is -0 on one side, an empty sum +0 on the other)."""
    E.assert_bit_equal(got + 0, ref + 0, name)


def _ordered(x):
    """Bit patterns of a float tensor as integers that are monotonic in the value (-0 and +0 coincide)."""
    bits = 16 if x.dtype == BF16 else 32
    i = x.contiguous().view(E._INT[x.dtype]).to(torch.int64)
    return torch.where(i >= 0, i, -(i & ((1 << (bits - 1)) - 1)))


def assert_within_one_ulp(got, want, name):
    """`got` is `want` (given in float64 / float32, rounded to got's type here) or one of its two neighbours in got's type."""
    w = want.float().to(got.dtype).reshape(got.shape)
    assert torch.isfinite(got.float()).all(), name + ": non-finite output"
    diff = (_ordered(got) - _ordered(w)).abs()
    n = int((diff > 1).sum().item())
    if n:
        i = tuple(int(x) for x in torch.nonzero(diff > 1)[0])
        raise AssertionError("%s: %d of %d elements are more than one ulp of %s away; first at %s: got %r want %r"
                             % (name, n, diff.numel(), got.dtype, i, got[i].item(), w[i].item()))


def assert_all_zero(x, name):
    n = int((x != 0).sum().item())
    assert n == 0, "%s: %d of %d elements are not exactly 0 (largest %.3e)" % (name, n, x.numel(), x.float().abs().max().item())


def assert_same(a, b, name):
    assert torch.equal(a, b), "%s: %d of %d elements differ between the two runs" % (name, int((a != b).sum().item()), a.numel())


def rel_to_max(got, ref):
    got, ref = got.double(), ref.double().reshape(got.shape)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def assert_close(got, ref, tol, name, out=None):
    assert torch.isfinite(got.float()).all(), name + ": non-finite output"
    err = rel_to_max(got, ref)
    if out:
        out("%s: rel-to-max error %.3e (tol %.2e)" % (name, err, tol))
    assert err <= tol, "%s: rel-to-max error %.3e (tol %.2e)" % (name, err, tol)


def fits(x, dtype):
    """Every element of the float64 tensor is exactly representable in `dtype`."""
    return bool((x.float().to(dtype).double() == x).all())


def make_mask(c, gen, device, allowed=None):
    """A key mask [B / kv_group, Lk] with `allowed` unmasked keys per row (default: about two thirds), at random positions; key 0
    stays unmasked (under the causal mask query 0 sees nothing else)."""
    Bkv = c.B // c.kv_group
    n = max(1, (2 * c.Lk + 2) // 3) if allowed is None else allowed
    km = torch.zeros(Bkv, c.Lk, device=device)
    for b in range(Bkv):
        idx = torch.randperm(c.Lk - 1, generator=gen, device=device)[:n - 1] + 1
        km[b, idx] = 1
        km[b, 0] = 1
    return km


# ---------------------------------------------------------------------------------------------- C. one-hot attention
def check_onehot(be, c, seed=0):
    """K[k] = the binary code of k in +-16, repeated floor(d / bits) times (signs flipped per (batch row, head, column) so that a
    wrong head or batch offset scrambles the scores); Q[q] = K[sel(q)] with sel random over the allowed keys.  The selected score
    is 256 * reps * bits * scale, every other at least 2 * 256 * reps * scale >= 181 lower: exp underflows to an exact 0, P is
    exactly one-hot, l = 1, and O[q] = fac * keep[q, sel(q)] * V[sel(q)] bit for bit.  Backward (integer V and dO): dV[k] = sum of
    fac * keep * dO[q] over the queries that selected k, exactly; dQ = dK = 0 exactly (dP * fac - delta cancels)."""
    dev, dt = be.device, DT[c.dtype]
    gen = generator(1000 + seed, dev)
    km = make_mask(c, gen, dev) if seed % 3 != 2 else None
    nb = max(1, (c.Lk - 1).bit_length())
    reps = c.d // nb
    assert reps >= 1 and 2 * 256 * reps * scale32(c.d) > 104
    k = torch.arange(c.Lk, device=dev)
    code = torch.zeros(c.Lk, c.d, device=dev)
    code[:, :nb * reps] = (((k[:, None] >> torch.arange(nb, device=dev)[None, :]) & 1) * 32.0 - 16.0).repeat(1, reps)
    Bkv = c.B // c.kv_group
    sign = torch.randint(0, 2, (Bkv, 1, c.nh, c.d), generator=gen, device=dev).float() * 2 - 1
    K = code[None, :, None, :] * sign                                          # [Bkv, Lk, nh, d]
    al = allowed_keys(c, km, dev).expand(c.B, c.nh, c.Lq, c.Lk)
    sel = torch.multinomial(al.reshape(-1, c.Lk).float(), 1, generator=gen).view(c.B, c.nh, c.Lq)
    bidx = torch.arange(c.B, device=dev)[:, None, None]
    hidx = torch.arange(c.nh, device=dev)[None, :, None]
    Kx = K.repeat_interleave(c.kv_group, 0)
    Q = Kx[bidx, sel, hidx].permute(0, 2, 1, 3)                                # [B, Lq, nh, d]
    if c.has_bwd:
        V = integers((Bkv, c.Lk, c.nh, c.d), 64, gen, torch.float32, dev)
    else:
        V = torch.randn(Bkv, c.Lk, c.nh, c.d, generator=gen, device=dev).bfloat16().float()
    dO = integers((c.B, c.Lq, c.nh, c.d), 3, gen, torch.float32, dev)
    out, keep = launch(be, c, dict(Q=Q, K=K, V=V, dO=dO, key_mask=km), seed, c.id + ": one-hot")
    fac = 1.0 / (1.0 - c.p)
    assert fac in (1.0, 2.0)
    w = torch.full((c.B, c.nh, c.Lq), fac, device=dev, dtype=torch.float64)
    if keep is not None:
        w = w * keep.gather(-1, sel[..., None]).squeeze(-1).double()
    Vx = V.repeat_interleave(c.kv_group, 0).double()
    want_O = w.permute(0, 2, 1)[..., None] * Vx[bidx, sel, hidx].permute(0, 2, 1, 3)
    assert_bit_equal(out["O"], want_O, c.id + ": one-hot O")
    s_sel = torch.tensor(256.0 * reps * nb, dtype=torch.float32) * torch.tensor(scale32(c.d), dtype=torch.float32)   # fl(s * fl(scale))
    assert_within_one_ulp(out["LSE"], s_sel.to(dev).expand(c.B, c.nh, c.Lq), c.id + ": one-hot LSE")
    if not c.has_bwd:
        return
    want_dV = torch.zeros(c.B, c.Lk, c.nh, c.d, dtype=torch.float64, device=dev)
    flat = want_dV.permute(0, 2, 1, 3).reshape(c.B * c.nh * c.Lk, c.d)
    rows = ((bidx * c.nh + hidx) * c.Lk + sel).reshape(-1)
    flat.index_add_(0, rows, (w[..., None] * dO.double().permute(0, 2, 1, 3)).reshape(-1, c.d))
    want_dV = flat.view(c.B, c.nh, c.Lk, c.d).permute(0, 2, 1, 3)
    assert_bit_equal(out["dV"], want_dV, c.id + ": one-hot dV")
    assert_bit_equal(out["delta"], (dO.double() * want_O).sum(-1).permute(0, 2, 1), c.id + ": one-hot delta")
    assert_all_zero(out["dQ"], c.id + ": one-hot dQ")
    assert_all_zero(out["dK"], c.id + ": one-hot dK")


# ---------------------------------------------------------------------------------------------- D. uniform attention
def uniform_must_be_exact(c):
    """The mode check_uniform MUST reach for a case, from the table alone: wherever every query sees a power-of-two number of
    keys (no causal mask, or one query) fp32 is bit-exact (d = 64) or within one ulp (d = 32 / 128), and bf16 d = 64 without
    dropout and with n <= 128 keys is bit-exact (the 8-bit guard on the float64 intermediates must hold there: dP - delta is
    (n a - b) / n with |a| <= 1 and b the column sum of n values in {-1, 0, 1}, below 2^8 for n <= 128 unless all n agree); None:
    the data decide (bf16 with dropout or 256 keys: a ninth bit may appear) or the tolerance applies (ragged counts under the
    causal mask, bf16 d = 32 / 128)."""
    if not c.has_bwd or (c.causal and c.Lq > 1):
        return None
    if c.dtype == "f32":
        return "exact" if c.d == 64 else "ulp"
    return "exact" if c.d == 64 and c.p == 0 and c.Lk < 256 else None


def check_uniform(be, c, seed=0, out=None):
    """Q = 0: every allowed key has probability 1 / n(q), O[q] = fl32(sum of the allowed V rows) * fl32(1 / n) rounded to the
    output type -- bit-equal when n is a power of two, within one rounding of the output type otherwise -- and LSE = log n.
    V in {-1, 0, 1}, K in [-3, 3], dO = +-1 in one column per row: with n a power of two P, P * fac, O (|sum| <= n: 8 bits),
    dP * fac - delta (a multiple of 1 / n below 2 + 2) and dS (d = 64: scale 1 / 8) are dyadic rationals of at most 8 significant
    bits, so the bf16 roundings of P and dS are exact too and dQ, dK, dV are bit-equal to the float64 reference (guarded below
    on the float64 intermediates; uniform_must_be_exact() names the cases for which that guard MUST hold).  d = 32 / 128 in fp32:
    the scale fl32(1 / sqrt(d)) is not dyadic, every dS term is rounded once, and a SUM of such terms cannot be held to one ulp of
    the result (first run on the MI355X with K dense in [-3, 3]: |dQ - ref| up to 4.1e-8 where 2^-23 * sum |dS| |K| was 2.9e-8).
    Those cases therefore take a K with ONE term per element of dQ: K[k] = +-1 or +-2 times e_(k mod d) for the keys of one block
    of d keys (which block: by the seed), 0 elsewhere -- dQ[q, col] = s_k * fl32(x * fl32(scale)) with x dyadic, one rounding, and
    the assertion is the issue's: within one fp32 ulp of the float64 reference; dV and delta stay bit-equal (the scale is not in
    them).  That dQ check therefore sees the dS of ONE block of d keys per case, not of every key: the seed moves the block from
    case to case, the keys of the other blocks are counted by O and dV, and every key's dS is walked by the d = 64 cases (dense
    K) and by check_dropout_masks' dQ recovery.  Everything else: the tolerance of test_ops_gpu.py, unchanged.  Returns the mode.
    """
    dev, dt = be.device, DT[c.dtype]
    gen = generator(2000 + seed, dev)
    pow2 = 1 << (c.Lk.bit_length() - 1)
    if pow2 == c.Lk and c.Lk > 1 and seed % 2:
        pow2 //= 2
    km = make_mask(c, gen, dev, allowed=pow2) if (pow2 < c.Lk or seed % 3 == 0) else None
    Bkv = c.B // c.kv_group
    Q = torch.zeros(c.B, c.Lq, c.nh, c.d, device=dev)
    K = integers((Bkv, c.Lk, c.nh, c.d), 3, gen, torch.float32, dev)
    if dt == F32 and c.d != 64:
        kk = torch.arange(c.Lk, device=dev)
        live = (kk // c.d) == seed % (-(-c.Lk // c.d))
        sk = (torch.randint(0, 2, (Bkv, c.Lk, c.nh), generator=gen, device=dev).float() * 2 - 1) * (1 + torch.randint(0, 2, (Bkv, c.Lk, c.nh), generator=gen, device=dev).float())
        K = torch.zeros_like(K)
        K[:, kk[live], :, kk[live] % c.d] = sk[:, kk[live]].permute(1, 0, 2)
    V = integers((Bkv, c.Lk, c.nh, c.d), 1, gen, torch.float32, dev)
    col = torch.randint(0, c.d, (c.B, c.Lq, c.nh, 1), generator=gen, device=dev)
    dO = torch.zeros(c.B, c.Lq, c.nh, c.d, device=dev).scatter_(-1, col, torch.randint(0, 2, col.shape, generator=gen, device=dev).float() * 2 - 1)
    inp = dict(Q=Q, K=K, V=V, dO=dO, key_mask=km)
    got, keep = launch(be, c, inp, seed, c.id + ": uniform")
    ref = reference(c, inp, keep)
    al = allowed_keys(c, km, dev)
    n = al.sum(-1)                                                             # [B, 1, Lq]
    assert int(n.min()) >= 1
    all_pow2 = bool(((n & (n - 1)) == 0).all())
    f = (keep.double() / (1.0 - c.p)) if keep is not None else torch.ones((), dtype=torch.float64, device=dev)
    ssum = torch.einsum("bhqk,bkhd->bqhd", (al.double() * f).expand(c.B, c.nh, c.Lq, c.Lk), V.double().repeat_interleave(c.kv_group, 0))
    want_O = (ssum.float() * (1.0 / n.float()).permute(0, 2, 1)[..., None]).double()          # fl32(sum) * fl32(1 / n), one fp32 multiply
    if all_pow2:
        assert_bit_equal(got["O"], want_O, c.id + ": uniform O")
    else:
        assert_within_one_ulp(got["O"], want_O, c.id + ": uniform O")
    assert_close(got["LSE"], torch.log(n.double()).expand(c.B, c.nh, c.Lq), 2 * TOL[F32], c.id + ": uniform LSE")
    if not c.has_bwd:
        return "forward"
    exact = all_pow2 and (dt == F32 or (fits(ref["Pd"], BF16) and fits(ref["O"], BF16) and (c.d != 64 or fits(ref["dS"], BF16))))
    if exact:
        assert_bit_equal(got["dV"], ref["dV"], c.id + ": uniform dV")
        assert_bit_equal(got["delta"], ref["delta"], c.id + ": uniform delta")
    if exact and c.d == 64:
        assert_bit_equal(got["dQ"], ref["dQ"], c.id + ": uniform dQ")
        mode = "exact"
    elif exact and dt == F32:
        assert_within_one_ulp(got["dQ"], ref["dQ"], c.id + ": uniform dQ")
        mode = "ulp"
    else:
        mode = "tol"
        for nme in ("dQ", "dV"):
            assert_close(got[nme], ref[nme], 4 * TOL[dt], "%s: uniform %s" % (c.id, nme))
    assert_all_zero(got["dK"], c.id + ": uniform dK")                          # dK = dS^T Q with Q = 0
    must = uniform_must_be_exact(c)
    assert must is None or mode == must, "%s: uniform backward was checked as %r, the construction promises %r" % (c.id, mode, must)
    if out:
        out("%s: uniform backward checked as %s" % (c.id, mode))
    return mode


# ---------------------------------------------------------------------------------------------- E. invariances
def random_inputs(c, gen, dev, km=None):
    dt, Bkv = DT[c.dtype], c.B // c.kv_group

    def rn(*shape):
        return (torch.randn(*shape, generator=gen, device=dev) * 0.5).to(dt).float()
    return dict(Q=rn(c.B, c.Lq, c.nh, c.d), K=rn(Bkv, c.Lk, c.nh, c.d), V=rn(Bkv, c.Lk, c.nh, c.d), dO=rn(c.B, c.Lq, c.nh, c.d), key_mask=km)


def _names(c):
    return ("O", "LSE", "dQ", "dK", "dV") if c.has_bwd else ("O", "LSE")


def check_mask_none_vs_ones(be, c, seed=0):
    dev = be.device
    inp = random_inputs(c, generator(3000 + seed, dev), dev)
    a, _ = launch(be, c, inp, seed, c.id + ": no key mask")
    b, _ = launch(be, c, dict(inp, key_mask=torch.ones(c.B // c.kv_group, c.Lk, device=dev)), seed + 1, c.id + ": key mask of ones")
    for n in _names(c):
        assert_same(a[n], b[n], "%s: key mask None vs ones: %s" % (c.id, n))


def check_masked_rows_do_not_matter(be, c, seed=0):
    """The K and V rows of masked keys are replaced by other finite values (V: by 1e4 too; K by 1e4 only where the mask term is
    -1e9 -- against -10000 a score of that size is legitimately larger): nothing changes, and dK, dV of masked keys are exactly 0."""
    dev = be.device
    gen = generator(3100 + seed, dev)
    km = make_mask(c, gen, dev)
    inp = random_inputs(c, gen, dev, km)
    a, _ = launch(be, c, inp, seed, c.id + ": masked rows, first contents")
    masked = (km == 0)[:, :, None, None]
    other = random_inputs(c, gen, dev, km)
    K2 = torch.where(masked, other["K"] * (2e4 if c.neg < -1e8 else 1.0), inp["K"])
    V2 = torch.where(masked, other["V"] + 1e4, inp["V"])
    b, _ = launch(be, c, dict(inp, K=K2, V=V2), seed + 1, c.id + ": masked rows, other contents")
    for n in _names(c):
        if n in ("dK", "dV"):
            m = masked.repeat_interleave(c.kv_group, 0).expand_as(a[n])
            assert_all_zero(a[n][m], "%s: %s of masked keys" % (c.id, n))
            assert_all_zero(b[n][m], "%s: %s of masked keys (other contents)" % (c.id, n))
        assert_same(a[n], b[n], "%s: contents of masked K / V rows changed %s" % (c.id, n))


def check_causal_later_keys(be, c, seed=0):
    """Causal mask: the K / V rows of keys after position t are replaced; O, LSE and dQ of the queries <= t do not change."""
    assert c.causal
    dev = be.device
    gen = generator(3200 + seed, dev)
    inp = random_inputs(c, gen, dev, make_mask(c, gen, dev) if seed % 2 else None)
    t = min(c.Lq, c.Lk) // 2
    other = random_inputs(c, gen, dev)
    later = (torch.arange(c.Lk, device=dev) > t)[None, :, None, None]
    a, _ = launch(be, c, inp, seed, c.id + ": causal, first contents")
    b, _ = launch(be, c, dict(inp, K=torch.where(later, other["K"], inp["K"]), V=torch.where(later, other["V"] * 3, inp["V"])), seed + 1,
                  c.id + ": causal, later keys replaced")
    for n in ("O", "dQ") if c.has_bwd else ("O",):
        assert_same(a[n][:, :t + 1], b[n][:, :t + 1], "%s: keys after %d changed %s of queries <= %d" % (c.id, t, n, t))
    assert_same(a["LSE"][..., :t + 1], b["LSE"][..., :t + 1], "%s: keys after %d changed LSE of queries <= %d" % (c.id, t, t))
    # queries <= q_max = Lq - 1 see no key > Lq - 1 at all
    if c.Lk > c.Lq:
        beyond = (torch.arange(c.Lk, device=dev) >= c.Lq)[None, :, None, None]
        b2, _ = launch(be, c, dict(inp, K=torch.where(beyond, other["K"], inp["K"]), V=torch.where(beyond, other["V"] + 1e4, inp["V"])), seed,
                       c.id + ": causal, keys past the last query replaced")
        for n in _names(c):
            assert_same(a[n][:, :c.Lq] if n in ("dK", "dV") else a[n], b2[n][:, :c.Lq] if n in ("dK", "dV") else b2[n],
                        "%s: keys past the last query changed %s" % (c.id, n))


def check_appended_masked_keys(be, c, r, seed=0):
    """Lk -> Lk + r trailing masked keys (same kernels: the case with r more keys names the same routes), dropout off: O, LSE, dQ
    and the first Lk rows of dK / dV are unchanged."""
    assert c.p == 0 and r > 0 and not c.fused
    dev = be.device
    gen = generator(3300 + seed, dev)
    c2 = c._replace(Lk=c.Lk + r, kv_bstride=c.kv_bstride + r if c.kv_bstride else 0)
    km = make_mask(c, gen, dev)
    inp = random_inputs(c, gen, dev, km)
    more = random_inputs(c2, gen, dev)
    inp2 = dict(inp, K=torch.cat([inp["K"], more["K"][:, :r]], 1), V=torch.cat([inp["V"], more["V"][:, :r] + 100], 1),
                key_mask=torch.cat([km, torch.zeros(km.shape[0], r, device=dev)], 1))
    a, _ = launch(be, c, inp, seed, c.id + ": before appending")
    b, _ = launch(be, c2, inp2, seed + 1, c2.id + ": masked keys appended")
    for n in _names(c):
        assert_same(a[n], b[n][:, :c.Lk] if n in ("dK", "dV") else b[n], "%s: %d masked keys appended changed %s" % (c.id, r, n))


def check_permutation(be, c, seed=0):
    """Batch rows and heads permuted (dropout off): the outputs permute."""
    assert c.p == 0 and c.kv_group == 1
    dev = be.device
    gen = generator(3400 + seed, dev)
    inp = random_inputs(c, gen, dev, make_mask(c, gen, dev))
    pb, ph = torch.randperm(c.B, generator=gen, device=dev), torch.randperm(c.nh, generator=gen, device=dev)
    inp2 = {k: (v[pb][:, :, ph] if k != "key_mask" else v[pb]) for k, v in inp.items()}
    a, _ = launch(be, c, inp, seed, c.id + ": identity order")
    b, _ = launch(be, c, inp2, seed, c.id + ": permuted order")
    for n in _names(c):
        want = a[n][pb][:, ph] if n == "LSE" else a[n][pb][:, :, ph]
        assert_same(want, b[n], "%s: permuting batch rows and heads did not permute %s" % (c.id, n))


def check_keep_bits_vs_hash(be, c, seed=0):
    """The one-pass backward with forward's keep bits and with hashed draws: bit-identical outputs; the bits are the mask probe."""
    assert c.bits and c.p > 0
    dev = be.device
    gen = generator(3500 + seed, dev)
    inp = random_inputs(c, gen, dev, make_mask(c, gen, dev))
    a, keep = launch(be, c, inp, seed, c.id + ": keep bits")
    b, _ = launch(be, c._replace(bits=False, bwd="onepass"), inp, seed, c.id + ": hashed draws")
    for n in _names(c):
        assert_same(a[n], b[n], "%s: keep bits vs hashed draws: %s" % (c.id, n))
    # element (b, h, q, k) <-> word (k & 3) of tile (q >> 4, k >> 4), bit 16 * ((k & 15) >> 2) + (q & 15)
    w = a["drop_bits"].view(c.B, c.nh, (c.Lq + 15) // 16, (c.Lk + 15) // 16, 4)
    qi = torch.arange(c.Lq, device=dev)[:, None].expand(c.Lq, c.Lk)
    ki = torch.arange(c.Lk, device=dev)[None, :].expand(c.Lq, c.Lk)
    got = ((w[:, :, qi >> 4, ki >> 4, ki & 3] >> (16 * ((ki & 15) >> 2) + (qi & 15))) & 1) != 0
    assert_same(got, keep, c.id + ": keep bits vs the mask probe")


# ---------------------------------------------------------------------------------------------- F. the dropout masks applied
def _decode_levels(x, hi, name, frac=0.125):
    """Every element of x is within frac * hi of 0 or of hi (hi broadcastable); returns the boolean 'is hi'."""
    x, hi = x.double(), hi.double().expand_as(x)
    up = x > 0.5 * hi
    off = torch.where(up, (x - hi).abs(), x.abs())
    bad = int((off > frac * hi).sum().item())
    assert bad == 0, "%s: %d element(s) decode neither as dropped nor as kept" % (name, bad)
    return up


def check_dropout_masks(be, c, seed=0):
    """Q = 0, p = 0.5, no key mask, indicator operands, one launch per block of d keys / queries:
      forward:  V[k, col] = [k in block j, k mod d == col]                 -> O[q, col]  = (2 / n) keep[q, k_col]
      dK / dV:  dO[q, col] = [q in block i, q mod d == col]                -> dV[k, col] = (2 / n(q_col)) keep[q_col, k]
      dQ:       V[k, :] = dO[q, :] = e_0, K[k, col] = [k in block j, ...]  -> dQ[q, col] = (scale / n) (2 keep[q, k_col] - delta[q])
    Every element of every (b, h) of each recovered matrix equals the mask probe; under the causal mask the disallowed elements
    decode as 'contributes nothing' (0 for the first two; dQ exactly 0)."""
    assert c.p == 0.5 and c.kv_group == 1
    dev, d = be.device, c.d
    al = allowed_keys(c, None, dev).expand(c.B, c.nh, c.Lq, c.Lk)
    n = al.sum(-1).double()                                                   # [B, nh, Lq]
    zeros_q = torch.zeros(c.B, c.Lq, c.nh, d, device=dev)
    zeros_k = torch.zeros(c.B, c.Lk, c.nh, d, device=dev)
    kk, qq = torch.arange(c.Lk, device=dev), torch.arange(c.Lq, device=dev)
    rec_f = torch.zeros(c.B, c.nh, c.Lq, c.Lk, dtype=torch.bool, device=dev)
    rec_kv, rec_q = rec_f.clone(), rec_f.clone()
    probe = None
    nkb, nqb = -(-c.Lk // d), -(-c.Lq // d)
    for blk in range(max(nkb, nqb) if c.has_bwd else nkb):
        V = zeros_k.clone()
        ks = kk[(kk // d) == blk]
        V[:, ks, :, ks % d] = 1.0
        dO = zeros_q.clone()
        qs = qq[(qq // d) == blk]
        dO[:, qs, :, qs % d] = 1.0
        got, keep = launch(be, c, dict(Q=zeros_q, K=zeros_k, V=V, dO=dO, key_mask=None), seed, "%s: draws, block %d" % (c.id, blk))
        probe = keep if probe is None else probe
        assert torch.equal(probe, keep)
        if len(ks):
            o = got["O"].permute(0, 2, 1, 3)[..., ks % d]                     # [B, nh, Lq, |ks|]
            rec_f[..., ks] = _decode_levels(o, (2.0 / n)[..., None], c.id + ": forward draws")
        if c.has_bwd and len(qs):
            dv = got["dV"].permute(0, 2, 1, 3)[..., qs % d].transpose(-1, -2)   # [B, nh, |qs|, Lk]
            rec_kv[:, :, qs] = _decode_levels(dv, (2.0 / n[..., qs])[..., None], c.id + ": dK / dV draws")
    assert_same(rec_f, probe & al, c.id + ": the draws the forward applied vs the mask probe")
    if not c.has_bwd:
        return
    assert_same(rec_kv, probe & al, c.id + ": the draws the key-owning backward applied vs the mask probe")
    sc = scale32(d)
    e0 = torch.zeros(d, device=dev)
    e0[0] = 1.0
    for blk in range(nkb):
        K = zeros_k.clone()
        ks = kk[(kk // d) == blk]
        K[:, ks, :, ks % d] = 1.0
        got, keep = launch(be, c, dict(Q=zeros_q, K=K, V=zeros_k + e0, dO=zeros_q + e0, key_mask=None), seed, "%s: dQ draws, block %d" % (c.id, blk))
        assert torch.equal(probe, keep)
        delta = got["delta"].double()                                          # = O[q, 0] = (2 / n) * number of kept allowed keys
        x = got["dQ"].permute(0, 2, 1, 3)[..., ks % d].double()               # [B, nh, Lq, |ks|]
        lo, gap = (-(sc / n) * delta)[..., None], (2.0 * sc / n)[..., None]
        a = al[..., ks]
        rec_q[..., ks] = _decode_levels(torch.where(a, x - lo, torch.zeros_like(x)), gap, c.id + ": dQ draws")
        assert_all_zero(x[~a], c.id + ": dQ of keys the causal mask rules out")
    assert_same(rec_q, probe & al, c.id + ": the draws the query-owning backward applied vs the mask probe")


# ---------------------------------------------------------------------------------------------- G. a fully masked row
G_BOUND = 4 * 2.0 ** -10


def check_all_masked_row(be, c, seed=0, out=None):
    """Batch row 0: every key masked; the others partly.  With mask_neg = -10000 the additive term is the same for every key of
    the row and cancels: the reference (float64 softmax of s * scale + mask_neg) is the softmax of the raw scores.  The kernels
    form s * scale - 10000 in fp32, where one ulp is 2^-10: the score carries an absolute error of up to 2^-11 in forward's
    `val` and again in the backward's recomputation, each probability a relative error of about 2 * 2^-10 once the normalisation
    is counted, so O and LSE of that row are asserted within 4 * 2^-10 relative-to-max (fp32 mode; plus tol(bf16) in bf16 mode)
    and its gradients dQ, dK, dV -- the same probabilities, recomputed -- within 4 * 2^-10 plus the 4 * tol(dtype) the other rows'
    gradients get.  The other rows keep the ordinary tolerance.  First run on the MI355X, largest error over the cases of each
    kernel (fp32 / bf16): O 4.1e-4 / 4.2e-3, LSE 7e-8, dQ 7.3e-4 / 5.2e-3, dK 6.5e-4 / 4.9e-3, dV 8.1e-4 / 4.7e-3.  With mask_neg = -1e9 one ulp is 64 and rounding decides the result, in the
    reference too: every output is finite and the implied probabilities sum to 1 (O of a constant V is that constant)."""
    dev, dt = be.device, DT[c.dtype]
    assert c.B >= 2 and c.kv_group == 1
    gen = generator(4000 + seed, dev)
    km = make_mask(c, gen, dev)
    km[0] = 0
    inp = random_inputs(c, gen, dev, km)
    if c.neg < -1e8:
        inp["V"] = torch.full_like(inp["V"], 0.75)
        inp["dO"] = inp["dO"] * (inp["dO"].abs() > 0.6)
    got, keep = launch(be, c, inp, seed, c.id + ": a fully masked row")
    for nme, x in got.items():
        if x.dtype.is_floating_point:
            assert torch.isfinite(x.float()).all(), "%s: fully masked row: non-finite %s" % (c.id, nme)
    if c.neg < -1e8:
        if c.p == 0:
            assert_close(got["O"][0], torch.full_like(got["O"][0], 0.75, dtype=torch.float64), 2 * TOL[dt], c.id + ": masked row, constant V", out)
        return
    ref = reference(c, inp, keep)      # (under the causal mask too the term is added once: every key of row 0 carries it)
    row_tol = G_BOUND + (TOL[BF16] if dt == BF16 else 0.0)
    assert_close(got["O"][0], ref["O"][0], row_tol, c.id + ": masked row O", out)
    assert_close(got["LSE"][0], ref["LSE"][0], row_tol, c.id + ": masked row LSE", out)
    assert_close(got["O"][1:], ref["O"][1:], 2 * TOL[dt], c.id + ": other rows O", out)
    assert_close(got["LSE"][1:], ref["LSE"][1:], 2 * TOL[dt], c.id + ": other rows LSE", out)
    if c.has_bwd:
        for nme in ("dQ", "dK", "dV"):
            assert_close(got[nme][1:], ref[nme][1:], 4 * TOL[dt], "%s: other rows %s" % (c.id, nme), out)
            assert_close(got[nme][0], ref[nme][0], G_BOUND + 4 * TOL[dt], "%s: masked row %s" % (c.id, nme), out)


# ---------------------------------------------------------------------------------------------- exact sums
def unit_of(x):
    """The largest power of two of which every element of the float64 tensor is a multiple (1.0 for an all-zero tensor)."""
    nz = x[x != 0]
    if nz.numel() == 0:
        return 1.0
    m, e = torch.frexp(nz)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()                                                  # the lowest set bit of the 53-bit significand
    return float((torch.log2(low) + e.double() - 53).min().exp2())


def sum_is_exact(eq, a, b):
    """The fp32 sums einsum(eq, a, b) are exact in ANY order of additions: every term is a multiple of unit_of(a) * unit_of(b) and
    the sum of the terms' magnitudes -- which bounds every partial sum -- stays below 2^24 of these units."""
    peak = float(torch.einsum(eq, a.abs(), b.abs()).max())
    return peak < 2.0 ** 24 * unit_of(a) * unit_of(b)


def sums_are_exact(c, ref, inp):
    """sum_is_exact for the four products of one launch (O, dV, dQ, dK) from the float64 intermediates of reference()."""
    x = lambda n: inp[n].double().repeat_interleave(c.kv_group, 0) if n in ("K", "V") else inp[n].double()
    return (sum_is_exact("bhqk,bkhd->bqhd", ref["Pd"], x("V")) and sum_is_exact("bhqk,bqhd->bkhd", ref["Pd"], x("dO"))
            and sum_is_exact("bhqk,bkhd->bqhd", ref["dS"], x("K")) and sum_is_exact("bhqk,bqhd->bkhd", ref["dS"], x("Q")))


# ---------------------------------------------------------------------------------------------- H. uniform attention, dK != 0
H_SCALE = 2.0 ** -3


def disjoint_inputs(c, gen, dev):
    """The operands of family H: K in [-3, 3] on the columns [0, d / 2), Q in {-2, -1, 1, 2} on the columns [d / 2, d) -- every
    score is exactly 0 --, V in {-1, 0, 1}, dO = +-1 in one column per row."""
    Bkv, h = c.B // c.kv_group, c.d // 2
    K = integers((Bkv, c.Lk, c.nh, c.d), 3, gen, torch.float32, dev)
    K[..., h:] = 0
    Q = (torch.randint(0, 2, (c.B, c.Lq, c.nh, c.d), generator=gen, device=dev).float() * 2 - 1) * (1 + torch.randint(0, 2, (c.B, c.Lq, c.nh, c.d), generator=gen, device=dev).float())
    Q[..., :h] = 0
    V = integers((Bkv, c.Lk, c.nh, c.d), 1, gen, torch.float32, dev)
    col = torch.randint(0, c.d, (c.B, c.Lq, c.nh, 1), generator=gen, device=dev)
    dO = torch.zeros(c.B, c.Lq, c.nh, c.d, device=dev).scatter_(-1, col, torch.randint(0, 2, col.shape, generator=gen, device=dev).float() * 2 - 1)
    return dict(Q=Q, K=K, V=V, dO=dO)


def pow2_mask(c, gen, dev, seed):
    """check_uniform's key mask: a power-of-two number of allowed keys per row (None where Lk is one and the seed says so)."""
    pow2 = 1 << (c.Lk.bit_length() - 1)
    if pow2 == c.Lk and c.Lk > 1 and seed % 2:
        pow2 //= 2
    return make_mask(c, gen, dev, allowed=pow2) if (pow2 < c.Lk or seed % 3 == 0) else None


def disjoint_must_be_exact(c):
    """The mode check_uniform_dk MUST reach, from the table alone.  With the explicit scale 2^-3 no head size needs a rounding:
    wherever every query sees a power-of-two number of keys (no causal mask, or one query) fp32 is bit-exact at d = 32, 64 and
    128; bf16 without dropout and with n <= 128 keys too (uniform_must_be_exact's argument: V and dO are family D's, and the
    scale only moves the exponent of dS).  None: the data decide (bf16 with dropout or 256 keys) or the tolerance applies."""
    if not c.has_bwd or (c.causal and c.Lq > 1):
        return None
    return "exact" if c.dtype == "f32" or (c.p == 0 and c.Lk < 256) else None


def check_uniform_dk(be, c, seed=0, out=None):
    """Family D with Q and K on disjoint halves of the head dimension (disjoint_inputs) and the explicit scale 2^-3: every score
    is exactly 0 as with Q = 0, so P, O, LSE, dV and delta are check_uniform's, but dK = dS^T Q is nonzero in the Q columns (and
    dQ = dS K lives in the K columns).  Where every query sees a power-of-two number of keys, the bf16 operands formed on the
    device (P * fac, dS; and the stored O) are exact (guarded on the float64 intermediates) and every partial sum of the four
    products stays below 2^24 units (sums_are_exact), dQ, dK, dV and delta are bit-equal to the float64 reference at every head
    size; disjoint_must_be_exact() names the cases for which that MUST hold.  Elsewhere: 4 x TOL, as for D -- but dV and delta stay
    bit-equal wherever P * fac and O are exact (only dS carries the ninth bit).  Returns the mode."""
    dev, dt = be.device, DT[c.dtype]
    gen = generator(6000 + seed, dev)
    km = pow2_mask(c, gen, dev, seed)
    inp = dict(disjoint_inputs(c, gen, dev), key_mask=km)
    got, keep = launch(be, c, inp, seed, c.id + ": uniform, disjoint columns", scale=H_SCALE)
    ref = reference(c, inp, keep, scale=H_SCALE)
    assert_all_zero(torch.einsum("bqhd,bkhd->bhqk", inp["Q"], inp["K"].repeat_interleave(c.kv_group, 0)), c.id + ": disjoint scores")
    n = allowed_keys(c, km, dev).sum(-1)
    assert int(n.min()) >= 1
    all_pow2 = bool(((n & (n - 1)) == 0).all())
    # O as check_uniform asserts it: fl32(sum of the kept allowed V rows) * fl32(1 / n) -- the reference itself for n a power of two
    al = allowed_keys(c, km, dev)
    f = (keep.double() / (1.0 - c.p)) if keep is not None else torch.ones((), dtype=torch.float64, device=dev)
    ssum = torch.einsum("bhqk,bkhd->bqhd", (al.double() * f).expand(c.B, c.nh, c.Lq, c.Lk), inp["V"].double().repeat_interleave(c.kv_group, 0))
    want_O = (ssum.float() * (1.0 / n.float()).permute(0, 2, 1)[..., None]).double()
    if all_pow2:
        assert_bit_equal(got["O"], want_O, c.id + ": disjoint O")
        assert_bit_equal(got["O"], ref["O"], c.id + ": disjoint O")
    else:
        assert_within_one_ulp(got["O"], want_O, c.id + ": disjoint O")
    assert_close(got["LSE"], torch.log(n.double()).expand(c.B, c.nh, c.Lq), 2 * TOL[F32], c.id + ": disjoint LSE")
    if not c.has_bwd:
        return "forward"
    half = all_pow2 and sums_are_exact(c, ref, inp) and (dt == F32 or (fits(ref["Pd"], BF16) and fits(ref["O"], BF16)))
    exact = half and (dt == F32 or fits(ref["dS"], BF16))
    for nme in ("delta", "dV", "dQ", "dK"):
        if exact or (half and nme in ("delta", "dV")):                         # (P * fac and O exact: dV and delta are, whatever dS holds)
            assert_bit_equal(got[nme], ref[nme], "%s: disjoint %s" % (c.id, nme))
        elif nme != "delta":
            assert_close(got[nme], ref[nme], 4 * TOL[dt], "%s: disjoint %s" % (c.id, nme))
    if exact:
        assert int((got["dK"] != 0).sum()) > 0 or int(n.max()) < 4, c.id + ": the construction gave dK = 0"      # (one key: dP * fac - delta cancels)
    mode = "exact" if exact else "tol"
    must = disjoint_must_be_exact(c)
    assert must is None or mode == must, "%s: disjoint-column backward was checked as %r, the construction promises %r" % (c.id, mode, must)
    if out:
        out("%s: disjoint-column backward checked as %s" % (c.id, mode))
    return mode


# ---------------------------------------------------------------------------------------------- I. subset attention
I_SCALE = 2.0 ** -2


I_MIN_TIED = {False: 0.5, True: 0.25}     # by `causal`: the first 2^(t - j) <= seen / 2 rows of a causal case cannot reach a second member of a spread subset


def keys_in_sight(c):
    """The most keys a query of the case may see: Lk, or min(Lq, Lk) under the causal mask."""
    return min(c.Lq, c.Lk) if c.causal else c.Lk


def subset_params(c, seed):
    """(nb, j, kind, free, masked, reps) of check_subset for a case and seed, each dealt by a digit of its own: nb code bits, j in
    1..3 free bits, low or high, the bit positions `free` as a mask, a key mask or none, reps columns per bit (2 * nb * reps
    columns are used: code and bias).  High: the j bits just below 2^t, t = floor(log2(Lk)) -- the subsets of all keys below 2^t
    are whole whatever Lk is (the TOP bits of the code would give classes of 6 or 7 keys at Lk = 200); under the causal mask t
    comes from the keys the last query sees."""
    nb, t = max(1, (c.Lk - 1).bit_length()), keys_in_sight(c).bit_length() - 1
    j = min(1 + seed % 3, t)
    kind = ("low", "high")[(seed // 3) % 2]
    reps = c.d // (2 * nb)
    assert reps >= 1 and 512 * reps * I_SCALE >= 104
    return nb, j, kind, ((1 << j) - 1) << (0 if kind == "low" else t - j), (seed // 6) % 3 != 2, reps


def check_subset(be, c, seed=0, out=None):
    """Family C with ties.  K[k] = the +-16 binary code of k over nb bits x reps columns, then nb * reps bias columns of +16
    (signs flipped per (row, head, column) as in C).  Q[q] = the code of sel(q) with j bit positions zeroed -- the j low bits, or
    the j high bits, by the seed -- and -16 in the first (nb - j) * reps bias columns: Q . K[k] = -512 reps * (number of kept bits
    in which k differs from sel), so with the explicit scale 2^-2 the 2^j keys that agree with sel on the kept bits tie at a
    score of exactly 0 and every other key is at least 128 lower (asserted): exp underflows to an exact 0 there, P = 1 / count on
    the tied keys, LSE = log(count).  Low free bits: 2^j adjacent keys; high free bits (subset_params): keys 2^(t - j) apart,
    spread over the tiles, chunks and key-owning waves -- equal maxima meet across chunk borders.  The key mask (by the seed)
    takes whole subsets in or out.  sel(q) is drawn among the keys whose subset, as Lk, the key mask and the causal mask leave it
    to that query, holds 2, 4 or 8 keys; a query that draws another key (one time in ten, or where it has no such key: the
    first rows under the causal mask) points at it alone (j = 0 for that query, the whole code kept).  So every count IS a
    power of two and no case needs a tolerance, and at least half (a quarter under the causal mask) of the queries of every case that sees two keys hold a tie and its
    reference dK is nonzero (both asserted: a case without ties would be family C again).
    tolerance.  V in [-4, 4], dO = +-1 in two columns per row: O, delta, dP * fac - delta, dS and the four products are dyadic
    with at most 8 significant bits where bf16 holds them (guarded, with sums_are_exact) and O, delta, dV, dQ, dK are asserted
    bit for bit against the float64 reference formed from the exact P -- dK nonzero exactly on selected keys, 0 on the others
    and on masked keys.  p = 0.5 runs under the launch's own keep mask."""
    dev, dt = be.device, DT[c.dtype]
    gen = generator(7000 + seed, dev)
    nb, j, kind, free, masked, reps = subset_params(c, seed)                  # free: the bit positions a query leaves out
    kk = torch.arange(c.Lk, device=dev)
    Bkv = c.B // c.kv_group
    km = None
    if masked:                                                                 # whole subsets in or out: the mask is a function of k & ~free
        cls = kk & ~free
        on = torch.rand(Bkv, 1 << nb, generator=gen, device=dev) < 0.67
        on[:, 0] = True                                                        # key 0 stays (query 0 under the causal mask)
        km = on[:, cls].float()
    bit = torch.arange(nb, device=dev)
    code = torch.zeros(c.Lk, c.d, device=dev)
    code[:, :nb * reps] = (((kk[:, None] >> bit[None, :]) & 1) * 32.0 - 16.0).repeat_interleave(reps, 1)
    code[:, nb * reps:2 * nb * reps] = 16.0
    sign = torch.randint(0, 2, (Bkv, 1, c.nh, c.d), generator=gen, device=dev).float() * 2 - 1
    K = code[None, :, None, :] * sign
    al = allowed_keys(c, km, dev).expand(c.B, c.nh, c.Lq, c.Lk)
    # per (query, key): how many allowed keys share the key's class; sel is drawn among the keys whose subset is whole for that
    # query (2, 4 or 8 allowed members), ten times less often among the others -- every key can still be pointed at
    same = ((kk[:, None] & ~free) == (kk[None, :] & ~free)).float()            # [Lk, Lk]
    size = (al.float() @ same).long()                                          # [B, nh, Lq, Lk]
    good = al & (size > 1) & ((size & (size - 1)) == 0)
    sel = torch.multinomial((good.float() + 0.1 * (al & ~good).float()).reshape(-1, c.Lk), 1, generator=gen).view(c.B, c.nh, c.Lq)
    tied = al & ((kk[None, None, None, :] & ~free) == (sel[..., None] & ~free))
    cnt = tied.sum(-1)
    whole = (cnt & (cnt - 1)) == 0                                             # [B, nh, Lq]: the subset's count is a power of two
    member = torch.where(whole[..., None], tied, kk[None, None, None, :] == sel[..., None])
    cnt = member.sum(-1)
    colbit = torch.arange(nb * reps, device=dev) // reps                       # the bit a code column carries
    keepcol = torch.where(whole[..., None], ((torch.full_like(colbit, free) >> colbit) & 1) == 0, torch.ones_like(colbit, dtype=torch.bool))      # [B, nh, Lq, nb * reps]
    bidx = torch.arange(c.B, device=dev)[:, None, None]
    hidx = torch.arange(c.nh, device=dev)[None, :, None]
    Kx = K.repeat_interleave(c.kv_group, 0)
    Qh = Kx[bidx, sel, hidx].clone()                                           # [B, nh, Lq, d]
    Qh[..., :nb * reps] *= keepcol
    nkept = keepcol.sum(-1, keepdim=True)                                      # (nb - j) * reps, or nb * reps
    Qh[..., nb * reps:2 * nb * reps] *= -(torch.arange(nb * reps, device=dev) < nkept).float()
    Q = Qh.permute(0, 2, 1, 3).contiguous()
    V = integers((Bkv, c.Lk, c.nh, c.d), 4, gen, torch.float32, dev)
    col = torch.randint(0, c.d, (c.B, c.Lq, c.nh, 2), generator=gen, device=dev)
    dO = torch.zeros(c.B, c.Lq, c.nh, c.d, device=dev).scatter_(-1, col, torch.randint(0, 2, col.shape, generator=gen, device=dev).float() * 2 - 1)
    inp = dict(Q=Q, K=K, V=V, dO=dO, key_mask=km)
    # the premise, in float64 (every score is an exact integer multiple of 128): members at 0, everything else at least 104 lower
    s = torch.einsum("bqhd,bkhd->bhqk", Q.double(), Kx.double()) * I_SCALE
    assert bool((s[member] == 0).all()) and float(s[al & ~member].max() if bool((al & ~member).any()) else -1e9) <= -104, c.id + ": subset scores"
    assert float(s.max()) == 0.0 and float(s.min()) > max(c.neg, -10000.0) + 104      # a masked key stays below every allowed one
    share = float((cnt > 1).float().mean())
    assert share >= I_MIN_TIED[c.causal] or keys_in_sight(c) == 1, "%s: subset: only %.0f %% of the queries hold a tie" % (c.id, 100 * share)
    got, keep = launch(be, c, inp, seed, c.id + ": subset", scale=I_SCALE)
    ref = reference(c, inp, keep, scale=I_SCALE, P=member.double() / cnt[..., None].double())
    assert 1.0 / (1.0 - c.p) in (1.0, 2.0)
    assert_bit_equal(got["O"], ref["O"], c.id + ": subset O")
    assert_close(got["LSE"], torch.log(cnt.double()), 2 * TOL[F32], c.id + ": subset LSE")
    if out:
        out("%s: subset attention, %d %s bit(s) free, %.0f %% of the queries tied, counts %s" % (c.id, j, kind, 100 * share, sorted(set(cnt.reshape(-1).tolist()))))
    if not c.has_bwd:
        return "forward"
    assert sums_are_exact(c, ref, inp), c.id + ": subset: a partial sum may pass 2^24 units"
    assert dt == F32 or (fits(ref["Pd"], BF16) and fits(ref["O"], BF16) and fits(ref["dS"], BF16)), c.id + ": subset: a ninth bit in a bf16 operand"
    # (a handful of rows can cancel by chance: two tied keys with equal V in the dO columns, or both dropped)
    assert int((ref["dK"] != 0).sum()) > 0 or keys_in_sight(c) == 1 or c.B * c.nh * c.Lq < 16, c.id + ": the construction gave dK = 0"
    for nme in ("delta", "dV", "dQ", "dK"):
        assert_bit_equal(got[nme], ref[nme], "%s: subset %s" % (c.id, nme))
    picked = member.any(2)                                                    # [B, nh, Lk]: some query selected the key
    assert_all_zero(got["dK"].permute(0, 2, 1, 3)[~picked], c.id + ": subset dK of keys no query selected")
    assert_all_zero(got["dV"].permute(0, 2, 1, 3)[~picked], c.id + ": subset dV of keys no query selected")
    return "exact"


# ---------------------------------------------------------------------------------------------- J. graded ("tent") rows
J_SCALE, J_DELTA = 2.0 ** -3, 0.5
J_MASS = 1.0 / 16
J_NEAR, J_NOISE = 3, 16
# The largest err / B (B: the first-order rounding bound of check_tent) the ROUNDED stand-in of tests/test_exact_attn_harness_cpu.py
# reaches over J_CASES-like shapes on the CPU -- fp32 arithmetic, online softmax per update group, bf16 rounding of P * fac and
# dS -- per type and for {O, LSE} / {dQ, dK, dV}; J_K is the smallest power of two >= 2 x that (the factor 2: second-order terms
# and the hardware's __expf).  test_tent_factors_are_twice_what_the_rounded_standin_reaches re-measures them.
# Measured over the 83 cases tent_case() selects: O 1.82 / 0.13, LSE 0.03 / 0.03, dQ 1.73 / 0.08, dK 1.85 / 0.07, dV 1.77 / 0.13 (bf16 / fp32).
J_MEASURED = {("bf16", "fwd"): 1.82, ("bf16", "bwd"): 1.85, ("f32", "fwd"): 0.13, ("f32", "bwd"): 0.13}
J_K = {("bf16", "fwd"): 4.0, ("bf16", "bwd"): 4.0, ("f32", "fwd"): 0.5, ("f32", "bwd"): 0.5}


def update_group(c):
    """Keys per softmax update of attn_fwd_body: 64 for d <= 64, 32 for d = 128."""
    return 64 if c.d <= 64 else 32


def tent_case(c):
    """The cases of `RUNNABLE` family J runs on: the smallest shapes at which the rescale can go wrong (key counts around one,
    two, four update groups, every query count up to 256 the table pairs with them), the causal 100 x 200 and the production
    shapes."""
    if c.nh > 2 or (c.Lq, c.Lk) == (100, 200):
        return True
    return c.kv_group == 1 and c.Lk in ((65, 129, 256, 293) if c.d <= 64 else (37, 65, 256)) and c.Lq in (1, 17, 63, 64, 65, 100, 256)


def tent_borders(c):
    """The key indices at which a new softmax update group begins."""
    return list(range(update_group(c), c.Lk, update_group(c)))


def tent_must_straddle(c):
    """From the table alone: the case has an update border with J_NEAR keys on each side in sight of some query (tent_mask keeps
    those keys unmasked), so assert_tent_condition MUST find a border to check.  The others -- 65 keys at d <= 64 and the border
    at key 128 of 129 (ONE key beyond: 4.5 % of the mass at best), fewer keys than one update group, and the causal cases whose
    last query sees fewer than J_NEAR keys past the first border -- still run, with no border that counts."""
    return any(c.Lk - x >= J_NEAR and (not c.causal or c.Lq - x >= J_NEAR) for x in tent_borders(c))


def tent_mask(c, gen, dev):
    """make_mask with the J_NEAR keys on either side of every update border left unmasked: which borders can be straddled is
    then a property of the case, not of the draw."""
    km = make_mask(c, gen, dev)
    for x in tent_borders(c):
        km[:, x - J_NEAR:x + J_NEAR] = 1
    return km


def tent_reach(c, al):
    """[B, Lq, borders] bool: the row may see at least J_NEAR keys on each side of the border."""
    nal = torch.cumsum(al.expand(c.B, 1, c.Lq, c.Lk)[:, 0].long(), -1)
    nl = torch.stack([nal[..., x - 1] for x in tent_borders(c)], -1)
    return (nl >= J_NEAR) & (nal[..., -1:] - nl >= J_NEAR), nl, nal[..., -1:] - nl


def tent_inputs(c, gen, dev, km):
    """K[k] has a 1 in column tile(k) = k // 16; Q[q, t] = -(delta / scale) |t - peak(q)| for t < ntiles: the scaled score of key k
    is -delta * |tile(k) - peak(q)| plus the noise of the next J_NOISE columns ({-1, 0, 1} in Q and K; the rest 0, so that the
    noise has the same size at every head dimension), all exact integers times 2^-3.  peak(q) is dealt inside every 16-query
    tile: the rows that can straddle an update border (tent_reach) take, in turn, a tile next to each such border -- the left
    one, or the one on the side with fewer than 16 keys -- and the other rows go round-robin (rotated by the head) over the
    remaining tiles with a key the row may see.  So one wave holds rows whose maximum moves at a given update and rows whose
    maximum does not, and a short last tile still meets the borders."""
    nt = -(-c.Lk // 16)
    al = allowed_keys(c, km, dev)                                              # [B, 1, Lq, Lk]
    pad = torch.zeros(c.B, c.Lq, nt * 16 - c.Lk, dtype=torch.bool, device=dev)
    seen = torch.cat([al[:, 0], pad], -1).view(c.B, c.Lq, nt, 16).any(-1).cpu()      # [B, Lq, nt]: the tile has a key the row may see
    borders = tent_borders(c)
    if borders:
        reach, nl, nr = (x.cpu() for x in tent_reach(c, al))
    peak = torch.zeros(c.B, c.nh, c.Lq, dtype=torch.long)
    for b in range(c.B):
        rank = 0
        for q in range(c.Lq):
            rank = 0 if q % 16 == 0 else rank
            first = []
            for n, x in enumerate(borders):
                if reach[b, q, n]:
                    side = 1 if nr[b, q, n] < 16 and nr[b, q, n] <= nl[b, q, n] else 0
                    first.append(x // 16 - 1 + side)
            rest = [t for t in range(nt) if seen[b, q, t] and t not in first]
            for h in range(c.nh):
                peak[b, h, q] = first[rank] if rank < len(first) else rest[(q % 16 + h) % len(rest)] if rest else first[rank % len(first)]
            rank += 1 if first else 0
    peak = peak.to(dev)
    Bkv = c.B // c.kv_group
    Q = integers((c.B, c.Lq, c.nh, c.d), 1, gen, torch.float32, dev)
    K = integers((Bkv, c.Lk, c.nh, c.d), 1, gen, torch.float32, dev)
    Q[..., nt + J_NOISE:] = 0
    K[..., nt + J_NOISE:] = 0
    t = torch.arange(nt, device=dev)
    Q[..., :nt] = (-(J_DELTA / J_SCALE) * (t[None, None, None, :] - peak[..., None]).abs().float()).permute(0, 2, 1, 3)
    K[..., :nt] = (torch.arange(c.Lk, device=dev)[:, None] // 16 == t[None, :]).float()[None, :, None, :]
    V = integers((Bkv, c.Lk, c.nh, c.d), 4, gen, torch.float32, dev)
    dO = integers((c.B, c.Lq, c.nh, c.d), 3, gen, torch.float32, dev)
    return dict(Q=Q, K=K, V=V, dO=dO, key_mask=km)


def assert_tent_condition(c, P, al, name):
    """The condition of family J, in float64: every (batch row, head, 16-query tile) holds, for every border between two update
    groups, a row with at least 1 / 16 of its probability on each side.  Two things bound it.  A border COUNTS for a tile when
    every row of the tile that can straddle a border at all can straddle this one (tent_reach: J_NEAR = 3 keys in sight on each
    side; with ONE key beyond the border, as at 65 and 129 keys, that key holds 1 / (1 + 16 (e^-0.5 + e^-1 + ...)) = 4.5 % at
    best).  And a tile with fewer such rows than counting borders (one query against 293 keys) must straddle as many borders as
    it has rows.  For a full tile without the causal mask that is the condition as stated.  Returns the number of (batch row,
    tile, border) it required."""
    borders = tent_borders(c)
    if not borders:
        return 0
    cum = torch.cumsum(P, -1)                                                  # [B, nh, Lq, Lk]
    left = torch.stack([cum[..., x - 1] for x in borders], -1)                 # [B, nh, Lq, borders]: mass on the left
    hit = (left >= J_MASS) & (1 - left >= J_MASS)
    reach = tent_reach(c, al)[0]                                               # [B, Lq, borders]
    checked = 0
    for q0 in range(0, c.Lq, 16):
        rows = slice(q0, min(q0 + 16, c.Lq))
        r = reach[:, rows]
        can = r.any(-1)                                                        # [B, rows]
        counts = (r | ~can[..., None]).all(1) & can.any(1)[:, None]            # [B, borders]
        need = torch.minimum(can.sum(1), counts.sum(1))                        # [B]
        have = (hit[:, :, rows].any(2) & counts[:, None]).sum(-1)              # [B, nh]
        assert bool((have >= need[:, None]).all()), "%s: queries %d..%d: rows straddle %s of the counting borders, %s are required" % (
            name, rows.start, rows.stop - 1, have.tolist(), need.tolist())
        checked += int(need.sum())
    return checked


def tent_bounds(c, ref, inp, dtype, delta_term=True):
    """The first-order rounding bounds of check_tent, element by element, in float64."""
    if dtype == BF16:
        u = uo = 2.0 ** -9                                                     # one rounding of the MFMA operand formed on the device, one of the stored value
    else:
        u, uo = (max(c.Lq, c.Lk) + 8) * 2.0 ** -24, 2.0 ** -24                 # exact_attn_maps.check_integer_scores' form
    x = lambda n: (inp[n].double().repeat_interleave(c.kv_group, 0) if n in ("K", "V") else inp[n].double()).abs()
    Pd, dS = ref["Pd"].abs(), ref["dS"].abs()
    b = dict(O=u * torch.einsum("bhqk,bkhd->bqhd", Pd, x("V")) + uo * ref["O"].abs(),
             LSE=(c.Lk + 8) * 2.0 ** -23 * torch.clamp(ref["LSE"].abs(), min=1.0))
    if "dS" in ref:
        # delta = rowsum(dO * O) is an fp32 sum of d terms in both modes, and dP * fac - delta cancels: that error is relative to
        # sum |dO| |O|, not to |dS|, so it gets a term of its own (dP itself is exact: integer V and dO)
        ed = ((c.d + 8) * 2.0 ** -24 * torch.einsum("bqhd,bqhd->bhq", x("dO"), ref["O"].abs()))[..., None] * ref["P"] * ref["scale"] * float(delta_term)
        b.update(dV=u * torch.einsum("bhqk,bqhd->bkhd", Pd, x("dO")) + uo * ref["dV"].abs(),
                 dQ=torch.einsum("bhqk,bkhd->bqhd", u * dS + ed, x("K")) + uo * ref["dQ"].abs(),
                 dK=torch.einsum("bhqk,bqhd->bkhd", u * dS + ed, x("Q")) + uo * ref["dK"].abs())
    return b


def check_tent(be, c, seed=0, out=None, factors=None, delta_term=True):
    """Scores with a designed profile (tent_inputs): every row's running maximum moves by 0.5 per 16-key tile towards its peak
    and the rows of one 16-query tile peak at different tiles, so the online-softmax rescale of attn_fwd_body runs with factors
    strictly between 0 and 1 in some lanes of a wave and with 1 in others, on rows that keep a sixteenth of their mass on both
    sides of an update border (assert_tent_condition).  Every output is judged element by element against the float64 reference
    under the launch's own keep mask (delta from the O the launch stored): |got - ref| <= J_K x the first-order rounding bound
    of tent_bounds().  `factors`: other factors than J_K (the CPU harness measures with infinity); `delta_term`: tent_bounds
    without its term for delta (the CPU harness shows that a correct fp32 implementation fails then).  Returns the largest
    err / bound per output."""
    dev, dt = be.device, DT[c.dtype]
    gen = generator(8000 + seed, dev)
    km = tent_mask(c, gen, dev) if seed % 3 != 2 else None
    inp = tent_inputs(c, gen, dev, km)
    got, keep = launch(be, c, inp, seed, c.id + ": tent", scale=J_SCALE)
    ref = reference(c, inp, keep, scale=J_SCALE, O_stored=got["O"])
    checked = assert_tent_condition(c, ref["P"], allowed_keys(c, km, dev), c.id + ": tent")
    assert (checked > 0) == tent_must_straddle(c), "%s: tent: %d border(s) checked, the table says %r" % (c.id, checked, tent_must_straddle(c))
    bound = tent_bounds(c, ref, inp, dt, delta_term)
    k = J_K if factors is None else factors
    ratios, fail = {}, []
    for nme in ("O", "LSE") + (("dQ", "dK", "dV") if c.has_bwd else ()):
        g = got[nme].double()
        assert torch.isfinite(g).all(), "%s: tent %s: non-finite output" % (c.id, nme)
        r = ref[nme].reshape(g.shape)
        err, b = (g - r).abs(), bound[nme].reshape(g.shape)
        ratios[nme] = float(torch.where(b > 0, err / b, torch.where(err > 0, float("inf"), 0.0).to(err)).max())
        kk = k[(c.dtype, "fwd" if nme in ("O", "LSE") else "bwd")]
        if ratios[nme] > kk:
            i = tuple(int(x) for x in torch.nonzero((err > kk * b))[0])
            fail.append("%s: tent %s: error %.2f x the first-order bound (allowed %g x); first at %s: got %r want %r"
                        % (c.id, nme, ratios[nme], kk, i, g[i].item(), r[i].item()))
    if out:
        out("%s: tent (%d borders straddled) err / bound: %s" % (c.id, checked, ", ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not fail, "\n".join(fail)
    return ratios


# ---------------------------------------------------------------------------------------------- which cases run which layer
def first_per_kernel(cases, pred=lambda c: True, per=1):
    """The first `per` cases of `cases` for every (forward kernel, backward kernel, block order) that satisfy `pred`."""
    seen, r = collections.Counter(), []
    for c in cases:
        key = (c.fwd_kernel, c.bwd_kernel, c.bwd)
        if pred(c) and seen[key] < per:
            seen[key] += 1
            r.append(c)
    return r


def lib_path():
    return E.lib_path()
