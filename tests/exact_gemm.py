"""Exact layer of the GEMM tests: integer operands, write canaries, poisoned padding.

Operands are small integers, so every product, every partial sum in ANY order and every epilogue step is an integer (or an
integer / 8) far below 2^24: exactly representable in fp32 whatever the MFMA accumulation order, ring depth, split-K partition
or tile shape.  A float64 reference is therefore exact, an fp32 output must be BIT-equal to it and a bf16 output bit-equal to
its round-to-nearest-even image -- no tolerance to tune.  Every output is a window inside a larger allocation filled with a
fixed bit pattern (nothing outside the window may change); every input is a window inside an allocation whose surroundings are
NaN (anything read from outside an operand poisons the result and fails the exact comparison).  The surroundings belong to the
same allocation: nothing here reads or writes memory the process does not own.

Plain helper module: no fixtures, no hooks.  Allocator, reference and assertions take the device as a parameter, so
tests/test_exact_harness_cpu.py proves them on the CPU against a stand-in kernel written in torch.
"""
import collections
import os
import re

import torch

BF16, F32 = torch.bfloat16, torch.float32
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int64: torch.int64}
# canary bit patterns: finite, far from anything an integer GEMM produces, and not the image of one another's halves
# (int64: the attention keep-bit buffer of tests/exact_attn.py)
CANARY = {torch.bfloat16: 0x4B5A, torch.float32: 0x4B5A17C3, torch.int64: 0x4B5A17C32D693C87}
A_RANGE, E_RANGE = 3, 8                 # operands uniform in [-3, 3]; bias / addend in [-8, 8]
EXACT_LIMIT = 2 ** 24
SPLITK_COUNTER_BYTES = 4096             # counter area at the head of the split-K scratch (csrc/gemm_dma.hip: SPLITK_MAX_TILES * 4)


def generator(seed, device):
    return torch.Generator(device=torch.device(device)).manual_seed(int(seed))


def integers(shape, bound, gen, dtype, device):
    """Integer-valued tensor of `dtype`, uniform in [-bound, bound]."""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=gen, device=torch.device(device)).to(dtype)


class Window(object):
    """`batch` blocks of rows x cols elements, row stride `ld` >= cols, block stride `stride` >= rows * ld, inside ONE larger
    flat allocation: `guard` whole rows in front of the first and behind the last block, the pad columns cols..ld of every row
    and the gap between two blocks all hold `fill` -- "canary" (a fixed finite bit pattern: for outputs) or "poison" (NaN: for
    inputs).  The window base is 16-byte aligned, plus `misalign` elements when asked (the 4-byte aligned bias vector)."""

    def __init__(self, rows, cols, dtype, device, fill, ld=None, batch=1, stride=None, guard=2, misalign=0):
        assert fill in ("canary", "poison")
        self.rows, self.cols, self.dtype, self.fill, self.batch = rows, cols, dtype, fill, batch
        self.ld = cols if ld is None else ld
        self.stride = rows * self.ld if stride is None else stride
        assert self.ld >= cols and self.stride >= rows * self.ld
        unit = 16 // torch.empty((), dtype=dtype).element_size()
        pre = -(-max(guard * self.ld, 1) // unit) * unit
        self.offset = pre + misalign
        total = self.offset + (batch - 1) * self.stride + rows * self.ld + max(guard * self.ld, unit)
        self.flat = torch.empty(total, dtype=dtype, device=torch.device(device))
        if fill == "canary":
            self.flat.view(_INT[dtype]).fill_(CANARY[dtype])
        else:
            self.flat.fill_(float("nan"))
        assert self.flat.data_ptr() % 16 == 0
        self.view3 = torch.as_strided(self.flat, (batch, rows, cols), (self.stride, self.ld, 1), self.offset)
        self.view = self.view3[0] if batch == 1 else self.view3
        assert (self.view.data_ptr() - misalign * self.flat.element_size()) % 16 == 0
        inside = torch.zeros(total, dtype=torch.bool, device=self.flat.device)
        torch.as_strided(inside, (batch, rows, cols), (self.stride, self.ld, 1), self.offset).fill_(True)
        self.inside = inside

    def vector(self):
        """The window of a 1 x cols allocation as a 1-D tensor (bias, column sums)."""
        assert self.rows == 1 and self.batch == 1
        return self.view[0]

    def set(self, values):
        self.view3.copy_(values.reshape(self.batch, self.rows, self.cols))
        return self

    def assert_surroundings_untouched(self, name):
        """Everything outside the windows still holds the fill, bit for bit (compared as integers; NaN poison: still NaN)."""
        out = self.flat[~self.inside]
        if self.fill == "canary":
            bad = out.view(_INT[self.dtype]) != CANARY[self.dtype]
        else:
            bad = ~torch.isnan(out)
        n = int(bad.sum().item())
        if n:
            where = torch.nonzero(~self.inside).flatten()[bad][:8] - self.offset
            at = ["(block %d, row %d, col %d)" % (int(i) // self.stride if self.batch > 1 else 0,
                                                 (int(i) % self.stride if self.batch > 1 else int(i)) // self.ld,
                                                 (int(i) % self.stride if self.batch > 1 else int(i)) % self.ld) for i in where]
            raise AssertionError("%s: %d element(s) outside the %d x %d x %d window (ld %d) were written; first at %s"
                                 % (name, n, self.batch, self.rows, self.cols, self.ld, ", ".join(at)))


def reference(A, B, a_km, b_km, alpha=1.0, bias=None, addend=None, aux=None, mask=None):
    """float64 image of epi(alpha * A(m,k) B(n,k)) in the kernels' epilogue order -- alpha * acc, + bias, + addend, * aux
    (DGELU), * dropout factor -- and the largest magnitude any step of it reached (for the exact-range guard).  Operands may
    carry a leading batch dimension; a 2-D B is shared by the batch."""
    a, b = A.double(), B.double()
    a = a.transpose(-1, -2) if a_km else a
    b = b if b_km else b.transpose(-1, -2)
    r = a @ b
    peak = r.abs().max().item()
    r = r * alpha
    for term in (bias, addend):
        if term is not None:
            r = r + term.double()
            peak = max(peak, r.abs().max().item(), peak * abs(alpha))
    for factor in (aux, mask):
        if factor is not None:
            r = r * factor.double()
            peak = max(peak, r.abs().max().item())
    return r, max(peak, peak * abs(alpha))


def assert_exact_range(peak, name):
    """The case stays where fp32 arithmetic on its values is exact in any order; one that leaves it fails loudly instead of
    silently turning the bit comparison into a comparison of rounding orders."""
    assert peak * 2 < EXACT_LIMIT, "%s: magnitude %.0f leaves the exact range of fp32 (2^24 / 2)" % (name, peak)


def rne(ref, dtype):
    """The image of the float64 reference in the output type: exact in fp32, round to nearest even in bf16."""
    return ref.float().to(dtype)


def assert_bit_equal(got, ref, name):
    """`got` (the output window) equals the image of the exact reference bit for bit."""
    want = rne(ref, got.dtype).reshape(got.shape)
    gi, wi = got.contiguous().view(_INT[got.dtype]), want.contiguous().view(_INT[got.dtype])
    bad = gi != wi
    n = int(bad.sum().item())
    if n == 0:
        return
    idx = torch.nonzero(bad)[:6]
    shown = ["%s: got %r want %r (exact %r)" % (tuple(int(x) for x in i), got[tuple(i)].item(), want[tuple(i)].item(),
                                                ref.reshape(got.shape)[tuple(i)].item()) for i in idx]
    # a finding about rounding looks different from an arithmetic error: say which one this is
    r32 = ref.reshape(got.shape).float()
    tie = (r32.view(torch.int32) & 0xFFFF) == 0x8000 if got.dtype == torch.bfloat16 else torch.zeros_like(bad)
    kind = "all at exact bf16 ties" if bool(tie[bad].all()) and got.dtype == torch.bfloat16 else "not only at bf16 ties"
    raise AssertionError("%s: %d of %d elements differ from the exact reference (%s, %d NaN); %s"
                         % (name, n, bad.numel(), kind, int(torch.isnan(got.float()).sum().item()), "; ".join(shown)))


def assert_counters_zero(scratch, name):
    """The arrival counters at the head of a split-K scratch are zero again after the launch."""
    cnt = scratch[:SPLITK_COUNTER_BYTES].view(torch.int32)
    n = int((cnt != 0).sum().item())
    assert n == 0, "%s: %d split-K counter(s) left non-zero (first: tile %d)" % (name, n, int(torch.nonzero(cnt)[0]) if n else -1)


def assert_close_rel_to_max(got, ref, tol, name):
    """The tolerance metric of tests/test_ops_gpu.py (GELU cases only: erf is not exact arithmetic)."""
    got, ref = got.float(), ref.float().reshape(got.shape)
    assert torch.isfinite(got).all(), name + ": non-finite output"
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item() / scale
    assert err <= tol, "%s: rel-to-max error %.3e (scale %.3e, tol %.1e)" % (name, err, scale, tol)


# ---------------------------------------------------------------------------------------------- the case table
LAYOUTS = {"nt": (False, False), "nn": (False, True), "tn": (True, True), "tt": (True, False)}      # (a_kmajor, b_kmajor)
_OT = {"bf16": "DF16b", "f32": "f"}      # Itanium mangling of the output type in a kernel's template arguments


def _lb(lay):
    a, b = LAYOUTS[lay]
    return "Lb%dELb%dE" % (a, b)


# Substring of the mangled symbol a case of a route must launch, from what the case fixes (output type, layout) -- NOT from the
# dispatch's thresholds: when those move, the case's shape lands on another kernel and the census assertion fails.
ROUTES = {
    "gemv4":   lambda c: "gemv16_kernelILi4ELb%dE" % (c.out == "f32"),
    "gemv8":   lambda c: "gemv16_kernelILi8ELb%dE" % (c.out == "f32"),
    "nt64_4":  lambda c: "gemm_pc256_nt64_kernelI%sLi4E" % _OT[c.out],
    "nt64_3":  lambda c: "gemm_pc256_nt64_kernelI%sLi3E" % _OT[c.out],
    "pc256_4": lambda c: "gemm_pc256_kernelI%s%sLi4E" % (_OT[c.out], _lb(c.lay)),
    "pc256_3": lambda c: "gemm_pc256_kernelI%s%sLi3E" % (_OT[c.out], _lb(c.lay)),
    "dma256_4": lambda c: "gemm_dma256_kernelI%s%sLi4E" % (_OT[c.out], _lb(c.lay)),
    "dma256_3": lambda c: "gemm_dma256_kernelI%s%sLi3E" % (_OT[c.out], _lb(c.lay)),
    "dma128":  lambda c: "gemm_dma_kernelI%sLi128ELi128ELi2ELi4E%sLi3ELi0E" % (_OT[c.out], _lb(c.lay)),
    "dma96":   lambda c: "gemm_dma_kernelI%sLi128ELi128ELi4ELi2E%sLi3ELi3E" % (_OT[c.out], _lb(c.lay)),
    "dma64":   lambda c: "gemm_dma_kernelI%sLi64ELi64ELi2ELi2E%sLi3ELi0E" % (_OT[c.out], _lb(c.lay)),
    "splitk":  lambda c: "gemm_dma_splitk_kernelI%sLi64ELi64ELi2ELi2E%sLi8E" % (_OT[c.out], _lb(c.lay)),
    "f32_128": lambda c: "gemm_kernelIffLi128ELi128ELi2ELi2E%s" % _lb(c.lay),
    "f32_64":  lambda c: "gemm_kernelIffLi64ELi64ELi2ELi2E%s" % _lb(c.lay),
}

_Case = collections.namedtuple("Case", "route M N K lay out inp batch pad ldc_odd bias add alpha epi drop shared_b splits")


class Case(_Case):
    """One launch through ops.gemm.  pad: extra elements on (lda, ldb, ldc / ldadd / ldaux); ldc_odd: ldc % 8 == 4 (the tile-wise
    epilogue of the bf16 kernels); bias: None, "a" (16-byte aligned) or "u" (4-byte aligned only); epi: None, "dgelu" or "gelu";
    splits: the split count ops.splitk_plan must choose (split-K route only)."""
    __slots__ = ()

    @property
    def kernel(self):
        return ROUTES[self.route](self)

    @property
    def id(self):
        s = "%s-%s-%dx%dx%d-%s" % (self.route, self.lay, self.M, self.N, self.K, self.out)
        if self.inp != "bf16": s += "-in" + self.inp
        if self.batch > 1: s += "-b%d%s" % (self.batch, "s" if self.shared_b else "")
        if any(self.pad): s += "-pad%d.%d.%d" % self.pad
        if self.ldc_odd: s += "-ldc4"
        if self.bias: s += "-bias" + self.bias
        if self.add: s += "-add"
        if self.alpha != 1.0: s += "-alpha%g" % self.alpha
        if self.epi: s += "-" + self.epi
        if self.drop: s += "-drop"
        return s


def case(route, M, N, K, lay="nt", out="bf16", inp="bf16", batch=1, pad=(0, 0, 0), ldc_odd=False, bias=None, add=False, alpha=1.0,
         epi=None, drop=False, shared_b=False, splits=None):
    return Case(route, M, N, K, lay, out, inp, batch, tuple(pad), ldc_odd, bias, add, alpha, epi, drop, shared_b, splits)


def conditions(route, M, N, K, lays, batched=True, fused=True, n4=None, bshape=None, **kw):
    """The conditions every route is run under, dealt round-robin over the route's layouts `lays`: tile-wise epilogue
    (ldc % 8 != 0), a bias that is only 4-byte aligned, N % 8 == 4 (shape `n4`; row-major B only), padded leading dimensions,
    batches with guard gaps, each epilogue term alone and all together, GELU (tolerance; canaries on C and aux).  The N % 8 == 4
    shapes come with ldc % 8 == 0 (pad 4 / 12: the row-wise epilogue's 16-byte stores could pass N) and with ldc % 8 == 4.
    fused=False: the route has no DGELU / dropout epilogue (the skinny kernel); bshape: (M, N) of the batched variants, where the
    route's grid range needs another shape once the batch multiplies the tiles."""
    f32in = kw.get("inp") == "f32"
    out = kw.pop("out", "bf16")
    variants = [dict(), dict(ldc_odd=True, bias="a", add=True), dict(bias="u"), dict(pad=(8, 16, 24), bias="a", add=True),
                dict(bias="a"), dict(add=True), dict(alpha=2.0), dict(alpha=0.125, bias="a")]
    if not f32in:
        variants.append(dict(out="f32", add=True))
    if fused:
        variants += [dict(epi="dgelu"), dict(drop=True),
                     dict(bias="u", add=True, alpha=0.125, epi="dgelu", drop=True, out="f32", pad=(8, 8, 8)),
                     dict(bias="a", add=True, alpha=2.0, epi="dgelu", drop=True, pad=(0, 0, 8))]
    else:
        variants.append(dict(bias="u", add=True, alpha=0.125, out="f32", pad=(8, 8, 8)))
    variants.append(dict(epi="gelu", bias="a", alpha=0.125, pad=(0, 0, 8)))
    if batched:
        nb = 3 if batched is True else batched
        variants += [dict(batch=nb, bias="a", pad=(8, 0, 8)), dict(batch=nb, shared_b=True, add=True, drop=fused)]
    cases = []
    for i, v in enumerate(variants):
        v = dict(kw, **v)
        v.setdefault("out", out)
        m, n = (M, N) if v.get("batch", 1) == 1 or bshape is None else bshape
        cases.append(case(route, m, n, K, lay=lays[i % len(lays)], **v))
    if n4 is not None:
        rm = [l for l in lays if not LAYOUTS[l][1]] if not f32in else list(lays)
        m4, nn4, k4 = n4
        for j, v in enumerate([dict(pad=(0, 0, 4), bias="a", add=True), dict(ldc_odd=True, bias="u"),
                               dict(pad=(0, 0, 12), epi="dgelu" if fused else None)]):
            v = dict(kw, **v)
            v.setdefault("out", out)
            cases.append(case(route, m4, nn4, k4, lay=rm[j % len(rm)], **v))
    return cases


def build_cases():
    """One group per route of the dispatch (csrc/gemm.hip, gemm_dma.hip, gemm_dma256.hip, gemv.hip, ops.splitk_plan), each at the
    M / N / K edges of ITS tile, then under conditions()."""
    c = []
    # -- gemv16_kernel<4> / <8>: M <= 16, NT, no DGELU / dropout; K >= 2048 picks <8>; one workgroup per 16 columns, K steps of 32
    for out in ("bf16", "f32"):
        for M, N, K in [(1, 16, 8), (3, 36, 2040), (16, 72, 1024), (16, 260, 40)]:
            c.append(case("gemv4", M, N, K, out=out, bias="a"))
        for M, N, K in [(1, 20, 2048), (3, 64, 3072), (16, 136, 2056)]:
            c.append(case("gemv8", M, N, K, out=out, add=True))
    c += conditions("gemv4", 16, 264, 200, ["nt"], batched=False, fused=False, n4=(3, 132, 72))
    c += conditions("gemv8", 7, 96, 3072, ["nt"], batched=False, fused=False, n4=(16, 20, 2048))
    # -- gemm_pc256_nt64_kernel: NT, M, N >= 256, 120..512 tiles, K % 64 == 0, K >= 128.  pick_niu: 192-wide tiles when they need
    #    no more rounds of 256 CUs (2816 x 3072: 11 x 16 = 176 tiles against 132), 256-wide when the narrower tiles would spill
    #    into a second round (3584 x 3584: 14 x 14 = 196 tiles against 14 x 19 = 266)
    for out in ("bf16", "f32"):
        c += [case("nt64_3", 2816, 3072, 128, out=out, bias="a"), case("nt64_4", 3584, 3584, 128, out=out, bias="a"),
              case("nt64_3", 2824, 3064, 192, out=out, add=True), case("nt64_4", 3576, 3592, 256, out=out, add=True)]
    c += conditions("nt64_3", 3000, 2824, 128, ["nt"], n4=(2816, 3076, 128), bshape=(1024, 1288), batched=6)
    c += conditions("nt64_4", 3592, 3576, 192, ["nt"], n4=(3584, 3588, 128), bshape=(1024, 1784), batched=7)
    # -- gemm_pc256_kernel: same grid range, K % 64 != 0 or K < 128 (NT), or a k-major operand (NN, TN); 32-deep K steps
    for out in ("bf16", "f32"):
        for lay in ("nt", "nn", "tn"):
            c += [case("pc256_3", 2816, 3072, 72, lay=lay, out=out, bias="a"), case("pc256_4", 3584, 3584, 104, lay=lay, out=out, add=True)]
    c += [case("pc256_3", 2824, 3064, 8, lay="nt"), case("pc256_4", 3576, 3592, 32, lay="nn"), case("pc256_3", 2808, 3080, 24, lay="tn"),
          case("pc256_4", 3592, 3584, 64, lay="nt"), case("pc256_3", 2816, 3072, 136, lay="nn"), case("pc256_4", 3584, 3576, 160, lay="tn")]
    c += conditions("pc256_3", 3000, 2824, 72, ["nt", "nn", "tn"], n4=(2816, 3076, 104), bshape=(1024, 1288), batched=6)
    c += conditions("pc256_4", 3592, 3576, 40, ["nn", "tn", "nt"], n4=(3584, 3588, 8), bshape=(1024, 1784), batched=7)
    # -- gemm_dma256_kernel: more than 512 tiles (the expensive shapes: K kept small, one case per layout, width and output type)
    for out in ("bf16", "f32"):
        for i, lay in enumerate(("nt", "nn", "tn")):
            c += [case("dma256_4", 6144, 6400, 64 + 8 * i, lay=lay, out=out, bias="au"[i % 2], add=(out == "bf16")),
                  case("dma256_3", 8192, 4224, 72 + 8 * i, lay=lay, out=out, add=(i == 1), epi="dgelu" if i == 2 else None)]
    c += [case("dma256_4", 6152, 6404, 72, lay="nt", ldc_odd=True, bias="u", drop=True),
          case("dma256_3", 8184, 4220, 104, lay="nt", pad=(8, 8, 4), bias="a", add=True, alpha=0.125, epi="dgelu", drop=True),
          case("dma256_4", 2056, 2816, 64, lay="nn", batch=6, pad=(8, 8, 8), add=True),
          case("dma256_4", 6144, 6392, 64, lay="tn", pad=(0, 0, 8), epi="gelu", bias="a", alpha=0.125)]
    # -- gemm_dma_kernel 128 x 128 and 128 x 96: M >= 256, N >= 128, >= 96 tiles of 128, below the 256-tile threshold; 96-wide
    #    whenever that needs no more rounds of 256 CUs (2048 x 768: 128 tiles against 96), 128-wide when it would (1536 x 2048:
    #    192 tiles against 264); all four layouts (a k-major A with a row-major B never takes another kernel)
    for out in ("bf16", "f32"):
        for lay in ("nt", "nn", "tn", "tt"):
            c += [case("dma128", 1536, 2048, 64, lay=lay, out=out, bias="a"), case("dma96", 2048, 768, 72, lay=lay, out=out, add=True)]
    c += [case("dma128", 1528, 2056, 8, lay="nt"), case("dma96", 2040, 760, 200, lay="nn"), case("dma128", 1544, 2040, 136, lay="tt"),
          case("dma96", 1928, 776, 64, lay="tn")]
    c += conditions("dma128", 1500, 2040, 72, ["nt", "nn", "tn", "tt"], n4=(1530, 2052, 64), bshape=(760, 1664))
    c += conditions("dma96", 2000, 760, 104, ["tt", "nt", "nn", "tn"], n4=(1930, 764, 72), bshape=(760, 768))
    # -- gemm_dma_kernel 64 x 64: everything smaller
    for out in ("bf16", "f32"):
        for lay in ("nt", "nn", "tn", "tt"):
            c += [case("dma64", 64, 64, 64, lay=lay, out=out, bias="a"), case("dma64", 72, 136, 200, lay=lay, out=out, add=True)]
    for M in (8, 60, 64, 68):
        for N in (4, 60, 64, 68):
            # (M <= 16 in the NT layout is the skinny kernel's unless the epilogue carries dropout)
            c.append(case("dma64", M, N, {4: 8, 60: 64, 64: 72, 68: 200}[N], lay="nt", bias="a", drop=(M == 8)))
    c += [case("dma64", 8, 8, 8, lay="tn"), case("dma64", 56, 72, 72, lay="nn"), case("dma64", 64, 64, 200, lay="tt"), case("dma64", 72, 56, 8, lay="tt")]
    c += conditions("dma64", 200, 136, 72, ["nt", "nn", "tn", "tt"], n4=(37, 132, 200))
    # -- gemm_dma_splitk_kernel: ops.splitk_plan > 1 (few 64-tiles, >= 10 K-tiles per split); splits 2..8; a short last split and
    #    K % 64 != 0 (1992 = 31 K-tiles + 8); N % 8 == 4
    for out in ("bf16", "f32"):
        for lay in ("nt", "nn", "tn"):
            c.append(case("splitk", 72, 136, 1992, lay=lay, out=out, bias="a", add=True, splits=3))
    c += [case("splitk", 400, 768, 1280, lay="nt", splits=2), case("splitk", 128, 512, 3072, lay="nn", splits=4),
          case("splitk", 64, 256, 3072, lay="tn", splits=4), case("splitk", 200, 64, 3072, lay="nt", splits=4),
          case("splitk", 40, 64, 3072, lay="nn", splits=4), case("splitk", 64, 128, 3008, lay="nt", splits=4),
          case("splitk", 100, 192, 2048, lay="nt", splits=3), case("splitk", 64, 64, 3072, lay="tn", out="f32", splits=4),
          case("splitk", 128, 136, 3072, lay="nn", splits=4), case("splitk", 17, 64, 2568, lay="nt", splits=4),
          case("splitk", 24, 64, 3072, lay="nt", splits=4), case("splitk", 16, 72, 3072, lay="nn", splits=4)]
    c += [case("splitk", 64, 64, 64 * n, lay="nt", splits=s) for n, s in ((20, 2), (30, 3), (48, 4))]
    c += [case("splitk", 24, 8, 8 * k, lay="tn", bias="a", splits=s) for k, s in ((375, 4), (384, 4))]
    c += conditions("splitk", 200, 136, 1992, ["nt", "nn", "tn"], batched=False, n4=(37, 132, 1992), splits=3)
    # -- gemm_kernel: fp32 in and out, 128 x 128 (M >= 256, N >= 128, >= 96 tiles of 128) and 64 x 64, four layouts, 32-deep K tiles
    for lay in ("nt", "nn", "tn", "tt"):
        c += [case("f32_128", 1536, 1024, 68, lay=lay, inp="f32", out="f32", bias="a"), case("f32_64", 72, 132, 200, lay=lay, inp="f32", out="f32", add=True),
              case("f32_64", 64, 64, 4, lay=lay, inp="f32", out="f32"), case("f32_128", 1532, 1028, 4, lay=lay, inp="f32", out="f32")]
    c += conditions("f32_128", 1500, 1020, 36, ["nt", "nn", "tn", "tt"], n4=(1532, 1028, 68), inp="f32", out="f32")
    c += conditions("f32_64", 60, 68, 200, ["tt", "nt", "nn", "tn"], n4=(36, 132, 68), inp="f32", out="f32")
    return [normalise(x) for x in c]


def normalise(c):
    """k-major operands are read in 16-byte units along M / N (the ABI's M % ve, N % ve rule): round a k-major extent up."""
    ve = 4 if c.inp == "f32" else 8
    a_km, b_km = LAYOUTS[c.lay]
    M = -(-c.M // ve) * ve if a_km else c.M
    N = -(-c.N // ve) * ve if b_km else c.N
    return c._replace(M=M, N=N)


CASES = build_cases()


def route_counts(cases=None):
    n = collections.OrderedDict()
    for c in (CASES if cases is None else cases):
        n[c.route] = n.get(c.route, 0) + 1
    return n


# ---------------------------------------------------------------------------------------------- running one case
class Problem(object):
    """The windows of one case: poisoned inputs (A, B, bias, addend, DGELU's aux), canary outputs (C, GELU's aux)."""

    def __init__(self, c, seed, device):
        self.c, self.device = c, device
        gen = generator(seed, device)
        it, ot = (F32 if c.inp == "f32" else BF16), (F32 if c.out == "f32" else BF16)
        a_km, b_km = LAYOUTS[c.lay]
        pa, pb, pc = c.pad
        if c.ldc_odd:
            pc = pc - pc % 8 + 4 + (0 if c.N % 8 == 0 else 4)          # ldc % 8 == 4
        Bn, M, N, K = c.batch, c.M, c.N, c.K

        def win(rows, cols, dtype, fill, pad, batch=Bn, gap=0, **kw):
            ld = cols + pad
            return Window(rows, cols, dtype, device, fill, ld=ld, batch=batch, stride=(rows + gap) * ld if batch > 1 else None, **kw)
        ar, ac = (K, M) if a_km else (M, K)
        br, bc = (K, N) if b_km else (N, K)
        self.A = win(ar, ac, it, "poison", pa, gap=1).set(integers((Bn, ar, ac), A_RANGE, gen, it, device))
        nb = 1 if c.shared_b else Bn
        self.B = win(br, bc, it, "poison", pb, batch=nb, gap=2).set(integers((nb, br, bc), A_RANGE, gen, it, device))
        self.C = win(M, N, ot, "canary", pc, gap=3)
        self.bias = self.add = self.aux = None
        if c.bias:
            self.bias = Window(1, N, F32, device, "poison", misalign=1 if c.bias == "u" else 0).set(integers((N,), E_RANGE, gen, F32, device))
        if c.add:                                   # the addend has the OUTPUT's type
            self.add = win(M, N, ot, "poison", pc, gap=2).set(integers((Bn, M, N), E_RANGE, gen, ot, device))
        if c.epi == "dgelu":                        # the multiplier has the INPUT's type
            self.aux = win(M, N, it, "poison", pc, gap=1).set(integers((Bn, M, N), 2, gen, it, device))
        elif c.epi == "gelu":
            self.aux = win(M, N, it, "canary", pc, gap=1)

    def gemm_kwargs(self):
        """Keyword arguments of ops.gemm for this problem (positional: A, B, C, M, N, K)."""
        c = self.c
        a_km, b_km = LAYOUTS[c.lay]
        kw = dict(a_km=a_km, b_km=b_km, alpha=c.alpha, lda=self.A.ld, ldb=self.B.ld, ldc=self.C.ld)
        if self.bias is not None:
            kw["bias"] = self.bias.vector()
        if self.add is not None:
            kw.update(addend=self.add.view, ldadd=self.add.ld)
        if self.aux is not None:
            kw.update(aux=self.aux.view, ldaux=self.aux.ld)
        if c.batch > 1:
            kw.update(batch=c.batch, sA=self.A.stride, sB=0 if c.shared_b else self.B.stride, sC=self.C.stride,
                      sAdd=self.add.stride if self.add is not None else 0, sAux=self.aux.stride if self.aux is not None else 0)
        return kw

    def expected(self, mask=None):
        """(float64 reference of the window, peak magnitude); `mask`: the dropout factors (0 or 2) the launch applied.
        GELU cases: the pre-activation (the caller applies gelu and its tolerance)."""
        c = self.c
        B = self.B.view if not c.shared_b or c.batch == 1 else self.B.view3[0]
        return reference(self.A.view, B, *LAYOUTS[c.lay], alpha=c.alpha, bias=self.bias.vector() if self.bias is not None else None,
                         addend=self.add.view if self.add is not None else None,
                         aux=self.aux.view if c.epi == "dgelu" else None, mask=mask)

    def assert_surroundings(self, name):
        for tag, w in (("C", self.C), ("A", self.A), ("B", self.B), ("bias", self.bias), ("addend", self.add), ("aux", self.aux)):
            if w is not None:
                w.assert_surroundings_untouched("%s: %s" % (name, tag))


# ---------------------------------------------------------------------------------------------- census of the built library
KERNEL_RE = re.compile(rb"_Z\d+(?:gemm_\w*kernel|gemv16\w*kernel)\w*")


def library_kernels(lib_path, pattern):
    """Mangled names of every kernel instantiation of the built library that the (bytes) regular expression matches."""
    with open(lib_path, "rb") as f:
        blob = f.read()
    return sorted(set(m.decode() for m in pattern.findall(blob)))


def library_gemm_kernels(lib_path):
    """Mangled names of every GEMM kernel instantiation the built library carries."""
    return library_kernels(lib_path, KERNEL_RE)


def lib_path():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(root, "gst_visdial_amd", "lib", "libgstvd_hip.so")
