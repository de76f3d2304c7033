"""The exact layer of the LayerNorm tests proves itself on the CPU (tests/exact_ln.py): the whole harness runs
against a stand-in of the kernels written in torch (all three modes, both directions, the reductions), and against deliberately
wrong stand-ins, each of which must fail the check meant for it.  Nothing here touches a GPU."""
import pytest
import torch

import exact_ln as X
from exact_gemm import BF16, F32

CPU = torch.device("cpu")


def _raw(t, rows, cols, ld, extra=0):
    """[rows, cols] elements from the first element of view `t` on, row stride ld -- pointer semantics, as a kernel sees it."""
    return torch.as_strided(t, (rows, cols), (ld, 1), t.storage_offset() + extra)


class Torch(object):
    """fp32 stand-in of ops.ln_fwd / ln_bwd / colsum* / ColsumBatch / locgrad with the kernels' block geometry.  `defect`: one
    planted error (see DEFECTS)."""

    def __init__(self, defect=None):
        self.device, self.defect = CPU, defect

    def keep(self, n, p, site):
        g = torch.Generator().manual_seed(7919 * site + 1)
        return (torch.rand(n, generator=g) >= p).float() / (1.0 - p)

    def blocks(self, M, H=None, mode=None):
        rw = 1 if M <= 8192 else 2
        if H is not None and M >= 2048 and mode != "embed" and H <= 768 and rw == 1:
            return (M + 15) // 16
        return (M + 4 * rw - 1) // (4 * rw)

    # -- LayerNorm
    def _keeps(self, kw):
        M, H = kw["M"], kw["H"]
        one = torch.ones(M, H)
        pre = self.keep(M * H, kw["p_pre"], kw["site_pre"]).view(M, H) if kw["p_pre"] > 0 and kw["mode"] == "resid" else one
        post = self.keep(M * H, kw["p_post"], kw["site_post"]).view(M, H) if kw["p_post"] > 0 else one
        return pre, post

    def _h(self, kw, pre):
        M, H, mode = kw["M"], kw["H"], kw["mode"]
        if mode == "embed":
            rows = torch.arange(M)
            tpos = rows % kw["T"] + (0 if self.defect == "pos_offset" else kw["pos_offset"])
            seg = kw["segs"] if kw["segs"] is not None else torch.zeros(M, dtype=torch.int64)
            tv = kw["type_vocab"]
            in_tt = seg < tv
            ext = kw["tt_ext"][(seg - tv).clamp(min=0)]
            if self.defect == "seg_from_tt":
                in_tt = torch.ones_like(in_tt)
            typ = torch.where(in_tt[:, None], kw["tt"][seg.clamp(max=tv - 1)], ext)
            return kw["word"][kw["ids"]] + kw["pos"][tpos] + typ
        x = kw["x"]
        if self.defect == "pad_read":                       # the last column comes from the first pad column
            wide = _raw(x, M, H + 1, x.stride(0) if M > 1 else H + 4)
            x = torch.cat([wide[:, :H - 1], wide[:, H:]], 1)
        x = x.float()
        if mode == "resid":
            h = x * pre
            return h + kw["res"].float() if kw["res"] is not None else h
        return x + (kw["loc"] @ kw["w_loc"].t() + kw["b_loc"])

    def _store(self, dst, val):
        if dst.dtype == BF16 and self.defect == "truncate":
            val = (val.contiguous().view(torch.int32) & -65536).view(torch.float32)
        dst.copy_(val)

    def ln_fwd(self, kw, expect=None):
        M, H = kw["M"], kw["H"]
        assert M > 0 and H > 0 and H % 4 == 0 and H <= 2048
        pre, post = self._keeps(kw)
        h = self._h(kw, pre)
        s = h[:, :H - 4].sum(1, keepdim=True) if self.defect == "rowsum" else h.sum(1, keepdim=True)
        mean = s / H
        var = ((h - mean) ** 2).sum(1, keepdim=True) / H
        rstd = 1.0 / torch.sqrt(var + (1e-3 if self.defect == "eps" else kw["eps"]))
        kw["mean"].copy_(mean[:, 0]), kw["rstd"].copy_(rstd[:, 0])
        y = (kw["gamma"] * ((h - mean) * rstd) + kw["beta"]) * post
        self._store(kw["y"], y)
        if self.defect == "tail":
            ld = kw["y"].stride(0) if M > 1 else H
            _raw(kw["y"], 1, 1, 1, M * ld).fill_(1.0)

    def ln_bwd(self, kw, bw, expect=None):
        M, H, mode = kw["M"], kw["H"], kw["mode"]
        pre, post = self._keeps(kw)
        h = self._h(kw, pre)
        rstd = kw["rstd"][:, None]
        xh = (h - kw["mean"][:, None]) * rstd
        dyv = bw["dy"].float() * post
        gy = dyv * kw["gamma"]
        c1 = gy.sum(1, keepdim=True) / H
        c2 = (gy * xh).sum(1, keepdim=True) / H
        if self.defect == "c1":
            c1 = c1 * 0
        dh = (gy - c1 - xh * c2) * rstd
        narrow, wide = self.blocks(M), self.blocks(M, H, mode)
        nblk = bw["nblk"] or narrow
        assert nblk in (narrow, wide), "GSTVD_E_SHAPE"
        rpb = 16 if (nblk == wide and wide != narrow) else 4 * (1 if M <= 8192 else 2)
        vecs = [dyv * xh, dyv]
        if mode == "resid":
            dx = dh * pre
            if bw.get("dres") is not None:
                self._store(bw["dres"], dh)
            if bw.get("dx") is not None and (bw["dx"].data_ptr() != bw["dres"].data_ptr() or kw["p_pre"] > 0):
                self._store(bw["dx"], dx)
            vecs.append(dx)
        elif mode == "image":
            self._store(bw["dres"], dh)
            vecs.append(dh)
        else:
            seg = kw["segs"] if kw["segs"] is not None else torch.zeros(M, dtype=torch.int64)
            tv = kw["type_vocab"]
            s0, s1 = seg == 0, (seg == 1) & (tv > 1)
            vecs += [dh * s0[:, None], dh * s1[:, None]]
            rest = ~(s0 | s1)
            for tab, sel, idx in ((bw["dtt"], rest & (seg < tv), seg), (bw["dtt_ext"], rest & (seg >= tv), seg - tv)):
                tab.index_add_(0, idx[sel], dh[sel])
            bw["dword"].index_add_(0, kw["ids"], dh)
            bw["dpos"].index_add_(0, torch.arange(M) % kw["T"] + kw["pos_offset"], dh)
        v = torch.cat(vecs, 1)
        v = torch.cat([v, torch.zeros(nblk * rpb - M, v.shape[1])], 0).view(nblk, rpb, -1).sum(1)
        part = bw["partial"]
        if self.defect == "slab" and nblk > 1:
            part[:nblk - 1].copy_(v[:nblk - 1])
        else:
            part.copy_(v)

    # -- reductions
    def colsum_partials(self, partial, nblk, nvec, H, o0, o1, o2, accumulate):
        src = _raw(partial, nblk, nvec * H, 3 * H)
        s = src.sum(0) + (src[0] if self.defect == "colsum_twice" else 0)
        for j, o in enumerate((o0, o1, o2)):
            if o is not None and j < nvec:
                o.copy_(s[j * H:(j + 1) * H] + (o if accumulate else 0))

    def _slabs(self, x, M, N, scratch):
        nslab = (M + 63) // 64
        xs = x.float()
        scratch_rows = _raw(scratch, nslab, N, N)
        for s in range(nslab):
            scratch_rows[s].copy_(xs[s * 64:(s + 1) * 64].sum(0))
        return scratch_rows

    def colsum_slabs(self, x, M, N, scratch):
        assert N % 4 == 0 and M > 0
        self._slabs(x, M, N, scratch)

    def colsum(self, x, M, N, out, scratch, accumulate):
        assert N % 4 == 0 and M > 0
        out.copy_(self._slabs(x, M, N, scratch).sum(0) + (out if accumulate else 0))

    def batch(self):
        return _Batch(self)

    def locgrad(self, dh, loc, M, H, dw, accumulate):
        dw.copy_(dh.float().t() @ loc + (dw if accumulate else 0))


class _Batch(object):
    """ops.ColsumBatch: entries are queued and run at flush(); an entry naming an output already queued flushes first."""

    def __init__(self, be):
        self.be, self.entries, self.slabs, self.targets = be, [], [], set()

    def add_slabs(self, x, M, N, scratch, out, accumulate):
        self.slabs.append((x, M, N, scratch))
        self.add(scratch, (out, None, None), (M + 63) // 64, N, N, 1, (accumulate, False, False))

    def add(self, partial, outs, nblk, stride, H, nvec, accs):
        ptrs = [o.data_ptr() for o in outs if o is not None]
        if any(p in self.targets for p in ptrs):
            self.flush()
        self.targets.update(ptrs)
        self.entries.append((partial, outs, nblk, stride, H, nvec, accs))

    def flush(self):
        for x, M, N, scratch in self.slabs:
            self.be._slabs(x, M, N, scratch)
        for partial, outs, nblk, stride, H, nvec, accs in self.entries:
            src = _raw(partial, nblk, nvec * H, stride)
            s = src.sum(0) + (src[0] if self.be.defect == "colsum_twice" else 0)
            for j in range(nvec):
                if outs[j] is not None:
                    outs[j].copy_(s[j * H:(j + 1) * H] + (outs[j] if accs[j] else 0))
        self.entries, self.slabs, self.targets = [], [], set()


SMALL = [c for c in X.CASES if c.M * c.H <= 60000]


def ids(cs):
    return [c.id for c in cs]


def test_the_small_cases_cover_every_mode_type_and_direction():
    assert len(SMALL) >= 60
    for mode in X.MODES:
        for dt in X.DT:
            assert any(c.mode == mode and c.dtype == dt and c.bwd for c in SMALL)
            assert any(c.mode == mode and c.dtype == dt and c.p_post > 0 for c in SMALL)
    assert any(c.mode == "embed" and c.pos_offset and c.T == 1 and not c.bwd for c in SMALL)
    assert set(c.carrier for c in SMALL if c.mode == "embed") == {"word", "pos", "tt"}
    assert set(c.segs for c in SMALL if c.mode == "embed") == {"mix", "zero", "none"}
    assert set(c.type_vocab for c in SMALL if c.mode == "embed") == {1, 2}


@pytest.mark.parametrize("c", SMALL, ids=ids(SMALL))
def test_harness_accepts_the_stand_in(c):
    X.run_case(Torch(), c, X.CASES.index(c))


def test_the_wide_and_two_row_geometries_of_the_stand_in():
    """One 16-wave, one two-rows-per-wave shape (narrow columns: quick on the CPU)."""
    be = Torch()
    X.run_case(be, X.case("resid", "bf16", 2049, 4, nw=16, wide=True, p_pre=0.5, p_post=0.5))
    X.run_case(be, X.case("resid", "bf16", 2049, 4, nw=4, wide="narrow", p_pre=0.5))
    X.run_case(be, X.case("embed", "f32", 0, 4, B=8, T=1025, rw=2, carrier="pos", kmax=2))
    with pytest.raises(AssertionError, match="GSTVD_E_SHAPE"):
        c = X.case("resid", "f32", 2049, 4, nw=16, wide=True)
        p = X.Problem(be, c)
        p.build_backward()
        kw, bw = p.bwd_args()
        be.ln_bwd(kw, dict(bw, nblk=7))


@pytest.mark.parametrize("H", [4, 96, 260, 768, 832, 2048])
@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_closed_form_reference_equals_float64_autograd_without_eps(H, drop):
    """The reference of Problem (y_ref, ref) is the float64 autograd of LayerNorm without eps, bit for bit, for every k in -1..3."""
    be = Torch()
    p = X.Problem(be, X.case("resid", "f32", 23, H, p_post=drop, nv=1), seed=H)
    p.build_backward()
    assert set(p.k.flatten().tolist()) == {-1.0, 0.0, 1.0, 2.0, 3.0}
    y, dh, dg, db = X.autograd_reference(p)
    assert torch.equal(y, p.y_ref) and torch.equal(dh, p.ref["dh"])
    assert torch.equal(dg, p.ref["dgamma"]) and torch.equal(db, p.ref["dbeta"])
    assert p.nonzero_c > 0.5                      # c1 / c2 are not both zero on most rows
    # ... while eps = 1e-12 in float64 is NOT the same reference: it moves exact zeros and ones by 1e-12
    assert not torch.equal(1.0 / torch.sqrt(4.0 ** p.k + 1e-12), 2.0 ** -p.k)


def test_bf16_gradients_need_rounding_somewhere():
    """The truncating-store defect can only be seen where dh is not a bf16 number: the construction provides such elements, ties
    among them."""
    p = X.Problem(Torch(), X.case("resid", "bf16", 13, 768), seed=3)
    p.build_backward()
    dh = p.ref["dh"]
    assert int((dh.to(BF16).double() != dh).sum()) > 100


def test_exact_range_guard_refuses_what_leaves_2p24():
    X.exact_range("ok", s=(torch.full((4, 1000), 16000.0, dtype=torch.float64), 1))
    with pytest.raises(AssertionError, match="outside the exact range"):
        X.exact_range("big", s=(torch.full((4, 1100), 16000.0, dtype=torch.float64), 1))
    with pytest.raises(AssertionError, match="outside the exact range"):
        X.exact_range("fine bits", s=(torch.full((4, 1100), 16000.0 / 1024 + 1.0 / 1024, dtype=torch.float64), 1))
    with pytest.raises(AssertionError, match="not representable"):
        X.fits(torch.tensor([257.0], dtype=torch.float64), BF16, "x")


# ------------------------------------------------------------------------------------------ reductions and invariances
def test_reduction_checks_accept_the_stand_in():
    be = Torch()
    for nblk in (1, 3, 4, 5):
        for nvec in (1, 2, 3):
            X.check_colsum_partials(be, nblk, nvec, 68, accumulate=(nblk + nvec) % 2 == 0, none_out=nvec == 3 and nblk == 3)
    X.check_colsum_batch(be)
    for dt in X.DT:
        X.check_colsum(be, dt, 65, 260, True)
        X.check_colsum(be, dt, 1, 4, False)
        X.check_add_slabs(be, dt, [(63, 256), (130, 260)])
        X.check_locgrad(be, dt, 17, 260, True)
        X.check_locgrad(be, dt, 1, 4, False)


def _first(pred):
    return next(c for c in SMALL if pred(c))


def test_invariance_checks_accept_the_stand_in():
    be = Torch()
    X.check_surroundings_do_not_matter(be, _first(lambda c: c.mode == "resid" and c.bwd and c.res and c.dtype == "bf16"))
    X.check_surroundings_do_not_matter(be, _first(lambda c: c.mode == "image" and c.bwd))
    X.check_reproducible(be, _first(lambda c: c.mode == "embed" and c.bwd))
    X.check_segs_none_equals_zeros(be, X.case("embed", "f32", 0, 64, B=4, T=5, segs="zero", carrier="pos"))
    X.check_alias(be, X.case("resid", "bf16", 9, 260))
    X.check_batch_permutation(be, X.case("embed", "f32", 0, 64, B=8, T=5, pos_offset=2, carrier="word"))


def test_census_check_on_a_synthetic_symbol_list():
    syms = sorted(set(["_Z13" + c.fwd_kernel + "v10gstvd_ln_t" for c in X.CASES] + ["_Z13" + c.bwd_kernel + "v14gstvd_ln_bwd_t" for c in X.CASES if c.bwd]))
    red = ["_Z9" + r + "Ev" for r in X.REDUCTIONS]
    X.check_census(syms + red, out=lambda s: None)
    with pytest.raises(AssertionError, match="named by"):
        X.check_census(syms + red + ["_Z13ln_bwd_kernelIfLi0ELi16ELi1ELi4EEv14gstvd_ln_bwd_t"], out=lambda s: None)
    with pytest.raises(AssertionError, match="absent from the library"):
        X.check_census(syms[1:] + red, out=lambda s: None)


def test_the_table_holds_what_the_issue_lists():
    cs = X.CASES
    assert {1, 3, 4, 5} <= set(c.M for c in cs if not c.bwd)
    assert {1, 5, 2047} <= set(c.M for c in cs if c.bwd and c.nw == 4 and c.rw == 1)
    for mode in ("resid", "image"):                   # 16-wave shapes: nblk of the 16-wave geometry, of the 4-wave one, and 0
        for dt in X.DT:
            for wide, nw in ((True, 16), ("narrow", 4)):
                assert {2048, 2049, 2063} <= set(c.M for c in cs if c.mode == mode and c.dtype == dt and c.wide is wide and c.nw == nw
                                                 and c.H <= 768 and c.rw == 1), (mode, dt, wide)
    assert {2048, 2049, 2063} <= set(c.M for c in cs if c.nw == 4 and c.wide is False and c.H <= 768)
    assert {2048, 2049, 2063} <= set(c.M for c in cs if c.nw == 16) and {2048, 2049, 2063} <= set(c.M for c in cs if c.nw == 4 and c.H <= 768)
    assert {8193, 8200} <= set(c.M for c in cs if c.rw == 2) and any(c.M == 8192 and c.rw == 1 for c in cs)
    assert any(c.M == 8200 and c.H == 768 and c.wide for c in cs) and any(c.M == 8200 and c.H == 2048 for c in cs)
    for mode in ("resid", "image"):
        assert set(X.HS) <= set(c.H for c in cs if c.mode == mode and c.bwd)
    assert any(c.H == 772 and c.M >= 2048 and c.wide and c.nw == 4 for c in cs)
    assert all(c.nw == 16 for c in cs if c.H in (256, 768) and 2048 <= c.M <= 8192 and c.wide is True)
    emb = set((c.B, c.T, c.H, c.pos_offset) for c in cs if c.mode == "embed")
    assert {(3, 24, 64, 0), (4, 3, 768, 0), (8, 5, 256, 7), (8, 5, 1024, 0), (4, 3, 2048, 1), (8, 1025, 64, 0), (12, 683, 64, 0)} <= emb
    assert (4096, 768, 16) in set((c.M, c.H, c.nw) for c in cs if c.mode == "resid")
    assert any(c.mode == "embed" and c.B == 16 and c.M == 4096 and c.H == 768 for c in cs)
    assert any(c.mode == "image" and c.M == 592 and c.H == 1024 for c in cs)
    assert any(c.p_pre and c.p_post for c in cs if c.mode == "resid") and any(not c.res for c in cs if c.mode == "resid")
    assert all(c.pad >= (8 if c.dtype == "bf16" else 4) for c in cs)


# ------------------------------------------------------------------------------------------ planted defects
RESID = X.case("resid", "bf16", 13, 768, p_pre=0.5, p_post=0.5)
RESID32 = X.case("resid", "f32", 13, 260)
POS = X.case("embed", "f32", 0, 64, B=4, T=5, pos_offset=3, carrier="pos")
TT = X.case("embed", "f32", 0, 64, B=4, T=9, carrier="tt")
DEFECTS = [
    ("rowsum", RESID32, ": mean"),                    # a row sum that skips the last four columns
    ("c1", RESID32, ": dres"),                        # c1 dropped
    ("pos_offset", POS, ": (mean|rstd|y)"),           # pos_offset ignored
    ("seg_from_tt", TT, ": (mean|rstd|y)"),           # segment >= type_vocab read from tt
    ("truncate", RESID, ": dres"),                    # a truncating bf16 store
    ("tail", RESID, "outside the"),                   # one element written behind row M - 1
    ("pad_read", RESID32, ": mean"),                  # one input read from a pad column
    ("slab", RESID32, "never written"),               # a partial slab left unwritten
    ("colsum_twice", RESID32, ": dgamma"),            # a column sum that adds one block twice
    ("eps", RESID32, ": rstd"),                       # eps large enough to matter
]


@pytest.mark.parametrize("defect,c,match", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_fails_the_check_meant_for_it(defect, c, match):
    X.run_case(Torch(), c, 1)                         # (the sound stand-in passes the very same case)
    with pytest.raises(AssertionError, match=match):
        X.run_case(Torch(defect), c, 1)


def test_planted_defects_in_the_reduction_checks():
    with pytest.raises(AssertionError, match="colsum_partials"):
        X.check_colsum_partials(Torch("colsum_twice"), 5, 3, 68, False)
    with pytest.raises(AssertionError, match="ColsumBatch"):
        X.check_colsum_batch(Torch("colsum_twice"))
