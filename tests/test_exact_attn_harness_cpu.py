"""The exact attention harness (tests/exact_attn.py) proved on the CPU: a stand-in for the HIP kernels written in plain torch,
with the kernels' conventions -- additive mask term added once under causal x padding, draws indexed over round4(Lk), factor
1 / (1 - p), delta from the stored O, keep bits in forward's tile layout -- behind the call shape the GPU tests use.  Every check
of the layers C-G passes on it, and each deliberately wrong stand-in is caught by the layer meant to catch it.  (Torch functions
on the CPU; nothing here touches a GPU.)"""
import os

import pytest
import torch

import exact_attn as A

DEV = torch.device("cpu")
MUTANTS = ("skip64", "causal_ge", "masked_weight", "draw_plus1", "zero_row", "zero_row_grads", "store_past", "read_pad")


class StandIn(object):
    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.device, self.mutant = DEV, mutant

    def _draws(self, c, shift=0):
        Lkp = A.round4(c.Lk)
        n = c.B * c.nh * c.Lq * Lkp
        flat = torch.rand(n + 1, generator=torch.Generator().manual_seed(99)) >= c.p
        return flat[shift:shift + n].view(c.B, c.nh, c.Lq, Lkp)[..., :c.Lk]

    def keep(self, p):
        return self._draws(p.c)

    def run(self, p):
        c, mu = p.c, self.mutant
        dt = A.DT[c.dtype]
        Q, K, V = p.t("Q").double(), p.t("K").double().repeat_interleave(c.kv_group, 0), p.t("V").double().repeat_interleave(c.kv_group, 0)
        sc = A.scale32(c.d)
        km = p.km.clone() if p.km is not None else None
        if mu == "masked_weight" and km is not None:
            for b in range(km.shape[0]):
                z = torch.nonzero(km[b] == 0)
                if len(z):
                    km[b, z[0]] = 1                          # one masked key is given weight
        al = A.allowed_keys(c._replace(causal=False), km, DEV)
        if c.causal:
            kk, qq = torch.arange(c.Lk)[None, :], torch.arange(c.Lq)[:, None]
            al = al & ((kk < qq) if mu == "causal_ge" else (kk <= qq))[None, None]
        s = torch.einsum("bqhd,bkhd->bhqk", Q, K) * sc + torch.where(al, 0.0, c.neg).double()
        if mu == "skip64" and c.Lk > 64:
            s[..., 64] = -float("inf")                       # the first key of the second chunk is skipped
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        P = e / l
        lse = (m + torch.log(l)).squeeze(-1)
        f = torch.ones_like(P)
        if c.p > 0:
            f = self._draws(c, 1 if mu == "draw_plus1" else 0).double() / (1.0 - c.p)
        Pd = P * f
        O = torch.einsum("bhqk,bkhd->bqhd", e * f, V) * (1.0 / l).squeeze(-1).permute(0, 2, 1)[..., None]      # unnormalised sum, then 1 / l: as the kernels
        if mu == "zero_row" and p.km is not None:
            dead = (p.km == 0).all(-1).repeat_interleave(c.kv_group, 0)
            O[dead] = 0
            lse[dead] = 0
        if mu == "read_pad" and "V" in p.wins:
            w = p.wins["V"]
            O = O + 0.0 * w.flat[w.offset + w.cols].double()  # a pad column of V reaches the result
        p.t("O").copy_(O.float())
        p.t("LSE").copy_(lse.float())
        if mu == "store_past":
            w = p.wins["O"]
            w.flat[w.offset + (w.batch - 1) * w.stride + w.rows * w.ld] = 1.0      # one row past the window
        if p.bits is not None:
            keep = self._draws(c)
            qi = torch.arange(c.Lq)[:, None].expand(c.Lq, c.Lk)
            ki = torch.arange(c.Lk)[None, :].expand(c.Lq, c.Lk)
            nqt, nkt = (c.Lq + 15) // 16, (c.Lk + 15) // 16
            word = ((qi >> 4) * nkt + (ki >> 4)) * 4 + (ki & 3)
            bit = torch.ones((), dtype=torch.int64) << (16 * ((ki & 15) >> 2) + (qi & 15))
            w = torch.zeros(c.B, c.nh, nqt * nkt * 4, dtype=torch.int64)
            w.scatter_add_(-1, word.reshape(1, 1, -1).expand(c.B, c.nh, -1), (keep.long() * bit).reshape(c.B, c.nh, -1))
            p.bits.copy_(w.reshape(-1))
        if not c.has_bwd:
            return
        dO = p.t("dO").double()
        delta = (dO * p.t("O").double()).sum(-1).permute(0, 2, 1)
        dP = torch.einsum("bqhd,bkhd->bhqk", dO, V)
        dS = P * (dP * f - delta[..., None]) * sc
        p.t("dV").copy_(torch.einsum("bhqk,bqhd->bkhd", Pd, dO).float())
        p.t("dQ").copy_(torch.einsum("bhqk,bkhd->bqhd", dS, K).float())
        p.t("dK").copy_(torch.einsum("bhqk,bqhd->bkhd", dS, Q).float())
        p.t("delta").copy_(delta.float())
        if mu == "zero_row_grads" and p.km is not None:      # "masked keys do no work" in the backward: a dead row gets no gradient
            dead = (p.km == 0).all(-1)
            for nme in ("dQ", "dK", "dV"):
                p.t(nme)[dead] = 0


def small(pred=lambda c: True, per=1):
    return A.first_per_kernel(A.CASES, lambda c: c.bwd != "refuse" and c.Lq <= 130 and c.Lk <= 130 and c.nh <= 2 and pred(c), per)


def ids(cs):
    return [c.id for c in cs]


# ---------------------------------------------------------------------------------------------- the table
def test_table_covers_what_it_promises():
    cs = A.CASES
    assert len(set(c.id for c in cs)) == len(cs)
    for dt in ("bf16", "f32"):
        for d in (32, 64, 128):
            mine = [c for c in cs if c.dtype == dt and c.d == d]
            for fwd in ("tiled", "decode"):
                assert set(A.KEYS) <= set(c.Lk for c in mine if c.fwd == fwd), (dt, d, fwd)
            assert set(A.QUERIES) | {1} <= set(c.Lq for c in mine if c.fwd == "tiled")
            assert set(A.KEYS) <= set(c.Lk for c in mine if c.has_bwd) and set(A.QUERIES) | {1} <= set(c.Lq for c in mine if c.has_bwd)
            assert any(c.Lq == 1 and c.p > 0 and c.fwd == "tiled" for c in mine) and any(c.Lq == 1 and c.causal and c.fwd == "tiled" for c in mine)
            assert any(c.causal and c.Lq != c.Lk for c in mine) and any(c.bwd == "refuse" for c in mine)
            assert any(c.kv_group > 1 and c.kv_bstride and c.fwd == f for c in mine for f in ("tiled", "decode"))
            assert {"two0", "two1"} <= set(c.bwd for c in mine)
    one = [c for c in cs if c.bwd in ("onepass", "onepass_bits")]
    assert all(c.dtype == "bf16" and c.d == 64 and not c.causal and 64 < c.Lk <= 256 and 64 <= c.Lq <= 1024 for c in one)
    for bwd in ("onepass", "onepass_bits"):
        mine = [c for c in one if c.bwd == bwd]
        assert {65, 256} <= set(c.Lk for c in mine) and {64, 1024} <= set(c.Lq for c in mine), bwd
    near = [c for c in cs if c.dtype == "bf16" and c.d == 64 and not c.causal and c.bwd in ("two0", "two1")]
    assert any(c.Lk == 64 and c.Lq >= 64 for c in near) and any(c.Lk == 257 and c.Lq >= 64 for c in near)
    assert any(c.Lq == 63 and 64 < c.Lk <= 256 for c in near) and any(c.Lq == 1025 and 64 < c.Lk <= 256 for c in near)


def library_symbols():
    if not os.path.exists(A.lib_path()):
        pytest.fail("libgstvd_hip.so is not built")
    return A.E.library_kernels(A.lib_path(), A.ATTN_KERNEL_RE)


def test_census_of_the_built_library():
    """The census runs without a GPU too: it reads the symbols of the built library."""
    lines = []
    A.check_census(library_symbols(), out=lines.append)
    assert sum("EXEMPT" in x for x in lines) == len(A.EXEMPT)


def test_census_notices_a_kernel_nobody_names():
    syms = library_symbols()
    with pytest.raises(AssertionError):
        A.check_census(syms + ["_Z15attn_new_kernelIfLi64EEv12gstvd_attn_t"], out=lambda s: None)
    with pytest.raises(AssertionError):
        A.check_census([s for s in syms if "decode_kernelIfLi32" not in s], out=lambda s: None)


# ---------------------------------------------------------------------------------------------- the layers on the stand-in
C_CASES = small(per=2)


@pytest.mark.parametrize("c", C_CASES, ids=ids(C_CASES))
def test_standin_passes_onehot_and_uniform(c):
    be = StandIn()
    A.check_onehot(be, c, A.CASES.index(c))
    A.check_uniform(be, c, A.CASES.index(c))


def test_standin_uniform_backward_is_checked_exactly_in_both_types():
    for dt in ("f32", "bf16"):
        c = next(c for c in A.CASES if c.dtype == dt and c.d == 64 and c.has_bwd and not c.causal and c.p == 0 and c.Lk == 17)
        assert A.check_uniform(StandIn(), c, 0) == "exact"
    c = next(c for c in A.CASES if c.dtype == "f32" and c.d == 32 and c.has_bwd and not c.causal and c.p == 0 and c.Lk == 17)
    assert A.check_uniform(StandIn(), c, 0) == "ulp"


def test_uniform_exactness_promise_names_cases_of_every_kind():
    """uniform_must_be_exact is not vacuous: it promises bit-exact backward cases in both types at key counts on both sides of
    every 16 / 64 border, and check_uniform (which asserts the promise itself) keeps it on the stand-in."""
    for dt, mode, d in (("f32", "exact", 64), ("bf16", "exact", 64), ("f32", "ulp", 32), ("f32", "ulp", 128)):
        mine = [c for c in A.CASES if c.dtype == dt and c.d == d and A.uniform_must_be_exact(c) == mode]
        assert {15, 16, 17, 63, 64, 65, 127, 128, 129, 255} <= set(c.Lk for c in mine), (dt, mode)
        assert {"two0", "two1"} <= set(c.bwd for c in mine)
        for c in mine:
            if c.Lq <= 65:
                assert A.check_uniform(StandIn(), c, A.CASES.index(c)) == mode
    assert any(A.uniform_must_be_exact(c) == "exact" for c in A.CASES if c.bwd == "onepass")


E_CASES = small(lambda c: c.Lk > 16 and c.Lq > 1)


@pytest.mark.parametrize("c", E_CASES, ids=ids(E_CASES))
def test_standin_passes_the_invariances(c):
    be, i = StandIn(), A.CASES.index(c)
    A.check_mask_none_vs_ones(be, c, i)
    A.check_masked_rows_do_not_matter(be, c, i)
    if c.causal:
        A.check_causal_later_keys(be, c, i)
    if c.p == 0 and c.kv_group == 1 and not c.fused:
        A.check_appended_masked_keys(be, c, 2, i)
        A.check_permutation(be, c, i)
    if c.bits:
        A.check_keep_bits_vs_hash(be, c, i)


F_CASES = [A.case("bf16", 32, 37, 67, "tiled", "two1", causal=True, p=0.5), A.case("f32", 64, 65, 63, "tiled", "two0", p=0.5),
           A.case("bf16", 64, 64, 70, "tiled", "onepass", p=0.5)]


@pytest.mark.parametrize("c", F_CASES, ids=ids(F_CASES))
def test_standin_passes_the_dropout_mask_recovery(c):
    A.check_dropout_masks(StandIn(), c, 0)


G_CASES = small(lambda c: c.B >= 2 and c.kv_group == 1 and c.Lk > 16, per=1)


@pytest.mark.parametrize("c", G_CASES, ids=ids(G_CASES))
def test_standin_passes_the_fully_masked_row(c):
    A.check_all_masked_row(StandIn(), c, A.CASES.index(c))


# ---------------------------------------------------------------------------------------------- mutants
def pick(**kw):
    return next(c for c in A.CASES if c.bwd != "refuse" and all(getattr(c, k) == v for k, v in kw.items()))


def caught(check, *a, **kw):
    with pytest.raises(AssertionError):
        check(*a, **kw)


def test_mutant_one_key_skipped_at_index_64():
    c = pick(dtype="bf16", d=64, Lk=65, fwd="tiled", causal=False)
    A.check_uniform(StandIn(), c, 0)
    caught(A.check_uniform, StandIn("skip64"), c, 0)                      # D: one key too few
    c = pick(dtype="f32", d=32, Lk=128, fwd="tiled", causal=False)
    caught(A.check_uniform, StandIn("skip64"), c, 0)


def test_mutant_onehot_sees_a_skipped_key():
    c = pick(dtype="bf16", d=64, Lk=127, fwd="tiled", causal=False)
    A.check_onehot(StandIn(), c, 5)
    caught(A.check_onehot, StandIn("skip64"), c, 5)                       # C: the queries that point at key 64 get another row


def test_mutant_causal_off_by_one():
    for c in (pick(dtype="bf16", d=64, causal=True, Lq=65), pick(dtype="f32", d=128, causal=True, Lq=65)):
        A.check_uniform(StandIn(), c, 1)
        caught(A.check_uniform, StandIn("causal_ge"), c, 1)               # D: the diagonal key is missing from every mean
        caught(A.check_onehot, StandIn("causal_ge"), c, 1)                # C: queries that point at themselves


def test_mutant_masked_key_given_weight():
    c = pick(dtype="bf16", d=64, Lq=63, Lk=17)
    caught(A.check_masked_rows_do_not_matter, StandIn("masked_weight"), c, 0)      # E
    caught(A.check_uniform, StandIn("masked_weight"), c, 0)                        # D: one key too many


def test_mutant_draw_taken_from_the_next_index():
    for c in F_CASES:
        caught(A.check_dropout_masks, StandIn("draw_plus1"), c, 0)        # F
    caught(A.check_onehot, StandIn("draw_plus1"), pick(dtype="bf16", d=64, Lk=65, p=0.5, fwd="tiled"), 0)     # C sees it too


def test_mutant_fully_masked_row_returned_as_zeros():
    for c in (pick(dtype="bf16", d=64, Lq=63, Lk=17), pick(dtype="f32", d=128, Lq=1, Lk=63, fwd="decode")):
        assert c.neg == -10000.0 and c.B >= 2
        A.check_all_masked_row(StandIn(), c, 0)
        caught(A.check_all_masked_row, StandIn("zero_row"), c, 0)         # G


def test_mutant_fully_masked_row_gets_no_gradient():
    for c in (pick(dtype="bf16", d=64, Lq=63, Lk=17), pick(dtype="bf16", d=64, Lq=65, Lk=127, bwd="onepass"), pick(dtype="f32", d=32, Lq=63, Lk=17)):
        assert c.neg == -10000.0 and c.B >= 2
        A.check_all_masked_row(StandIn(), c, 0)
        with pytest.raises(AssertionError, match="masked row d[QKV]"):
            A.check_all_masked_row(StandIn("zero_row_grads"), c, 0)       # G, backward


def test_mutant_store_one_row_past_the_window():
    c = pick(dtype="bf16", d=64, Lq=63, Lk=17)
    for check in (A.check_onehot, A.check_uniform, A.check_mask_none_vs_ones, A.check_all_masked_row):
        with pytest.raises(AssertionError, match="outside the"):
            check(StandIn("store_past"), c, 0)                            # B, in every layer


def test_mutant_read_of_a_pad_column():
    c = pick(dtype="f32", d=64, Lq=63, Lk=17)
    for check in (A.check_onehot, A.check_uniform, A.check_masked_rows_do_not_matter):
        with pytest.raises(AssertionError, match="NaN"):
            check(StandIn("read_pad"), c, 0)                              # B: the poison reaches the result


def test_mutant_output_element_never_written():
    class Lazy(StandIn):
        def run(self, p):
            keepback = p.t("O")[0, 0, 0, 0].clone()
            StandIn.run(self, p)
            p.t("O")[0, 0, 0, 0] = keepback
    with pytest.raises(AssertionError, match="never written"):
        A.check_uniform(Lazy(), pick(dtype="bf16", d=64, Lq=63, Lk=17), 0)
