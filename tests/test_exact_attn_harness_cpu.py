"""The exact attention harness (tests/exact_attn.py) proved on the CPU: a stand-in for the HIP kernels written in plain torch,
with the kernels' conventions -- additive mask term added once under causal x padding, draws indexed over round4(Lk), factor
1 / (1 - p), delta from the stored O, keep bits in forward's tile layout -- behind the call shape the GPU tests use.  Every check
of the layers C-J passes on it (H, I, J also on its rounded mode: fp32, online softmax, bf16 operand roundings), and each
deliberately wrong stand-in is caught by the layer meant to catch it.  (Torch functions
on the CPU; nothing here touches a GPU.)"""
import os

import pytest
import torch

import exact_attn as A

DEV = torch.device("cpu")
MUTANTS = ("skip64", "causal_ge", "masked_weight", "draw_plus1", "zero_row", "zero_row_grads", "store_past", "read_pad",
           "dk_zero", "dk_scale_twice", "dk_q_row_plus1", "dk_skip_tile", "tie_first_only", "bwd_lse_one_row_off", "bwd_p_without_scale_on_dk")
ROUNDED_MUTANTS = ("rescale_skip_acc", "rescale_twice", "rescale_max_lanes_only", "bwd_lse_one_row_off", "bwd_p_without_scale_on_dk")


def next_row_in_tile(x, dim):
    """x with row q replaced by row q + 1 of the same 16-row tile (the last row of a tile, and the last row, by the tile's first)."""
    n = x.shape[dim]
    q = torch.arange(n)
    nxt = torch.where(((q & 15) == 15) | (q == n - 1), q & ~15, q + 1)
    return x.index_select(dim, nxt)


class StandIn(object):
    """float64 arithmetic, softmax formed over the whole row.  `rounded`: the kernels' arithmetic instead -- fp32, the forward as
    an online softmax per update group (64 keys, 32 at d = 128) with the running maximum, the partial sum and the accumulator
    rescaled when the maximum moves, bf16 rounding of P * fac and dS in bf16 mode, outputs rounded to the case's type."""

    def __init__(self, mutant=None, rounded=False):
        assert mutant is None or mutant in (ROUNDED_MUTANTS if rounded else MUTANTS)
        self.device, self.mutant, self.rounded = DEV, mutant, rounded

    def _draws(self, c, shift=0):
        Lkp = A.round4(c.Lk)
        n = c.B * c.nh * c.Lq * Lkp
        flat = torch.rand(n + 1, generator=torch.Generator().manual_seed(99)) >= c.p
        return flat[shift:shift + n].view(c.B, c.nh, c.Lq, Lkp)[..., :c.Lk]

    def keep(self, p):
        return self._draws(p.c)

    def run(self, p):
        if self.rounded:
            return self.run_rounded(p)
        c, mu = p.c, self.mutant
        dt = A.DT[c.dtype]
        Q, K, V = p.t("Q").double(), p.t("K").double().repeat_interleave(c.kv_group, 0), p.t("V").double().repeat_interleave(c.kv_group, 0)
        sc = p.scale
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
        if mu == "tie_first_only":                               # of equal maxima only the first key keeps its weight
            tie = s == m
            e = torch.where(tie & (torch.cumsum(tie.long(), -1) > 1), torch.zeros_like(e), e)
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
        if mu == "bwd_lse_one_row_off":                          # the backward recomputes P against LSE[q + 1]
            P = torch.exp(s - next_row_in_tile(lse, 2)[..., None])
            Pd = P * f
        dS = P * (dP * f - delta[..., None]) * sc
        p.t("dV").copy_(torch.einsum("bhqk,bqhd->bkhd", Pd, dO).float())
        p.t("dQ").copy_(torch.einsum("bhqk,bkhd->bqhd", dS, K).float())
        p.t("dK").copy_(self.dk(c, mu, dS, Q, sc).float())
        p.t("delta").copy_(delta.float())
        if mu == "zero_row_grads" and p.km is not None:      # "masked keys do no work" in the backward: a dead row gets no gradient
            dead = (p.km == 0).all(-1)
            for nme in ("dQ", "dK", "dV"):
                p.t(nme)[dead] = 0


    @staticmethod
    def dk(c, mu, dS, Q, sc):
        """dK = dS^T Q, and the ways of getting it wrong."""
        if mu == "dk_q_row_plus1":                               # dS[q] paired with Q[q + 1] inside a 16-query tile
            Q = next_row_in_tile(Q, 1)
        if mu == "dk_skip_tile":                                 # queries 16..31 of each 64-query chunk left out (of dK only)
            dS = dS * ((torch.arange(c.Lq) % 64) // 16 != 1).to(dS.dtype)[None, None, :, None]
        dK = torch.einsum("bhqk,bqhd->bkhd", dS, Q)
        return {"dk_zero": dK * 0, "dk_scale_twice": dK * sc, "bwd_p_without_scale_on_dk": dK / sc}.get(mu, dK)

    def run_rounded(self, p):
        c, mu = p.c, self.mutant
        bf = A.DT[c.dtype] == A.BF16
        rnd = (lambda x: x.bfloat16().float()) if bf else (lambda x: x)
        Q, K, V = p.t("Q").float(), p.t("K").float().repeat_interleave(c.kv_group, 0), p.t("V").float().repeat_interleave(c.kv_group, 0)
        sc = torch.tensor(p.scale, dtype=torch.float32)
        al = A.allowed_keys(c, p.km, DEV)
        s = torch.einsum("bqhd,bkhd->bhqk", Q, K) * sc + torch.where(al, 0.0, c.neg).float()       # [B, nh, Lq, Lk]
        f = torch.ones_like(s)
        if c.p > 0:
            f = self._draws(c).float() / torch.tensor(1.0 - c.p, dtype=torch.float32)
        m_run = torch.full((c.B, c.nh, c.Lq), -1e30)
        l = torch.zeros(c.B, c.nh, c.Lq)
        acc = torch.zeros(c.B, c.nh, c.Lq, c.d)
        grp = A.update_group(c)
        for gi, k0 in enumerate(range(0, c.Lk, grp)):
            sg = s[..., k0:k0 + grp]
            m_new = torch.maximum(m_run, sg.max(-1).values)
            alpha = torch.exp(m_run - m_new)                     # 1 for the rows whose maximum did not move
            a_acc = alpha
            if mu == "rescale_skip_acc" and gi == 2:             # at the third update l is rescaled, the accumulator is not
                a_acc = torch.ones_like(alpha)
            if mu == "rescale_twice":
                alpha = a_acc = alpha * alpha
            if mu == "rescale_max_lanes_only" and gi > 0:        # only the rows of a 16-query tile whose maximum moved MOST rescale
                move = m_new - m_run
                pad = (-c.Lq) % 16
                top = torch.nn.functional.pad(move, (0, pad), value=0.0).view(c.B, c.nh, -1, 16).max(-1, keepdim=True).values
                top = top.expand(-1, -1, -1, 16).reshape(c.B, c.nh, -1)[..., :c.Lq]
                alpha = a_acc = torch.where(move == top, alpha, torch.ones_like(alpha))
            pg = torch.exp(sg - m_new[..., None])
            l = l * alpha + pg.sum(-1)
            acc = acc * a_acc[..., None] + torch.einsum("bhqk,bkhd->bhqd", rnd(pg * f[..., k0:k0 + grp]), V[:, k0:k0 + grp])
            m_run = m_new
        p.t("O").copy_((acc * (1.0 / l)[..., None]).permute(0, 2, 1, 3))
        lse = m_run + torch.log(l)
        p.t("LSE").copy_(lse)
        assert p.bits is None or c.p == 0, "the rounded stand-in writes no keep bits"
        if not c.has_bwd:
            return
        dO = p.t("dO").float()
        delta = (dO * p.t("O").float()).sum(-1).permute(0, 2, 1)
        if mu == "bwd_lse_one_row_off":
            lse = next_row_in_tile(lse, 2)
        P = torch.exp(s - lse[..., None])
        dS = P * (torch.einsum("bqhd,bkhd->bhqk", dO, V) * f - delta[..., None]) * sc
        p.t("dV").copy_(torch.einsum("bhqk,bqhd->bkhd", rnd(P * f), dO))
        p.t("dQ").copy_(torch.einsum("bhqk,bkhd->bqhd", rnd(dS), K))
        p.t("dK").copy_(self.dk(c, mu, rnd(dS), Q, sc))
        p.t("delta").copy_(delta)


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


# ---------------------------------------------------------------------------------------------- H, I, J on both stand-ins
RUNNABLE = [c for c in A.CASES if c.bwd != "refuse"]
H_CASES = small(lambda c: c.has_bwd, per=2)
I_CASES = small(per=2)
J_ALL = [c for c in RUNNABLE if A.tent_case(c)]
J_SMALL = [c for c in J_ALL if c.nh <= 2 and c.Lq <= 130 and c.Lk <= 130]
NO_FACTOR = {k: float("inf") for k in A.J_K}


def unbitted(c):
    """The rounded stand-in writes no keep bits: the same case with hashed draws."""
    return c._replace(bits=False, bwd="onepass") if c.bits else c


@pytest.mark.parametrize("c", H_CASES, ids=ids(H_CASES))
def test_both_standins_pass_uniform_attention_on_disjoint_columns(c):
    for be in (StandIn(), StandIn(rounded=True)):
        A.check_uniform_dk(be, unbitted(c) if be.rounded else c, A.CASES.index(c))


@pytest.mark.parametrize("c", I_CASES, ids=ids(I_CASES))
def test_both_standins_pass_subset_attention(c):
    for be in (StandIn(), StandIn(rounded=True)):
        A.check_subset(be, unbitted(c) if be.rounded else c, A.CASES.index(c))


@pytest.mark.parametrize("c", J_SMALL, ids=ids(J_SMALL))
def test_both_standins_pass_the_graded_rows(c):
    for be in (StandIn(), StandIn(rounded=True)):
        A.check_tent(be, unbitted(c) if be.rounded else c, A.CASES.index(c))


def test_disjoint_columns_promise_names_cases_of_every_kind():
    """disjoint_must_be_exact is not vacuous: bit-exact dK is promised in fp32 at all three head sizes and in bf16, at key counts
    on both sides of every 16 / 64 border and for both block orders, and kept on the stand-in."""
    for dt in ("f32", "bf16"):
        for d in (32, 64, 128):
            mine = [c for c in A.CASES if c.dtype == dt and c.d == d and A.disjoint_must_be_exact(c) == "exact"]
            assert {15, 16, 17, 63, 64, 65, 127, 128, 129, 255} <= set(c.Lk for c in mine), (dt, d)
            assert {"two0", "two1"} <= set(c.bwd for c in mine)
            for c in mine:
                if c.Lq <= 65 and c.nh <= 2:
                    assert A.check_uniform_dk(StandIn(), c, A.CASES.index(c)) == "exact"
    assert any(A.disjoint_must_be_exact(c) == "exact" for c in A.CASES if c.bwd == "onepass")


ONEPASS_BORDERS = [c for c in RUNNABLE if c.dtype == "bf16" and c.d == 64 and not c.causal and c.has_bwd and c.p > 0 and not c.fused and c.nh <= 2
                   and ((c.Lk in (64, 65, 256, 257) and c.Lq in (64, 100)) or (c.Lq in (63, 64) and c.Lk == 200))]
I_GPU = A.first_per_kernel(RUNNABLE, per=2)
I_GPU += [c for c in ONEPASS_BORDERS + [c for c in RUNNABLE if c.nh > 2] if c not in I_GPU]      # the list tests/test_attn_exact_gpu.py runs


def test_subset_attention_deals_kind_j_and_mask_independently_and_ties_across_chunks():
    """The case list of family I on the GPU meets low and high free bits, j = 1, 2, 3 and a key mask or none in every
    combination, and -- high bits free -- tied keys in different 64-key chunks."""
    par = [A.subset_params(c, A.CASES.index(c)) for c in I_GPU]
    assert set((j, kind, masked) for nb, j, kind, free, masked, reps in par) >= set((j, k, m) for j in (1, 2, 3) for k in ("low", "high") for m in (True, False))
    assert any(kind == "high" and (free & -free) >= 64 for nb, j, kind, free, masked, reps in par)
    assert any(p[2] == "high" for p, c in zip(par, I_GPU) if c.bwd in ("onepass", "onepass_bits"))


def test_every_subset_case_of_the_gpu_list_holds_ties_that_a_wrong_dk_or_tie_rule_fails():
    """No case of the list degenerates to family C: on each, check_subset itself asserts the share of tied queries, and the
    stand-in that keeps only the first of equal maxima (on O) and the one that writes dK = 0 (on dK) fail it."""
    for c in I_GPU:
        if c.B * c.nh * c.Lq * c.Lk > 1e6 or A.keys_in_sight(c) == 1:
            continue
        i = A.CASES.index(c)
        A.check_subset(StandIn(), c, i)
        caught_on("O", A.check_subset, StandIn("tie_first_only"), c, i)
        if c.has_bwd and c.B * c.nh * c.Lq >= 16:
            caught_on("dK", A.check_subset, StandIn("dk_zero"), c, i)


def test_tent_cases_are_the_shapes_and_routes_the_family_is_for():
    for dt in ("bf16", "f32"):
        mine = [c for c in J_ALL if c.dtype == dt]
        assert {65, 129, 256, 293} <= set(c.Lk for c in mine if c.d <= 64) and {37, 65, 256} <= set(c.Lk for c in mine if c.d == 128)
        assert {1, 17, 63, 65, 100, 256} <= set(c.Lq for c in mine) and (dt == "f32" or 64 in set(c.Lq for c in mine))     # (64 queries: the one-pass border)
        assert {(1, 65), (1, 293)} <= set((c.Lq, c.Lk) for c in mine if c.fwd == "decode")
        assert any(c.Lq == 1 and c.Lk == 293 and c.fwd == "tiled" and c.p > 0 for c in mine)
        assert any(c.causal and (c.Lq, c.Lk) == (100, 200) for c in J_ALL) and any(c.causal and c.Lk == 129 for c in mine)
        assert sum(1 for c in mine if c.nh > 2) == 7                           # the production shapes (six and the decode step)
    assert {"two0", "two1", "onepass", "onepass_bits"} == set(c.bwd for c in J_ALL)
    assert all(A.update_group(c) < c.Lk for c in J_ALL if c.nh <= 2)           # at least two softmax updates
    # the mass condition is asserted (check_tent: a border MUST be found) on 48 of the 83 cases, the d = 128 shapes with 37 keys among
    # them; the exempt ones are what tent_must_straddle's docstring lists
    must = [c for c in J_ALL if A.tent_must_straddle(c)]
    assert len(J_ALL) == 83 and len(must) == 48 and all(A.tent_must_straddle(c) for c in J_ALL if c.d == 128 and c.Lk == 37)
    assert all(c.Lk < A.update_group(c) + A.J_NEAR or c.Lk == 129 or c.causal for c in J_ALL if c not in must)
    assert set(c.bwd for c in must) == {"two0", "two1", "onepass", "onepass_bits"}


def test_the_tent_bound_needs_its_term_for_delta():
    """Without the term for the fp32 error of delta = rowsum(dO * O) the first-order bound of dQ / dK is relative to |dS| alone,
    and the correct fp32 stand-in misses it by orders of magnitude on a row where dP * fac - delta nearly cancels."""
    c = pick(dtype="f32", d=64, Lq=25, Lk=25, nh=12)
    i = A.CASES.index(c)
    A.check_tent(StandIn(rounded=True), c, i)
    r = A.check_tent(StandIn(rounded=True), c, i, factors=NO_FACTOR, delta_term=False)
    assert max(r["dQ"], r["dK"]) > 1000 * A.J_K[("f32", "bwd")], r


def test_tent_factors_are_twice_what_the_rounded_standin_reaches():
    """J_K is derived, not tuned on a kernel: the largest err / bound of the rounded stand-in over every case of the family is
    what J_MEASURED records, and J_K is the smallest power of two >= twice that."""
    top = {k: 0.0 for k in A.J_K}
    for c in J_ALL:
        r = A.check_tent(StandIn(rounded=True), unbitted(c), A.CASES.index(c), factors=NO_FACTOR)
        for n, v in r.items():
            key = (c.dtype, "fwd" if n in ("O", "LSE") else "bwd")
            top[key] = max(top[key], v)
    for key, v in top.items():
        assert abs(v - A.J_MEASURED[key]) <= 0.01, (key, v)
        assert A.J_K[key] / 2 < 2 * A.J_MEASURED[key] <= A.J_K[key], key


# ---------------------------------------------------------------------------------------------- mutants of H, I, J
def caught_on(output, check, *a, **kw):
    with pytest.raises(AssertionError, match=": (disjoint|subset|tent) (%s)[ :]" % output):
        check(*a, **kw)


HM = [pick(dtype="f32", d=32, Lq=65, fwd="tiled", causal=False, p=0.0), pick(dtype="bf16", d=64, Lq=63, Lk=17),
      pick(dtype="bf16", d=64, bwd="onepass", Lq=65), pick(dtype="f32", d=128, Lq=64, causal=False)]


def test_mutants_of_dk_are_caught_by_the_disjoint_columns():
    for c in HM:
        i = A.CASES.index(c)
        assert A.check_uniform_dk(StandIn(), c, i) == "exact"
        for mu in ("dk_zero", "dk_scale_twice", "dk_q_row_plus1", "dk_skip_tile"):
            A.check_uniform(StandIn(mu), c, i)                                # family D cannot see them: its dK is 0
            caught_on("dK", A.check_uniform_dk, StandIn(mu), c, i)


def test_mutants_of_dk_and_of_ties_are_caught_by_subset_attention():
    for c in HM:
        i = A.CASES.index(c)
        A.check_subset(StandIn(), c, i)
        for mu in ("dk_zero", "dk_q_row_plus1"):
            A.check_onehot(StandIn(mu), c, i)                                 # family C cannot see them: its dK is 0
            caught_on("dK", A.check_subset, StandIn(mu), c, i)
        A.check_onehot(StandIn("tie_first_only"), c, i)                       # ... and has no ties
        caught_on("O", A.check_subset, StandIn("tie_first_only"), c, i)


def tent_excess(mu, c, rounded=True):
    """err / (J_K x bound) per output of the mutant on case c (the stand-in itself passes)."""
    i = A.CASES.index(c)
    A.check_tent(StandIn(rounded=rounded), c, i)
    r = A.check_tent(StandIn(mu, rounded=rounded), c, i, factors=NO_FACTOR)
    return {n: v / A.J_K[(c.dtype, "fwd" if n in ("O", "LSE") else "bwd")] for n, v in r.items()}


JM = [c for c in J_ALL if c.has_bwd and not c.causal and not c.bits and c.nh <= 2 and c.Lq > 1 and c.Lk >= 4 * A.update_group(c)]


def test_mutants_of_the_rescale_are_caught_by_the_graded_rows_on_o():
    assert set((c.dtype, c.d) for c in JM) == set((dt, d) for dt in ("bf16", "f32") for d in (32, 64, 128))
    for c in A.first_per_kernel(JM):
        for mu in ("rescale_skip_acc", "rescale_twice", "rescale_max_lanes_only"):
            x = tent_excess(mu, c)
            assert x["O"] > (4 if c.dtype == "f32" else 1), (c.id, mu, x)
            caught_on("O", A.check_tent, StandIn(mu, rounded=True), c, A.CASES.index(c))


def test_mutants_of_the_backward_probabilities_are_caught_by_the_graded_rows():
    for c in A.first_per_kernel(JM):
        for rounded in (False, True):
            x = tent_excess("bwd_lse_one_row_off", c, rounded)
            assert min(x["dQ"], x["dK"], x["dV"]) > (4 if c.dtype == "f32" else 1) and x["O"] <= 1, (c.id, x)
            caught_on("dQ", A.check_tent, StandIn("bwd_lse_one_row_off", rounded=rounded), c, A.CASES.index(c))
            x = tent_excess("bwd_p_without_scale_on_dk", c, rounded)
            assert x["dK"] > (4 if c.dtype == "f32" else 1) and max(x["dQ"], x["dV"]) <= 1, (c.id, x)
            caught_on("dK", A.check_tent, StandIn("bwd_p_without_scale_on_dk", rounded=rounded), c, A.CASES.index(c))
