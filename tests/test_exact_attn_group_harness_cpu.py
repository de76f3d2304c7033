"""The harness of the grouped cross-attention backward (tests/exact_attn_group.py) proved on the CPU: a stand-in for
gstvd_attn_fwd / gstvd_attn_group_bwd / gstvd_attn_bwd written in plain torch with the kernels' conventions (mask and K / V of row
b / G, draws indexed by the query row over round4(Lk), factor 1 / (1 - p), delta from the stored O, dK / dV summed over the group
and written once).  Every check passes on it, and each deliberately wrong stand-in -- the mask taken from the query row, the last
group member dropped, the draws indexed by the K / V row -- is caught.  (Torch functions on the CPU; nothing here touches a GPU.)"""
import pytest
import torch

import exact_attn_group as X

A = X.A
DEV = torch.device("cpu")
MUTANTS = ("mask_of_query_row", "last_member_dropped", "draws_of_kv_row", "row_not_written", "writes_when_refusing",
           "dk_zero", "dk_first_member_only")


class StandIn(object):
    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.device, self.mutant = DEV, mutant

    def _draws(self, c):
        Lkp = A.round4(c.Lk)
        n = c.B * c.nh * c.Lq * Lkp
        return (torch.rand(n, generator=torch.Generator().manual_seed(99)) >= c.p).view(c.B, c.nh, c.Lq, Lkp)[..., :c.Lk]

    def keep(self, p):
        return self._draws(p.c)

    def run_plain(self, p):
        assert p.c.kv_group == 1
        self._run(p, None)

    def run(self, p):
        self._run(p, self.mutant)

    def _run(self, p, mu):
        c = p.c
        G, Bkv = c.kv_group, c.B // c.kv_group
        Q, K, V = p.t("Q").double(), p.t("K").double().repeat_interleave(G, 0), p.t("V").double().repeat_interleave(G, 0)
        sc = p.scale
        al = torch.ones(c.B, 1, c.Lq, c.Lk, dtype=torch.bool)
        if p.km is not None:
            row = torch.arange(c.B) % Bkv if mu == "mask_of_query_row" else torch.arange(c.B) // G
            al = al & (p.km[row] != 0)[:, None, None, :]
        s = torch.einsum("bqhd,bkhd->bhqk", Q, K) * sc + torch.where(al, 0.0, c.neg).double()
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        P = e / l
        f = torch.ones_like(P)
        if c.p > 0:
            keep = self._draws(c)
            if mu == "draws_of_kv_row":
                keep = keep[torch.arange(c.B) // G]
            f = keep.double() / (1.0 - c.p)
        Pd = P * f
        O = torch.einsum("bhqk,bkhd->bqhd", e * f, V) * (1.0 / l).squeeze(-1).permute(0, 2, 1)[..., None]
        p.t("O").copy_(O.float())
        p.t("LSE").copy_((m + torch.log(l)).squeeze(-1).float())
        dO = p.t("dO").double()
        delta = (dO * p.t("O").double()).sum(-1).permute(0, 2, 1)
        dS = P * (torch.einsum("bqhd,bkhd->bhqk", dO, V) * f - delta[..., None]) * sc
        dV, dK = torch.einsum("bhqk,bqhd->bkhd", Pd, dO), torch.einsum("bhqk,bqhd->bkhd", dS, Q)
        if mu == "last_member_dropped" and G > 1:
            live = (torch.arange(c.B) % G != G - 1)[:, None, None, None]
            dV, dK = dV * live, dK * live
        if mu == "dk_first_member_only":                         # dK (not dV) keeps the first member's part only
            dK = dK * (torch.arange(c.B) % G == 0)[:, None, None, None]
        dVs, dKs = X.group_sum(dV, G).float(), X.group_sum(dK, G).float()
        if mu == "dk_zero":
            dKs = dKs * 0
        if mu == "row_not_written":
            dVs[-1, -1] = p.t("dV")[-1, -1].float()
        p.t("dV").copy_(dVs)
        p.t("dK").copy_(dKs)
        p.t("dQ").copy_(torch.einsum("bhqk,bkhd->bqhd", dS, K).float())
        p.t("delta").copy_(delta.float())

    def refuse(self, p, null=None, **change):
        if self.mutant == "writes_when_refusing":
            p.t("delta")[0, 0, 0] = 0.0


SMALL = [c for c in X.CASES if c.d == 32 or (c.d == 64 and c.Lk <= 70)]
EXACT = [c._replace(p=0.5 if c.p else 0.0) for c in SMALL]


def ids(cs):
    return [c.id for c in cs]


def caught(check, *a, **kw):
    with pytest.raises(AssertionError):
        check(*a, **kw)


def test_the_table_holds_what_the_issue_names():
    assert len(set(c.id for c in X.CASES)) == len(X.CASES) == 60
    for dt in ("bf16", "f32"):
        for d in (32, 64, 128):
            mine = [c for c in X.CASES if c.dtype == dt and c.d == d]
            assert set((c.B, c.kv_group, c.nh, c.Lq, c.Lk) for c in mine) == set(X.SHAPES)
            for shp in X.SHAPES:
                assert set(c.p for c in mine if (c.B, c.kv_group, c.nh, c.Lq, c.Lk) == shp) == {0.0, 0.1}
    assert not any(A.ATTN_KERNEL_RE.search(("_Z10" + X.kernel_of(c)).encode()) for c in X.CASES)
    # the shape of the group-of-one comparison is not one the one-pass backward claims
    assert all(not (64 < c.Lk <= 256 and c.Lq >= 64) for c in X.CASES if c.kv_group == 1)


@pytest.mark.parametrize("c", SMALL, ids=ids(SMALL))
def test_standin_passes_the_comparisons(c):
    be, i = StandIn(), X.CASES.index(c)
    if c.kv_group == 1:
        X.check_group_of_one(be, c, i)
    X.check_dq_matches_replicated(be, c, i)
    X.check_dkv(be, c, i)


@pytest.mark.parametrize("c", EXACT, ids=ids(EXACT))
def test_standin_passes_the_exact_families(c):
    be, i = StandIn(), EXACT.index(c)
    X.check_onehot(be, c, i)
    X.check_uniform(be, c, i)
    X.check_uniform_dk(be, c, i)
    if c.B // c.kv_group >= 2:
        X.check_all_masked_row(be, c, i)


def test_disjoint_columns_promise_a_bit_exact_grouped_dk_in_both_types():
    """disjoint_must_be_exact is not vacuous: groups of two, three and four members with a bit-exact dK in fp32 and in bf16, and check_uniform_dk
    (which asserts the promise itself) keeps it on the stand-in."""
    for dt in ("f32", "bf16"):
        mine = [c for c in EXACT if c.dtype == dt and X.disjoint_must_be_exact(c) == "exact"]
        assert {2, 3, 4} <= set(c.kv_group for c in mine), dt
        for c in mine:
            assert X.check_uniform_dk(StandIn(), c, EXACT.index(c)) == "exact"


def test_mutants_of_the_grouped_dk():
    for c in (X.case("bf16", 32, X.SHAPES[0]), X.case("f32", 64, X.SHAPES[1], p=0.5), X.case("f32", 32, X.SHAPES[2])):
        X.check_uniform_dk(StandIn(), c, 0)
        X.check_uniform(StandIn("dk_zero"), c, 0)                                     # family D cannot see it: dK is 0 there
        X.check_uniform(StandIn("dk_first_member_only"), c, 0)
        for mu in ("dk_zero", "dk_first_member_only"):
            with pytest.raises(AssertionError, match="disjoint dK"):
                X.check_uniform_dk(StandIn(mu), c, 0)
        with pytest.raises(AssertionError, match="disjoint dK|disjoint dV"):   # (dV is compared first, and is wrong too)
            X.check_uniform_dk(StandIn("last_member_dropped"), c, 0)


DRAWS = [X.case("bf16", 32, X.SHAPES[0], p=0.5), X.case("f32", 64, X.SHAPES[1], p=0.5)]


@pytest.mark.parametrize("c", DRAWS, ids=ids(DRAWS))
def test_standin_passes_the_dropout_mask_recovery_and_the_refusals(c):
    X.check_dropout_masks(StandIn(), c, 0)
    X.check_refusals(StandIn(), c, 0)


# ---------------------------------------------------------------------------------------------- mutants

def test_mutant_mask_taken_from_the_query_row():
    for c in (X.case("bf16", 32, X.SHAPES[1], p=0.1), X.case("f32", 64, X.SHAPES[0])):
        X.check_dq_matches_replicated(StandIn(), c, 0)
        caught(X.check_dq_matches_replicated, StandIn("mask_of_query_row"), c, 0)      # dQ of rows whose mask is another row's
        caught(X.check_dkv, StandIn("mask_of_query_row"), c, 1)
        caught(X.check_uniform, StandIn("mask_of_query_row"), c._replace(p=0.0), 0)


def test_mutant_last_group_member_dropped():
    for c in (X.case("bf16", 32, X.SHAPES[0]), X.case("f32", 32, X.SHAPES[2], p=0.1), X.case("f32", 64, X.SHAPES[4])):
        caught(X.check_dkv, StandIn("last_member_dropped"), c, 0)
        e = c._replace(p=0.5 if c.p else 0.0)
        caught(X.check_onehot, StandIn("last_member_dropped"), e, 0)
        caught(X.check_uniform, StandIn("last_member_dropped"), e, 0)
    caught(X.check_dropout_masks, StandIn("last_member_dropped"), DRAWS[0], 0)


def test_mutant_draws_indexed_by_the_key_row():
    for c in DRAWS:
        caught(X.check_dropout_masks, StandIn("draws_of_kv_row"), c, 0)
    c = X.case("bf16", 32, X.SHAPES[1], p=0.1)
    caught(X.check_dq_matches_replicated, StandIn("draws_of_kv_row"), c, 0)
    caught(X.check_onehot, StandIn("draws_of_kv_row"), c._replace(p=0.5), 0)


def test_mutant_a_key_row_never_written_and_a_write_while_refusing():
    c = X.case("f32", 32, X.SHAPES[1])
    with pytest.raises(AssertionError, match="NaN"):
        X.check_dkv(StandIn("row_not_written"), c, 0)
    caught(X.check_refusals, StandIn("writes_when_refusing"), c, 0)
