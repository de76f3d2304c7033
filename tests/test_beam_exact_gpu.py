"""The two beam-search kernels alone (gstvd_beam_step, gstvd_beam_reorder) against a float64 host restatement of the step rule
and `index_select`, with canaries around everything they write.

Inputs of the step are integer multiples of 1/8 in a small range (exact in bf16 and fp32): a background in [-6, -2] and twelve
distinct larger values in [0, 4] per row, so the best continuations of a beam differ by >= 1/8 and only the log-sum-exp carries
rounding.  Apart from the designed ties the float64 reference's gap between the K-th and the (K+1)-th candidate is >= 1e-3 in
every case (three orders above the fp32 rounding of a log-sum-exp over 30 522 terms): the seed of a case is advanced on the CPU
until the reference says so.  tok / parent / done are compared bit for bit, scores within 1e-5."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS, PAD = 102, 0
CANARY_I, CANARY_F = -7777, 1234.5
GAP = 1e-3
NEG = -float("inf")


def ref_step(z, s, done, K):
    """The step rule in float64.  z [B*K, V], s [B, K], done [B, K] (numpy) -> tok, parent, score, done [B, K] and the smallest
    gap between the K-th and the (K+1)-th candidate of any dialog row (inf where a row has only K candidates)."""
    B = s.shape[0]
    V = z.shape[1]
    tok, par = np.zeros((B, K), np.int64), np.zeros((B, K), np.int32)
    sc, dn = np.zeros((B, K), np.float64), np.zeros((B, K), np.int32)
    gap = float("inf")
    for b in range(B):
        cands = []
        for j in range(K):
            if done[b, j]:
                cands.append((-s[b, j], j, PAD))
                continue
            row = z[b * K + j].astype(np.float64)
            m = row.max()
            score = s[b, j] + ((row - m) - np.log(np.exp(row - m).sum()))
            order = np.lexsort((np.arange(V), -score))[:K + 1]               # score descending, then v ascending
            cands += [(-score[v], j, int(v)) for v in order]
        cands.sort()
        if len(cands) > K:
            g = cands[K][0] - cands[K - 1][0]
            gap = min(gap, 0.0 if np.isnan(g) else g)                           # (-inf against -inf: a tie)
        for i, (neg, j, v) in enumerate(cands[:K]):
            tok[b, i], par[b, i], sc[b, i], dn[b, i] = v, j, -neg, int(bool(done[b, j]) or v == EOS)
    return tok, par, sc, dn, gap


def make_rows(rng, n, V):
    z = rng.integers(-48, -15, size=(n, V)).astype(np.float64) / 8.0            # [-6, -2]
    for r in range(n):
        pos = rng.choice(V, size=12, replace=False)
        z[r, pos] = rng.choice(np.arange(0, 33), size=12, replace=False) / 8.0  # distinct values in [0, 4]
    return z


def make_state(rng, B, K):
    """Row 0: the state in front of the first step; row 1: some beams done (K > 1); row 2: every beam done.  B = 1: row kind 1."""
    s = -rng.choice(np.arange(0, 49), size=(B, K), replace=False if B * K <= 49 else True) / 8.0
    done = np.zeros((B, K), np.int32)
    kinds = [1] if B == 1 else [0, 1, 2][:B]
    for b, kind in enumerate(kinds):
        if kind == 0:
            s[b, 1:], s[b, 0] = NEG, 0.0
        elif kind == 1 and K > 1:
            d = rng.permutation(K)[:rng.integers(1, K)]
            done[b, d] = 1
        elif kind == 2:
            done[b] = 1
    return s, done


def run_step(z, s, done, K, dtype, ld=None):
    """Runs the kernel inside canaries and returns (tok, parent, score, done) after checking every write window."""
    from gst_visdial_amd import ops
    B, V = s.shape[0], z.shape[1]
    ld = V if ld is None else ld
    lg = torch.full((B * K, ld), 77.0, dtype=dtype, device=DEV)                 # (columns >= V: large, must never be read)
    lg[:, :V] = torch.from_numpy(z).to(DEV, dtype)
    assert torch.equal(lg[:, :V].double().cpu(), torch.from_numpy(z))           # the inputs are exact in `dtype`
    s_in, d_in = torch.from_numpy(s).float().to(DEV), torch.from_numpy(done).to(DEV)
    pad = 8
    guard = {n: torch.full((B * K + 2 * pad,), c, dtype=t, device=DEV)
             for n, c, t in (("s", CANARY_F, torch.float32), ("d", CANARY_I, torch.int32), ("p", CANARY_I, torch.int32))}
    view = {n: g[pad:pad + B * K].view(B, K) for n, g in guard.items()}
    positions, pos, stride = 4, 2, B * K + 3
    ids = torch.full((positions, stride), CANARY_I, dtype=torch.long, device=DEV)
    ws = ops.beam_workspace(B, K, DEV)
    keep = (lg.clone(), s_in.clone(), d_in.clone())
    ops.beam_step(lg[:, :V], s_in, d_in, view["s"], view["d"], view["p"], ids, pos, ws, EOS, PAD)
    torch.cuda.synchronize()
    assert torch.equal(lg.view(torch.int16 if dtype is torch.bfloat16 else torch.int32), keep[0].view(torch.int16 if dtype is torch.bfloat16 else torch.int32))
    assert torch.equal(s_in, keep[1]) and torch.equal(d_in, keep[2])
    for n, g in guard.items():                                                   # canaries in front of and behind every output
        c = CANARY_F if n == "s" else CANARY_I
        assert (g[:pad] == c).all() and (g[pad + B * K:] == c).all(), n
    assert (ids[pos, B * K:] == CANARY_I).all()                                  # the unused columns of the time-major id row
    assert (ids[:pos] == CANARY_I).all() and (ids[pos + 1:] == CANARY_I).all()   # the other positions of the id buffer
    return ids[pos, :B * K].view(B, K).cpu().numpy(), view["p"].cpu().numpy(), view["s"].cpu().numpy(), view["d"].cpu().numpy()


def compare(got, want):
    tok, par, sc, dn = got
    rt, rp, rs, rd, _ = want
    assert np.array_equal(tok, rt), (tok, rt)
    assert np.array_equal(par, rp), (par, rp)
    assert np.array_equal(dn, rd), (dn, rd)
    inf = np.isinf(rs)
    assert np.array_equal(np.isinf(sc) & (sc < 0), inf)
    print("max |score - float64| = %.3e" % (np.abs(sc[~inf] - rs[~inf]).max() if (~inf).any() else 0.0))
    assert np.all(np.abs(sc[~inf] - rs[~inf]) < 1e-5)


VOCABS = {600: 600, 1025: 1025, 30522: 30528}                                   # V -> ld (30528: the engine's padded LM-head width)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("V", [600, 1025, 30522])
def test_beam_step_matches_the_float64_rule(V, K, B, dtype):
    for seed in itertools.count(1000 * V + 10 * K + B):                          # chosen on the CPU: the first seed with a clear gap
        rng = np.random.default_rng(seed)
        z = make_rows(rng, B * K, V)
        s, done = make_state(rng, B, K)
        want = ref_step(z, s, done, K)
        if want[4] >= GAP:
            break
    assert want[4] >= GAP
    compare(run_step(z, s, done, K, dtype, VOCABS[V]), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [600, 1025])
def test_equal_logits_inside_a_beam_order_by_token(V, dtype):
    K = 5
    rng = np.random.default_rng(V)
    z = rng.integers(-48, -15, size=(K, V)).astype(np.float64) / 8.0
    z[0, [400, 17, 333, 5]] = 3.0                                                # four equal best continuations
    z[0, 250], z[0, 90] = 2.5, 1.0                                               # the fifth, clear of the sixth
    s = np.array([[0.0] + [NEG] * (K - 1)])
    want = ref_step(z, s, np.zeros((1, K), np.int32), K)
    assert want[0].tolist() == [[5, 17, 333, 400, 250]] and want[4] >= GAP
    compare(run_step(z, s, np.zeros((1, K), np.int32), K, dtype), want)
    # every live beam: the tie sits at the K-th place -- of the equal (score, v = 7) and (score, v = 9) only the smaller v goes through
    z2 = rng.integers(-48, -15, size=(2, V)).astype(np.float64) / 8.0
    z2[0, [9, 7]] = 3.0
    z2[1] = -6.0
    z2[1, 3] = 0.0
    s2 = np.array([[0.0, -20.0]])
    want = ref_step(z2, s2, np.zeros((1, 2), np.int32), 2)
    assert want[0].tolist() == [[7, 9]] and want[1].tolist() == [[0, 0]]
    compare(run_step(z2, s2, np.zeros((1, 2), np.int32), 2, dtype), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [600, 1025])
def test_identical_beam_rows_with_identical_scores_order_by_beam(V, dtype):
    K = 3
    rng = np.random.default_rng(V + 1)
    z = make_rows(rng, K, V)
    z[1] = z[0]
    s = np.array([[-1.5, -1.5, -30.0]])
    want = ref_step(z, s, np.zeros((1, K), np.int32), K)
    v1, v2 = np.argsort(-z[0], kind="stable")[:2]
    # (0, v1) = (1, v1) > (0, v2) = (1, v2): the K = 3 places go to beam 0, beam 1, beam 0 -- the tie at the boundary to the smaller j
    assert want[0].tolist() == [[v1, v1, v2]] and want[1].tolist() == [[0, 1, 0]] and want[4] == 0.0
    compare(run_step(z, s, np.zeros((1, K), np.int32), K, dtype), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [600, 1025])
@pytest.mark.parametrize("done_first", [True, False])
def test_a_done_beams_frozen_score_ties_with_a_live_candidate(V, dtype, done_first):
    K = 3
    rng = np.random.default_rng(V + 2)
    z = make_rows(rng, K, V)
    live, dead = (1, 0) if done_first else (0, 1)
    z[live] = -80.0
    z[live, 77] = 40.0                                                           # one dominant logit: logp[77] is exactly 0
    s = np.array([[-1.0, -1.0, -3.0]])
    done = np.zeros((1, K), np.int32)
    done[0, dead] = 1
    want = ref_step(z, s, done, K)
    assert want[2][0, 0] == -1.0 and want[2][0, 1] == -1.0                       # an exact tie in float64, decided by j
    assert want[1][0, :2].tolist() == [0, 1]
    assert want[0][0, :2].tolist() == ([PAD, 77] if done_first else [77, PAD])
    assert want[3][0, :2].tolist() == ([1, 0] if done_first else [0, 1])
    got = run_step(z, s, done, K, dtype)
    compare(got, want)
    assert got[2][0, 0] == -1.0 and got[2][0, 1] == -1.0                         # ... and exact on the device


def test_eos_marks_the_new_beam_done():
    K, V = 2, 600
    rng = np.random.default_rng(5)
    z = make_rows(rng, K, V)
    z[0, EOS] = 6.0                                                              # beam 0's best continuation ends it
    s = np.array([[-0.5, -0.75]])
    want = ref_step(z, s, np.zeros((1, K), np.int32), K)
    assert want[0][0, 0] == EOS and want[3][0].tolist() == [1, 0]
    compare(run_step(z, s, np.zeros((1, K), np.int32), K, torch.float32), want)


# ---- cache reorder --------------------------------------------------------------------------------------------------------------
def _parents(kind, B, K, gen):
    if kind == "identity":
        return torch.arange(K).repeat(B, 1)
    if kind == "all_to_one":
        return torch.full((B, K), K - 1)
    if kind == "reversal":                                                       # the case an in-place copy gets wrong
        return torch.arange(K - 1, -1, -1).repeat(B, 1)
    return torch.randint(0, K, (B, K), generator=gen)                           # random with repeats


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("B,K", [(2, 5), (3, 1), (1, 8)])
def test_beam_reorder_moves_exactly_the_kv_columns_of_the_surviving_beams(B, K, H, dtype):
    from gst_visdial_amd import ops
    L, Umax, rows = 2, 7, B * K
    gen = torch.Generator().manual_seed(B * 100 + K)
    n = (rows + 2) * Umax * 3 * H
    bits = torch.int32 if dtype is torch.float32 else torch.int16

    def pattern(offset):
        # a distinct integer per element: exact in fp32 (< 2^24); for bf16 the 16-bit pattern of the element (compared as bits)
        a = torch.arange(n, dtype=torch.int64) + offset
        if dtype is torch.float32:
            return a.float().view(rows + 2, Umax, 3 * H).to(DEV)
        return (a % 65521 - 32760).to(torch.int16).view(torch.bfloat16).view(rows + 2, Umax, 3 * H).to(DEV)

    for t, kind in itertools.product((0, 3, 6), ("identity", "all_to_one", "reversal", "random")):
        parent = _parents(kind, B, K, gen).to(torch.int32).to(DEV)
        src_g = [pattern(l * 7) for l in range(L)]                                # guard rows: one cache row before and after
        dst_g = [pattern(1000003 + l * 11) for l in range(L)]
        src, dst = [x[1:-1] for x in src_g], [x[1:-1] for x in dst_g]
        want = [x.clone() for x in dst_g]
        pick = (torch.arange(B, device=DEV)[:, None] * K + parent.long()).view(-1)
        for l in range(L):
            want[l][1:-1, :t + 1, H:] = src[l].index_select(0, pick)[:, :t + 1, H:]
        src_before = [x.clone() for x in src_g]
        ops.beam_reorder(src, dst, parent, t, H)
        torch.cuda.synchronize()
        for l in range(L):
            # K | V columns of positions <= t: index_select exactly; Q columns, later positions, guard rows: as before
            assert torch.equal(dst_g[l].view(bits), want[l].view(bits)), (t, kind, l)
            assert torch.equal(src_g[l].view(bits), src_before[l].view(bits)), (t, kind, l)
