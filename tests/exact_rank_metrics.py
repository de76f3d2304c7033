"""The rule of the device ranking metrics in numpy, in this file's own words, and the case table both test layers walk
(tests/test_exact_rank_metrics_harness_cpu.py proves the rule against torch.sort and the reference's fixture on the CPU;
tests/test_rank_metrics_exact_gpu.py holds the kernel to the rule bit for bit).

The rule (include/gstvd_hip.h is the authority for the kernel; this is the same statement made independently):
  * order of keys: fp32 comparison, except that NaN is above everything and equal to NaN, and -0.0 == +0.0;
    rank[i] = 1 + #{j : key_j > key_i} + #{j < i : key_j == key_i}          -- ranks by COUNTING, no sort is called here;
  * gt_rank = rank[gt] for 0 <= gt < O, else 0 (counted as skipped, the histogram unchanged);
  * NDCG of a list with relevance row rel: k = #{rel != 0}; dcg = sum_{p<k} rel[option of rank p+1] / discounts[p]; ideal = the same
    with the options ranked by rel itself; every term one fp32 division, the terms added in ascending p as Python floats
    (float64, sequentially), each sum rounded to fp32, the ratio one fp32 division; k = 0 gives NaN;
  * the accumulator: Python ints for every count and for the histogram, and ndcg_sum a Python float that gains, per call, the
    sequential float64 sum of the call's finite ratios in ascending list order.
"""
import math

import numpy as np

MAX_OPTIONS = 128
N_SPARSE, N_GT_SKIPPED, N_NDCG, N_NDCG_EMPTY, N_REL_SKIPPED, N_CALLS, NDCG_SUM, HIST = 0, 1, 2, 3, 4, 5, 6, 8
ACC_SLOTS = HIST + MAX_OPTIONS + 1

O_VALUES = (1, 2, 63, 64, 65, 100, 127, 128)        # the lane-ownership boundaries (a lane owns options i and i + 64)
L_VALUES = (1, 3, 4, 5, 257)                        # the wave, workgroup (4 lists) and tail-launch (64 ratios a pass) boundaries


def ranks_rule(x):
    """x fp32 [L, O] -> int64 [L, O] ranks by counting."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    a, b = x[:, :, None], x[:, None, :]                                   # a = key_j (axis 1), b = key_i (axis 2)
    na, nb = nan[:, :, None], nan[:, None, :]
    with np.errstate(invalid="ignore"):
        greater = (na & ~nb) | (~na & ~nb & (a > b))
        equal = (na & nb) | (~na & ~nb & (a == b))
    o = x.shape[1]
    before = np.arange(o)[:, None] < np.arange(o)[None, :]                # j < i
    return (1 + greater.sum(1) + (equal & before[None]).sum(1)).astype(np.int64)


def _dcg(rel, order, k, discounts):
    s = 0.0
    for p in range(k):
        s += float(np.float32(rel[order[p]]) / np.float32(discounts[p]))
    return np.float32(s)


def ndcg_rule(ranks_row, rel, discounts):
    """One list: its ranks [O] and its relevance row [O] -> (fp32 ratio, k)."""
    rel = np.asarray(rel, dtype=np.float32)
    k = int((rel != 0).sum())
    if k == 0:
        return np.float32(np.nan), 0
    by_score = np.argsort(ranks_row, kind="stable")                        # ranks are a permutation: position p -> option
    by_rel = np.argsort(ranks_rule(rel[None])[0], kind="stable")
    with np.errstate(all="ignore"):
        return np.float32(_dcg(rel, by_score, k, discounts) / _dcg(rel, by_rel, k, discounts)), k


def empty_acc():
    return {"slots": [0] * ACC_SLOTS, "ndcg_sum": 0.0}


def run_rule(case, acc=None):
    """A case -> dict(ranks [L, O], gt_rank [L] or None, ndcg [L] or None, k [L]); `acc` (empty_acc()) is added to in place."""
    x = case["scores"]
    n, o = x.shape
    ranks = ranks_rule(x)
    out = {"ranks": ranks, "gt_rank": None, "ndcg": None, "k": np.zeros(n, dtype=np.int64)}
    slots = acc["slots"] if acc is not None else [0] * ACC_SLOTS
    slots[N_CALLS] += 1
    if case["gt_index"] is not None:
        out["gt_rank"] = np.zeros(n, dtype=np.int32)
        for l, g in enumerate(case["gt_index"].tolist()):
            if 0 <= g < o:
                r = int(ranks[l, g])
                out["gt_rank"][l] = r
                slots[N_SPARSE] += 1
                slots[HIST + r] += 1
            else:
                slots[N_GT_SKIPPED] += 1
    if case["relevance"] is not None:
        rel, idx = case["relevance"], case["rel_index"]
        out["ndcg"] = np.full(n, np.nan, dtype=np.float32)
        total = 0.0
        for l in range(n):
            r = l if idx is None else int(idx[l])
            if not 0 <= r < rel.shape[0]:
                if r != -1:
                    slots[N_REL_SKIPPED] += 1
                continue
            q, k = ndcg_rule(ranks[l], rel[r], case["discounts"])
            out["ndcg"][l], out["k"][l] = q, k
            if math.isfinite(float(q)):
                slots[N_NDCG] += 1
                total += float(q)
            else:
                slots[N_NDCG_EMPTY] += 1
        if acc is not None:
            acc["ndcg_sum"] = acc["ndcg_sum"] + total
    return out


# ------------------------------------------------------------------------------------------------------------ the case table
SCORE_PATTERNS = ("distinct", "all_equal", "tie_63_64", "zeros", "nan", "inf", "few_values")
REL_PATTERNS = ("all_zero", "one", "all", "tied", "tiny")


def _scores(rng, o, pattern, l):
    x = rng.permutation(4 * o)[:o].astype(np.float32) * np.float32(0.25) - np.float32(o / 2)         # distinct, exact
    if pattern == "all_equal":
        x[:] = np.float32(0.75)
    elif pattern == "tie_63_64":                       # tied pairs across the two owned options of a lane and across lanes 63 / 0
        for a, b in ((63, 64), (0, 64), (62, 127), (1, o - 1), (0, o // 2)):
            if a < o and b < o:
                x[b] = x[a]
    elif pattern == "zeros":                           # +0 and -0 are one key; small values around them
        x[:: 2] = np.float32(0.0)
        x[1:: 4] = np.float32(-0.0)
    elif pattern == "nan":                             # NaN in 1..3 places
        for i in rng.permutation(o)[: 1 + l % 3]:
            x[i] = np.float32(np.nan)
    elif pattern == "inf":
        pick = rng.permutation(o)
        x[pick[0]] = np.float32(np.inf)
        if o > 1:
            x[pick[1]] = np.float32(-np.inf)
        if o > 3:
            x[pick[2]], x[pick[3]] = np.float32(np.inf), np.float32(np.nan)
    elif pattern == "few_values":                      # what bf16 scoring and saturated probabilities look like: many ties
        x = rng.randint(0, 4, o).astype(np.float32)
    return x


def _relevance(rng, o, pattern):
    r = np.zeros(o, dtype=np.float32)
    if pattern == "one":
        r[rng.randint(o)] = np.float32(0.6)
    elif pattern == "all":
        r[:] = (rng.randint(1, 6, o) / 5.0).astype(np.float32)
    elif pattern == "tied":
        r[:] = rng.choice(np.asarray([0.0, 0.2, 0.4], dtype=np.float32), o)
        r[0] = np.float32(0.4)
    elif pattern == "tiny":                            # 2^-20 beside 1.0: lost in an fp32 running sum, kept by the float64 one
        r[rng.permutation(o)[: max(1, o // 2)]] = np.float32(2.0 ** -20)
        r[rng.randint(o)] = np.float32(1.0)
    return r


def discounts_host(o):
    """The uploaded discounts, computed the way the product does: on the host, in torch, once per O."""
    import torch
    return torch.log2(torch.arange(o).float() + 2).numpy()


def make_case(cid, o, n, seed, rel_mode="null", with_gt=True, strides=None):
    """rel_mode: None (no relevance) | "null" (rel_index NULL, one row per list) | "mixed" (-1, out of range both ways, two lists
    naming one row).  strides: None or (scores, ranks, relevance) row strides in elements."""
    rng = np.random.RandomState(seed)
    x = np.stack([_scores(rng, o, SCORE_PATTERNS[(l + seed) % len(SCORE_PATTERNS)], l) for l in range(n)])
    gt = None
    if with_gt:
        edge = (0, o - 1, -1, o)
        gt = np.asarray([edge[(l + seed) % 4] if (l + seed) % 3 else rng.randint(o) for l in range(n)], dtype=np.int64)
    rel = idx = None
    if rel_mode is not None:
        n_rel = n if rel_mode == "null" else max(2, (n + 1) // 2)
        rel = np.stack([_relevance(rng, o, REL_PATTERNS[(r + seed) % len(REL_PATTERNS)]) for r in range(n_rel)])
        if rel_mode == "mixed":
            idx = rng.randint(0, n_rel, n).astype(np.int32)
            for l, v in zip(range(n), (-1, n_rel, 0, 0, -2, 2 ** 31 - 1)):      # lists 2 and 3 name row 0 both
                idx[(l + seed) % n] = v
    return dict(id=cid, scores=x, gt_index=gt, relevance=rel, rel_index=idx, discounts=discounts_host(o), strides=strides)


def _table():
    cases, seed = [], 0
    for o in O_VALUES:
        for n in L_VALUES:
            seed += 1
            cases.append(make_case("O%d_L%d_%s" % (o, n, "mixed" if seed % 2 else "null"), o, n, seed, "mixed" if seed % 2 else "null"))
    cases.append(make_case("strided_O100_L5", 100, 5, 101, "mixed", strides=(160, 131, 107)))
    cases.append(make_case("strided_O65_L9_null", 65, 9, 102, "null", strides=(65, 200, 128)))
    cases.append(make_case("no_gt_O100_L6", 100, 6, 103, "null", with_gt=False))
    cases.append(make_case("no_rel_O100_L6", 100, 6, 104, None))
    cases.append(make_case("ranks_only_O128_L7", 128, 7, 105, None, with_gt=False))
    return cases


CASES = _table()
CASE_IDS = [c["id"] for c in CASES]
