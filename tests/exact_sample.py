"""Exact layer of the sampling tests: kept sets known in float64, a probe in every CDF interval and on its steps.

gstvd_sample_topk (csrc/sample.hip) draws ONE id per row, so a test that draws at a random uniform sees a wrong kept set only when
u falls into the affected tail.  Here one launch holds B <= 64 copies of one row with B chosen uniforms:

  midpoints   u at the float64 midpoint of a kept token's CDF interval: the id must be exactly that token.  The intervals partition
              [0, 1), so one token too many, one missing or one wrong shifts the midpoints.
  steps       the fp32 value nearest a CDF step and its two fp32 neighbours: the id must be the kept token that ends at the step
              or the next kept token, never anything else (a filtered or banned token in particular).
  ends        u = 2^-24 gives the first kept token, u = 1 - 2^-24 the last one (not the clamp's V - 1).

Reference: float64 on the CPU, the rule of include/gstvd_hip.h.  z = fp32(logit) / fp32(temperature) as an fp32 division (that the
device rounds it the same way is a PREMISE; the division-tie rows assert it); banned and n-gram-banned tokens (the mask comes from
decoding._ngram_blocking_loop) -> -inf; top-k by value (ties with the k-th value stay; top_k >= V or 0: off); top-p by value on
what top-k left (a token stays iff the mass of the strictly larger logits is <= top_p; 0 or >= 1: off).

Rows.  Tie rows: every kept token carries the row maximum, the weights are __expf(0) == 1 (a premise: premise_case() asserts it by name,
every tie case relies on it), all partial sums are integers below 2^24; with n = 2^m kept tokens and u = j / n the draw is known
bit for bit on the steps too (the j-th kept token; its upper neighbour gives the next one).  Level rows: a few distinct levels with
chosen multiplicities, dealt onto an explicit index pattern.  Noise rows: Gaussian logits, fp32 and bf16 (many ties).

Conditions on the inputs, asserted in float64 by reference() for every row, never skipped on: every kept token has probability
>= 2^-10 (a token whose weight underflows -- 150 or more below the maximum -- counts as probability 0 and must never be drawn) and
the mass in front of every distinct level differs from top_p by >= 2^-10.  The kernel's CDF error is about 60 fp32 roundings plus
__expf, below 1e-5 relative: two orders of magnitude inside these margins, so no tolerance on the kernel's arithmetic is needed.

Placement.  Kept tokens, the k-th value, its ties and the banned maximum sit on the borders of BOTH layouts of the kernel: the
strided one (i = tid + 1024 j: 0, 1023 / 1024, V - 1, the last partial stripe) and the contiguous one of the inverse CDF
([t seg, (t + 1) seg) with seg = ceil(V / 1024) | 1: t seg - 1 and t seg, the wave borders 64 seg w, the last thread that owns
anything), with runs of zero-weight tokens that span many threads in between.

Windows.  logits: ld = V + pad, NaN in the padding and around the allocation (+inf in column V for V = 1025 and 30522: a kernel
built on compares steps over a NaN, not over an infinity); banned: banned_ld > V, padding True; out: a strided
column of a canary-filled id buffer; u, hist and ids_tm inside poisoned allocations (hist: a kept, non-special id, and every history ends with the
generated prefix, so a window read past hist_T bans that id; ids_tm: an id that matches nothing).  An all-banned row returns id 0 (total = 0, nothing is counted; the reference's clamp gives
the same): pinned by all_banned_case().

Plain helper module: no fixtures, no hooks.  Everything takes a backend `be` (be.device, be.sample(...) with the signature of
ops.sample_topk), so tests/test_exact_sample_harness_cpu.py proves it on the CPU against a torch stand-in and fifteen wrong ones
and tests/test_sample_exact_gpu.py runs it on the HIP kernel.

The table (V: route; seg of the contiguous layout in brackets):
  V = 1, 2, 63, 64, 97 [1]   one partial stripe          1023, 1024 [1]   the last one-stripe shapes      1025 [3]   seg 1 -> 3
  2048 [3]   3072 [3], 3073 [5]   seg 3 -> 5             30522 [31]   production                         30720 [31]   even stripes
  31744 [31]   the limit
  top-k iterative k = 1, 2, 7, 16; bisection k = 17, 64, 65, 1000, V - 1; off: 0, V, V + 5
"""
import collections

import numpy as np
import torch

from exact_gemm import BF16, CANARY, F32, Window

NT, NWV, VMAX = 1024, 16, 31 * 1024
MARGIN = 2.0 ** -10
UNDERFLOW = -150.0                      # z - zmax at or below this: weight 0 in fp32 under any exp
SPECIAL = (0, 100, 101, 102, 103)
SPECIAL8 = (0, 5, 100, 101, 102, 103, 7, 9)
DT = {"f32": F32, "bf16": BF16}
U_FIRST, U_LAST = 2.0 ** -24, 1.0 - 2.0 ** -24
NEG = -float("inf")
INF_PAD = (1025, 30522)                 # rows of these V carry +inf instead of NaN in column V of the logits' padding (both dtypes)


def seg_of(V):
    return ((V + NT - 1) // NT) | 1


def edges(V):
    """Indices on the borders of both layouts (see the header), ascending."""
    seg = seg_of(V)
    stripe = (V - 1) // NT * NT
    s = set([0, V - 1, NT - 1, NT, stripe - 1, stripe])
    for t in (1, 2, 63, 64, 65, 511, (V - 1) // seg):                   # thread borders; t = 64: a wave border as well
        s.update((t * seg - 1, t * seg))
    for w in (1, 8, 15):                                               # wave borders of the two-level scan
        s.update((64 * seg * w - 1, 64 * seg * w))
    return sorted(i for i in s if 0 <= i < V)


def positions(V, n, force=()):
    """n distinct indices: `force`, the layout borders (thinned evenly when there are more than n, always with 0 and V - 1), then
    the pattern 11 + 53 i mod V."""
    assert 0 < n <= V
    pos = list(dict.fromkeys(force))
    e = [i for i in edges(V) if i not in pos]
    room = n - len(pos)
    if len(e) > room:
        e = [e[(j * (len(e) - 1)) // max(room - 1, 1)] for j in range(room)] if room > 0 else []
    pos = list(dict.fromkeys(pos + e))
    have = set(pos)
    i = 0
    while len(pos) < n and i < V:
        c = (11 + 53 * i) % V
        if c not in have:
            pos.append(c), have.add(c)
        i += 1
    c = 0
    while len(pos) < n:
        if c not in have:
            pos.append(c), have.add(c)
        c += 1
    return sorted(pos)


_Row = collections.namedtuple("Row", "name V dtype logits T k p ban ngram tie lv")


class Row(_Row):
    """One row.  logits: float32 [V], every value representable in `dtype`; ban: bool [V] or None; ngram: None or a dict
    (hist, ids, cur_len, n, special); tie: the draw is predictable on the steps; lv: the indices of every level (level rows)."""
    __slots__ = ()


def _fits(x, dtype):
    assert bool((x.to(dtype).float() == x).all()), "logits not representable in %s" % dtype
    return x


def level_row(name, V, dtype, levels, fill=(-8.0,), T=1.0, k=0, p=0.0, ban_fill=False, ngram=None, tie=False, force=(), force_lv=2):
    """levels: (value, count) or (value, count, "ban"): dealt round-robin, in index order, onto positions(V, total); every other
    index takes the `fill` values in turn (ban_fill: and is banned by the mask).  p: a number, or ("after", j): the fp32
    midpoint between the mass in front of kept level j and of level j + 1 (float64, from the reference with top-p off).
    ngram: None or f(lv) -> dict.  force: indices that carry level `force_lv` whatever the pattern says."""
    total = sum(l[1] for l in levels)
    pos = positions(V, total, force)
    left = [l[1] for l in levels]
    lv = [[] for _ in levels]
    if force:
        lv[force_lv] = list(force)
        left[force_lv] -= len(force)
        assert left[force_lv] >= 0
    li = 0
    for i in pos:
        if i in force:
            continue
        while left[li % len(levels)] == 0:
            li += 1
        lv[li % len(levels)].append(i)
        left[li % len(levels)] -= 1
        li += 1
    fillv = torch.tensor(fill, dtype=torch.float32)
    lg = fillv[torch.arange(V) % len(fill)].clone()
    ban = torch.zeros(V, dtype=torch.bool)
    if ban_fill:
        ban[:] = True
        ban[torch.tensor(pos)] = False
    for (l, idx) in zip(levels, lv):
        lg[torch.tensor(idx)] = l[0]
        if len(l) > 2 and l[2] == "ban":
            ban[torch.tensor(idx)] = True
    row = Row(name, V, dtype, _fits(lg, DT[dtype]), T, k, 0.0, ban if bool(ban.any()) else None, ngram(lv) if ngram else None, tie, lv)
    if isinstance(p, tuple):
        g = _compute(row).level_front
        j = p[1]
        assert j + 1 < len(g), "%s: no level behind level %d" % (name, j)
        p = float(np.float32((g[j] + g[j + 1]) / 2))
    return row._replace(p=p)


def noise_row(name, V, dtype, seed, T, k, p=0.0, sigma=1.0, nban=0):
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(V, generator=g) * sigma).to(DT[dtype]).float()
    ban = None
    if nban:
        ban = torch.zeros(V, dtype=torch.bool)
        ban[lg.topk(nban).indices[::2]] = True                         # every other one of the largest values, the maximum included
    row = Row(name, V, dtype, lg, T, k, 0.0, ban, None, False, None)
    if isinstance(p, tuple):
        gf = _compute(row).level_front
        p = float(np.float32((gf[p[1]] + gf[p[1] + 1]) / 2))
    return row._replace(p=p)


def division_tie_row(name, V, T, k):
    """Two adjacent fp32 logits a < b whose quotients by T are ONE fp32 value under a true division and two under a multiplication
    by the rounded reciprocal.  b sits k times in the row, a once: by division the k-th value is tied with a and k + 1 tokens stay;
    a kernel that multiplies keeps k.  (The premise of the layer -- both sides round the division alike -- asserted where it can be.)"""
    t = np.float32(T)
    a = (np.float32(1.5) + np.arange(200000, dtype=np.float32) * np.float32(2.0 ** -23)).astype(np.float32)   # (quotients in a coarser binade)
    b = np.nextafter(a, np.float32(4))
    hit = np.nonzero(((a / t) == (b / t)) & ((a * (np.float32(1) / t)) != (b * (np.float32(1) / t))))[0]
    assert len(hit), "no division tie near 1.0 for T = %r" % T
    a, b = float(a[hit[0]]), float(b[hit[0]])
    row = level_row(name, V, "f32", [(b, k), (a, 1)], fill=(0.0, -1.0), T=T, k=k)
    return row


_Ref = collections.namedtuple("Ref", "kept prob cdf level_front margin_prob margin_p nzero")


def ngram_reference(row):
    """bool [V]: the n-gram bans of the row, from decoding._ngram_blocking_loop (ids outside [0, V) land in spare columns)."""
    from gst_visdial_amd import decoding
    g, V = row.ngram, row.V
    hist, ids = list(g["hist"]), list(g["ids"])[:g["cur_len"]]
    W = max([V] + [t + 1 for t in hist]) + 1
    assert all(0 <= t < W - 1 for t in ids), "generated ids must be ordinary tokens"
    hist = [t if t >= 0 else W - 1 for t in hist]
    lg = torch.zeros(1, W)
    out = decoding._ngram_blocking_loop(lg, torch.tensor([hist], dtype=torch.int64).reshape(1, -1), torch.tensor([ids], dtype=torch.int64).reshape(1, -1),
                                        g["n"], special_token_ids=tuple(g["special"] if g["special"] is not None else SPECIAL))
    return (out[0, :V] == NEG).numpy()


_REF = {}


def reference(row):
    """float64 kept set and probabilities of a row, with the input conditions asserted."""
    key = (row.name, row.p)
    if key not in _REF:
        _REF[key] = _compute(row, True)
    return _REF[key]


def _compute(row, check=False):
    V = row.V
    z = (row.logits.numpy().astype(np.float32) / np.float32(row.T)).astype(np.float64)
    dead = np.zeros(V, dtype=bool)
    if row.ban is not None:
        dead |= row.ban.numpy()
    if row.ngram is not None:
        dead |= ngram_reference(row)
    z[dead] = NEG
    keep = z > NEG
    if 0 < row.k < V:
        kth = np.sort(z)[::-1][row.k - 1]
        keep &= z >= kth
    if not keep.any():
        return _Ref(np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0), np.zeros(0), 1.0, 1.0, 0)
    zmax = z[keep].max()
    d = np.where(keep, z - zmax, NEG)
    under = keep & (d <= UNDERFLOW)
    w = np.where(keep & ~under, np.exp(np.where(keep, d, 0.0)), 0.0)
    order = np.argsort(-z, kind="stable")
    zs, ws = z[order], w[order]
    excl = np.cumsum(ws) - ws
    first = np.searchsorted(-zs, -zs, side="left")
    front = (excl[first] / w.sum())                                      # mass of the strictly larger logits, sorted order
    live = (keep & ~under)[order]
    lvl = np.unique(first[live])
    level_front = front[lvl]
    margin_p = 1.0
    if 0.0 < row.p < 1.0:
        margin_p = float(np.abs(level_front - row.p).min())
        stay = np.zeros(V, dtype=bool)
        stay[order] = front <= row.p
        keep &= stay
        w = np.where(keep, w, 0.0)
    kept = np.nonzero(keep & ~under)[0]
    prob = w[kept] / w[kept].sum()
    nzero = int((keep & under).sum())
    assert not check or prob.min() >= MARGIN, "%s: a kept token has probability %.3g < 2^-10" % (row.name, prob.min())
    assert not check or margin_p >= MARGIN, "%s: the mass in front of a level is within %.3g of top_p = %r" % (row.name, margin_p, row.p)
    if row.tie:
        n = len(kept)
        assert n & (n - 1) == 0 and bool((z[kept] == zmax).all()), "%s: a tie row keeps 2^m tokens, all at the maximum" % row.name
        cdf = np.arange(1, n + 1, dtype=np.float64) / n
    else:
        cdf = np.cumsum(prob)
        cdf[-1] = 1.0
    return _Ref(kept, prob, cdf, level_front, float(prob.min()), margin_p, nzero)


def _thin(idx, limit, must):
    """At most `limit` of the ascending list idx: `must` first, the rest evenly."""
    if len(idx) <= limit:
        return list(idx)
    must = [i for i in idx if i in must][:limit // 2]
    rest = [i for i in idx if i not in must]
    room = limit - len(must)
    pick = [rest[(j * (len(rest) - 1)) // (room - 1)] for j in range(room)]
    return sorted(set(must + pick))


def probes(row, kind):
    """(u float32 [B], lo int64 [B], hi int64 [B], what [B]): the id of probe b must be lo[b] or hi[b]."""
    r = reference(row)
    kept, n = r.kept, len(r.kept)
    e = set(edges(row.V))
    near = set(j for j in range(n) if int(kept[j]) in e) | set([0, n - 1])
    u, lo, hi, what = [], [], [], []
    if kind == "mid":
        start = r.cdf - (1.0 / n if row.tie else r.prob)
        for j in _thin(range(n), 62, near):
            m = np.float32((start[j] + r.cdf[j]) / 2)
            assert start[j] + MARGIN / 4 < float(m) < r.cdf[j] - MARGIN / 4
            u.append(m), lo.append(kept[j]), hi.append(kept[j]), what.append("midpoint of kept token %d (id %d)" % (j, kept[j]))
        for uu, j, tag in ((U_FIRST, 0, "u = 2^-24: the first kept token"), (U_LAST, n - 1, "u = 1 - 2^-24: the last kept token")):
            u.append(np.float32(uu)), lo.append(kept[j]), hi.append(kept[j]), what.append(tag)
    else:
        assert kind == "step" and n >= 2
        for j in _thin(range(1, n), 21, set(j for j in range(1, n) if j in near or j - 1 in near)):
            u0 = np.float32(r.cdf[j - 1])
            um, up = np.nextafter(u0, np.float32(0)), np.nextafter(u0, np.float32(1))
            a, b = kept[j - 1], kept[j]
            tag = "step %d between ids %d and %d" % (j, a, b)
            if row.tie:
                assert float(u0) == r.cdf[j - 1]
                exp = ((um, a, a), (u0, a, a), (up, b, b))
            else:
                exp = ((um, a, b), (u0, a, b), (up, a, b))
            for (uu, x, y), side in zip(exp, ("below", "on", "above")):
                u.append(uu), lo.append(x), hi.append(y), what.append("%s, %s it" % (tag, side))
    u = torch.tensor(np.array(u, dtype=np.float32))
    assert len(u) <= 64 and bool(((u > 0) & (u < 1)).all())
    return u, torch.tensor(np.array(lo, dtype=np.int64)), torch.tensor(np.array(hi, dtype=np.int64)), what


# ---------------------------------------------------------------------------------------------- the table
def ng(n, ids, windows, lead=3, special=None, cur_len=None, tail=0, end=()):
    """An n-gram spec: the history is `lead` pads, then every window followed by one pad (id 0, special), then `tail` pads, then
    `end` with NO pad behind it: the generated prefix, so that a window read one column past hist_T matches and bans whatever the
    padding of the allocation holds."""
    hist = [0] * lead
    for w in windows:
        hist += list(w) + [0]
    return dict(hist=hist + [0] * tail + list(end), ids=list(ids), cur_len=len(ids) if cur_len is None else cur_len, n=n, special=special)


LV5 = [(3.0, 1), (2.0, 1), (1.0, 3), (0.0, 4), (-1.0, 8)]              # cumulative 1, 2, 5, 9, 17: k = 7 and 16 cross a tie


def build_rows():
    R = []
    # -- tie rows: n = 2^m kept tokens at the maximum (weights 1, integer sums): every probe exact, the steps included
    R += [level_row("tie-v1", 1, "f32", [(0.5, 1)], tie=True),
          level_row("tie-v2-k1", 2, "bf16", [(-2.0, 2)], k=1, tie=True),                                   # c >= k at the maximum
          level_row("tie-v63-k7-T0.5", 63, "f32", [(1.5, 32)], fill=(1.0, -3.0), T=0.5, k=7, tie=True),
          level_row("tie-v64-all", 64, "bf16", [(-0.0, 64)], tie=True),
          level_row("tie-v1023-k16-T2", 1023, "f32", [(3.0, 16)], fill=(2.5, 0.0, -0.0), T=2.0, k=16, tie=True),
          level_row("tie-v1024-k1000", 1024, "bf16", [(-1.0, 1024)], k=1000, tie=True),                   # c >= k, k > 16: the else-if
          level_row("tie-v1025-k17-maxbanned", 1025, "f32", [(5.0, 3, "ban"), (2.0, 64)], fill=(1.0, -1.0), k=17, tie=True),
          level_row("tie-v3073-underflow-T0.5", 3073, "bf16", [(4.0, 128)], fill=(-96.0,), T=0.5, tie=True),      # 200 below, k = 0
          level_row("tie-v30522-k64", 30522, "bf16", [(2.0, 256)], fill=(1.0, 0.0, -7.0), k=64, tie=True),
          level_row("tie-v31744-rest-banned", 31744, "f32", [(-3.0, 512)], fill=(9.0,), ban_fill=True, tie=True),
          level_row("tie-v30720-p-max-only", 30720, "bf16", [(1.0, 8)], fill=(-6.0,), p=2.0 ** -9, tie=True),      # only the ties at the maximum stay
          level_row("tie-v2048-k2-T2", 2048, "f32", [(6.0, 4)], fill=(5.0, 1.0), T=2.0, k=2, tie=True)]
    # -- iterative top-k (k <= 16): the k-th value tied across k, on four routes
    for (V, dt, T) in ((97, "f32", 1.0), (1025, "bf16", 0.5), (3072, "f32", 2.0), (30522, "bf16", 1.0)):
        for k in (1, 2, 7, 16):
            R.append(level_row("iter-v%d-%s-k%d-T%g" % (V, dt, k, T), V, dt, [(v * T, n) for v, n in LV5], fill=(-2.0 * T, -3.5 * T, -9.0 * T), T=T, k=k))
    R += [level_row("iter-v64-few-finite-k7", 64, "f32", [(1.0, 2), (0.0, 3)], ban_fill=True, k=7),       # fewer than k finite: nothing goes
          level_row("iter-v1024-few-finite-k16", 1024, "bf16", [(1.0, 5), (0.0, 9)], ban_fill=True, k=16),
          level_row("iter-v3073-c-ge-k", 3073, "f32", [(2.0, 9), (1.0, 4)], fill=(0.0,), k=7),             # c >= k at the maximum
          level_row("iter-v30720-max-banned-k7", 30720, "f32", [(4.0, 2, "ban"), (3.0, 1), (2.0, 2), (1.0, 5), (0.0, 4)], fill=(-1.0, -2.0), k=7)]
    # -- bisection (k > 16)
    R += [level_row("bis-v2048-k17-negative", 2048, "f32", [(-1.0, 4), (-2.0, 4), (-3.0, 8), (-4.0, 8)], fill=(-5.0, -6.0, -30.0), k=17),
          level_row("bis-v3073-k64-kth-negative", 3073, "bf16", [(2.0, 10), (1.0, 20), (0.0, 15), (-0.0, 15), (-1.0, 10)], fill=(-2.0, -3.0), k=64),
          level_row("bis-v3073-k50-kth-zero", 3073, "bf16", [(2.0, 10), (1.0, 20), (0.0, 15), (-0.0, 15), (-1.0, 10)], fill=(-2.0, -3.0), k=50),
          level_row("bis-v1024-k65-T0.5", 1024, "f32", [(0.5, 30), (0.0, 30), (-0.5, 10)], fill=(-1.0, -2.0), T=0.5, k=65),
          level_row("bis-v30522-k1000", 30522, "bf16", [(1.0, 600), (0.984375, 401)], fill=(0.5, -1.0), k=1000),
          level_row("bis-v97-k96", 97, "f32", [(1.0, 40), (0.0, 40), (-1.0, 16)], fill=(-2.0,), k=96),
          level_row("bis-v64-k63", 64, "bf16", [(0.0, 20), (-1.0, 30), (-2.0, 13)], fill=(-2.5,), k=63),
          level_row("bis-v1025-c-ge-k64", 1025, "f32", [(1.0, 70), (0.0, 20)], fill=(-1.0,), k=64),
          level_row("bis-v31744-k17-few-finite", 31744, "bf16", [(1.0, 6), (-1.0, 6)], ban_fill=True, k=17),
          # a level ONE float key below the k-th value: a threshold one key low lets it in
          level_row("bis-v2048-k17-key-neighbour", 2048, "f32", [(1.0, 9), (0.5, 8), (float(np.nextafter(np.float32(0.5), np.float32(0))), 6)], fill=(0.0, -1.0), k=17),
          level_row("off-v63-k0", 63, "f32", [(1.0, 20), (0.0, 23), (-1.0, 20)], k=0),
          level_row("off-v64-kV", 64, "bf16", [(1.0, 20), (0.0, 24), (-1.0, 20)], k=64),
          level_row("off-v97-kV+5", 97, "f32", [(1.0, 40), (0.0, 40), (-1.0, 17)], k=102)]
    # -- top-p
    P4 = [(2.0, 2), (1.0, 4), (0.0, 8), (-1.0, 16)]
    R += [level_row("p-v1025-alone", 1025, "f32", P4, fill=(-9.0, -12.0), p=("after", 1)),
          level_row("p-v1025-alone-T0.5", 1025, "bf16", P4, fill=(-9.0, -12.0), T=0.5, p=("after", 0)),
          level_row("p-v30522-narrow-k7", 30522, "bf16", P4, fill=(-3.0, -4.0), k=7, p=("after", 1)),      # k = 7 keeps 14; p cuts to 6
          level_row("p-v30522-wide-k1000", 30522, "f32", [(6.0, 8), (5.0, 8), (4.0, 8), (-2.0, 990)], fill=(-3.0,), k=1000, p=("after", 1)),
          level_row("p-v2048-max-only", 2048, "f32", P4, fill=(-9.0,), p=2.0 ** -9),
          level_row("p-v64-just-under-1", 64, "f32", [(1.0, 20), (0.0, 24), (-1.0, 20)], p=1.0 - 2.0 ** -10),
          level_row("p-v64-zero-off", 64, "bf16", [(1.0, 20), (0.0, 24), (-1.0, 20)], p=0.0),
          level_row("p-v64-one-off", 64, "f32", [(1.0, 20), (0.0, 24), (-1.0, 20)], p=1.0),
          level_row("p-v3072-underflow", 3072, "f32", [(100.0, 3), (99.0, 5)], fill=(-100.0,), p=("after", 0)),
          level_row("off-v3072-underflow-k0", 3072, "bf16", [(100.0, 3), (99.0, 5)], fill=(-100.0,)),
          level_row("p-v1023-kth-inf", 1023, "bf16", [(1.0, 3), (0.0, 5), (-1.0, 9)], ban_fill=True, k=64, p=("after", 1)),
          level_row("p-v31744-k64-T2", 31744, "f32", [(2.0, 6), (0.0, 12), (-2.0, 24), (-4.0, 30)], fill=(-6.0, -8.0), T=2.0, k=64, p=("after", 2))]
    # -- noise rows
    R += [noise_row("noise-v30522-f32-k40-T0.7", 30522, "f32", 1, 0.7, 40),
          noise_row("noise-v30522-bf16-k7-T1.3", 30522, "bf16", 2, 1.3, 7),
          noise_row("noise-v30522-f32-k64-T1.3", 30522, "f32", 3, 1.3, 64, nban=6),
          noise_row("noise-v30720-bf16-k17-T0.7", 30720, "bf16", 4, 0.7, 17),
          noise_row("noise-v31744-f32-k40-T1.3", 31744, "f32", 5, 1.3, 40),
          noise_row("noise-v3072-f32-k64-p-T1.3", 3072, "f32", 6, 1.3, 64, p=("after", 20)),
          noise_row("noise-v3073-bf16-k16-T0.7", 3073, "bf16", 7, 0.7, 16, nban=4),
          noise_row("noise-v2048-f32-k65-T0.7", 2048, "f32", 8, 0.7, 65),
          noise_row("noise-v1025-bf16-k17-T1.3", 1025, "bf16", 9, 1.3, 17),
          division_tie_row("div-tie-v1025-k7-T1.3", 1025, 1.3, 7),
          division_tie_row("div-tie-v30522-k17-T0.7", 30522, 0.7, 17)]
    # -- n-gram bans.  Levels: 0 the maximum, 1..3 below; a = lv[3][0] .. are ordinary kept tokens used as the generated prefix
    NG = [(3.0, 2), (2.0, 3), (1.0, 4), (0.0, 6)]

    def spec(n, V, T=0, special=None, both=False, big=False):
        def f(lv):
            top, t2, t3, dec = lv[0][1], lv[1][1], lv[2][-1], lv[1][0]          # (lv[0][0] is id 0, a special id)
            sp102 = 102
            a, b, c, x, q = lv[3][0], lv[3][1], lv[3][2], lv[3][3], lv[3][4]
            pre = {1: (), 2: (c,), 4: (a, b, c)}[n]
            off = {1: (), 2: (b,), 4: (x, a, b)}[n]                 # what a prefix read one step early would be
            ids = [q, x, a, b, c]
            wins = [pre + (top,), pre + (t2,), pre + (top,), pre + (sp102,), pre + (V,), pre + (V + 7,), pre + (-3,)]
            if n > 1:
                wins += [off + (dec,), pre[:-1] + (101, t3)]
            if special is not None:
                wins += [pre + (5,), pre + (7,), pre + (9,)]
            lead = 3
            if big:                                                    # hist_T > 1024: a thread serves two windows
                lead = 1023
                wins = wins[:1] + [pre + (t3,)] + wins[1:]
            return ng(n, ids, wins, lead=lead, special=special, tail=T, end=pre)
        return f

    NG17 = NG[:3] + [(0.0, 12)]                                        # (k = 17: the bisection behind the n-gram filter)
    for (n, V, dt, k) in ((1, 1025, "bf16", 7), (2, 1025, "f32", 7), (4, 1025, "bf16", 7), (2, 30522, "bf16", 7), (4, 30522, "f32", 17)):
        R.append(level_row("ngram-n%d-v%d-%s-k%d" % (n, V, dt, k), V, dt, NG17 if k == 17 else NG, fill=(-1.0, -2.0), k=k, ngram=spec(n, V), force=(102,)))
    R += [level_row("ngram-n4-v3073-with-mask", 3073, "f32", [(4.0, 2, "ban")] + NG, fill=(-1.0, -2.0), k=7, ngram=lambda lv: spec(4, 3073)(lv[1:]), force=(102,), force_lv=3),
          level_row("ngram-n2-v30720-hist1100", 30720, "bf16", NG, fill=(-1.0, -2.0), k=7, ngram=spec(2, 30720, big=True, T=60), force=(102,)),
          level_row("ngram-n4-v2048-special8", 2048, "f32", NG, fill=(-1.0, -2.0), k=7, ngram=spec(4, 2048, special=SPECIAL8), force=(102, 5, 7, 9)),
          level_row("ngram-n4-v1024-short-prefix", 1024, "bf16", NG, fill=(-1.0, -2.0), k=7, force=(102,),
                    ngram=lambda lv: dict(spec(4, 1024)(lv), cur_len=2)),                                  # cur_len < n - 1: nothing
          level_row("ngram-n4-v97-short-hist", 97, "f32", NG, fill=(-1.0, -2.0), k=7,
                    ngram=lambda lv: dict(hist=[lv[3][0], lv[3][1], lv[0][0]], ids=[lv[3][0], lv[3][1], lv[3][2]], cur_len=3, n=4, special=None))]
    names = [r.name for r in R]
    assert len(set(names)) == len(names)
    return R


_Case = collections.namedtuple("Case", "row kind")


class Case(_Case):
    __slots__ = ()

    @property
    def id(self):
        return "%s-%s" % (self.row.name, self.kind)


def build_cases():
    cs = []
    for r in build_rows():
        n = len(reference(r).kept)
        cs.append(Case(r, "mid"))
        if n >= 2:
            cs.append(Case(r, "step"))
    return cs


CASES = build_cases()
BY_ID = dict((c.id, c) for c in CASES)


# ---------------------------------------------------------------------------------------------- one launch
def int_window(rows, cols, ld, fill, device, guard=2):
    """int64 [rows, cols] with row stride ld inside one allocation filled with `fill`."""
    flat = torch.full(((rows + 2 * guard) * ld,), fill, dtype=torch.int64, device=device)
    return flat, torch.as_strided(flat, (rows, cols), (ld, 1), guard * ld)


class Launch(object):
    """The windows of one case: B copies of the row, B uniforms."""

    def __init__(self, be, row, u):
        dev, B, V, dt = be.device, len(u), row.V, DT[row.dtype]
        self.B, self.row = B, row
        self.logits = Window(B, V, dt, dev, "poison", ld=V + (8 if dt == BF16 else 4))
        self.logits.set(row.logits.to(dt)[None].expand(B, V).contiguous())
        if V in INF_PAD:                                               # (a compare-based kernel steps over NaN: +inf would win the maximum)
            torch.as_strided(self.logits.flat, (B,), (self.logits.ld,), self.logits.offset + V).fill_(float("inf"))
        self.u = Window(1, B, F32, dev, "poison").set(u)
        self.out = Window(B, 1, torch.int64, dev, "canary", ld=3)
        self.banned = None
        if row.ban is not None:
            bld = V + 5
            self.ban_flat = torch.ones((B + 4) * bld, dtype=torch.bool, device=dev)
            self.banned = torch.as_strided(self.ban_flat, (B, V), (bld, 1), 2 * bld)
            self.banned.copy_(row.ban[None].expand(B, V))
        self.ngram = None
        if row.ngram is not None:
            g = row.ngram
            r = reference(row)
            sp = set(g["special"] if g["special"] is not None else SPECIAL)
            hot = [int(i) for i in r.kept if int(i) not in sp][0]       # the padding: a kept, non-special id -- its ban would show
            T, L = len(g["hist"]), len(g["ids"])
            _, hist = int_window(B, T, T + 5, hot, dev)
            hist.copy_(torch.tensor(g["hist"], dtype=torch.int64)[None].expand(B, T))
            _, ids = int_window(L + 1, B, B + 3, CANARY[torch.int64], dev)
            ids[:L].copy_(torch.tensor(g["ids"], dtype=torch.int64)[:, None].expand(L, B))
            self.ngram = (hist, ids, g["cur_len"], g["n"]) + ((tuple(g["special"]),) if g["special"] is not None else ())

    def run(self, be):
        o = self.out.view[:, 0]
        be.sample(self.logits.view, self.row.T, self.row.k, self.u.vector(), o, self.banned, ngram=self.ngram, top_p=self.row.p)
        return o.clone().cpu()

    def assert_windows(self, name):
        self.out.assert_surroundings_untouched(name + ": out")
        if self.row.V in INF_PAD:                                      # (the +inf column: still +inf; NaN for the window's own check)
            col = torch.as_strided(self.logits.flat, (self.B,), (self.logits.ld,), self.logits.offset + self.row.V)
            assert bool((col.float() == float("inf")).all()), name + ": column V of the logits' padding was written"
            col.fill_(float("nan"))
            self.logits.assert_surroundings_untouched(name + ": logits")
            col.fill_(float("inf"))
        else:
            self.logits.assert_surroundings_untouched(name + ": logits")
        self.u.assert_surroundings_untouched(name + ": u")


def run_case(be, c):
    """One launch, its ids against the float64 reference, a second launch on the same inputs, every window."""
    row = c.row
    u, lo, hi, what = probes(row, c.kind)
    L = Launch(be, row, u)
    got = L.run(be)
    again = L.run(be)
    L.assert_windows(c.id)
    bad = torch.nonzero((got != lo) & (got != hi)).flatten().tolist()
    if bad:
        r = reference(row)
        kept = set(int(i) for i in r.kept)
        msg = ["%s (u = %.9g): got id %d (%s), want %s" % (what[b], float(u[b]), int(got[b]), "a kept token" if int(got[b]) in kept else "NOT in the kept set",
                                                          int(lo[b]) if lo[b] == hi[b] else "%d or %d" % (lo[b], hi[b])) for b in bad[:6]]
        premise = "tie row -- the PREMISE __expf(0) == 1 (weights exactly 1, integer sums) fails, or the draw is wrong: " if row.tie else ""
        raise AssertionError(premise + "%s: %d of %d probes wrong (kept %d tokens, smallest probability %.3g); %s" % (c.id, len(bad), len(u), len(r.kept), r.margin_prob, "; ".join(msg)))
    assert torch.equal(got, again), c.id + ": a second launch on the same inputs drew other ids"
    return got


def premise_case(be):
    """__expf(0) == 1: 64 tied tokens, u = j / 64 on EVERY step.  With weights of exactly 1 the sums are the integers 1 .. 64 and
    x = u * 64 = j, so the draw is the j-th kept token bit for bit; a weight c != 1 leaves j * c and (j / 64) * (64 c) to round apart."""
    row = level_row("premise-expf0", 3073, "f32", [(1.25, 64)], fill=(0.0, -2.0), k=7, tie=True)
    kept = reference(row).kept
    u = torch.arange(1, 64, dtype=torch.float32) / 64
    L = Launch(be, row, u)
    got = L.run(be)
    L.assert_windows(row.name)
    want = torch.tensor(kept[:63].astype(np.int64))
    assert torch.equal(got, want), "the premise __expf(0) == 1 does not hold (or the draw on an exact step is wrong): u = j / 64 drew %r, want %r" % (
        got[got != want].tolist()[:8], want[got != want].tolist()[:8])


def all_banned_case(be, V=1025, dtype="bf16"):
    """Every token banned: 0 <= id < V, and the id is 0 (what the kernel has always returned: total = 0, nothing counted)."""
    row = Row("all-banned", V, dtype, torch.zeros(V), 1.0, 7, 0.5, torch.ones(V, dtype=torch.bool), None, False, None)
    u = torch.tensor([U_FIRST, 0.25, 0.5, U_LAST], dtype=torch.float32)
    L = Launch(be, row, u)
    got = L.run(be)
    L.assert_windows("all-banned")
    assert bool(((got >= 0) & (got < V)).all()) and bool((got == 0).all()), "all-banned row: ids %r, pinned 0" % got.tolist()


def lib_path():
    import exact_gemm
    return exact_gemm.lib_path()
