"""Exact layer of the dropout-stream tests: the ONE numpy restatement of the counter-based dropout of
csrc/common.h -- mix32, the key that make_drop forms from (seed, offset, site), the threshold, the pair draw of drop_draw /
drop_hash, the element rule and the kept factor -- and the checks that anchor the device's generator to it.  Every other dropout
test of the suite regenerates its mask with the library's own probe (ops.dropout_mask), i.e. with the code under test; here the
probe itself is compared, factor for factor, with arithmetic written down a second time.

All integer arithmetic is uint64 masked to 32 bits; __umul24 is the product of the low 24 bits of both operands, low 32 bits kept.

The checks take a backend `be`:
    be.mask(n, p, site, seed, offset) -> the n float32 factors of a site (a numpy array, a torch tensor, or anything take() reads)
    be.advance(seed, offset, times)   -> (seed, offset) after `times` Rng.advance() calls
so the same code runs against a stand-in on the CPU (tests/test_exact_dropout_harness_cpu.py, which proves that every check
bites) and against the device (tests/test_dropout_exact_gpu.py).

`rule` names where the counter's top byte enters the pair draw: "behind" (the library: XORed into the product of mix32's first
multiply), "front" (the previous hash: XORed in front of that multiply, where it only permutes one table of 2^24 draws) and "none"
(the hash before that).  The checks default to the library's rule; the other two exist for the harness and for running the
checks on an older build."""
import numpy as np

U = np.uint64
M32 = U(0xFFFFFFFF)
M24 = U(0xFFFFFF)
TOP = 0x9E3779                       # the 24-bit odd constant the counter's top byte is multiplied with
RULE = "behind"


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def umul24(a, b):
    return ((_u64(a) & M24) * (_u64(b) & M24)) & M32


def _mix(x, mid=None):
    """mix32 on uint64 lanes; `mid` is XORed into the product of the first multiply."""
    x = _u64(x) & M32
    x = x ^ (x >> U(16))
    x = umul24(x, 0xeb352d)
    if mid is not None:
        x = x ^ mid
    x = x ^ (x >> U(15))
    x = umul24(x, 0x6ca68b)
    x = x ^ (x >> U(16))
    return x


def mix32(x):
    """csrc/common.h mix32."""
    return _mix(x).astype(np.uint32)


def pair_draw(e2, key, rule=RULE):
    """drop_draw: the 32-bit draw of pair counter e2 (element index >> 1, up to 64 bits) under `key`."""
    e2 = _u64(e2)
    lo, hi = e2 & M32, e2 >> U(32)
    top = umul24(lo >> U(24), TOP)
    high = (hi * U(0x9E3779B1)) & M32
    x = lo ^ U(key)
    if rule == "front":
        return _mix(((x ^ top) + high) & M32).astype(np.uint32)
    x = (x + high) & M32
    return _mix(x, top if rule == "behind" else None).astype(np.uint32)


def drop_hash(c, key, rule=RULE):
    """drop_hash: the draw of a 32-bit counter, the path of the attention kernels; one stream with pair_draw."""
    return pair_draw(_u64(c) & M32, key, rule)


def make_key(seed, offset, site):
    """The key make_drop forms from the Rng state (seed, offset) and the site number."""
    seed, off, site = int(seed), int(offset), int(site) & 0xFFFFFFFF
    m = 0xFFFFFFFF
    a = int(mix32(np.array([(seed & m) ^ ((0x9E3779B9 * ((site + 1) & m)) & m)]))[0])
    b = int(mix32(np.array([((seed >> 32) + 0x85EBCA6B * (off & m) + site) & m]))[0])
    c = int(mix32(np.array([((off >> 32) & m) ^ ((a + b) & m)]))[0])
    return a ^ ((b * 0xC2B2AE35) & m) ^ c


def threshold(p):
    """thr = uint32(fp32(p) * 65536.f + 0.5f): an element is kept iff its 16 bits are >= thr."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def kept_factor(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_rate(p):
    """The rate the threshold really gives (not 1 - p)."""
    return 1.0 - threshold(p) / 65536.0


def rank_seed(seed, rank):
    """ops.rank_seed, restated (the harness compares the two)."""
    return (int(seed) + int(rank) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF


def u16_at(idx, key, rule=RULE):
    """The 16 bits of elements idx: the even element takes the low half of its pair's draw, the odd element the high half."""
    idx = _u64(idx)
    r = pair_draw(idx >> U(1), key, rule).astype(np.uint64)
    return np.where((idx & U(1)) == 1, r >> U(16), r & U(0xFFFF))


def mask_at(idx, p, site, seed, offset, rule=RULE):
    """The float32 factors of elements idx of a site: all ones without rng for p = 0, else 1/(1-p) if kept and 0 if dropped."""
    idx = _u64(idx)
    if not np.float32(p) > 0:
        return np.ones(idx.shape, np.float32)
    keep = u16_at(idx, make_key(seed, offset, site), rule) >= U(threshold(p))
    return np.where(keep, kept_factor(p), np.float32(0)).astype(np.float32)


def mask(n, p, site, seed, offset, rule=RULE):
    return mask_at(np.arange(n, dtype=np.uint64), p, site, seed, offset, rule)


def parent_distance(t):
    """d_t of the rule "front": there draw(c | t << 24) == draw(c ^ d_t) for every key and every c < 2^24.  The first multiply
    reads, after the fold, the bytes (b2, b1 ^ b3, b0 ^ b2) of its input; with T = umul24(t, TOP) the inputs of the two counters
    differ by D = (t << 24) ^ T ^ d_t, and D folds to nothing iff D0 = D2 = 0 and D1 = D3."""
    T = t * TOP & 0xFFFFFFFF
    return (T & 0xFF00FF) | ((((T >> 8) ^ t ^ (T >> 24)) & 0xFF) << 8)


def take(m, idx=None):
    """The values of mask m at elements idx (all of it for None) as numpy: m is numpy, a torch tensor on any device, or an
    object whose [] takes an index array (the stand-in's lazy large site)."""
    if type(m).__module__.startswith("torch"):
        import torch
        if idx is not None:
            m = m[torch.from_numpy(np.ascontiguousarray(idx).astype(np.int64)).to(m.device)]
        return m.cpu().numpy()
    return np.asarray(m if idx is None else m[np.asarray(idx).astype(np.int64)])


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d factors differ, first at %d: got %r want %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------ A: bit-exact grid
GRID_N = 4099                        # odd: the last pair is used by half
BASE = (1234, 0, 1, 0.1)             # seed, offset, site, p
SEEDS = [0, 1, 1234, 2 ** 32, 2 ** 32 + 1234, 2 ** 63 - 1] + [rank_seed(1234, r) for r in (1, 2, 3)]
OFFSETS = [0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3]
SITES = [0, 1, 2, 7, 255, 256, 2 ** 31, 2 ** 32 - 1]
PS = [0.1, 0.25, 0.3, 0.5, 0.9, 2.0 ** -17, 1e-6, 0.99999, 1 - 2.0 ** -17]
THRS = {0.1: 6554, 0.25: 16384, 0.3: 19661, 0.5: 32768, 0.9: 58982, 2.0 ** -17: 1, 1e-6: 0, 0.99999: 65535, 1 - 2.0 ** -17: 65536}


def grid_cases():
    """One axis at a time around BASE, then 30 random combinations of the listed values (fixed generator)."""
    s0, o0, t0, p0 = BASE
    cases = [(s, o0, t0, p0) for s in SEEDS] + [(s0, o, t0, p0) for o in OFFSETS]
    cases += [(s0, o0, t, p0) for t in SITES] + [(s0, o0, t0, p) for p in PS]
    rs = np.random.RandomState(20241021)
    for _ in range(30):
        cases.append((SEEDS[rs.randint(len(SEEDS))], OFFSETS[rs.randint(len(OFFSETS))], SITES[rs.randint(len(SITES))],
                      PS[rs.randint(len(PS))]))
    return cases


def check_grid(be, rule=RULE, n=GRID_N):
    for seed, off, site, p in grid_cases():
        got = take(be.mask(n, p, site, seed, off))
        what = "seed %d offset %d site %d p %r" % (seed, off, site, p)
        same(got, mask(n, p, site, seed, off, rule), what)
        if threshold(p) == 0:            # the restatement decides the extremes: everything kept with factor 1/(1-p) ...
            same(got, np.full(n, kept_factor(p), np.float32), what + " (thr 0)")
        if threshold(p) == 65536:        # ... and everything dropped
            same(got, np.zeros(n, np.float32), what + " (thr 65536)")
    for seed, off, site in ((1234, 0, 1), (2 ** 63 - 1, 2 ** 40 + 3, 2 ** 32 - 1)):
        same(take(be.mask(n, 0.0, site, seed, off)), np.ones(n, np.float32), "p = 0: all ones, no rng")
    check_threshold_edge(be, rule)


EDGE_N = 1 << 20


def check_threshold_edge(be, rule=RULE, n=EDGE_N):
    """Part of A.  A threshold that is off by one, or `>` for `>=`, moves one element in 65536 -- a handful per grid case, or none.
    So for every listed p the elements of a 2^20-element site whose 16 bits ARE thr - 1 (dropped) or thr (kept) are looked up
    in the restatement (about 16 each) and compared on their own."""
    seed, off, site, _ = BASE
    u = u16_at(np.arange(n, dtype=np.uint64), make_key(seed, off, site), rule)
    for p in PS:
        thr = threshold(p)
        below, at = np.flatnonzero(u == U(thr) - U(1)) if thr else np.zeros(0, np.int64), np.flatnonzero(u == U(thr))
        assert (below.size >= 4 or thr == 0) and (at.size >= 4 or thr == 65536), (p, below.size, at.size)
        idx = np.concatenate([below, at]).astype(np.uint64)
        want = mask_at(idx, p, site, seed, off, rule)
        assert not want[:below.size].any() and (want[below.size:] == kept_factor(p)).all()
        same(take(be.mask(n, p, site, seed, off), idx), want, "threshold edge p %r" % p)


# ------------------------------------------------------------------------------------------------ B: offset advance
def check_advance(be, rule=RULE, n=GRID_N):
    seed, _, site, p = BASE
    state = (seed, 0)
    for k in (1, 2, 3):
        state = be.advance(state[0], state[1], 1)
        assert tuple(int(v) for v in state) == (seed, k), state
        same(take(be.mask(n, p, site, *state)), mask(n, p, site, seed, k, rule), "offset %d after %d advances" % (k, k))
    for seed in (1234, 2 ** 63 - 1):     # the carry into the word make_drop hashes on its own
        state = be.advance(seed, 2 ** 32 - 1, 1)
        assert tuple(int(v) for v in state) == (seed, 2 ** 32), state
        want = mask(n, p, site, seed, 2 ** 32, rule)
        same(take(be.mask(n, p, site, *state)), want, "offset 2^32 by a carry")
        assert not np.array_equal(want, mask(n, p, site, seed, 0, rule))      # premise: the carry is visible


# ------------------------------------------------------------------------------------------------ C: large site
LARGE_N = 1 << 26
LARGE = (77, 0, 5)                   # seed, offset, site: the case of tests/test_ops_gpu.py


def large_indices(n=LARGE_N):
    w = 1 << 16
    win = [np.arange(s, s + w, dtype=np.uint64) for s in (0, (n >> 1) - (w >> 1), n - w)]
    return np.concatenate(win + [np.arange(0, n, 1021, dtype=np.uint64)])


def check_large_site(be, rule=RULE, n=LARGE_N):
    """n = 2^26 elements = 2^25 pair draws: the second window straddles the first 2^24-draw boundary (element 2^25)."""
    seed, off, site = LARGE
    idx = large_indices(n)
    assert n != LARGE_N or ((idx >> U(1)) >= U(1 << 24)).sum() > (1 << 16)
    for p in (0.25, 0.5):
        same(take(be.mask(n, p, site, seed, off), idx), mask_at(idx, p, site, seed, off, rule), "large site p %r" % p)


def check_high_word_changes_the_draws(rule=RULE):
    """Elements >= 2^33 (pair counters >= 2^32) are out of the probe's reach: on the host only, the high word of the pair
    counter must give other draws than its low word alone, and other draws for another high word."""
    lo = np.arange(1 << 16, dtype=np.uint64) * U(65521)
    for key in (0, 0x12345678, make_key(1234, 0, 1)):
        d0 = pair_draw(lo, key, rule)
        d1, d2 = pair_draw(lo | (U(1) << U(32)), key, rule), pair_draw(lo | (U(2) << U(32)), key, rule)
        for a, b in ((d0, d1), (d0, d2), (d1, d2)):
            assert (a == b).mean() < 1e-3


# ------------------------------------------------------------------------------------------------ D: independence
IND_N = 1 << 20
Z_MAX = 5.0
RATE_KEYS = [(0, 0, 1), (1234, 0, 1), (1234, 1, 1), (77, 5, 40), (2 ** 63 - 1, 2 ** 32 - 1, 200), (2 ** 40 + 5, 2 ** 32, 3)]
LAGS = [1, 2, 3, 4, 64, 768, 1024, 1 << 15, 1 << 19]


def z_rate(keep, q):
    n = keep.size
    return (float(keep.sum()) - n * q) / np.sqrt(n * q * (1 - q))


def z_agree(a, b, q):
    n, g = a.size, q * q + (1 - q) * (1 - q)
    return (float((a == b).sum()) - n * g) / np.sqrt(n * g * (1 - g))


def check_independence(be, n=IND_N, report=None):
    """z = (observed - expected) / binomial sigma of keep rates and of keep-bit agreements; |z| <= 5 everywhere.  The expected
    keep rate is q = 1 - thr/65536, the expected agreement of two independent masks q^2 + (1-q)^2.  `report` collects the worst
    |z| of every set."""
    worst = {}

    def z(name, v):
        worst[name] = max(worst.get(name, 0.0), abs(v))

    def keep(p, seed, off, site):
        return take(be.mask(n, p, site, seed, off)) != 0

    for p in (0.1, 0.25, 0.3, 0.5):
        for seed, off, site in RATE_KEYS:
            z("keep rate", z_rate(keep(p, seed, off, site), keep_rate(p)))
    seed, off, site, p = BASE
    q = keep_rate(p)
    base = keep(p, seed, off, site)
    for s in range(2, 34):
        z("sites", z_agree(base, keep(p, seed, off, s), q))
    for o in range(1, 33):
        z("offsets", z_agree(base, keep(p, seed, o, site), q))
    for r in range(1, 9):
        z("rank seeds", z_agree(base, keep(p, rank_seed(seed, r), off, site), q))
    for s in range(1235, 1251):
        z("seeds", z_agree(base, keep(p, s, off, site), q))
    for lag in LAGS:
        if lag < n:
            z("lags", z_agree(base[:-lag], base[lag:], q))
    z("halves", z_agree(base[0:n & ~1:2], base[1::2], q))
    if report is not None:
        report.update(worst)
    bad = {k: v for k, v in worst.items() if not v <= Z_MAX}
    assert not bad, "independence: |z| > %g in %r (all sets: %r)" % (Z_MAX, bad, worst)


# ------------------------------------------------------------------------------------------------ E: no repeated blocks
BLOCK = 1 << 24
SHARE_MAX = 1e-3
BLOCK_PAIRS = [(0, 1), (0, 255), (1, 3)]


def worst_distance_share(draws_a, tb, key, rule=RULE, m=1 << 20):
    """Largest share of the m counters ((13 i + 7) mod 2^24) | tb << 24 whose draw is found in block a (`draws_a`: all 2^24 draws
    of it, in counter order; leftmost match in value order) at one and the same XOR distance of the low 24 bits."""
    order = np.argsort(draws_a, kind="stable")
    srt = draws_a[order]
    low = (np.arange(m, dtype=np.uint64) * U(13) + U(7)) & U(BLOCK - 1)
    d = drop_hash(low | (U(tb) << U(24)), key, rule)
    pos = np.minimum(np.searchsorted(srt, d, side="left"), BLOCK - 1)
    hit = srt[pos] == d
    dist = (order[pos][hit].astype(np.uint64) ^ low[hit]).astype(np.int64)
    return (np.bincount(dist, minlength=1).max() if dist.size else 0) / float(m), hit.mean()


def check_no_block_repeats(rule=RULE, key=None, pairs=BLOCK_PAIRS, m=1 << 20, report=None):
    """Host only, on the restatement: no block of 2^24 counters is (partly) a block seen before, read at a fixed XOR distance.
    The cap is a condition, not a tolerance: a share s of exact repeats shifts a keep-bit agreement by at most s/2."""
    key = make_key(*LARGE) if key is None else key
    blocks = {}
    for ta, tb in pairs:
        if ta not in blocks:
            blocks[ta] = drop_hash(np.arange(BLOCK, dtype=np.uint64) | (U(ta) << U(24)), key, rule)
        share, hits = worst_distance_share(blocks[ta], tb, key, rule, m)
        if report is not None:
            report[(ta, tb)] = (share, hits)
        assert share <= SHARE_MAX, "blocks %d and %d: share %.3g of the draws repeat at one distance" % (ta, tb, share)


# ------------------------------------------------------------------------------------------------ F: device side of E
def check_large_site_pairs(be, n=LARGE_N, ts=(1, 2, 3), report=None):
    """Keep bits of elements e = 2^23 + arange(2^22) against their partners at the distance d_t | t << 24 of the previous hash,
    for every t whose partners fall inside the site (n = 2^26 holds those of t = 1 only): agreement within 5 sigma of
    q^2 + (1-q)^2 = 0.625.  The previous hash gives 1.0."""
    seed, off, site = LARGE
    p = 0.25
    m = be.mask(n, p, site, seed, off)
    e = (1 << 23) + np.arange(1 << 22, dtype=np.uint64)
    a = take(m, e) != 0
    done = 0
    for t in ts:
        partner = ((((e >> U(1)) ^ U(parent_distance(t))) | (U(t) << U(24))) << U(1)) | (e & U(1))
        inside = partner < U(n)
        if not inside.any():
            continue
        assert inside.all()
        b = take(m, partner) != 0
        zt, agree = z_agree(a, b, keep_rate(p)), float((a == b).mean())
        if report is not None:
            report[t] = (zt, agree)
        assert abs(zt) <= Z_MAX, "t = %d: agreement %.5f, z = %.1f" % (t, agree, zt)
        done += 1
    assert done >= 1 and (n < (1 << 27) or done == len(ts))
