"""CPU proof of the dropout-stream checks (tests/exact_dropout.py): a stand-in backend built on the restatement passes A-F, and
every named defect of the stand-in -- in the key, the threshold, the element rule, the factor, the top-byte term of the pair draw
and the offset advance -- is caught by a named check.  E (no repeated blocks) is host-only and runs here in full.  The device side
is tests/test_dropout_exact_gpu.py."""
import numpy as np
import pytest

import exact_dropout as X

U = np.uint64
M32 = 0xFFFFFFFF


class Lazy(object):
    """A large site of the stand-in: factors are computed for the elements that are read."""

    def __init__(self, n, at):
        self.n, self.at = n, at

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        idx = np.asarray(idx)
        assert idx.min() >= 0 and idx.max() < self.n
        return self.at(idx.astype(np.uint64))


class StandIn(object):
    def __init__(self, defect=None):
        self.defect = defect
        self.rule = {"no_top_term": "none", "top_in_front": "front"}.get(defect, X.RULE)

    def at(self, idx, p, site, seed, off):
        d = self.defect
        if not np.float32(p) > 0:
            return np.ones(idx.shape, np.float32)
        site = 0 if d == "site_ignored" else site
        off = off & ~M32 if d == "offset_low_ignored" else off & M32 if d == "offset_high_ignored" else off
        seed = seed & M32 if d == "seed_high_ignored" else seed
        key = X.make_key(seed, off, site)
        thr = int(np.float32(p) * np.float32(65536.0)) if d == "thr_truncated" else X.threshold(p)
        r = X.pair_draw(idx if d == "pair_index_e" else idx >> U(1), key, self.rule).astype(np.uint64)
        odd = (idx & U(1)) == (0 if d == "halves_swapped" else 1)
        u = np.where(odd, r >> U(16), r & U(0xFFFF))
        keep = u > U(thr) if d == "keep_gt" else u >= U(thr)
        f = np.float32(1.0 / (1.0 - thr / 65536.0)) if d == "factor_1_over_q" and thr < 65536 else X.kept_factor(p)
        return np.where(keep, f, np.float32(0)).astype(np.float32)

    def mask(self, n, p, site, seed, offset):
        if n > (1 << 22):
            return Lazy(n, lambda idx: self.at(idx, p, site, seed, offset))
        return self.at(np.arange(n, dtype=np.uint64), p, site, seed, offset)

    def advance(self, seed, offset, times):
        for _ in range(times):
            offset = (offset & ~M32) | ((offset + 1) & M32) if self.defect == "advance_no_carry" else offset + 1
        return seed, offset


def caught(check, *a, **kw):
    with pytest.raises(AssertionError):
        check(*a, **kw)


# ---------------------------------------------------------------------------------------------- premises
def test_the_listed_probabilities_give_the_claimed_thresholds():
    assert sorted(X.THRS) == sorted(X.PS)
    for p in X.PS:
        assert 0 <= p < 1 and X.threshold(p) == X.THRS[p], (p, X.threshold(p))
    assert {0, 1, 65535, 65536} <= set(X.THRS.values())
    assert X.threshold(0.3) == 19661 and int(np.float32(0.3) * np.float32(65536.0)) == 19660      # rounding, not truncation
    assert X.kept_factor(0.5) == 2 and X.kept_factor(1e-6) > 1 and X.kept_factor(0.25).dtype == np.float32
    assert X.keep_rate(0.25) == 0.75 and X.keep_rate(0.1) != 0.9


def test_rank_seeds_stay_below_2p63_and_match_the_library():
    from gst_visdial_amd import ops
    for r in range(9):
        assert X.rank_seed(1234, r) == ops.rank_seed(1234, r) and 0 <= X.rank_seed(1234, r) < 2 ** 63
    assert all(0 <= s < 2 ** 63 for s in X.SEEDS) and len(set(X.SEEDS)) == 9
    assert any(s >> 32 for s in X.SEEDS)


def test_the_grid_holds_what_the_issue_names():
    cases = X.grid_cases()
    assert len(cases) == 9 + 6 + 8 + 9 + 30
    for axis, vals in enumerate((X.SEEDS, X.OFFSETS, X.SITES, X.PS)):
        assert set(c[axis] for c in cases) == set(vals)
    assert X.GRID_N % 2 == 1


def test_the_parent_distances():
    """d_t of the previous hash: its draw of c | t << 24 is its draw of c ^ d_t, for every key -- and no longer in the library's."""
    assert X.parent_distance(1) == 0x9E3679
    c = (np.arange(1 << 16, dtype=np.uint64) * U(251)) & U(0xFFFFFF)
    for t in (1, 2, 3, 128, 255):
        for key in (0, 0x12345678, 0xdeadbeef):
            hi, lo = c | U(t << 24), c ^ U(X.parent_distance(t))
            assert np.array_equal(X.drop_hash(hi, key, "front"), X.drop_hash(lo, key, "front"))
            assert (X.drop_hash(hi, key) == X.drop_hash(lo, key)).mean() < 1e-3


def test_the_first_2p24_counters_keep_the_draws_of_the_previous_hash():
    """Every site up to 2^25 elements keeps its masks: all of block 0, three keys, against both earlier rules."""
    for key in (0, 0x12345678, X.make_key(*X.LARGE)):
        for lo in range(0, X.BLOCK, 1 << 22):
            c = np.arange(lo, lo + (1 << 22), dtype=np.uint64)
            new = X.drop_hash(c, key)
            assert np.array_equal(new, X.drop_hash(c, key, "front")) and np.array_equal(new, X.drop_hash(c, key, "none"))
            assert np.array_equal(new, X.mix32(c ^ U(key)))


def test_drop_hash_and_pair_draw_are_one_stream():
    c = np.random.RandomState(1).randint(0, 2 ** 32, size=1 << 16, dtype=np.uint64)
    for rule in ("behind", "front", "none"):
        assert np.array_equal(X.drop_hash(c, 0xabcdef12, rule), X.pair_draw(c, 0xabcdef12, rule))
    X.check_high_word_changes_the_draws()


# ---------------------------------------------------------------------------------------------- the stand-in passes
def test_standin_passes_grid_advance_and_large_site():
    be = StandIn()
    X.check_grid(be)
    X.check_advance(be)
    X.check_large_site(be)
    X.check_large_site_pairs(be)
    rep = {}
    X.check_large_site_pairs(be, n=1 << 27, report=rep)            # twice the device's site: the partners of t = 2 and 3 too
    assert sorted(rep) == [1, 2, 3]


def test_standin_passes_independence():
    rep = {}
    X.check_independence(StandIn(), report=rep)
    assert sorted(rep) == ["halves", "keep rate", "lags", "offsets", "rank seeds", "seeds", "sites"] and max(rep.values()) < 2


def test_no_block_repeats():
    rep = {}
    X.check_no_block_repeats(report=rep)
    assert sorted(rep) == sorted(X.BLOCK_PAIRS)
    for share, hits in rep.values():
        assert 0.55 < hits < 0.75          # a hash of 2^24 outputs: values coincide between blocks, at no particular distance


# ---------------------------------------------------------------------------------------------- the defects are caught
IND_SMALL = 1 << 17                    # the key defects make whole masks equal: z is in the hundreds at any n


def test_defect_site_ignored():
    caught(X.check_grid, StandIn("site_ignored"))
    caught(X.check_independence, StandIn("site_ignored"), n=IND_SMALL)


def test_defect_offset_low_word_ignored():
    caught(X.check_grid, StandIn("offset_low_ignored"))
    caught(X.check_advance, StandIn("offset_low_ignored"))
    caught(X.check_independence, StandIn("offset_low_ignored"), n=IND_SMALL)


def test_defect_offset_high_word_ignored():
    caught(X.check_grid, StandIn("offset_high_ignored"))
    caught(X.check_advance, StandIn("offset_high_ignored"))


def test_defect_seed_high_word_ignored():
    caught(X.check_grid, StandIn("seed_high_ignored"))


def test_defect_threshold_truncated():
    caught(X.check_grid, StandIn("thr_truncated"))
    with pytest.raises(AssertionError, match="threshold edge"):                 # one element in 65536: 19660 against 19661 at p = 0.3
        X.check_threshold_edge(StandIn("thr_truncated"))


def test_defect_keep_iff_greater():
    caught(X.check_grid, StandIn("keep_gt"))
    with pytest.raises(AssertionError, match="threshold edge"):
        X.check_threshold_edge(StandIn("keep_gt"))


def test_defect_halves_swapped():
    caught(X.check_grid, StandIn("halves_swapped"))


def test_defect_pair_index_is_the_element_index():
    caught(X.check_grid, StandIn("pair_index_e"))


def test_defect_factor_from_the_threshold():
    caught(X.check_grid, StandIn("factor_1_over_q"))


def test_defect_top_byte_term_left_out():
    be = StandIn("no_top_term")
    X.check_grid(be)                                               # invisible below 2^24 draws
    caught(X.check_large_site, be)
    caught(X.check_no_block_repeats, "none", pairs=[(0, 1)])


def test_defect_top_byte_term_in_front_of_the_first_multiply():
    be = StandIn("top_in_front")
    X.check_grid(be)
    X.check_independence(be, n=IND_SMALL)                          # nor do the statistics of small sites see it
    caught(X.check_large_site, be)
    rep = {}
    caught(X.check_large_site_pairs, be, report=rep)
    assert rep[1][1] == 1.0                                        # every partner repeats
    rep = {}
    caught(X.check_no_block_repeats, "front", pairs=[(0, 1)], report=rep)
    assert rep[(0, 1)][0] > 0.5 and rep[(0, 1)][1] == 1.0


def test_defect_advance_without_carry():
    X.check_grid(StandIn("advance_no_carry"))
    caught(X.check_advance, StandIn("advance_no_carry"))
