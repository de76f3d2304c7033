"""The exact layer of the sampling tests proves itself on the CPU (tests/exact_sample.py): every case runs
against a stand-in of gstvd_sample_topk written in torch after the rule documented in include/gstvd_hip.h, and against fifteen
deliberately wrong stand-ins, each of which must fail the case named for it.  The input conditions (probabilities and top-p
margins >= 2^-10) are asserted for every row.  Nothing here touches a GPU."""
import pytest
import torch

import exact_sample as X

CPU = torch.device("cpu")
NEG = -float("inf")


class Torch(object):
    """float64 stand-in of ops.sample_topk.  `defect`: one planted error, by its number in DEFECTS."""

    def __init__(self, defect=0):
        self.device, self.defect = CPU, defect

    def _ngram(self, ngram, B, V):
        d = self.defect
        hist, ids_tm, cur_len, n = ngram[:4]
        special = ngram[4] if len(ngram) > 4 else X.SPECIAL
        if n <= 0 or cur_len < n - 1 or hist.shape[1] < n:
            return None
        if d == 15:                                                    # one column past hist_T
            hist = torch.as_strided(hist, (B, hist.shape[1] + 1), hist.stride(), hist.storage_offset())
        win = hist.unfold(1, n, 1)
        clean = torch.ones(win.shape[:2], dtype=torch.bool)
        if d != 7:
            for s in special:
                clean &= ~(win == s).any(-1)
        hit = clean
        if n > 1:
            st = cur_len - (n - 1)
            if d == 8 and st >= 1:
                st -= 1
            prefix = ids_tm[st:st + n - 1, :B].t()
            hit = hit & (win[..., :n - 1] == prefix[:, None, :]).all(-1)
        last = win[..., n - 1]
        idx = torch.where(hit & (last >= 0) & (last < V), last, torch.full_like(last, V))
        return torch.zeros(B, V + 1, dtype=torch.bool).scatter_(1, idx, True)[:, :V]

    def sample(self, logits, temperature, top_k, u, out, banned=None, ngram=None, top_p=0.0):
        d = self.defect
        B, V = logits.shape
        t32 = torch.tensor(float(temperature), dtype=torch.float32)
        lg = logits.float()
        z = (lg * (torch.tensor(1.0, dtype=torch.float32) / t32) if d == 9 else lg / t32).double()
        dead = torch.zeros(B, V, dtype=torch.bool)
        if banned is not None:
            dead |= banned[:, :V].bool()
        if ngram is not None:
            m = self._ngram(ngram, B, V)
            if m is not None:
                dead |= m
        if d == 6:
            dead &= ~(z == z.max(1, keepdim=True).values)
        z = z.masked_fill(dead, NEG)
        zmax = z.max(1, keepdim=True).values
        if d == 10:                                                    # the row maximum takes in column V of the padding
            wide = torch.as_strided(logits, (B, V + 1), logits.stride(), logits.storage_offset())
            zmax = torch.maximum(zmax, (wide[:, V:].float() / t32).double())          # (NaN poisons it)
        keep = z > NEG
        k = int(top_k)
        if 0 < k < V:
            kth = z.sort(1, descending=True).values[:, k - 1:k]
            if d == 1:                                                 # exactly k tokens, whatever ties with the k-th
                keep &= torch.zeros(B, V, dtype=torch.bool).scatter_(1, z.topk(k, 1).indices, True)
            else:
                if d == 2:
                    lower = torch.where(z < kth, z, torch.full_like(z, NEG)).max(1, keepdim=True).values
                    kth = torch.where(lower > NEG, lower, kth)
                if d == 3 and k > X.NT // 64:                          # (k > 16: the bisection) one float key low
                    few = (z == zmax).sum(1, keepdim=True) < k
                    kth = torch.where(few, torch.nextafter(kth.float(), torch.full_like(kth, NEG).float()).double(), kth)
                keep &= z >= kth
        w_all = torch.where(z > NEG, torch.exp(z - zmax), torch.zeros_like(z))
        w = torch.where(keep, w_all, torch.zeros_like(z))
        if 0.0 < top_p < 1.0:
            S = (w_all if d == 5 else w).sum(1, keepdim=True)
            neg = -z
            order = neg.argsort(dim=1, stable=True)
            ns, ws = neg.gather(1, order).contiguous(), w.gather(1, order)
            incl = ws.cumsum(1)
            if d == 4:                                                 # the level that crosses top_p goes
                lastj = torch.searchsorted(ns, ns, right=True) - 1
                stay = (incl.gather(1, lastj) <= top_p * S) | (ns == -zmax)
            else:
                first = torch.searchsorted(ns, ns)
                stay = (incl - ws).gather(1, first) <= top_p * S
            keep &= torch.zeros(B, V, dtype=torch.bool).scatter_(1, order, stay)
            w = torch.where(keep, w, torch.zeros_like(w))
        if d == 12:
            ids = self._segmented_scan(z, keep, zmax, u, V)
        else:
            c = w.cumsum(1)
            total = c[:, -1:]
            x = u.double()[:, None] * total
            if d == 13:
                x = torch.where(u[:, None] > 1.0 - 2.0 ** -23, total * 2, x)
            ids = ((c <= x) if d == 11 else (c < x)).sum(1).clamp(max=V - 1)
        if d == 14:
            torch.as_strided(out, (B,), (1,), out.storage_offset()).copy_(ids)
        else:
            out.copy_(ids)

    @staticmethod
    def _segmented_scan(z, keep, zmax, u, V):
        """fp32 image of the summation order of csrc/sample.hip's inverse CDF before the draw became a block minimum: per-thread sequential
        sums over contiguous segments, a 64-lane Hillis-Steele scan, pre = inc - s, the 16 wave totals in order, cnt = #{run < x}."""
        B, seg = z.shape[0], X.seg_of(V)
        w = torch.where(keep, torch.exp((z - zmax).float()), torch.zeros(1)).float()
        e = torch.zeros(B, X.NT * seg)
        e[:, :V] = w
        e = e.view(B, X.NT, seg)
        s = torch.zeros(B, X.NT)
        for j in range(seg):
            s = s + e[:, :, j]
        inc = s.view(B, X.NWV, 64).clone()
        lane = torch.arange(64)
        o = 1
        while o < 64:
            up = torch.cat([torch.zeros(B, X.NWV, o), inc[:, :, :-o]], 2)
            inc = torch.where(lane >= o, inc + up, inc)
            o *= 2
        swave = inc[:, :, 63]
        pre = inc - s.view(B, X.NWV, 64)
        total = torch.zeros(B)
        for wv in range(X.NWV):
            pre[:, wv + 1:, :] = pre[:, wv + 1:, :] + swave[:, wv, None, None]
            total = total + swave[:, wv]
        x = (u.float() * total)[:, None]
        run = pre.reshape(B, X.NT)
        cnt = torch.zeros(B, dtype=torch.int64)
        i0 = torch.arange(X.NT) * seg
        for j in range(seg):
            run = run + e[:, :, j]
            cnt += ((i0 + j < V) & (run < x)).sum(1)
        return cnt.clamp(max=V - 1)


def ids(cs):
    return [c.id for c in cs]


@pytest.mark.parametrize("c", X.CASES, ids=ids(X.CASES))
def test_the_stand_in_passes_every_case_and_every_row_keeps_its_margins(c):
    r = X.reference(c.row)
    assert r.margin_prob >= X.MARGIN and r.margin_p >= X.MARGIN
    X.run_case(Torch(), c)


def test_the_all_banned_row_is_pinned_to_id_zero():
    X.all_banned_case(Torch())


def test_the_premise_check_passes_with_unit_weights():
    X.premise_case(Torch())


def test_the_table_reaches_every_route():
    rows = dict((c.row.name, c.row) for c in X.CASES)
    vs = set(r.V for r in rows.values())
    assert vs >= set([1, 2, 63, 64, 97, 1023, 1024, 1025, 2048, 3072, 3073, 30522, 30720, 31744])
    for V in (64, 1024, 1025, 3073, 30522, 30720, 31744):
        assert set(r.dtype for r in rows.values() if r.V == V) == set(["f32", "bf16"]), V
    ks = set(r.k for r in rows.values())
    assert ks >= set([0, 1, 2, 7, 16, 17, 64, 65, 1000])
    assert any(r.k == r.V - 1 for r in rows.values()) and any(r.k >= r.V for r in rows.values())
    assert set(r.ngram["n"] for r in rows.values() if r.ngram) == set([1, 2, 4])
    assert any(r.ngram and len(r.ngram["hist"]) > 1024 for r in rows.values())
    assert set(r.T for r in rows.values()) == set([0.5, 0.7, 1.0, 1.3, 2.0])
    assert all(len(X.probes(c.row, c.kind)[0]) <= 64 for c in X.CASES)


# the planted defects and the case each must fail (12: every named step case, and NO midpoint / end case of the table)
DEFECTS = {
    1: ("top-k drops ties with the k-th value", "iter-v97-f32-k7-T1-mid"),
    2: ("top-k keeps k + 1 distinct values", "iter-v30522-bf16-k2-T1-mid"),
    3: ("the bisection threshold is one float key low", "bis-v2048-k17-key-neighbour-mid"),
    4: ("top-p drops the token that crosses top_p", "p-v1025-alone-mid"),
    5: ("top-p takes its total over the unfiltered row", "p-v30522-narrow-k7-mid"),
    6: ("a ban is ignored for the row maximum", "iter-v30720-max-banned-k7-mid"),
    7: ("the n-gram filter ignores the special-token rule", "ngram-n4-v2048-special8-mid"),
    8: ("the n-gram prefix is read one time step early", "ngram-n4-v1025-bf16-k7-mid"),
    9: ("multiplication by 1 / temperature instead of a division", "div-tie-v1025-k7-T1.3-mid"),
    10: ("column V of the padding is read", "noise-v30522-f32-k40-T0.7-mid"),
    11: ("the draw uses run <= x", "tie-v30522-k64-step"),
    12: ("the inverse CDF sums in the kernel's segmented fp32 order (not monotone across threads)", "noise-v30522-f32-k64-T1.3-step"),
    13: ("the end clamp returns V - 1", "noise-v30522-f32-k40-T0.7-mid"),
    14: ("out is written densely, ignoring out_stride", "tie-v64-all-mid"),
    15: ("the history is read one column past hist_T", "ngram-n4-v30522-f32-k17-mid"),
}


@pytest.mark.parametrize("d", sorted(DEFECTS), ids=["%d-%s" % (d, DEFECTS[d][0].replace(" ", "_")) for d in sorted(DEFECTS)])
def test_every_planted_defect_is_caught_by_its_named_case(d):
    with pytest.raises(AssertionError):
        X.run_case(Torch(d), X.BY_ID[DEFECTS[d][1]])


def test_defects_are_also_caught_where_they_matter_most():
    """Further named cases: the second division-tie row, the n-gram cases of n = 2, the other end of the off-by-one key."""
    for d, cid in ((9, "div-tie-v30522-k17-T0.7-mid"), (8, "ngram-n2-v1025-f32-k7-mid"), (7, "ngram-n1-v1025-bf16-k7-mid"),
                   (11, "tie-v1024-k1000-step"), (1, "bis-v30522-k1000-mid"), (6, "tie-v1025-k17-maxbanned-mid")):
        with pytest.raises(AssertionError):
            X.run_case(Torch(d), X.BY_ID[cid])


def test_the_segmented_scan_is_caught_by_the_step_probes_and_only_by_them():
    """Defect 12 over the WHOLE table: every midpoint / end case passes; the step cases that fail return an id outside the kept set,
    and the named one is among them."""
    be = Torch(12)
    failed = []
    for c in X.CASES:
        if c.kind == "mid":
            X.run_case(be, c)
        else:
            try:
                X.run_case(be, c)
            except AssertionError as e:
                assert "NOT in the kept set" in str(e), str(e)
                failed.append(c.id)
    assert DEFECTS[12][1] in failed, failed
    assert not [f for f in failed if f.startswith("tie-")], failed     # (integer sums: monotone in any order)
