"""gstvd_subseq_replace on a real MI355X, bit for bit against tests/exact_synonym.py's `replace_rule` / `refresh_rule`.
Every launch writes into poisoned windows between guard rows that are checked afterwards."""
import numpy as np
import pytest
import torch

import exact_synonym as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLS, SEP, PAD = 101, 102, 0
MAX_SEP, GUARD, POISON = 25, 2, -777


def launch(ids, plans, cont=None, refresh=False, start_seg=None):
    from gst_visdial_amd import ops
    n, T = ids.shape
    dev_ids = torch.from_numpy(ids).to(DEV)
    out_buf = torch.full((n + 2 * GUARD, T), POISON, dtype=torch.int64, device=DEV)
    cnt_buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device=DEV)
    kw = {}
    bufs = {}
    if refresh:
        bufs = dict(segments=torch.full((n + 2 * GUARD, T), POISON, dtype=torch.int64, device=DEV),
                    sep_indices=torch.full((n + 2 * GUARD, MAX_SEP), POISON, dtype=torch.int64, device=DEV),
                    att_mask=torch.full((n + 2 * GUARD, T), float("nan"), dtype=torch.float32, device=DEV))
        kw = {k: v[GUARD:GUARD + n] for k, v in bufs.items()}
        if start_seg is not None:
            kw["start_seg"] = torch.tensor(start_seg, dtype=torch.int64, device=DEV)
    c = None if cont is None else torch.from_numpy(cont).to(DEV)
    out, cnt = ops.subseq_replace(dev_ids, plans, cls=CLS, sep=SEP, pad=PAD, cont=c, out=out_buf[GUARD:GUARD + n],
                                  n_replaced=cnt_buf[GUARD:GUARD + n], **kw)
    torch.cuda.synchronize()
    assert torch.equal(dev_ids.cpu(), torch.from_numpy(ids))                     # the input is never written
    for b in (out_buf, cnt_buf) + tuple(v for k, v in bufs.items() if k != "att_mask"):
        assert bool((b[:GUARD] == POISON).all()) and bool((b[GUARD + n:] == POISON).all()), "guard rows written"
    if refresh:
        a = bufs["att_mask"]
        assert bool(torch.isnan(a[:GUARD]).all()) and bool(torch.isnan(a[GUARD + n:]).all())
    return out.cpu().numpy(), cnt.cpu().numpy(), {k: v.cpu().numpy() for k, v in kw.items() if k != "start_seg"}


def check(ids, plans, cont=None, start_seg=None):
    want, want_n = X.replace_rule(ids, plans, SEP, PAD, cont)
    got, got_n, _ = launch(ids, plans, cont)                                      # refresh outputs null
    assert np.array_equal(got, want) and np.array_equal(got_n, want_n)
    got, got_n, extra = launch(ids, plans, cont, refresh=True, start_seg=start_seg)
    assert np.array_equal(got, want) and np.array_equal(got_n, want_n)
    seg, sepi, att = X.refresh_rule(want, SEP, PAD, MAX_SEP, start_seg)
    assert np.array_equal(extra["segments"], seg) and np.array_equal(extra["sep_indices"], sepi)
    assert np.array_equal(extra["att_mask"], att)
    return want, want_n


def row(T, utterances):
    r = [CLS]
    for u in utterances:
        r += list(u) + [SEP]
    assert len(r) <= T
    return np.array(r + [PAD] * (T - len(r)), np.int64)


@pytest.mark.parametrize("T", [8, 64, 256])
def test_utterances_and_lengths(T):
    if T == 8:
        ids = np.stack([row(T, [[5, 6], [7], [5]])])
        for u, want_row in ((0, [CLS, 9, 9, 6, SEP, 7, SEP, 5]), (2, [CLS, 5, 6, SEP, 7, SEP, 9, 9]), (3, None), (1, None)):
            want, n = check(ids, [[(u, [5], [9, 9])]])
            if want_row is not None:
                assert want[0].tolist() == want_row and n[0] == 1                 # utterance 2: its [SEP] is pushed out
            else:
                assert np.array_equal(want, ids) and n[0] == 0
        return
    long_a, long_b = list(range(200, 216)), list(range(300, 316))
    utts = [[5, 6, 7, 5, 6], [8, 5, 9], long_a + [5], [5, 6], [11, 12, 5]]
    ids = np.stack([row(T, utts)] * 2)
    for u in (0, 2, 4, 5):                                                        # first, a middle one, the last, a missing one
        for a, b in (([5, 6], [40]), ([5], [41, 42, 43]), ([5], [44]), (long_a, [45]), ([5], long_b)):
            want, n = check(ids, [[(u, a, b)], []])
            assert np.array_equal(want[1], ids[1]) and n[1] == 0                  # a row with an empty list
            if u == 5:
                assert np.array_equal(want[0], ids[0]) and n[0] == 0
    want, n = check(ids, [[(2, long_a, [45])], [(0, [5, 6], [40])]], start_seg=[1, 0])
    assert n.tolist() == [1, 2]


def test_matching_rules():
    T = 64
    x = 30
    ids = np.stack([row(T, [[x, x, x], [x, x, x, x, 7], [7, x], [x]])])
    want, n = check(ids, [[(0, [x, x], [50])]])                                   # overlapping candidates: one match, left first
    assert want[0, :4].tolist() == [CLS, 50, x, SEP] and n[0] == 1
    want, n = check(ids, [[(1, [x, x], [50])]])
    assert n[0] == 2
    want, n = check(ids, [[(2, [7], [51]), (2, [x], [52])]])                      # first and last token of an utterance
    assert n[0] == 2
    want, n = check(ids, [[(2, [x, SEP, x], [53])], ])                            # straddles a [SEP]: wholly inside fails
    assert n[0] == 0 and np.array_equal(want, ids)
    want, n = check(ids, [[(1, [7, SEP], [53])]])
    assert n[0] == 0
    want, n = check(ids, [[(0, [x], [60, 61]), (0, [61, 60], [62])]])             # the second matches text the first produced
    assert n[0] == 3 + 2 and want[0, :6].tolist() == [CLS, 60, 62, 62, 61, SEP]


def test_continuation_pieces():
    T = 64
    cont = np.zeros(400, np.uint8)
    cont[300:] = 1                                                                # ids from 300 on are "##" pieces
    ids = np.stack([row(T, [[20, 21, 300, 20, 21], [310, 20, 21, 22], [20, 21]])])
    want, n = check(ids, [[(0, [20, 21], [70])]], cont)                           # the first is followed by a ## piece: no match
    assert n[0] == 1 and want[0, :6].tolist() == [CLS, 20, 21, 300, 70, SEP]
    _, n = check(ids, [[(0, [20, 21], [70])]])                                    # without cont both match
    assert n[0] == 2
    _, n = check(ids, [[(1, [310, 20], [71])]], cont)                             # starts on a ## piece
    assert n[0] == 0
    _, n = check(ids, [[(1, [20, 21], [72]), (2, [20, 21], [73])]], cont)         # followed by a word / by the utterance's end
    assert n[0] == 2
    _, n = check(ids, [[(1, [500], [72])]], cont)                                 # ids outside the vocabulary read nothing
    assert n[0] == 0


def test_growth_past_T_drops_tokens():
    T = 64
    big = list(range(300, 316))
    utts = [[5] * 10, [6] * 10, [7] * 10, [8] * 10, [9] * 10]                     # 56 tokens
    ids = np.stack([row(T, utts)])
    want, n = check(ids, [[(0, [5], big)]])                                       # 10 x 16 tokens: utterance 0 alone overflows
    assert n[0] == 10 and int((want[0] == SEP).sum()) == 0 and int((want[0] == PAD).sum()) == 0
    want, n = check(ids, [[(1, [6], [40, 41])]])                                  # +10: the last [SEP] and one token fall out
    assert n[0] == 10 and int((want[0] == SEP).sum()) == 4 and want[0, -1] == 9
    want, n = check(ids, [[(1, [6], [40, 41]), (4, [9], [77])]])                  # utterance 4 has lost its [SEP]: a no-op now
    assert n[0] == 10
    want, n = check(ids, [[(0, [5] * 10, [1])]])                                  # shrinks: padded behind
    assert n[0] == 1 and int((want[0] == PAD).sum()) == 8 + 9


def test_hundred_rows():
    T = 256
    rng = np.random.RandomState(5)
    rows, plans = [], []
    for r in range(100):
        utts = [rng.randint(10, 16, size=rng.randint(1, 12)).tolist() for _ in range(rng.randint(4, 15))]
        rows.append(row(T, utts))
        plan = []
        for _ in range(rng.randint(0, 5)):
            a = rng.randint(10, 16, size=rng.randint(1, 3)).tolist()
            b = rng.randint(10, 16, size=rng.randint(1, 17)).tolist()
            plan.append((int(rng.randint(0, 6)), a, b))
        plans.append(plan)
    ids = np.stack(rows)
    want, n = check(ids, plans, start_seg=rng.randint(0, 2, size=100).tolist())
    assert int(n.sum()) > 100 and int((n == 0).sum()) > 0
    check(ids[:1], plans[:1])                                                     # n = 1


def test_refusals():
    from gst_visdial_amd import ops, _lib
    ids = torch.zeros(2, 8, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.GstvdError):
        ops.subseq_replace(ids, [[(0, [], [1])], []])
    with pytest.raises(_lib.GstvdError):
        ops.subseq_replace(ids, [[(0, [1] * 17, [1])], []])
    with pytest.raises(_lib.GstvdError):
        ops.subseq_replace(ids, [[]])                                             # one plan for two rows
    with pytest.raises(_lib.GstvdError):
        ops.subseq_replace(ids, [[], []], out=ids)
