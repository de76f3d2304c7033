"""Exact layer of the self-training glue tests: both rules of csrc/dialog.hip stated in numpy, case tables,
and a harness that runs a backend on them inside canary-filled windows.

Both kernels are integer work on token ids, so there is no tolerance anywhere: every output must be torch.equal to the rule.

  append_rule   gstvd_context_append: `generate.append_to_context` per row, plus the attention mask, the full-row case (which the
                host function raises on: the rule records it in `full`) and the OR-ed `abnormal` flags.
  rows_rule     gstvd_dialog_rows: dataloader/dataloader_cc12m_gen.py:104-248 through utils/data_utils.encode_input, on token ids.
                tests/test_exact_dialog_harness_cpu.py pins it, bit for bit, to tests/golden/selftrain_rows.npz, which
                tools/make_golden_selftrain.py records from the reference's own encode_input.

Windows.  Every array a kernel writes is a window inside a larger allocation that holds a fixed canary pattern (exact_gemm.Window):
row stride > row length, guard rows in front and behind.  Nothing outside the window may change.  The logical outputs of
gstvd_dialog_rows are pre-filled with POISON, a value no rule produces: the kernel promises to write every element exactly once,
so an element it skips shows up.  In-place arrays of gstvd_context_append hold their inputs; the rule says which elements move.

Plain helper module: no fixtures, no hooks.  Everything takes a backend `be` (be.device, be.append(...) / be.rows(...) with the
signatures of ops.context_append / ops.dialog_rows), so the CPU harness test proves the harness on a numpy stand-in and
tests/test_dialog_exact_gpu.py runs it on the HIP kernels.
"""
import collections

import numpy as np
import torch

from exact_gemm import Window

CLS, SEP, MASK = 101, 102, 103
SPECIAL = (0, 100, 101, 102, 103)
S_MAX = 25
POISON = -7777777                       # no id, position, segment or label; as fp32 no mask value either
V0, V1 = 104, 320                       # ordinary token ids (the tiny vocabulary)


# ------------------------------------------------------------------------------------------------------------ the append rule
def append_rule(ctx_ids, ctx_len, new_ids, sep_id, segments=None, segment_value=0, att_mask=None, abnormal=None, full=None):
    """numpy statement of gstvd_context_append.  Returns a dict of NEW arrays: ctx_ids, ctx_len, segments, att_mask (None when not
    given), n_out, abnormal, full (the incoming flags OR-ed with this call's)."""
    ctx, ln = np.array(ctx_ids, dtype=np.int64), np.array(ctx_len, dtype=np.int64)
    seg = None if segments is None else np.array(segments, dtype=np.int64)
    att = None if att_mask is None else np.array(att_mask, dtype=np.float32)
    B, T = ctx.shape
    ab = np.zeros(B, np.int32) if abnormal is None else np.array(abnormal, dtype=np.int32)
    fu = np.zeros(B, np.int32) if full is None else np.array(full, dtype=np.int32)
    n_out = np.zeros(B, np.int64)
    for b in range(B):
        n, start = int((np.asarray(new_ids[b]) != 0).sum()), int(ln[b])
        if 0 <= start and start + n <= T:
            ctx[b, start:start + n] = np.asarray(new_ids[b])[:n]
            n_eff = n
        elif 0 <= start < T:
            ctx[b, start] = sep_id
            n_eff, ab[b] = 1, 1
        else:
            n_eff, ab[b], fu[b] = 0, 1, 1
        if seg is not None:
            seg[b, start:start + n_eff] = segment_value
        if att is not None:
            att[b, start:start + n_eff] = ctx[b, start:start + n_eff] != 0
        ln[b] += n_eff
        n_out[b] = n_eff
    return dict(ctx_ids=ctx, ctx_len=ln, segments=seg, att_mask=att, n_out=n_out, abnormal=ab, full=fu)


AppendCase = collections.namedtuple("AppendCase", "name ctx_ids ctx_len new_ids sep_id segments segment_value with_att abnormal full")


def _ctx(T, lens, gen):
    ids = np.zeros((len(lens), T), np.int64)
    for b, L in enumerate(lens):
        ids[b, :min(L, T)] = gen.integers(V0, V1, min(L, T))
    return ids


def _new(U, ns, gen, interior_zero=()):
    new = np.zeros((len(ns), U), np.int64)
    for b, n in enumerate(ns):
        new[b, :n] = gen.integers(V0, V1, n)
    for b, c in interior_zero:                                        # a zero among the first n entries; the count stays n
        new[b, c], new[b, ns[b]] = 0, int(gen.integers(V0, V1))
    return new


def append_edge_cases(T=32, U=6):
    """The edge table: start + n == T, == T + 1, start == T - 1 with n = 2, n = 0, a full row (start == T), an interior zero, with
    and without segments; flags that come in set stay set."""
    gen = np.random.default_rng(7)
    lens = [T - 4, T - 3, T - 1, 10, T, 12, 0, T - 6]
    ns = [4, 4, 2, 0, 3, 4, U, U]                                     # fits exactly | one over | T-1 + 2 | nothing | full | zero | empty ctx | U
    out = []
    for with_seg in (False, True):
        ids = _ctx(T, lens, gen)
        new = _new(U, ns, gen, interior_zero=[(5, 1)])
        seg = (ids != 0).astype(np.int64) * gen.integers(0, 2, ids.shape) if with_seg else None
        ab = np.zeros(len(lens), np.int32)
        ab[3] = 1                                                      # set by an earlier call: never cleared
        out.append(AppendCase("edges_T%d_U%d_%s" % (T, U, "seg" if with_seg else "noseg"), ids, np.array(lens, np.int64), new, SEP,
                              seg, 1, with_seg, ab, np.zeros(len(lens), np.int32)))
    return out


def append_random_cases(count, T=32, U=18, seed=11, allow_full=False):
    """`count` single-row cases folded into batches of 8: random context lengths and answer lengths, overflow included."""
    gen = np.random.default_rng(seed)
    out = []
    for i in range(0, count, 8):
        rows = min(8, count - i)
        lens = [int(x) for x in gen.integers(0, T + (1 if allow_full else 0), rows)]
        ns = [int(x) for x in gen.integers(0, U + 1, rows)]
        zero = [(b, int(gen.integers(0, ns[b]))) for b in range(rows) if 2 <= ns[b] < U and gen.random() < 0.25]
        ids, new = _ctx(T, lens, gen), _new(U, ns, gen, interior_zero=zero)
        with_seg = bool(i // 8 % 2)
        seg = gen.integers(0, 2, ids.shape).astype(np.int64) if with_seg else None
        out.append(AppendCase("random%d_T%d_U%d" % (i, T, U), ids, np.array(lens, np.int64), new, SEP, seg, int(gen.integers(0, 2)),
                              bool(i // 8 % 3), np.zeros(rows, np.int32), np.zeros(rows, np.int32)))
    return out


# -------------------------------------------------------------------------------------------------------------- the rows rule
def utterances(cap, ques, ans, special=SPECIAL):
    """(caption, questions, answers) of one dialog as lists of ids under the rule's definitions."""
    cap = [int(v) for v in cap]
    cap = cap[:cap.index(0)] if 0 in cap else cap
    keep = lambda row: [int(v) for v in row if int(v) not in special]
    return cap, [keep(r) for r in ques], [keep(r) for r in ans]


def rows_rule(cap, ques, ans, ppl, T, Ud, select_data, threshold, mask_prob, valid=None, u_tok=None, cls=CLS, sep=SEP, mask=MASK,
              special=SPECIAL, S=S_MAX):
    """numpy statement of gstvd_dialog_rows.  Returns the nine output arrays, [B, R, .]."""
    cap, ques, ans, ppl = np.asarray(cap), np.asarray(ques), np.asarray(ans), np.asarray(ppl, dtype=np.float32)
    B, R, U = ques.shape
    assert R >= 1 and 2 * R <= S and U <= 64 and cap.shape[1] <= 64 and T >= 2 and Ud >= 3
    assert mask_prob == 0 or u_tok is not None
    o = dict(enc_ids=np.zeros((B, R, T), np.int64), enc_seg=np.zeros((B, R, T), np.int64), enc_mlm=np.full((B, R, T), -1, np.int64),
             enc_att=np.zeros((B, R, T), np.float32), enc_sep=np.zeros((B, R, S), np.int64), enc_hist_len=np.zeros((B, R), np.int64),
             dec_ids=np.zeros((B, R, Ud), np.int64), dec_labels=np.zeros((B, R, Ud), np.int64), dec_att=np.zeros((B, R, Ud), np.float32))
    for b in range(B):
        c, qs, as_ = utterances(cap[b], ques[b], ans[b], special)
        for j in range(R):
            utts = [c]
            for k in range(j):
                utts += [qs[k], as_[k]]
            utts.append(qs[j])
            ids, seg, mlm, seps, cur = [cls], [1], [-1], [], 1
            for utt in utts:
                for t in utt:
                    p = len(ids)
                    hit = u_tok is not None and p < T and float(np.float64(np.float32(u_tok[b, j, p]))) < float(mask_prob)
                    ids.append(mask if hit else t), seg.append(cur), mlm.append(t if hit else -1)
                ids.append(sep), seg.append(cur), mlm.append(-1)
                seps.append(len(ids) - 1)
                cur ^= 1
            n = min(len(ids), T)
            o["enc_ids"][b, j, :n], o["enc_seg"][b, j, :n], o["enc_mlm"][b, j, :n] = ids[:n], seg[:n], mlm[:n]
            o["enc_att"][b, j] = o["enc_ids"][b, j] != 0
            o["enc_sep"][b, j, :min(len(seps), S)] = seps[:S]
            o["enc_hist_len"][b, j] = 2 * j + 1
            dec = ([cls] + as_[j][:Ud - 2] + [sep] + [0] * Ud)[:Ud]
            dec = np.array(dec, np.int64)
            o["dec_att"][b, j] = dec != 0
            zero = (bool(select_data) and float(np.float64(ppl[b, j])) >= float(threshold)) or (valid is not None and int(valid[b]) == 0)
            if not zero:
                o["dec_labels"][b, j, :-1] = dec[1:]
            dec[dec == sep] = 0
            o["dec_ids"][b, j] = dec
    return o


RowsCase = collections.namedtuple("RowsCase", "name cap ques ans ppl valid u_tok T Ud select_data threshold mask_prob")
ROWS_OUT = ("enc_ids", "enc_seg", "enc_mlm", "enc_att", "enc_sep", "enc_hist_len", "dec_ids", "dec_labels", "dec_att")


def _utt_rows(shape, gen, U):
    """Sampled-looking rows: 1..U-1 ordinary tokens, then [SEP] and padding -- or U tokens without [SEP]; some rows empty (a lone
    [SEP]) and some with special ids 100 / 101 / 103 inside."""
    rows = np.zeros(shape + (U,), np.int64)
    for idx in np.ndindex(*shape):
        kind = gen.random()
        n = 0 if kind < 0.1 else U if kind < 0.25 else int(gen.integers(1, U))
        rows[idx][:n] = gen.integers(V0, V1, n)
        if n < U:
            rows[idx][n] = SEP
        if n >= 3 and gen.random() < 0.3:
            rows[idx][int(gen.integers(0, n))] = (100, 101, 103)[int(gen.integers(0, 3))]
    return rows


def rows_cases(B=3, T=32):
    """The table: U in {6, 18} x Lc in {8, 38} x R in {1, 3, 12}, mask_prob 0 and 0.15, Ud 6 and 25, perplexities on both sides of
    the threshold (at it, one fp32 below, +inf, NaN), one invalid dialog."""
    gen = np.random.default_rng(23)
    thr = 50.0
    below = float(np.nextafter(np.float32(thr), np.float32(0)))
    out = []
    for U in (6, 18):
        for Lc in (8, 38):
            for R in (1, 3, 12):
                cap = np.zeros((B, Lc), np.int64)
                for b, n in enumerate([Lc, max(1, Lc // 3), 0][:B]):           # full width (no zero), short, empty
                    cap[b, :n] = gen.integers(V0, V1, n)
                ques, ans = _utt_rows((B, R), gen, U), _utt_rows((B, R), gen, U)
                ppl = gen.choice(np.array([thr, below, np.inf, np.nan, 3.5, 70.0], np.float32), (B, R)).astype(np.float32)
                mp = 0.15 if (R + U + Lc) % 2 else 0.0
                u = gen.random((B, R, T)).astype(np.float32)
                u.flat[::7] = np.float32(0.15)                                  # the strict comparison: never masked
                u.flat[3::7] = np.nextafter(np.float32(0.15), np.float32(0))
                valid = np.array([1, 1, 0][:B], np.int32) if R == 3 else None
                out.append(RowsCase("U%d_Lc%d_R%d_p%g" % (U, Lc, R, mp), cap, ques, ans, ppl, valid, u if (mp > 0 or R == 12) else None,
                                    T, 6 if U == 6 else 25, 1 if R != 1 else 0, thr, mp))
    return out


# ------------------------------------------------------------------------------------------------------------------ the harness
def _t(x, device, dtype=None):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=dtype).to(device)


def _window(values, dtype, device, pad):
    """A canary-surrounded window (row stride = cols + pad) that holds `values`."""
    v = torch.as_tensor(np.asarray(values)).to(dtype)
    w = Window(v.shape[0], v.shape[1], dtype, device, "canary", ld=v.shape[1] + pad)
    w.view.copy_(v.to(device))
    return w


def _vec(values, dtype, device):
    """A 1-D array as the window of a 1 x n allocation (contiguous, canaries in front and behind)."""
    v = torch.as_tensor(np.asarray(values)).to(dtype).reshape(1, -1)
    w = Window(1, v.shape[1], dtype, device, "canary", guard=1)
    w.view.copy_(v.to(device))
    return w


def _i32_vec(values, device):
    """int32 flags: a slice of a larger int32 buffer whose surroundings hold a pattern (Window knows no int32)."""
    v = torch.as_tensor(np.asarray(values), dtype=torch.int32)
    buf = torch.full((v.numel() + 16,), 0x4B5A17C3, dtype=torch.int32, device=device)
    buf[8:8 + v.numel()] = v.to(device)
    return buf, buf[8:8 + v.numel()]


def _i32_intact(buf, n, name):
    assert bool((buf[:8] == 0x4B5A17C3).all()) and bool((buf[8 + n:] == 0x4B5A17C3).all()), "%s: written outside the flags" % name


def run_append_case(be, c):
    """One launch of `be.append` on case c inside windows, against append_rule; then once more from the same inputs: same bits."""
    dev = be.device
    want = append_rule(c.ctx_ids, c.ctx_len, c.new_ids, c.sep_id, c.segments, c.segment_value,
                       (np.asarray(c.ctx_ids) != 0).astype(np.float32) if c.with_att else None, c.abnormal, c.full)
    B = len(c.ctx_len)
    got = []
    for rep in range(2):
        ctx = _window(c.ctx_ids, torch.int64, dev, 3)
        seg = None if c.segments is None else _window(c.segments, torch.int64, dev, 5)
        att = _window((np.asarray(c.ctx_ids) != 0), torch.float32, dev, 1) if c.with_att else None
        ln, n_out = _vec(c.ctx_len, torch.int64, dev), _vec(np.full(B, POISON), torch.int64, dev)
        new = _t(c.new_ids, dev, torch.int64)
        ab_buf, ab = _i32_vec(c.abnormal, dev)
        fu_buf, fu = _i32_vec(c.full, dev)
        new0 = new.clone()
        be.append(ctx.view, ln.vector(), new, c.sep_id, ab, fu, segments=None if seg is None else seg.view,
                  segment_value=c.segment_value, att_mask=None if att is None else att.view, n_out=n_out.vector())
        res = dict(ctx_ids=ctx.view, ctx_len=ln.vector(), n_out=n_out.vector(), abnormal=ab, full=fu)
        if seg is not None:
            res["segments"] = seg.view
        if att is not None:
            res["att_mask"] = att.view
        for k, v in res.items():
            ref = torch.as_tensor(want[k]).to(v.dtype)
            assert torch.equal(v.cpu(), ref), "%s: %s differs from the rule\n%s\n%s" % (c.name, k, v.cpu(), ref)
        for w, name in ((ctx, "ctx_ids"), (seg, "segments"), (att, "att_mask"), (ln, "ctx_len"), (n_out, "n_out")):
            if w is not None:
                w.assert_surroundings_untouched("%s %s" % (c.name, name))
        _i32_intact(ab_buf, B, c.name + " abnormal"), _i32_intact(fu_buf, B, c.name + " full")
        assert torch.equal(new, new0), c.name + ": new_ids was written"
        got.append({k: v.cpu().clone() for k, v in res.items()})
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), "%s: %s differs between two launches" % (c.name, k)
    return got[0]


def rows_windows(B, R, T, Ud, device, S=S_MAX):
    """The nine outputs as windows [B * R, .]: POISON inside, canaries around; the enc_* arrays share one row stride, the dec_* too."""
    n = B * R
    cols = dict(enc_ids=T, enc_seg=T, enc_mlm=T, enc_att=T, enc_sep=S, dec_ids=Ud, dec_labels=Ud, dec_att=Ud)
    pad = dict(enc_ids=3, enc_seg=3, enc_mlm=3, enc_att=3, enc_sep=2, dec_ids=1, dec_labels=1, dec_att=1)
    w = {}
    for k, ccount in cols.items():
        dtype = torch.float32 if k.endswith("att") else torch.int64
        w[k] = Window(n, ccount, dtype, device, "canary", ld=ccount + pad[k])
        w[k].view.fill_(POISON)
    w["enc_hist_len"] = Window(1, n, torch.int64, device, "canary", guard=1)
    w["enc_hist_len"].view.fill_(POISON)
    return w


def check_rows(name, w, want, B, R):
    for k in ROWS_OUT:
        v = (w[k].vector() if k == "enc_hist_len" else w[k].view).cpu()
        assert not bool((v == POISON).any()), "%s: %s has elements the launch did not write" % (name, k)
        ref = torch.as_tensor(want[k]).reshape(v.shape).to(v.dtype)
        assert torch.equal(v, ref), "%s: %s differs from the rule at %s" % (name, k, (v != ref).nonzero()[:6].tolist())
        w[k].assert_surroundings_untouched("%s %s" % (name, k))


def run_rows_case(be, c, want=None):
    """`be.rows` on case c into poisoned windows, against rows_rule (or the recorded `want`); twice: same bits."""
    dev = be.device
    B, R, _ = np.asarray(c.ques).shape
    if want is None:
        want = rows_rule(c.cap, c.ques, c.ans, c.ppl, c.T, c.Ud, c.select_data, c.threshold, c.mask_prob, c.valid, c.u_tok)
    ins = [_t(c.cap, dev, torch.int64), _t(c.ques, dev, torch.int64), _t(c.ans, dev, torch.int64), _t(c.ppl, dev, torch.float32)]
    keep = [x.clone() for x in ins]
    got = []
    for rep in range(2):
        w = rows_windows(B, R, c.T, c.Ud, dev)
        out = {k: (w[k].vector() if k == "enc_hist_len" else w[k].view) for k in ROWS_OUT}
        be.rows(ins[0], ins[1], ins[2], ins[3], c.T, c.Ud, c.select_data, c.threshold, c.mask_prob, valid=_t(c.valid, dev, torch.int32),
                u_tok=_t(c.u_tok, dev, torch.float32), out=out)
        check_rows(c.name, w, want, B, R)
        got.append({k: out[k].cpu().clone() for k in ROWS_OUT})
    for k in ROWS_OUT:
        assert torch.equal(got[0][k], got[1][k]), "%s: %s differs between two launches" % (c.name, k)
    for x, y in zip(ins, keep):
        bits = (lambda t: t.view(torch.int32)) if x.dtype == torch.float32 else (lambda t: t)      # NaN perplexities: compare bits
        assert torch.equal(bits(x), bits(y)), c.name + ": an input was written"
    return got[0]


def fixture_cases(g):
    """The cases of tests/golden/selftrain_rows.npz (a dict of numpy arrays) as (RowsCase, recorded outputs) pairs."""
    names = sorted(set(k.split("::")[0] for k in g))
    out = []
    for n in names:
        f = lambda k: np.asarray(g["%s::%s" % (n, k)])
        has = lambda k: ("%s::%s" % (n, k)) in g
        c = RowsCase(n, f("cap"), f("ques"), f("ans"), f("ppl"), f("valid") if has("valid") else None, f("u_tok") if has("u_tok") else None,
                     int(f("T")), int(f("Ud")), int(f("select_data")), float(f("threshold")), float(f("mask_prob")))
        out.append((c, {k: f("out_" + k) for k in ROWS_OUT}))
    return out


class NumpyBackend(object):
    """Stand-in backend: the rules themselves, written into the caller's tensors (proves the harness without a GPU)."""
    device = "cpu"

    def append(self, ctx_ids, ctx_len, new_ids, sep_id, abnormal, full, segments=None, segment_value=0, att_mask=None, n_out=None):
        r = append_rule(ctx_ids.numpy(), ctx_len.numpy(), new_ids.numpy(), sep_id, None if segments is None else segments.numpy(),
                        segment_value, None if att_mask is None else att_mask.numpy(), abnormal.numpy(), full.numpy())
        for dst, k in ((ctx_ids, "ctx_ids"), (ctx_len, "ctx_len"), (segments, "segments"), (att_mask, "att_mask"), (n_out, "n_out"),
                       (abnormal, "abnormal"), (full, "full")):
            if dst is not None:
                dst.copy_(torch.as_tensor(r[k]))

    def rows(self, cap, ques, ans, ppl, T, Ud, select_data, threshold, mask_prob, valid=None, u_tok=None, out=None):
        r = rows_rule(cap.numpy(), ques.numpy(), ans.numpy(), ppl.numpy(), T, Ud, select_data, threshold, mask_prob,
                      None if valid is None else valid.numpy(), None if u_tok is None else u_tok.numpy())
        for k in ROWS_OUT:
            out[k].copy_(torch.as_tensor(r[k]).reshape(out[k].shape))
        return out
