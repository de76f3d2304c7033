"""numpy statements of the two rules of the coreference attack's kernels, written from include/gstvd_hip.h (not from the
kernels): `topk_rule` for gstvd_cos_topk, `replace_rule` (+ `refresh_rule`) for gstvd_subseq_replace; and the exact-sum inputs
the bit-exact GPU tests use."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    """tests/golden/tiny_synonym.npz as numpy arrays (tools/make_golden_synonym.py; `words` is an array of strings)."""
    with np.load(os.path.join(GOLDEN, "tiny_synonym.npz")) as z:
        return {k: z[k] for k in z.files}


def topk_rule(dots, src, K, threshold=None):
    """dots [n, V] (any float type): dots[r, t] = dot(Ehat[src[r]], Ehat[t]); src [n] ints (outside [0, V): an empty row).
    -> idx int32 [n, K], val [n, K] in dots' dtype: the K best t != src[r] with dots >= threshold, larger value first, then the
    smaller index; unused slots -1 / 0."""
    dots = np.asarray(dots)
    n, V = dots.shape
    idx = np.full((n, K), -1, np.int32)
    val = np.zeros((n, K), dots.dtype)
    for r in range(n):
        s = int(src[r])
        if s < 0 or s >= V:
            continue
        order = np.lexsort((np.arange(V), -dots[r]))          # larger value first, then the smaller index
        keep = order[(order != s) & ((dots[r, order] >= threshold) if threshold is not None else True)][:K]
        idx[r, :keep.size] = keep
        val[r, :keep.size] = dots[r, keep]
    return idx, val


def exact_unit_rows(V, D, seed, nnz=16):
    """fp32 [V, D] rows with exactly `nnz` non-zeros of +-0.25 (D >= nnz): norm exactly 1 for nnz = 16, every dot product a
    multiple of 1/16 and exact in any summation order.  Few distinct values, hence many ties."""
    rng = np.random.RandomState(seed)
    E = np.zeros((V, D), np.float32)
    for v in range(V):
        cols = rng.choice(D, size=min(nnz, D), replace=False)
        E[v, cols] = rng.choice([-0.25, 0.25], size=cols.size)
    return E


def replace_rule(ids, plans, sep, pad, cont=None):
    """ids int64 [n, T]; plans: per row a list of (u, a, b).  -> (out int64 [n, T], n_replaced int32 [n])."""
    ids = np.asarray(ids)
    n, T = ids.shape
    out = np.empty_like(ids)
    count = np.zeros(n, np.int32)

    def is_cont(x):
        return cont is not None and 0 <= x < len(cont) and cont[x] != 0

    for r in range(n):
        row = [int(x) for x in ids[r]]
        for u, a, b in plans[r]:
            a, b = [int(x) for x in a], [int(x) for x in b]
            seps = [q for q, x in enumerate(row) if x == sep]
            if len(seps) < u + 1:
                continue
            lo = 1 if u == 0 else seps[u - 1] + 1
            hi = seps[u]
            new = row[:lo]
            q = lo
            while q < hi:
                hit = q + len(a) <= hi and row[q:q + len(a)] == a
                if hit and cont is not None:
                    hit = not is_cont(row[q]) and (q + len(a) == hi or not is_cont(row[q + len(a)]))
                if hit:
                    new += b
                    q += len(a)
                    count[r] += 1
                else:
                    new.append(row[q])
                    q += 1
            new += row[max(hi, lo):] if hi >= lo else row[lo:]
            row = (new + [pad] * T)[:T]
        out[r] = row
    return out, count


def refresh_rule(out_ids, sep, pad, max_sep, start_seg=None):
    """encode_input's segments, separator positions and attention mask, recomputed from a row of ids."""
    out_ids = np.asarray(out_ids)
    n, T = out_ids.shape
    seg = np.zeros((n, T), np.int64)
    sepi = np.zeros((n, max_sep), np.int64)
    att = (out_ids != pad).astype(np.float32)
    for r in range(n):
        cur = 0 if start_seg is None else int(start_seg[r])
        k = 0
        for q in range(T):
            x = int(out_ids[r, q])
            seg[r, q] = 0 if x == pad else cur
            if x == sep:
                if k < max_sep:
                    sepi[r, k] = q
                k += 1
                cur ^= 1
    return seg, sepi, att
