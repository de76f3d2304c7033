"""Numpy rules shared by the masked-LM fill-in tests (tests/test_mlm_fill_cpu.py, test_vocab_argmax_exact_gpu.py,
test_mlm_fill_gpu.py): the total order of the vocabulary arg-max, the fill rule of the random-token attack, and exact operands.

Total order (include/gstvd_hip.h): the larger value wins, equal values go to the SMALLER column; columns >= V are no candidates.

Exact operands: integer-valued entries in [-8, 8] (exact in bf16), so every partial sum of a dot product over H <= 768 terms is an
integer of magnitude <= 768 * 64 < 2^24 -- exact in fp32 in ANY order -- and a bias in halves keeps the sum exact.  The reference
is int64 / float64 arithmetic; the device result must equal it to the bit."""
import numpy as np


def round_up(x, m):
    return (x + m - 1) // m * m


def argmax_rows(z, V):
    """(idx [n] int64, val [n]) of z[:, :V] under the total order (numpy's argmax returns the first = smallest column)."""
    z = np.asarray(z)[:, :V]
    idx = z.argmax(axis=1).astype(np.int64)
    return idx, z[np.arange(z.shape[0]), idx]


def exact_logits(x, w, bias, V):
    """z[r, v] = sum_k x[r, k] * w[v, k] + bias[v] for v < V, in float64: the operands are small integers, so every product and
    partial sum is an integer far below 2^53 and the float64 product (BLAS, any order) IS the int64 one."""
    acc = np.asarray(x, dtype=np.float64) @ np.asarray(w, dtype=np.float64)[:V].T
    assert np.array_equal(acc, np.round(acc))
    return acc + np.asarray(bias, dtype=np.float64)[:V]


def exact_operands(n, H, V, seed):
    """x [n, H], w [round_up(V, 64), H] integer-valued in [-8, 8] (float32 arrays), bias [round_up(V, 64)] in halves in [-4, 4]."""
    rng = np.random.RandomState(seed)
    Vp = round_up(V, 64)
    x = rng.randint(-8, 9, size=(n, H)).astype(np.float32)
    w = rng.randint(-8, 9, size=(Vp, H)).astype(np.float32)
    bias = (rng.randint(-8, 9, size=(Vp,)) / 2.0).astype(np.float32)
    return x, w, bias


def poison_padding(w, bias, V):
    """Rows [V, Vp) of the table and of the bias get the largest values an operand can hold: chosen, they would win everywhere."""
    w[V:] = 8.0
    bias[V:] = 1.0e30
    return w, bias


def cap_bias(bias, V, cap=0.0):
    """No bias above `cap` among the candidates: a planted column (all-8 row, bias >= cap) cannot be beaten by an unplanted one
    whose dot product is at most equal."""
    bias[:V] = np.minimum(bias[:V], cap)


def fill_rule(input_ids, mask_token_id, logits=None, argmax=None):
    """The rule of the random-token attack, restated: only row 0 is read; its positions equal to mask_token_id receive, in
    ascending position order, the arg-max over the vocabulary of `logits` [n_mask, V] (or the given `argmax` [n_mask]); the result
    is that row repeated B times.  No mask position: row 0 repeated unchanged.  The input is not modified."""
    ids = np.asarray(input_ids)
    row = ids[0].copy()
    pos = np.nonzero(row == mask_token_id)[0]
    if pos.size:
        if argmax is None:
            argmax, _ = argmax_rows(logits, np.asarray(logits).shape[1])
        assert len(argmax) == pos.size
        row[pos] = np.asarray(argmax, dtype=row.dtype)
    return np.repeat(row[None, :], ids.shape[0], axis=0)
