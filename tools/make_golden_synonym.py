"""Fixture of the coreference attack's synonym table: tests/golden/tiny_synonym.npz.

Runs in the build container only.  It imports the reference tree through oracle.ref_harness and copies none of its text: it
writes a small word-vector file in the counter-fitted vectors' text format, RUNS the reference's own comp_cos_sim_mat.py on it
in a temporary directory (the script writes ./data/visdial/cos_sim_counter_fitting.npy and the two pickles relative to its
working directory), then CALLS the reference's TextAttack.pick_most_similar_words_batch (utils/text_attack.py:103-116) on the
matrix it wrote, on an instance made without its constructor, and records what comes back.

    python tools/make_golden_synonym.py

Embeddings: V = 512 words, D = 300, 128 clusters of four: centre + 0.6 x noise, both standard normal, so a word's three cluster
mates have cosine ~ 1 / 1.36 = 0.74 and every other word ~ N(0, 1 / sqrt(300)).  The generator asserts that no cosine lies
within 0.08 of the 0.5 cut.  The values are multiples of 2^-10, exact in fp32, and written with ten decimals, which states them exactly: the float64 numbers the
reference script parses are the fp32 values.

What is recorded:
  * emb fp32 [512, 300], words (one string per row, unique), K = 10, threshold = 0.5;
  * ref_idx int32 [512, 10], ref_val fp32 [512, 10]: the reference's neighbours of every word (its words mapped back through its
    own word2idx) and their values, -1 / 0 behind the last one that passes the cut; ref_count [512];
  * checked bool [512, 10]: for a used slot, whether the float64 cosine at that rank differs by more than GAP = 4e-5 from both of
    its neighbours in the row's sorted order (self excluded) -- where it does not, fp32 rounding may order the two either way and
    the index says nothing; unused slots are checked (nothing lies near the cut);
The unit rows are not stored: emb / norm in float64, cast to fp32, is what the reference script forms and what
SynonymTable.build forms.
The reference's coreference_attack itself is not driven here: it needs pytorch_transformers' BertTokenizer with the old `decode`
that returns a list of segments, which the installed transformers does not provide.
"""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                   # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, GOLDEN                # noqa: E402
from tools.make_golden_mlm_fill import install_tokenizer_stub          # noqa: E402

SEED, V, D, CLUSTER, NOISE, K, THRESHOLD, GAP, CLEAR = 7, 512, 300, 4, 0.6, 10, 0.5, 4e-5, 0.08


def main():
    rng = np.random.RandomState(SEED)
    centres = rng.standard_normal((V // CLUSTER, D))
    emb = np.repeat(centres, CLUSTER, axis=0) + NOISE * rng.standard_normal((V, D))
    emb = (np.round(emb * 1024.0) / 1024.0).astype(np.float32)          # multiples of 2^-10: ten decimals state them exactly
    emb = emb[rng.permutation(V)]                                       # cluster mates are not neighbours in the file
    words = ["w%04d" % i for i in range(V)]
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data", "visdial"))
        path = os.path.join(tmp, "vectors.txt")
        with open(path, "w") as f:
            for w, row in zip(words, emb):
                f.write(w + " " + " ".join("%.10f" % x for x in row) + "\n")
        back = np.array([[float(x) for x in line.split()[1:]] for line in open(path)], np.float64)
        assert np.array_equal(back.astype(np.float32), emb) and np.array_equal(back, emb.astype(np.float64))
        subprocess.run([sys.executable, os.path.join(RH.REFERENCE_ROOT, "comp_cos_sim_mat.py"), path], check=True, cwd=tmp)
        sim = np.load(os.path.join(tmp, "data", "visdial", "cos_sim_counter_fitting.npy"))
        with open(os.path.join(tmp, "data", "visdial", "cos_sim_idx2word.pickle"), "rb") as f:
            idx2word = pickle.load(f)
        with open(os.path.join(tmp, "data", "visdial", "cos_sim_word2idx.pickle"), "rb") as f:
            word2idx = pickle.load(f)
    assert sim.shape == (V, V) and sim.dtype == np.float32
    assert [idx2word[i] for i in range(V)] == words and all(word2idx[w] == i for i, w in enumerate(words))

    install_tokenizer_stub()
    from utils.text_attack import TextAttack
    attacker = object.__new__(TextAttack)
    sim_words, sim_values = attacker.pick_most_similar_words_batch(list(range(V)), sim, idx2word, ret_count=K, threshold=THRESHOLD)

    ehat = np.asarray(emb.astype(np.float64) / np.linalg.norm(emb.astype(np.float64), axis=1, keepdims=True), "float32")
    exact = ehat.astype(np.float64) @ ehat.astype(np.float64).T
    off = exact[~np.eye(V, dtype=bool)]
    assert np.abs(off - THRESHOLD).min() > CLEAR, "a cosine within %g of the cut: change SEED, not the bound" % CLEAR
    ref_idx = np.full((V, K), -1, np.int32)
    ref_val = np.zeros((V, K), np.float32)
    checked = np.ones((V, K), bool)
    count = np.zeros(V, np.int32)
    for r in range(V):
        n = len(sim_words[r])
        count[r] = n
        ref_idx[r, :n] = [word2idx[w] for w in sim_words[r]]
        ref_val[r, :n] = sim_values[r]
        row = np.sort(np.delete(exact[r], r))[::-1]
        for k in range(n):
            up = row[k - 1] - row[k] if k else np.inf
            down = row[k] - row[k + 1]
            checked[r, k] = up > GAP and down > GAP
    print("neighbours per row: mean %.2f, min %d, max %d; unchecked %.3f %%; |BLAS - fp64| max %.3e"
          % (count.mean(), count.min(), count.max(), 100.0 * (1.0 - checked.mean()),
             np.abs(sim.astype(np.float64) - exact).max()))
    files = write_npz(os.path.join(GOLDEN, "tiny_synonym.npz"), dict(
        emb=emb, words=np.array(words), K=np.asarray(K), threshold=np.asarray(THRESHOLD, np.float64),
        gap=np.asarray(GAP, np.float64), ref_idx=ref_idx, ref_val=ref_val, ref_count=count, checked=checked))
    assert len(files) == 1
    print("wrote", files[0], os.path.getsize(files[0]), "bytes")


if __name__ == "__main__":
    main()
