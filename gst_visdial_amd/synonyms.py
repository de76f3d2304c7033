"""Synonym table and id-level substitution of the coreference text attack (utils/text_attack.py:58-116).

The reference answers "the nearest neighbour of this word" out of cos_sim_counter_fitting.npy, the full V x V cosine matrix that
comp_cos_sim_mat.py writes (V^2 x 4 bytes: 17 GB for the published 65 713 counter-fitted vectors), and substitutes by decode ->
str.replace -> tokenize on one row.  Here:
  * SynonymTable keeps the unit rows Ehat [V, D] and, per word, its K best neighbours with cosine >= threshold -- what
    pick_most_similar_words_batch reads out of the matrix -- computed by ops.cos_topk (gstvd_cos_topk: f32-input MFMA product
    fused with a per-row top-K), so the matrix never exists;
  * CorefSubstituter restates coreference_attack on token ids: `plan` turns a chunk's coreference dependencies into
    substitutions (utterance, wordpiece ids of the word, wordpiece ids of its synonym), `apply` runs them on the device
    (ops.subseq_replace: gstvd_subseq_replace).  The word -> wordpiece-ids map is data the caller has from its tokenizer; this
    package carries no tokenizer and no word vectors.
Departures from the reference are listed in INTEGRATION.md ("Coreference attack").
"""
import collections

import numpy as np
import torch

from . import ops

SKIP_REASONS = ("not_in_table", "no_neighbour", "no_word_ids")


def unit_rows(embeddings):
    """comp_cos_sim_mat.py:13-16: rows divided by their float64 norm, cast to fp32.  -> torch fp32 [V, D] on the host."""
    e = np.asarray(embeddings.detach().cpu().numpy() if isinstance(embeddings, torch.Tensor) else embeddings, dtype=np.float64)
    if e.ndim != 2:
        raise ValueError("SynonymTable: embeddings must be [V, D]")
    norm = np.linalg.norm(e, axis=1, keepdims=True)
    return torch.from_numpy(np.asarray(e / norm, "float32"))


def first_occurrence(words):
    """word -> row of its first occurrence (comp_cos_sim_mat.py:23-28 keeps the first occurrence of a repeated word)."""
    word2idx = {}
    for i, w in enumerate(words):
        if w not in word2idx:
            word2idx[w] = i
    return word2idx


class SynonymTable(object):
    """words [V], idx int32 [V, K] (-1: unused), val fp32 [V, K]: each word's neighbours, best first.  `ehat` fp32 [V, D] on
    `device` when the table can still look up (`neighbours`); a table loaded without a device answers `nearest` only."""

    def __init__(self, words, idx, val, K, threshold, ehat=None):
        self.words = [str(w) for w in words] if words is not None else None
        self.word2idx = first_occurrence(self.words) if self.words is not None else {}
        self.idx, self.val = idx, val                                   # on ehat's device (or the host)
        self.idx_host, self.val_host = idx.cpu(), val.cpu()
        self.K, self.threshold, self.ehat = int(K), threshold, ehat
        if self.words is not None and len(self.words) != idx.shape[0]:
            raise ValueError("SynonymTable: %d words for %d rows" % (len(self.words), idx.shape[0]))

    @classmethod
    def build(cls, embeddings, words=None, K=10, threshold=0.5, device="cuda:0", route=None):
        """embeddings [V, D] (numpy or torch, any float type), D a multiple of 4 (the counter-fitted vectors have 300)."""
        ehat = unit_rows(embeddings).to(device)
        idx, val = ops.cos_topk(ehat, None, K=K, threshold=threshold, route=route)
        return cls(words, idx, val, K, threshold, ehat=ehat)

    def neighbours(self, src):
        """(idx int32 [n, K], val fp32 [n, K]) of the rows `src` (ints, or an int tensor), looked up on the table's Ehat by the
        few-sources route: the same bits as the built table's rows."""
        if self.ehat is None:
            raise RuntimeError("SynonymTable.neighbours: this table was loaded without its unit rows")
        src = torch.as_tensor(src, dtype=torch.int32).reshape(-1).to(self.ehat.device)
        return ops.cos_topk(self.ehat, src.contiguous(), K=self.K, threshold=self.threshold, route="few")

    def nearest(self, word):
        """The rank-0 neighbour of `word`, or None (not in the table, or no neighbour passes the threshold)."""
        i = self.word2idx.get(word)
        if i is None:
            return None
        j = int(self.idx_host[i, 0])
        return self.words[j] if j >= 0 else None

    def save(self, path, with_ehat=True):
        arrays = dict(idx=self.idx_host.numpy(), val=self.val_host.numpy(), K=np.asarray(self.K),
                      threshold=np.asarray(float("-inf") if self.threshold is None else self.threshold, np.float64))
        if self.words is not None:
            arrays["words"] = np.array(self.words)
        if with_ehat and self.ehat is not None:
            arrays["ehat"] = self.ehat.cpu().numpy()
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path, device=None):
        with np.load(path) as z:
            words = z["words"].tolist() if "words" in z.files else None
            idx, val = torch.from_numpy(z["idx"]), torch.from_numpy(z["val"])
            thr = float(z["threshold"])
            ehat = torch.from_numpy(z["ehat"]) if ("ehat" in z.files and device is not None) else None
            K = int(z["K"])
        if device is not None:
            idx, val = idx.to(device), val.to(device)
            ehat = ehat.to(device) if ehat is not None else None
        return cls(words, idx, val, K, None if thr == float("-inf") else thr, ehat=ehat)


class CorefSubstituter(object):
    """coreference_attack (utils/text_attack.py:58-91) on token ids.  `word_ids`: word -> list of its wordpiece ids (1..16),
    from the caller's tokenizer; `continuation`: uint8 [vocab], 1 for a "##" piece (None: matches need no word boundary)."""

    def __init__(self, table, word_ids, continuation=None, device=None, cls_id=101, sep_id=102, pad_id=0, max_sep=25, refresh=False):
        self.table, self.word_ids = table, word_ids
        self.device = torch.device(device if device is not None else (table.ehat.device if table.ehat is not None else "cuda:0"))
        self.cont = None if continuation is None else torch.as_tensor(np.asarray(continuation), dtype=torch.uint8).contiguous()
        self._cont_dev = None
        self.cls_id, self.sep_id, self.pad_id, self.max_sep, self.refresh = cls_id, sep_id, pad_id, max_sep, refresh
        self.skipped = collections.Counter()
        self.planned = 0

    def plan(self, coref_dependency):
        """-> [(utterance, word's ids, synonym's ids), ...] in the order coreference_attack applies them: keys in order, int(key)
        the dialog round; round 0 is the caption (utterance 0), round k its question and answer (utterances 2k - 1 and 2k).  A word
        is skipped -- and counted in `skipped` by reason -- when the table does not have it, when no neighbour passes the
        threshold, or when `word_ids` lacks the word or its synonym."""
        plan = []
        for key, word in (coref_dependency or {}).items():
            rnd = int(key)
            if word not in self.table.word2idx:
                self.skipped["not_in_table"] += 1
                continue
            synonym = self.table.nearest(word)
            if synonym is None:
                self.skipped["no_neighbour"] += 1
                continue
            if word not in self.word_ids or synonym not in self.word_ids:
                self.skipped["no_word_ids"] += 1
                continue
            a, b = list(self.word_ids[word]), list(self.word_ids[synonym])
            for u in ((0,) if rnd == 0 else (2 * rnd - 1, 2 * rnd)):
                plan.append((u, a, b))
            self.planned += 1
        return plan

    def apply(self, ids, plans, refresh=False, segments=None):
        """ids int64 [n, T] (host or device; never written), plans: one plan per row.  -> ids on the device; refresh True:
        (ids, segments, sep_indices, att_mask) recomputed from them, each row's first segment taken from `segments[:, 0]`."""
        ids = ids.to(self.device)
        if self.cont is not None and self._cont_dev is None:
            self._cont_dev = self.cont.to(self.device)
        kw = {}
        if refresh:
            n, T = ids.shape
            kw = dict(segments=torch.empty(n, T, dtype=torch.int64, device=self.device),
                      sep_indices=torch.empty(n, self.max_sep, dtype=torch.int64, device=self.device),
                      att_mask=torch.empty(n, T, dtype=torch.float32, device=self.device))
            if segments is not None:
                kw["start_seg"] = segments.to(self.device)[:, 0].to(torch.int64).contiguous()
        out, _ = ops.subseq_replace(ids.contiguous(), plans, cls=self.cls_id, sep=self.sep_id, pad=self.pad_id, cont=self._cont_dev, **kw)
        if refresh:
            return out, kw["segments"], kw["sep_indices"], kw["att_mask"]
        return out

    def attack_row(self, ids, coref_dependency, refresh=False, segments=None):
        """Row 0 of the chunk's context ids [rows, T] with the dependencies' substitutions made: [1, T] on the device (with
        refresh, the four tensors of `apply` for that row).  Nothing to substitute: row 0 itself, unchanged."""
        return self.apply(ids[:1], [self.plan(coref_dependency)], refresh=refresh, segments=None if segments is None else segments[:1])
