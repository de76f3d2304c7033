"""Rows of the discriminative (enc_only_a) model on the device, from token-id pools.

The reference builds them per dialog on the host: dataloader/dataloader_visdial_disc.py tokenises JSON text and assembles, with
Python lists, 10 x 100 eval rows (:299-401) or 10 x (1 + negatives) train rows (:125-288) of 256 int64 each -- 6 MB per dialog
that then travel to the device.  Everything those rows hold is the caption, ten questions, ten answers and 10 x 100 short options:
a few KB of ids.  Here the pools live on the device and `ops.disc_rows` (gstvd_disc_rows, one launch) writes exactly the rows that
are needed: a chunk of the eval rows, or the `batch_size` sampled train rows.

A pooled batch is a dict with
    cap [D, Lc], ques [D, R, U], ans [D, R, U], opts [D, R, O, U], gt_index [D, R]      int64 on the device, 0-padded, no [CLS] / [SEP]
    image_feat [D, regions, F], image_loc [D, regions, 5], image_mask [D, regions]        once per dialog
and, for training, image_target [D, regions, classes]; for `evaluate_disc`, round_id [D, 1] and gt_relevance [D, O] in the ORIGINAL
option order (`eval_targets` re-orders it).  `is_pooled` is the dispatch of evaluate_disc.score_batch / forward_disc: a batch with
`opts` and without `tokens`.  There is no CPU path.
"""
import torch

from . import ops
from ._lib import GstvdError

POOL_KEYS = ("cap", "ques", "ans", "opts", "gt_index")


def is_pooled(batch):
    return "opts" in batch and "tokens" not in batch


def _pools(batch, who):
    for k in POOL_KEYS:
        if k not in batch:
            raise GstvdError("%s: the pooled batch has no '%s'" % (who, k))
        if not batch[k].is_cuda:
            raise GstvdError("%s needs GPU tensors (%s is on %s); there is no CPU path" % (who, k, batch[k].device))
    return tuple(batch[k] for k in POOL_KEYS)


def _row_list(flat, rounds, slots):
    """Flat indices over [dialog, round, slot] -> the kernel's three int32 vectors (on the device `flat` lives on)."""
    return ((flat // (rounds * slots)).to(torch.int32), ((flat // slots) % rounds).to(torch.int32), (flat % slots).to(torch.int32))


def eval_option_order(gt_index, num_all, num_options):
    """The loader's option order of every round (:303-309): the ground truth first, then the first num_options - 1 of the other
    indices in increasing order.  gt_index [...] int64 -> [..., num_options] int64, on gt_index's device."""
    k = torch.arange(num_options, device=gt_index.device).expand(gt_index.shape + (num_options,))
    gt = gt_index.unsqueeze(-1)
    return torch.where(k == 0, gt.expand_as(k), torch.where(k - 1 < gt, k - 1, k))


def eval_targets(batch, params):
    """What the metrics of evaluate_disc need next to the scores of a pooled batch, on the host: gt_option_inds [D, R] (all zeros:
    the ground truth is slot 0) and gt_relevance [D, num_options] re-ordered by the slot rule (:316-319), or None without one."""
    gt = batch["gt_index"].cpu()
    rel = batch.get("gt_relevance")
    if rel is not None:
        order = eval_option_order(gt, batch["opts"].shape[2], int(params["num_options"]))
        d = torch.arange(gt.shape[0])
        rel = torch.gather(rel.cpu(), 1, order[d, batch["round_id"].cpu().view(-1) - 1])
    return torch.zeros_like(gt), rel


def eval_item(pools, start, end, params):
    """Rows [start, end) of the flattened [dialog, round, option] eval rows of a pooled batch as a `forward_disc` item: tokens,
    segments, mask [n, T], sep_indices [n, 25], hist_len [n], att fp32 [n, T] and the image tensors of each row's dialog, picked
    by index.  One launch; the row list is index arithmetic on the device.  params: max_seq_len, visdial_tot_rounds, num_options."""
    cap, ques, ans, opts, gt = _pools(pools, "eval_item")
    D, R = ques.shape[:2]
    slots = int(params["num_options"])
    if not 0 <= start <= end <= D * R * slots:
        raise GstvdError("eval_item: rows [%d, %d) are not among the %d x %d x %d rows of the batch" % (start, end, D, R, slots))
    rd, rj, rs = _row_list(torch.arange(start, end, device=ques.device), R, slots)
    o = ops.disc_rows(cap, ques, ans, opts, gt, rd, rj, rs, int(params["max_seq_len"]), int(params["visdial_tot_rounds"]), slots, False)
    d = rd.long()
    return dict(tokens=o["tokens"], segments=o["segments"], sep_indices=o["sep_indices"], mask=o["mask"], hist_len=o["hist_len"],
                att=o["att"], image_feat=pools["image_feat"][d], image_loc=pools["image_loc"][d], image_mask=pools["image_mask"][d])


def image_labels(feats, image_mask, u_img, forced_region, mask_prob):
    """utils/data_utils.py:89-111 on the device, per dialog: a real region has label 1 iff u < mask_prob, else -1, and its features
    zeroed iff additionally u / mask_prob < 0.9 (in float64, like selftrain.image_noise); padded regions get -1; then
    label[forced_region] = 1 -- forced_region in [1, regions - 1], padding or not -- and label[0] = 0.
    -> (features, image_label int64 [D, regions])."""
    real = image_mask != 0
    label = torch.full(image_mask.shape, -1, dtype=torch.int64, device=image_mask.device)
    if mask_prob > 0.0:
        u = u_img.to(torch.float64)
        hit = (u < mask_prob) & real
        label[hit] = 1
        feats = feats.masked_fill((hit & ((u / mask_prob) < 0.9)).unsqueeze(-1), 0)
    label.scatter_(1, forced_region.view(-1, 1), 1)
    label[:, 0] = 0
    return feats, label


def train_batch(pools, image, params, dense_scores=None, sample_indices=None, u_tok=None, u_neg=None, u_img=None, forced_region=None):
    """The sampled train rows of a pooled batch, with the keys `evaluate_disc.train_rows` returns.  The rows are
    randperm(D * R * (1 + num_negative_samples))[:batch_size] of the flattened [dialog, round, sample] order (train_disc.py:54-55),
    drawn on the host unless `sample_indices` gives them; only those rows are built (one `ops.disc_rows` launch in train mode).
    `image`: image_feat / image_loc / image_mask / image_target once per dialog; a row takes those of its dialog.
    dense_scores float64 [D, R, O]: the `-train_dense` soft labels of the negatives.
    Uniforms: u_tok fp32 [rows, T] ([MASK] noise by row position), u_neg fp32 [rows] (the negative of each row), u_img [D, regions]
    and forced_region int64 [D] (image noise, once per dialog as in the loader).  None: drawn from torch's generator on the device
    (mask_prob == 0 needs neither u_tok nor u_img); False: never drawn, and the call raises if the draw is needed.
    params: max_seq_len, visdial_tot_rounds, num_options, num_negative_samples, batch_size, mask_prob.
    token_rows / region_rows are taken from the device labels (one synchronisation each, as Engine.disc_step would)."""
    cap, ques, ans, opts, gt = _pools(pools, "train_batch")
    dev = ques.device
    D, R = ques.shape[:2]
    slots = 1 + int(params["num_negative_samples"])
    T, mask_prob = int(params["max_seq_len"]), float(params["mask_prob"])
    if mask_prob > 0.0 and (u_tok is False or u_img is False):
        raise GstvdError("train_batch: mask_prob = %g needs the uniforms u_tok [rows, %d] and u_img [D, regions]" % (mask_prob, T))
    if slots > 1 and u_neg is False:
        raise GstvdError("train_batch: %d negative samples per round need the uniforms u_neg [rows]" % (slots - 1))
    for k in ("image_feat", "image_loc", "image_mask", "image_target"):
        if not image[k].is_cuda:
            raise GstvdError("train_batch needs GPU tensors (%s is on %s); there is no CPU path" % (k, image[k].device))
    if sample_indices is None:
        sample_indices = torch.randperm(D * R * slots)[:params["batch_size"]]
    flat = sample_indices.to(dev)
    n = flat.numel()
    rd, rj, rs = _row_list(flat, R, slots)
    if u_tok is None or u_tok is False:
        u_tok = torch.rand(n, T, device=dev, dtype=torch.float32) if mask_prob > 0.0 else None
    if u_neg is None or u_neg is False:
        u_neg = torch.rand(n, device=dev, dtype=torch.float32)
    regions = image["image_mask"].shape[1]
    if u_img is None or u_img is False:
        u_img = torch.rand(D, regions, device=dev, dtype=torch.float64) if mask_prob > 0.0 else None
    if forced_region is None:
        forced_region = torch.randint(1, regions, (D,), device=dev)
    o = ops.disc_rows(cap, ques, ans, opts, gt, rd, rj, rs, T, int(params["visdial_tot_rounds"]), int(params["num_options"]), True,
                      mask_prob=mask_prob, u_tok=u_tok, u_neg=u_neg.to(dev), dense_scores=dense_scores)
    feats, label = image_labels(image["image_feat"], image["image_mask"], None if u_img is None else u_img.to(dev),
                                forced_region.to(dev), mask_prob)
    d = rd.long()
    out = dict(sample_indices=sample_indices, hist_len=o["hist_len"], tokens=o["tokens"], segments=o["segments"],
               sep_indices=o["sep_indices"], mask=o["mask"], next_sentence_labels=o["nsp_labels"], att=o["att"],
               neg_option=o["neg_option"], dialog_of_row=d, image_feat=feats[d], image_loc=image["image_loc"][d],
               image_mask=image["image_mask"][d], image_target=image["image_target"][d], image_label=label[d])
    out["token_rows"] = (out["mask"].reshape(-1) != -1).nonzero().view(-1)
    out["region_rows"] = (out["image_label"].reshape(-1) == 1).nonzero().view(-1)
    return out


_PINNED = ("dense_scores", "sample_indices", "u_tok", "u_neg", "u_img", "forced_region")


def train_batch_of(batch, params):
    """`train_batch` on a pooled batch that carries its own image tensors and, optionally, pinned draws under the keyword names."""
    return train_batch(batch, batch, params, **{k: batch[k] for k in _PINNED if k in batch})
