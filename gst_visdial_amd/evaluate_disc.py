"""Discriminative evaluation and training step: the build's counterpart of evaluate_disc.evaluate (evaluate_disc.py:27-118) and
of train_disc.forward, both branches (train_disc.py:27-124), for a `VisualDialogEncoder` with model = 'enc_only_a'.

Same batch contract (per-dialog tensors [B, rounds, options, L] from the disc eval dataloader; image tensors once per dialog)
and the same metrics.  Two things differ, neither changes a result:
  * the image tensors are expanded to one row per option by INDEXING the per-dialog tensors chunk by chunk, not by the
    reference's 100x `.expand(...).contiguous()` copy of the whole batch (evaluate_disc.py:52-58);
  * the ranking probability softmax(nsp_scores, 1)[:, 0] comes out of the head kernel itself (Engine.nsp_scores).
A batch that carries token-id pools instead of the loader's text tensors (`opts` present, `tokens` absent: disc_rows.is_pooled) has
its rows built on the device, chunk by chunk (disc_rows.eval_item) or for the sampled train rows (disc_rows.train_batch); a batch
with `tokens` takes the path below unchanged.
Index work (sequence lengths, masks, chunk bounds, the row -> dialog map) is integer-exact torch code, restated bit for bit by
tests/test_disc_cpu.py."""
import torch

from . import disc_rows
from . import metrics as _metrics
from .metrics import SparseGTMetrics, NDCGBatchSum, scores_to_ranks


def sequence_lengths(sep_indices, hist_len):
    """train_disc.py:97-98: position of the [SEP] that closes the last utterance of the row, plus one."""
    return torch.gather(sep_indices, 1, hist_len.view(-1, 1)).squeeze(1) + 1


def sequence_mask(lengths, max_len):
    """utils/data_utils.py:7-18, on the device `lengths` lives on: mask[b, t] = t < lengths[b] (bool)."""
    return torch.arange(max_len, device=lengths.device).unsqueeze(0) < lengths.unsqueeze(1)


def option_rows_to_dialog(num_dialogs, num_rounds, num_options):
    """Row r of the flattened [dialog, round, option] batch belongs to dialog r // (rounds * options): the index that replaces
    the reference's expand + contiguous of the image tensors (evaluate_disc.py:52-58)."""
    return torch.arange(num_dialogs).repeat_interleave(num_rounds * num_options)


def chunk_bounds(num_rows, rows_per_call):
    """[(start, end)] of consecutive chunks of at most `rows_per_call` rows (the last one may be shorter; the reference asserts
    divisibility, evaluate_disc.py:65)."""
    if rows_per_call <= 0:
        raise ValueError("rows_per_call must be positive")
    return [(s, min(s + rows_per_call, num_rows)) for s in range(0, num_rows, rows_per_call)]


def _module(encoder):
    return getattr(encoder, "module", encoder)          # nn.DataParallel(encoder, [gpu]) of evaluate_disc.py:167


def _prepare(item, params):
    """The tensor work of train_disc.forward's eval branch (train_disc.py:32-67,87-99; sample_indices = arange): flatten,
    move to the device, build the attention mask there."""
    dev = params["device"]
    tokens = item["tokens"]
    tokens = tokens.view(-1, tokens.shape[-1]).to(dev)
    segments = item["segments"].view(-1, item["segments"].shape[-1]).to(dev)
    sep_indices = item["sep_indices"].view(-1, item["sep_indices"].shape[-1]).to(dev)
    mask = item["mask"].view(-1, item["mask"].shape[-1]).to(dev)
    hist_len = item["hist_len"].view(-1).to(dev)
    f, l, m = item["image_feat"], item["image_loc"], item["image_mask"]
    features = f.view(-1, f.shape[-2], f.shape[-1]).to(dev)
    spatials = l.view(-1, l.shape[-2], l.shape[-1]).to(dev)
    image_mask = m.view(-1, m.shape[-1]).to(dev)
    att = item["att"] if "att" in item else sequence_mask(sequence_lengths(sep_indices, hist_len), tokens.shape[1])
    return tokens, features, spatials, sep_indices, segments, mask, att, image_mask


def train_rows(batch, params):
    """The host index work of train_disc.forward's train branch (train_disc.py:43-85): `batch_size` rows drawn with
    torch.randperm from the flattened [dialog, round, sample] rows, the text / label tensors of those rows, and the image
    tensors of each row's dialog.  The image tensors (image_feat, image_loc, image_mask, image_target, image_label) may come
    in the layout the reference builds (expanded to one copy per row, train_disc.py:266-276) or once per dialog: then row r
    takes those of dialog r // (rounds * samples) by index -- image_target is [37, 1601] fp32 per dialog, and its copy x rounds
    x samples per step is the largest host-to-device transfer of the reference's loop.  Also returns the flat indices of the
    masked tokens (label != -1) and regions (label == 1), computed here on the host: the device step needs no sync for them."""
    flat = lambda k: batch[k].reshape(-1, batch[k].shape[-1])
    hist_len = batch["hist_len"].reshape(-1)
    n = hist_len.shape[0]
    sample_indices = torch.randperm(n)[:params["batch_size"]]
    out = dict(sample_indices=sample_indices, hist_len=hist_len[sample_indices])
    for k in ("tokens", "segments", "sep_indices", "mask", "next_sentence_labels"):
        out[k] = flat(k)[sample_indices, :]
    per_dialog = batch["image_feat"].dim() == 3
    if per_dialog:
        dialogs = batch["image_feat"].shape[0]
        if n % dialogs:
            raise ValueError("%d rows do not divide into %d dialogs" % (n, dialogs))
        pick = sample_indices // (n // dialogs)
    out["dialog_of_row"] = pick if per_dialog else None
    for k, tail in (("image_feat", 2), ("image_loc", 2), ("image_mask", 1), ("image_target", 2), ("image_label", 1)):
        x = batch[k]
        out[k] = x[pick] if per_dialog else x.reshape(-1, *x.shape[-tail:])[sample_indices]
    out["token_rows"] = (out["mask"].reshape(-1) != -1).nonzero().view(-1)
    out["region_rows"] = (out["image_label"].reshape(-1) == 1).nonzero().view(-1)
    return out


def _forward_train(encoder, batch, params):
    """Train branch of train_disc.forward: sampled rows -> the encoder's three losses -> means, coefficients, their sum."""
    dev = params["device"]
    rows = disc_rows.train_batch_of(batch, params) if disc_rows.is_pooled(batch) else train_rows(batch, params)
    r = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in rows.items()}
    att = r["att"] if "att" in r else sequence_mask(sequence_lengths(r["sep_indices"], r["hist_len"]), r["tokens"].shape[1])
    lm_loss, img_loss, nsp_loss, nsp_scores, lm_scores, _, _ = encoder(
        r["tokens"], r["image_feat"], r["image_loc"], sep_indices=r["sep_indices"], token_type_ids=r["segments"],
        masked_lm_labels=r["mask"], attention_mask=att, next_sentence_label=r["next_sentence_labels"],
        image_attention_mask=r["image_mask"], image_label=r["image_label"], image_target=r["image_target"],
        token_rows=r["token_rows"], region_rows=r["region_rows"])
    lm_loss = params["lm_loss_coeff"] * lm_loss.mean()
    nsp_loss = params["nsp_loss_coeff"] * nsp_loss.mean()
    img_loss = params["img_loss_coeff"] * img_loss.mean()
    return lm_loss + nsp_loss + img_loss, lm_loss, nsp_loss, img_loss, nsp_scores, lm_scores


def forward_disc(encoder, item, params):
    """train_disc.forward -> its 6-tuple (loss, lm_loss, nsp_loss, img_loss, nsp_scores, lm_scores).  Eval modes: the losses are
    None as there.  Train modes: the weighted losses and their sum, differentiable.  lm_scores is None in both (the MLM logits
    over all tokens are not materialised; modules.VisualDialogEncoder)."""
    if "train" in params["mode"]:
        return _forward_train(encoder, item, params)
    if disc_rows.is_pooled(item):                           # every [dialog, round, option] row of the pools, built on the device
        D, R = item["ques"].shape[:2]
        item = disc_rows.eval_item(item, 0, D * R * int(params["num_options"]), params)
    tokens, features, spatials, sep_indices, segments, mask, att, image_mask = _prepare(item, params)
    _, _, _, nsp_scores, lm_scores, _, _ = encoder(tokens, features, spatials, sep_indices=sep_indices, token_type_ids=segments,
                                                   masked_lm_labels=mask, attention_mask=att, image_attention_mask=image_mask)
    return None, None, None, None, nsp_scores, lm_scores


def chunk_item(batch, dialog_of_row, start, end):
    """Rows [start, end) of a batch's flattened [dialog, round, option] rows as a train_disc.forward item; the image tensors of
    a row are those of its dialog, picked by index."""
    flat = lambda k: batch[k].reshape(-1, batch[k].shape[-1])
    d = dialog_of_row[start:end]
    return dict(tokens=flat("tokens")[start:end], segments=flat("segments")[start:end],
                sep_indices=flat("sep_indices")[start:end], mask=flat("mask")[start:end],
                hist_len=batch["hist_len"].reshape(-1)[start:end],
                image_feat=batch["image_feat"][d], image_loc=batch["image_loc"][d], image_mask=batch["image_mask"][d])


@torch.no_grad()
def score_batch(encoder, batch, params, rows_per_call=200):
    """-> softmax(nsp_scores, 1)[:, 0] of every answer option, [dialogs, rounds, options] fp32 on the device."""
    pooled = disc_rows.is_pooled(batch)
    if pooled:
        (B, rounds), options = batch["ques"].shape[:2], int(params["num_options"])
    else:
        B, rounds, options = batch["tokens"].shape[:3]
        dialog_of_row = option_rows_to_dialog(B, rounds, options)
    mod = _module(encoder)
    out = []
    for s, e in chunk_bounds(B * rounds * options, rows_per_call):
        item = disc_rows.eval_item(batch, s, e, params) if pooled else chunk_item(batch, dialog_of_row, s, e)
        tokens, features, spatials, _, segments, _, att, image_mask = _prepare(item, params)
        out.append(mod.nsp_scores(tokens, features, spatials, segments, att, image_mask)[1])
    return torch.cat(out, 0).view(B, rounds, options)


@torch.no_grad()
def evaluate_disc(encoder, dataloader, params, eval_batch_size=None, rows_per_call=200, metrics="host"):
    """evaluate_disc.py:27-118.  mode 'vd_eval_val': the metrics dict (r@1/5/10, mean, mrr, ndcg); any other eval mode
    ('vd_eval_test'): the ranks_json list.  `eval_batch_size` is kept for the reference's signature: dialogs per batch are read
    off each batch (the reference's expand needs every batch full).
    `metrics`: "host" -- the scores move to the host and the classes of metrics.py run there, as in the reference; "device" -- the
    scores stay on the device, the targets are uploaded once per batch, one metrics.DeviceRankMetrics.observe per batch, and the
    loop synchronises only in its retrieve (tied options are then ranked by the stable rule)."""
    mode = params["mode"]
    if metrics == "device":
        return _evaluate_disc_device(encoder, dataloader, params, rows_per_call)
    if metrics != "host":
        raise ValueError("evaluate_disc: metrics must be 'host' or 'device' (got %r)" % (metrics,))
    sparse, ndcg, ranks_json = SparseGTMetrics(), NDCGBatchSum(), []
    _module(encoder).eval()
    for batch in dataloader:
        output = score_batch(encoder, batch, params, rows_per_call).cpu()
        if mode == "vd_eval_val":
            if disc_rows.is_pooled(batch):
                gt_option_inds, gt_relevance = disc_rows.eval_targets(batch, params)
            else:
                gt_option_inds, gt_relevance = batch["gt_option_inds"], batch["gt_relevance"]
            sparse.observe(output, gt_option_inds)
            rid = batch["round_id"].cpu().squeeze(1)
            ndcg.observe(output[torch.arange(output.size(0)), rid - 1, :], gt_relevance)
        else:
            ranks = scores_to_ranks(output).squeeze(1)
            for i in range(output.shape[0]):
                ranks_json.append({"image_id": batch["image_id"][i].item(), "round_id": int(batch["round_id"][i].item()),
                                   "ranks": [r.item() for r in ranks[i][:]]})
    if mode == "vd_eval_val":
        metrics = {}
        metrics.update(sparse.retrieve(reset=True))
        metrics.update(ndcg.retrieve(reset=True))
        return metrics
    return ranks_json


def _evaluate_disc_device(encoder, dataloader, params, rows_per_call):
    """evaluate_disc(..., metrics="device"): the same loop with the metric state on the device."""
    from .evaluate import ranks_json_of
    mode = params["mode"]
    dev = _metrics.DeviceRankMetrics(params["device"])
    kept = ([], [], [])
    _module(encoder).eval()
    for batch in dataloader:
        output = score_batch(encoder, batch, params, rows_per_call)
        if mode == "vd_eval_val":
            if disc_rows.is_pooled(batch):
                gt_option_inds, gt_relevance = disc_rows.eval_targets(batch, params)
            else:
                gt_option_inds, gt_relevance = batch["gt_option_inds"], batch["gt_relevance"]
            dev.observe(output, gt_option_inds, gt_relevance, batch["round_id"])
        else:
            for keep, t in zip(kept, (_metrics.scores_to_ranks_device(output), batch["image_id"], batch["round_id"])):
                keep.append(t)
    if mode == "vd_eval_val":
        return dev.retrieve(reset=True)
    return ranks_json_of(*kept)
