"""Rows of the generative (enc_dec) model on the device, from token-id pools.

The reference builds them per dialog on the host: dataloader/dataloader_visdial_gen.py tokenises JSON text and assembles, with
Python lists, 10 x 100 context rows of 256 int64 three times over plus 10 x 100 decoder rows (eval :295-458), 100 + 100 rows of
one round (test :507-603) or 10 + 10 teacher rows (train :123-293).  Everything those rows hold is the caption, ten questions, ten
answers and 10 x 100 short options: a few KB of ids.  Here the pools live on the device and `ops.gen_rows` (gstvd_gen_rows, one
launch) writes exactly the rows a scoring call needs: one encoder row per round and its `num_options` decoder rows.

A pooled batch is a dict with
    cap [D, Lc], ques [D, R, U], ans [D, R, U], opts [D, R, O, U], gt_index [D, R]      int64 on the device, 0-padded, no [CLS] / [SEP]
    enc_image_feat [D, regions, F], enc_image_loc [D, regions, 5], enc_image_mask [D, regions]     once per dialog, on the device
and, for `evaluate.evaluate`, round_id [D, 1] and gt_relevance [D, O] in the ORIGINAL option order (`eval_targets` re-orders it).
A test-split batch has n_rounds int64 [D] (the rounds the dialog has; the last one is scored), opts [D, 1, O, U] or [D, R, O, U],
no gt_index, and image_id / round_id.  `is_pooled` is the dispatch of evaluate.score_batch: a batch with `opts` and without
`enc_input_ids`.  There is no CPU path.

Not covered (the loader stays in charge): `vd_gen_val`, whose context is the caption alone and which `generate_dialogs` already
starts from; the image side (encode_image_input and the feature reader); the tokenizer.
"""
import torch

from . import ops
from ._lib import GstvdError
from .disc_rows import eval_option_order

POOL_KEYS = ("cap", "ques", "ans", "opts", "gt_index")
IMAGE_KEYS = ("enc_image_feat", "enc_image_loc", "enc_image_mask")


def is_pooled(batch):
    return "opts" in batch and "enc_input_ids" not in batch


def _pools(batch, who, keys=POOL_KEYS):
    for k in keys:
        if k not in batch:
            raise GstvdError("%s: the pooled batch has no '%s'" % (who, k))
    for k in keys:
        if not batch[k].is_cuda:
            raise GstvdError("%s needs GPU tensors (%s is on %s); there is no CPU path" % (who, k, batch[k].device))
    return tuple(batch[k] for k in keys)


def _shape_params(params):
    params = params or {}
    return int(params.get("max_seq_len", 256)), int(params.get("max_utt_len", 25))


def noise_prob(params):
    """The [MASK] probability of the eval rows: mask_prob under attack == 'random_token', else 0 (:387)."""
    params = params or {}
    return float(params.get("mask_prob", 0.0)) if params.get("attack") == "random_token" else 0.0


def num_slots(pools, params):
    """Option rows per round of the eval order: params['num_options'], all O options without it."""
    return int((params or {}).get("num_options", pools["opts"].shape[2]))


def _item(o, dialog, group):
    return dict(enc_input_ids=o["tokens"], enc_segments=o["segments"], enc_att_mask=o["att"], enc_mlm_labels=o["mlm"],
                enc_sep_indices=o["sep_indices"], enc_hist_len=o["hist_len"], dec_input_ids=o["dec_ids"], dec_att_mask=o["dec_att"],
                dec_option=o["dec_option"], dialog=dialog, group=group)


def eval_rounds(pools, r0, r1, params, u_tok=None):
    """Rounds [r0, r1) of the flattened [dialog, round] order of a pooled batch, ready for `model.score_candidates(..., group)`:
    one encoder row per round and num_options decoder rows per round (group = num_options).  With the random-token noise
    (`noise_prob(params)` > 0) every option has its own copy of the context with its own draws -- u_tok fp32 [(r1 - r0) *
    num_options, T], drawn from torch's generator on the device when None -- and group = 1.  One launch; the row lists are index
    arithmetic on the device.  -> dict: enc_input_ids, enc_segments, enc_mlm_labels [n, T], enc_att_mask fp32 [n, T],
    enc_sep_indices, enc_hist_len, dec_input_ids [rounds * num_options, Ud], dec_att_mask, dec_option, dialog (int64, the dialog of
    every encoder row), group.  params: max_seq_len, max_utt_len, num_options, attack, mask_prob."""
    cap, ques, ans, opts, gt = _pools(pools, "eval_rounds")
    D, R = ques.shape[:2]
    T, Ud = _shape_params(params)
    slots = num_slots(pools, params)
    if not 0 <= r0 <= r1 <= D * R:
        raise GstvdError("eval_rounds: rounds [%d, %d) are not among the %d x %d rounds of the batch" % (r0, r1, D, R))
    dev = ques.device
    flat = torch.arange(r0 * slots, r1 * slots, device=dev)
    dd, dj, ds = (flat // (R * slots)).to(torch.int32), ((flat // slots) % R).to(torch.int32), (flat % slots).to(torch.int32)
    p = noise_prob(params)
    if p > 0.0:
        ed, ej, group = dd, dj, 1
        if u_tok is None:
            u_tok = torch.rand(flat.numel(), T, device=dev, dtype=torch.float32)
    else:
        rounds = torch.arange(r0, r1, device=dev)
        ed, ej, group, u_tok = (rounds // R).to(torch.int32), (rounds % R).to(torch.int32), slots, None
    o = ops.gen_rows(cap, ques, ans, opts, gt, "eval", T, Ud, (ed, ej), (dd, dj, ds), num_options=slots, mask_prob=p, u_tok=u_tok)
    return _item(o, ed.long(), group)


def test_rounds(pools, d0, d1, params):
    """Dialogs [d0, d1) of a pooled test-split batch: the one scored round of each, n_rounds[d] - 1 (computed on the device), its
    context and its O options in their original order.  -> the dict of `eval_rounds` with group = O."""
    cap, ques, ans, opts, n_rounds = _pools(pools, "test_rounds", ("cap", "ques", "ans", "opts", "n_rounds"))
    D = ques.shape[0]
    T, Ud = _shape_params(params)
    O = opts.shape[2]
    if not 0 <= d0 <= d1 <= D:
        raise GstvdError("test_rounds: dialogs [%d, %d) are not among the %d dialogs of the batch" % (d0, d1, D))
    dev = ques.device
    ed = torch.arange(d0, d1, device=dev)
    ej = (n_rounds.reshape(-1)[d0:d1] - 1).to(torch.int32)
    ed32 = ed.to(torch.int32)
    dec = (ed32.repeat_interleave(O), ej.repeat_interleave(O), torch.arange(O, device=dev, dtype=torch.int32).repeat(d1 - d0))
    o = ops.gen_rows(cap, ques, ans, opts, None, "test", T, Ud, (ed32, ej), dec, num_options=O)
    return _item(o, ed, O)


test_rounds.__test__ = False            # a public name that starts with "test": not a test


def eval_targets(batch, params, device=None):
    """What the metrics of `evaluate` need next to the scores of a pooled batch: gt_option_inds [D, R] (all zeros: the ground truth
    is slot 0) and gt_relevance [D, num_options] re-ordered by the slot rule (:337-341), or None without one.  `device` None: on the
    host; a device: there, from tensors that are there already without a host synchronisation."""
    gt = batch["gt_index"] if device is not None else batch["gt_index"].cpu()
    dev = gt.device
    rel = batch.get("gt_relevance")
    if rel is not None:
        order = eval_option_order(gt, batch["opts"].shape[2], num_slots(batch, params))
        d = torch.arange(gt.shape[0], device=dev)
        rel = torch.gather(rel.to(dev), 1, order[d, batch["round_id"].to(dev).view(-1) - 1])
    return torch.zeros_like(gt), rel


def train_batch(pools, image, params, model="enc_dec_a"):
    """The teacher rows of a pooled batch in the layout and with the keys of `selftrain.dialog_train_batch`, so that `step.forward`
    takes it unchanged: text tensors [D, R, 1, L], image tensors unexpanded.  model "enc_dec_a": context caption .. q_j, target
    a_j; "enc_dec_q": context caption .. a_(j-1), target q_j (:137-154).  The loader builds these rows without noise (mask_prob 0,
    :211, :286).  params: max_seq_len, max_utt_len."""
    if model not in ("enc_dec_a", "enc_dec_q"):
        raise GstvdError("train_batch: model must be 'enc_dec_a' or 'enc_dec_q' (got %r)" % (model,))
    cap, ques, ans = _pools(pools, "train_batch", ("cap", "ques", "ans"))
    for k in IMAGE_KEYS:
        if not image[k].is_cuda:
            raise GstvdError("train_batch needs GPU tensors (%s is on %s); there is no CPU path" % (k, image[k].device))
    D, R = ques.shape[:2]
    T, Ud = _shape_params(params)
    dev = ques.device
    rounds = torch.arange(D * R, device=dev)
    d, j = (rounds // R).to(torch.int32), (rounds % R).to(torch.int32)
    o = ops.gen_rows(cap, ques, ans, None, None, "train_a" if model == "enc_dec_a" else "train_q", T, Ud, (d, j), (d, j, torch.zeros_like(d)))
    names = (("enc_input_ids", "tokens"), ("enc_segments", "segments"), ("enc_sep_indices", "sep_indices"), ("enc_mlm_labels", "mlm"),
             ("enc_att_mask", "att"), ("dec_input_ids", "dec_ids"), ("dec_att_mask", "dec_att"), ("dec_labels", "dec_labels"))
    out = {k: o[src].view(D, R, 1, -1) for k, src in names}
    out["enc_hist_len"] = o["hist_len"].view(D, R, 1)
    out["enc_next_sentence_labels"] = torch.full((D, R, 1), -1, dtype=torch.long, device=dev)
    for k in IMAGE_KEYS:
        out[k] = image[k]
    return out
