"""Listwise candidate training on the dense annotations: the host side of `EncoderDecoderModel.rank_loss`.

The reference ships the dense-annotation loader (dataloader_dense_annotations.py: `gt_relevance`, `round_id`) and the NDCG metric
but no trainer that uses them; this is the step such a trainer takes.  A batch in the eval loader's layout -- [B, rounds, options,
L] token tensors, one image per dialog -- is cut down to the annotated round of every dialog (`rank_targets`), and that round's
options are trained on against ONE encoder pass (`forward_rank`): the loss is the cross entropy between the softmax of the
options' sequence log-likelihoods and the normalised relevance."""
import torch

from ._lib import GstvdError


def rank_targets(batch, sparse=False):
    """Host side: the annotated round `round_id - 1` of every dialog of `batch` (eval loader layout).
    -> dict of the encoder-side tensors [B, ...] (the round's context, taken from option 0 after checking that the options share
    it, as evaluate.score_batch checks), dec_input_ids / dec_att_mask [B * options, U], relevance [B, options] and num_options.
    `sparse` (or a batch without `gt_relevance`): one-hot targets from `gt_option_inds` instead of the dense relevance."""
    ids = batch["enc_input_ids"]
    if ids.dim() != 4:
        raise GstvdError("rank_targets: enc_input_ids must be [B, rounds, options, T], got %r" % (tuple(ids.shape),))
    B, R_, O, T = ids.shape
    rid = batch["round_id"].reshape(B).long() - 1
    if int(rid.min()) < 0 or int(rid.max()) >= R_:
        raise GstvdError("rank_targets: round_id outside 1..%d" % R_)
    ar = torch.arange(B)
    pick = lambda k: batch[k][ar, rid]                                # noqa: E731  [B, options, L]
    e_ids, e_seg, e_att = pick("enc_input_ids"), pick("enc_segments"), pick("enc_att_mask")
    for name, t in (("enc_input_ids", e_ids), ("enc_segments", e_seg), ("enc_att_mask", e_att)):
        if not bool((t == t[:, :1]).all()):
            raise GstvdError("rank_targets: the options of a round do not share one context (%s differs between options); "
                             "the listwise step encodes a round once" % name)
    if sparse or "gt_relevance" not in batch:
        gt = batch["gt_option_inds"][ar, rid].long()
        rel = torch.zeros(B, O).scatter_(1, gt.view(B, 1), 1.0)
    else:
        rel = batch["gt_relevance"].reshape(B, O).float()
    U = batch["dec_input_ids"].shape[-1]
    return dict(enc_image_features=batch["enc_image_feat"], enc_image_spatials=batch["enc_image_loc"], enc_image_mask=batch["enc_image_mask"],
                enc_input_ids=e_ids[:, 0].contiguous(), enc_segments=e_seg[:, 0].contiguous(), enc_attention_mask=e_att[:, 0].contiguous(),
                dec_input_ids=pick("dec_input_ids").reshape(B * O, U).contiguous(),
                dec_attention_mask=pick("dec_att_mask").reshape(B * O, U).contiguous(), relevance=rel, num_options=O)


def forward_rank(model, batch, params):
    """-> (loss, scores [B, options]) of the listwise step on the annotated round of every dialog of `batch`.  params:
    `rank_sparse_targets` (one-hot gt_option_inds instead of gt_relevance), `rank_temperature` (default 1.0), `device`."""
    t = rank_targets(batch, sparse=bool(params.get("rank_sparse_targets", False)))
    device = params["device"]
    O = t.pop("num_options")
    kw = {k: v.to(device) for k, v in t.items()}
    return model.rank_loss(num_options=O, temperature=float(params.get("rank_temperature", 1.0)), **kw)
