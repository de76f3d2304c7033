"""FGSM attack evaluation: the build's counterpart of evaluate_gen_attack.py with `-attack fgsm`.

The attack (evaluate_gen_attack.py:92-165) perturbs the image features of ONE dialog round per dialog -- the round whose 100
answer options carry human relevance scores -- by epsilon * sign(d loss / d features), where the loss is the relevance-weighted
sum over the options of each option's mean per-token loss, and then scores the options on the perturbed features.

What differs from the script, none of it in the numbers it defines:
  * an option with relevance 0 contributes 0 * loss: its gradient is exactly zero and its features come back unchanged.  The
    gradient pass therefore runs on the options with a non-zero relevance only (typically a third of the 100), found on the host
    before anything is copied to the device;
  * that pass replays the backward for the image-feature gradient alone (Engine.inputs_only): the attack discards every
    parameter gradient, so none is computed;
  * the rounds that are not attacked are scored with one encoder pass per round (EncoderDecoderModel.score_candidates), as
    evaluate.py does; the attacked round cannot be -- its 100 contexts differ after the perturbation.

`random_token` (evaluate_gen_attack.py:209-226) fills the [MASK] tokens of a chunk's context with the arg-max token of a masked
LM and scores the options on the filled-in context.  The masked LM is not part of this package's weights: the caller builds a
`mlm.MaskedLMFiller` from a BertForMaskedLM state dict and passes it as `textattack=` (or params["textattack"]).  The filled
chunk is row 0 repeated, so when its segments and attention masks are also one row repeated it is scored with ONE encoder pass
(score_candidates), where the reference runs 100.  Without a filler `random_token` raises.

`coreference` (evaluate_gen_attack.py:167-206, utils/text_attack.py:58-100) replaces, in the round that carries the relevance
scores, the words of the chunk's coreference dependencies by their nearest counter-fitted neighbour inside the utterances of
their dialog round, on row 0, and repeats that row over the chunk.  Neither the word vectors nor a tokenizer are part of this
package: the caller builds a `synonyms.CorefSubstituter` (a `SynonymTable` of the vectors -- nearest neighbours by a fused
product + top-K kernel, never the V x V matrix -- and its tokenizer's word -> wordpiece-ids map) and passes it as `coref=` (or
params["coref"]); the substitution runs on token ids on the device.  By default only the ids change, as in the reference
(segments, separator positions and mask stay as loaded); a substituter built with refresh=True recomputes them from the new ids.
Without a substituter `coreference` raises; a masked-LM filler is not one.  INTEGRATION.md lists the departures from the
reference's string-level substitution.
"""
import contextlib

import torch

from . import ops
from . import metrics as _metrics
from .metrics import SparseGTMetrics, NDCG, scores_to_ranks

ROWS_PER_CALL = 100         # evaluate_gen_attack.py:241

_MODEL_KEYS = ("enc_image_features", "enc_image_spatials", "enc_image_mask", "enc_image_target", "enc_image_label",
               "enc_next_sentence_labels", "enc_input_ids", "enc_segments", "enc_sep_indices", "enc_mlm_labels",
               "enc_attention_mask", "dec_input_ids", "dec_attention_mask", "dec_labels")


def _core(model):
    return getattr(model, "module", model)          # nn.DataParallel(model, [gpu]) as the reference's scripts wrap it


def relevant_rows(gt_relevance):
    """Host indices (ascending, int64) of the options whose relevance is not zero -- the only rows whose loss reaches the
    attack's gradient."""
    rel = gt_relevance.detach().reshape(-1).cpu()
    return (rel != 0).nonzero().view(-1)


def _feature_grad(model, kw, weights, inputs_only):
    """evaluate_gen_attack.py:101-130 on the rows of `kw`: -> (x, d loss / d x), loss = sum_b weights[b] * mean_u lm_loss[b, u]."""
    x = kw["enc_image_features"].detach().clone().requires_grad_(True)
    core = _core(model)
    mode = core.inputs_only() if inputs_only else contextlib.nullcontext()
    with torch.enable_grad(), mode:
        lm_loss, _ = model(**dict(kw, enc_image_features=x), loss_reduction=False)
        n, U = kw["dec_input_ids"].shape
        lm_loss = lm_loss.view(n, U).mean(dim=1)
        lm_loss = torch.sum(lm_loss * weights)
        lm_loss.backward()
    return x.detach(), x.grad


def fgsm_features(model, kw, gt_relevance, epsilon, inputs_only=True, grad_fn=None):
    """evaluate_gen_attack.py:101-131 -> adv_feats = features + epsilon * sign(d loss / d features), fp32, same shape.

    `kw`: the 14 keyword tensors of EncoderDecoderModel.forward on the device, dec_labels None; `gt_relevance` [B] (host or
    device; on the host nothing waits for the device).  Rows with relevance 0 are returned bit for bit and take no part in the
    gradient pass.  As in the reference, whose first forward replaces [SEP] by [PAD] in the caller's `dec_input_ids` in place
    (visual_dialog_decoder.py:57), kw["dec_input_ids"] leaves this function with that replacement made on EVERY row, so the
    forward that follows sees what the reference's second forward sees.  `inputs_only` False: the full backward, parameter
    gradients included, as the reference runs it.  `grad_fn(model, sub_kw, weights, inputs_only) -> (x, grad)` replaces the
    gradient pass (host-logic tests)."""
    if kw.get("dec_labels") is not None:
        raise ValueError("fgsm_features: dec_labels must be None (the attack's labels are the shifted dec_input_ids)")
    feats, dec_ids = kw["enc_image_features"], kw["dec_input_ids"]
    B = feats.shape[0]
    rel = gt_relevance.detach().reshape(-1)
    if rel.numel() != B:
        raise ValueError("fgsm_features: %d relevance scores for %d rows" % (rel.numel(), B))
    rows = relevant_rows(rel)
    adv = feats.detach().to(torch.float32, copy=True)
    if rows.numel():
        dev_rows = rows.to(feats.device)
        full = rows.numel() == B
        sub = {k: (v if (full or v is None) else v.index_select(0, dev_rows)) for k, v in kw.items()}
        if full:
            sub["dec_input_ids"] = dec_ids.clone()          # (the replacement below is made once, on the caller's tensor)
        weights = rel.to(feats.device, torch.float32)
        x, g = (grad_fn or _feature_grad)(model, sub, weights if full else weights.index_select(0, dev_rows), inputs_only)
        x, g = x.to(torch.float32).contiguous(), g.to(torch.float32).contiguous()
        if x.is_cuda:
            stepped = ops.fgsm_step(x, g, epsilon, out=x)
        else:                                                # host-logic tests only: the product path is on the device
            stepped = x + epsilon * torch.sign(g)
        if full:
            adv = stepped.view_as(adv)
        else:
            adv.index_copy_(0, dev_rows, stepped.view(rows.numel(), *adv.shape[1:]))
    dc = _core(model).decoder.config
    dec_ids.masked_fill_(dec_ids == dc.eos_token_id, dc.pad_token_id)
    return adv


def _flat(t, last):
    return t.reshape((-1,) + tuple(t.shape[-last:]))


def attacked_round(batch):
    """evaluate_gen_attack.py:94-100: the dialog round of the chunk (half the number of non-zero separator positions of its
    first row) is the one that carries the relevance scores."""
    sep = _flat(batch["enc_sep_indices"], 1)
    return int(int((sep[0] != 0).sum()) / 2) == int(batch["round_id"].reshape(-1)[0])


def _filler(params, textattack):
    return textattack if textattack is not None else params.get("textattack")


def _filled_ids(filler, batch):
    """random_token: the chunk's context ids after the fill-in, [rows, T] on the filler's device.  The [MASK] positions of row 0
    are found on the host tensor (no device round trip); the loader's tensor is left as it is."""
    ids = _flat(batch["enc_input_ids"], 1)
    return filler.fill(ids, _flat(batch["enc_segments"], 1), _flat(batch["enc_att_mask"], 1), rows=filler.host_rows(ids[:1]))


def _substituter(params, coref):
    return coref if coref is not None else params.get("coref")


def _coref_context(sub, batch):
    """coreference: what the attacked round's chunk feeds the encoder instead of the loader's tensors -- {model keyword: [1, .]
    device tensor}, row 0 with the substitutions made (text_attack.py:63, 90: the caller repeats it over the chunk).  No
    dependencies: nothing changes (text_attack.py:66), {} is returned.  The loader's tensors are not written."""
    dep = batch.get("coref_dependency")
    if not dep:
        return {}
    ids = _flat(batch["enc_input_ids"], 1)
    if getattr(sub, "refresh", False):
        out = sub.attack_row(ids, dep, refresh=True, segments=_flat(batch["enc_segments"], 1))
        return dict(zip(("enc_input_ids", "enc_segments", "enc_sep_indices", "enc_attention_mask"), out))
    return {"enc_input_ids": sub.attack_row(ids, dep)}


def forward_attack(model, batch, params, epsilon=1.0, inputs_only=True, textattack=None, coref=None):
    """The branches of evaluate_gen_attack.forward (evaluate_gen_attack.py:28-226) -> lm_scores [rows, U, vocab].  `batch`: one
    chunk of the eval loader's rows (host tensors) with its dialog's `round_id` and `gt_relevance` and, for `coreference`, the
    chunk's `coref_dependency` ({round: word}).  `textattack`: the masked-LM filler of `random_token` (mlm.MaskedLMFiller, or
    anything with its `fill` and `host_rows`); also read from params["textattack"].  `coref`: the substituter of `coreference`
    (synonyms.CorefSubstituter, or anything with its `attack_row`); also read from params["coref"]."""
    attack = params.get("attack")
    filler = _filler(params, textattack)
    sub = _substituter(params, coref)
    if (attack == "coreference" and sub is None) or (attack == "random_token" and filler is None):
        raise NotImplementedError(
            "attack=%r is a text attack (utils/text_attack.py): it needs a pretrained BertForMaskedLM, the counter-fitted word "
            "vectors (cos_sim_counter_fitting, cos_sim_idx2word, cos_sim_word2idx)%s, none of which this package carries.  "
            "Only attack='fgsm' is implemented without further inputs; attack='random_token' runs once a masked-LM filler is "
            "supplied as textattack= (gst_visdial_amd.mlm.MaskedLMFiller, loaded from a BertForMaskedLM state dict).  "
            "attack='coreference' runs once a substituter is supplied as coref= (gst_visdial_amd.synonyms.CorefSubstituter: a "
            "SynonymTable built from the word vectors and the tokenizer's word -> wordpiece-ids map)"
            % (attack, " and the coreference dependencies" if attack == "coreference" else ""))
    if attack not in ("fgsm", "random_token", "coreference"):
        raise NotImplementedError("attack=%r: no such attack (the reference has 'fgsm', 'coreference', 'random_token'; 'fgsm' "
                                  "is implemented as it stands, 'random_token' with a filler, 'coreference' with a substituter)" % (attack,))
    dev = params["device"]
    text = attack == "random_token"
    this_round = (not text) and attacked_round(batch)            # on the host tensors: no device round trip
    hit = attack == "fgsm" and this_round
    kw = dict.fromkeys(_MODEL_KEYS)
    kw.update(enc_input_ids=_filled_ids(filler, batch).to(dev) if text else _flat(batch["enc_input_ids"], 1).to(dev), enc_segments=_flat(batch["enc_segments"], 1).to(dev),
              enc_sep_indices=_flat(batch["enc_sep_indices"], 1).to(dev), enc_mlm_labels=_flat(batch["enc_mlm_labels"], 1).to(dev),
              enc_attention_mask=_flat(batch["enc_att_mask"], 1).to(dev),
              dec_input_ids=_flat(batch["dec_input_ids"], 1).to(dev, copy=True),     # (mutated below: never the loader's tensor)
              dec_attention_mask=_flat(batch["dec_att_mask"], 1).to(dev),
              enc_image_features=_flat(batch["enc_image_feat"], 2).to(dev), enc_image_spatials=_flat(batch["enc_image_loc"], 2).to(dev),
              enc_image_mask=_flat(batch["enc_image_mask"], 1).to(dev))
    if hit:
        kw["enc_image_features"] = fgsm_features(model, kw, batch["gt_relevance"], epsilon, inputs_only=inputs_only)
    if attack == "coreference" and this_round:                   # only the round that carries the relevance scores is attacked
        rows = kw["enc_input_ids"].shape[0]
        for k, v in _coref_context(sub, batch).items():
            kw[k] = v.to(dev).repeat(rows, 1)
    _, lm_scores = model(**kw)
    return lm_scores


def _same_context(batch, keys=("enc_input_ids", "enc_segments", "enc_att_mask")):
    return all(bool((batch[k] == batch[k][:1]).all()) for k in keys)


def score_chunk(model, item, params, epsilon, textattack=None, coref=None):
    """Scores [rows] of one chunk: the script's lines 321-333 for the round FGSM attacks, one encoder pass for any other.
    random_token: every chunk is filled in; the filled context is row 0 repeated, so it takes the one-pass route whenever the
    chunk's segments and attention masks are one row repeated too (they are in the eval loader's chunks).  coreference: the
    attacked round's context is row 0 repeated as well and takes the same route under the same condition."""
    dev = params["device"]
    core = _core(model)
    ids = item["dec_input_ids"]
    if params.get("attack") == "random_token":
        filler = _filler(params, textattack)
        if filler is None or not _same_context(item, ("enc_segments", "enc_att_mask")):
            many = True                                       # (no filler: forward_attack raises, naming what is missing)
        else:
            many = False
            item = dict(item, enc_input_ids=_filled_ids(filler, item)[:1])
    elif params.get("attack") == "coreference":
        sub = _substituter(params, coref)
        if sub is None:
            many = True                                       # (forward_attack raises, naming what is missing)
        elif not (attacked_round(item) and item.get("coref_dependency")):
            many = not _same_context(item)                    # not attacked: scored as evaluate.py scores it
        elif not _same_context(item, ("enc_segments", "enc_att_mask")):
            many = True
        else:
            many = False
            new = _coref_context(sub, item)
            item = dict(item, enc_input_ids=new["enc_input_ids"])
            if "enc_segments" in new:
                item.update(enc_segments=new["enc_segments"], enc_att_mask=new["enc_attention_mask"])
    else:
        many = attacked_round(item) or not _same_context(item)
    if many:
        forward_attack(model, item, params, epsilon, textattack=textattack, coref=coref)
        last = core.engine.last          # the second forward's logits and their log-sum-exp, still in the arena
        scores = torch.empty(ids.shape[0], dtype=torch.float32, device=dev)
        ops.answer_scores(last["logits"].t, last["lse"], ids.to(dev).contiguous(), ids.shape[0], ids.shape[1], scores)
        return scores
    return core.score_candidates(item["enc_image_feat"][:1].to(dev), item["enc_image_loc"][:1].to(dev),
                                 item["enc_image_mask"][:1].to(dev), item["enc_input_ids"][:1].to(dev),
                                 item["enc_segments"][:1].to(dev), item["enc_att_mask"][:1].to(dev), ids.to(dev),
                                 item["dec_att_mask"].to(dev), ids.shape[0])


@torch.no_grad()
def evaluate_attack(model, dataloader, params, epsilon=1.0, mode="vd_eval_val", textattack=None, coref=None, coref_dependency=None,
                    metrics="host"):
    """The loop of evaluate_gen_attack.evaluate (evaluate_gen_attack.py:233-369) for attack='fgsm', with a masked-LM filler
    (`textattack=` or params["textattack"]) attack='random_token', and with a substituter (`coref=` or params["coref"])
    attack='coreference': chunks of 100 option rows, the metrics of metrics.py; -> (ranks_json, metrics) as evaluate.evaluate
    returns them.  `coref_dependency`: the reference's dependency file, indexed [dialog]['coreference'][chunk] with the dialogs
    numbered in the loader's order (evaluate_gen_attack.py:318-319); a chunk's entry is a {round: word} dict, possibly empty.
    `metrics`: "host" -- the classes of metrics.py on the host; "device" -- one metrics.DeviceRankMetrics.observe per batch on the
    scores where they are, the loop's metric work synchronises only in retrieve (tied options ranked by the stable rule)."""
    if metrics not in ("host", "device"):
        raise ValueError("evaluate_attack: metrics must be 'host' or 'device' (got %r)" % (metrics,))
    on_device = metrics == "device"
    attack = params.get("attack")
    ready = attack == "fgsm" or (attack == "random_token" and _filler(params, textattack) is not None) \
        or (attack == "coreference" and _substituter(params, coref) is not None)
    if not ready:
        forward_attack(model, {}, params)           # raises, naming what is missing
    if attack == "coreference" and coref_dependency is None:
        raise ValueError("evaluate_attack: attack='coreference' needs coref_dependency= (per dialog, per chunk, a {round: word} dict)")
    if on_device:
        dev_metrics, kept, ranks_json = _metrics.DeviceRankMetrics(params["device"]), ([], [], []), []
    else:
        sparse, ndcg, ranks_json = SparseGTMetrics(), NDCG(), []
    model.eval()
    dialog_no = 0
    for batch in dataloader:
        ids = batch["enc_input_ids"]
        Bd, rounds, options = ids.shape[0], ids.shape[1], ids.shape[2]
        per_dialog = rounds * options
        if per_dialog % ROWS_PER_CALL:
            raise ValueError("evaluate_attack: %d rows per dialog are not a multiple of %d" % (per_dialog, ROWS_PER_CALL))
        text = {k: _flat(batch[k], 1) for k in ("enc_input_ids", "enc_segments", "enc_sep_indices", "enc_mlm_labels", "enc_att_mask",
                                                "dec_input_ids", "dec_att_mask")}
        out = []
        for d in range(Bd):
            for j in range(per_dialog // ROWS_PER_CALL):
                rows = slice(d * per_dialog + j * ROWS_PER_CALL, d * per_dialog + (j + 1) * ROWS_PER_CALL)
                item = {k: v[rows] for k, v in text.items()}
                # the loader holds the image tensors once per dialog; the chunk's rows all belong to dialog d
                item["enc_image_feat"] = batch["enc_image_feat"][d:d + 1].expand(ROWS_PER_CALL, -1, -1)
                item["enc_image_loc"] = batch["enc_image_loc"][d:d + 1].expand(ROWS_PER_CALL, -1, -1)
                item["enc_image_mask"] = batch["enc_image_mask"][d:d + 1].expand(ROWS_PER_CALL, -1)
                item["round_id"] = batch["round_id"][d:d + 1]
                item["gt_relevance"] = batch["gt_relevance"][d]
                if attack == "coreference":
                    item["coref_dependency"] = coref_dependency[dialog_no + d]["coreference"][j]
                out.append(score_chunk(model, item, params, epsilon, textattack=textattack, coref=coref))
        dialog_no += Bd
        scores = torch.cat(out, 0).view(Bd, rounds, options)
        if on_device:
            if mode == "vd_eval_val":
                with_rel = params.get("vd_version", "1.0") == "1.0"
                dev_metrics.observe(scores, batch["gt_option_inds"], batch["gt_relevance"] if with_rel else None,
                                    batch["round_id"] if with_rel else None)
            else:
                for keep, t in zip(kept, (_metrics.scores_to_ranks_device(scores), batch["image_id"], batch["round_id"])):
                    keep.append(t)
        elif mode == "vd_eval_val":
            sparse.observe(scores, batch["gt_option_inds"])
            if params.get("vd_version", "1.0") == "1.0":
                rid = batch["round_id"].reshape(Bd)
                ndcg.observe(scores[torch.arange(Bd), rid - 1, :], batch["gt_relevance"])
        else:
            ranks = scores_to_ranks(scores).squeeze(1)
            for i in range(Bd):
                ranks_json.append({"image_id": batch["image_id"][i].item(), "round_id": int(batch["round_id"][i].item()),
                                   "ranks": [r.item() for r in ranks[i][:]]})
    if on_device:
        from .evaluate import ranks_json_of
        return ranks_json_of(*kept), (dev_metrics.retrieve(reset=True) if mode == "vd_eval_val" else {})
    metrics = {}
    if mode == "vd_eval_val":
        metrics.update(sparse.retrieve(reset=True))
        if params.get("vd_version", "1.0") == "1.0":
            metrics.update(ndcg.retrieve(reset=True))
    return ranks_json, metrics
