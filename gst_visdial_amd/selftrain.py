"""Self-training on the device: whole-dialog generation and the student's train rows of the generated dialogs.

The reference closes its self-training loop through files: generate.py writes the dialogs as JSON text and the loader of
dataloader/dataloader_cc12m_gen.py:104-266 re-tokenises them (utils/data_utils.encode_input).  Neither the tokenizer nor the
loaders are part of this package, and neither is needed: everything between the sampled ids and the student's batch is integer
work on token ids.

  * `generate_dialogs`   -- `generate.dialog_round`'s sequence for `num_rounds` rounds, the two context updates per round done by
    `ops.context_append` (one launch each, attention mask included), so nothing inside the loop waits for the device; the
    "context already full" condition, which the reference raises per row, is recorded by the kernel and raised once, after the
    last round;
  * `dialog_train_batch` -- the loader's rows (context of every round under encode_input with the 15 % [MASK] noise, target with
    shifted labels, `-select_data` zeroing by perplexity) from the generation call's own tensors in one `ops.dialog_rows` launch,
    plus the image-feature noise of utils/data_utils.py:89-101, as a device batch in the layout of SURVEY appendix B;
  * that batch goes to the student through the existing driver: `step.forward(student, batch, params)`.
"""
import torch

from . import ops
from ._lib import GstvdError
from .generate import answer_perplexity

MAX_CAPTION_LEN = 38           # dataloader_cc12m_gen.py:75-79 / 110-115
_IMAGE_KEYS = (("enc_image_feat", "enc_image_features"), ("enc_image_loc", "enc_image_spatials"), ("enc_image_mask", "enc_image_mask"))


@torch.no_grad()
def generate_dialogs(q_model, a_model, batch, num_rounds=10, sep_id=102, q_kwargs=None, a_kwargs=None, q_uniforms=None,
                     a_uniforms=None, soft_top_k=None):
    """`num_rounds` question / answer rounds for every row of `batch` -- `dialog_round`'s `state` dict (enc_image_features,
    enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments, enc_input_len, dec_input_ids, dec_attention_mask on the models'
    device; the text tensors are updated in place, like `dialog_round`'s).  Per round: question, append, answer,
    answer_perplexity(reuse_decode_state=True), append with segment 1.  q_uniforms / a_uniforms [R, max_seq_len, rows]: slice r
    is round r's `uniforms=` keyword.  No host synchronisation inside the loop; one read of the kernel's `full` flags behind it
    (RuntimeError "context already full ..." if a row had no room for its [SEP], where the reference raises per row).
    Returns a dict: questions, answers [B, R, U] int64 (the answers as they stand after the perplexity pass: [SEP] -> [PAD]),
    ppl [B, R] fp32, abnormal [B] bool, and the final context enc_input_ids, enc_segments, enc_input_len.
    soft_top_k = K: also the teacher's soft labels of the perplexity pass -- soft_ids int64 / soft_logp fp32 [B, R, U, K] (the K
    best tokens of every answer position, gstvd_topk_logp) and soft_tgt int64 [B, R, U], the labels that pass was scored against."""
    q_kwargs = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=4) if q_kwargs is None else dict(q_kwargs)
    a_kwargs = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=0) if a_kwargs is None else dict(a_kwargs)
    ids, segs, lens = batch["enc_input_ids"], batch["enc_segments"], batch["enc_input_len"]
    if not ids.is_cuda:
        raise GstvdError("generate_dialogs needs GPU tensors (got %s); there is no CPU path" % ids.device)
    R = int(num_rounds)
    for name, u in (("q_uniforms", q_uniforms), ("a_uniforms", a_uniforms)):
        if u is not None and (u.dim() != 3 or u.shape[0] < R):
            raise GstvdError("%s must be [num_rounds = %d, max_seq_len, rows], got %s" % (name, R, tuple(u.shape)))
    B = ids.shape[0]
    dev = ids.device
    att = (ids != 0).float()                                # kept by the kernel from here on
    abnormal = torch.zeros(B, dtype=torch.int32, device=dev)
    full = torch.zeros(B, dtype=torch.int32, device=dev)
    questions = answers = ppls = soft_ids = soft_logp = soft_tgt = None
    for r in range(R):
        enc = dict(enc_image_features=batch["enc_image_features"], enc_image_spatials=batch["enc_image_spatials"],
                   enc_image_mask=batch["enc_image_mask"], enc_input_ids=ids, enc_segments=segs, enc_attention_mask=att)
        qk = q_kwargs if q_uniforms is None else dict(q_kwargs, uniforms=q_uniforms[r])
        ak = a_kwargs if a_uniforms is None else dict(a_kwargs, uniforms=a_uniforms[r])
        ques = q_model(dec_input_ids=batch["dec_input_ids"], dec_attention_mask=batch["dec_attention_mask"], **qk, **enc)
        ops.context_append(ids, lens, ques, sep_id, abnormal, full, att_mask=att)
        ans = a_model(dec_input_ids=batch["dec_input_ids"], dec_attention_mask=batch["dec_attention_mask"], **ak, **enc)
        if soft_top_k is None:
            ppl, _ = answer_perplexity(a_model, enc, ans, reuse_decode_state=True)
        else:
            ppl, _, soft = answer_perplexity(a_model, enc, ans, reuse_decode_state=True, soft_top_k=soft_top_k)
            if soft_ids is None:
                K = soft[0].shape[-1]
                soft_ids = torch.zeros(B, R, ans.shape[1], K, dtype=torch.long, device=dev)
                soft_logp = torch.zeros(B, R, ans.shape[1], K, dtype=torch.float32, device=dev)
                soft_tgt = torch.zeros(B, R, ans.shape[1], dtype=torch.long, device=dev)
            soft_ids[:, r], soft_logp[:, r], soft_tgt[:, r] = soft
        ops.context_append(ids, lens, ans, sep_id, abnormal, full, segments=segs, segment_value=1, att_mask=att)
        if questions is None:
            questions = torch.zeros(B, R, ques.shape[1], dtype=torch.long, device=dev)
            answers = torch.zeros(B, R, ans.shape[1], dtype=torch.long, device=dev)
            ppls = torch.zeros(B, R, dtype=torch.float32, device=dev)
        questions[:, r], answers[:, r], ppls[:, r] = ques, ans, ppl
    if R > 0 and bool(full.any()):                          # the loop's one host synchronisation
        raise RuntimeError("context already full: cannot place [SEP] (rows %s)" % full.nonzero().flatten().tolist())
    out = dict(questions=questions, answers=answers, ppl=ppls, abnormal=abnormal != 0, enc_input_ids=ids, enc_segments=segs,
               enc_input_len=lens)
    if soft_top_k is not None:
        out.update(soft_ids=soft_ids, soft_logp=soft_logp, soft_tgt=soft_tgt)
    return out


def align_soft_labels(soft_ids, soft_logp, soft_tgt, dec_labels):
    """The teacher's soft labels on the student's decoder rows, decided on whatever device the tensors live on without a host
    synchronisation.  soft_ids / soft_logp [..., Ut, K], soft_tgt [..., Ut] (the labels of the teacher's pass), dec_labels
    [..., Ud] (the student's).  Teacher position i serves train position i.  A row's soft labels are used only if
    soft_tgt[..., i] == dec_labels[..., i] at EVERY position with dec_labels != 0 (a position >= Ut with a label fails the row:
    the teacher never scored it); otherwise, and at positions >= Ut, the row gets ids = -1, logp = 0 and trains on its hard labels
    alone.  -> (dec_soft_ids int64, dec_soft_logp fp32) [..., Ud, K]."""
    Ut, K = soft_ids.shape[-2:]
    Ud = dec_labels.shape[-1]
    if soft_ids.shape != soft_logp.shape or soft_tgt.shape != soft_ids.shape[:-1] or soft_tgt.shape[:-1] != dec_labels.shape[:-1]:
        raise GstvdError("align_soft_labels: soft_ids / soft_logp [..., U, K], soft_tgt [..., U] and dec_labels [..., Ud] do not "
                         "belong together: %s %s %s %s" % (tuple(soft_ids.shape), tuple(soft_logp.shape), tuple(soft_tgt.shape),
                                                          tuple(dec_labels.shape)))
    n = min(Ut, Ud)
    lead = tuple(dec_labels.shape[:-1])
    tgt = dec_labels.new_zeros(lead + (Ud,))
    tgt[..., :n] = soft_tgt[..., :n]
    scored = torch.zeros(Ud, dtype=torch.bool, device=dec_labels.device)
    scored[:n] = True
    ok = (((tgt == dec_labels) & scored) | (dec_labels == 0)).all(-1)                   # [...]: the row's alignment holds
    use = ok[..., None] & scored                                                          # [..., Ud]
    ids = soft_ids.new_full(lead + (Ud, K), -1)
    logp = soft_logp.new_zeros(lead + (Ud, K))
    ids[..., :n, :] = soft_ids[..., :n, :]
    logp[..., :n, :] = soft_logp[..., :n, :]
    ids = torch.where(use[..., None], ids, torch.full_like(ids, -1))
    logp = torch.where(use[..., None], logp, torch.zeros_like(logp))
    return ids, logp


def image_noise(feats, image_mask, u_img, mask_prob):
    """utils/data_utils.py:89-101 on the device, literally and in float64: a real region i has its features zeroed iff
    u < mask_prob and u / mask_prob < 0.9; the global row 0 is not exempt.  Returns a new tensor."""
    u = u_img.to(torch.float64)
    hit = (u < mask_prob) & ((u / mask_prob) < 0.9) & (image_mask != 0)
    return feats.masked_fill(hit.unsqueeze(-1), 0)


def dialog_train_batch(dialogs, caption_ids, image, params, u_tok=None, u_img=None):
    """The student's batch of the dialogs `generate_dialogs` returned, on the device, in the layout of SURVEY appendix B: text
    tensors [B, R, 1, L] (one `ops.dialog_rows` launch, valid = ~abnormal), image tensors unexpanded [B, 37, ...].
    caption_ids int64 [B, Lc], 0-padded captions WITHOUT [CLS] / [SEP] (cut to 38 tokens here); `image`: a dict with
    enc_image_feat / enc_image_loc / enc_image_mask (or the generation state's enc_image_features / enc_image_spatials / ...);
    params: select_data, threshold, mask_prob, max_seq_len, max_utt_len.  u_tok fp32 [B, R, max_seq_len] / u_img [B, 37]: the
    uniforms of the [MASK] noise and of the image noise; None: drawn from torch's generator (mask_prob == 0 needs none); False:
    never drawn (the call then raises if mask_prob > 0).  image_label / image_target are dead inputs of the enc_dec path and are
    not produced.  Dialogs generated with soft_top_k carry the teacher's soft labels: the batch then has dec_soft_ids / dec_soft_logp
    [B, R, 1, Ud, K] (`align_soft_labels`), which `step.forward` hands to the student."""
    ques, ans, ppl = dialogs["questions"], dialogs["answers"], dialogs["ppl"]
    mask_prob = float(params["mask_prob"])
    T, Ud = int(params["max_seq_len"]), int(params.get("max_utt_len", 25))
    if ques.dim() != 3:
        raise GstvdError("dialog_train_batch: questions / answers must be [B, R, U]")
    B, R, _ = ques.shape
    if 2 * R > ops.DIALOG_MAX_SEP:
        raise GstvdError("dialog_train_batch: %d rounds give %d separators, more than max_sep_len = %d allows"
                         % (R, 2 * R, ops.DIALOG_MAX_SEP))
    if mask_prob > 0.0 and (u_tok is False or u_img is False):
        raise GstvdError("dialog_train_batch: mask_prob = %g needs the uniforms u_tok [B, R, %d] and u_img [B, regions]" % (mask_prob, T))
    if not ques.is_cuda:
        raise GstvdError("dialog_train_batch needs GPU tensors (got %s); there is no CPU path" % ques.device)
    dev = ques.device
    img = {k: (image[k] if k in image else image[alt]) for k, alt in _IMAGE_KEYS}
    if u_tok is None or u_tok is False:
        u_tok = torch.rand(B, R, T, device=dev, dtype=torch.float32) if mask_prob > 0.0 else None
    if u_img is None or u_img is False:
        u_img = torch.rand(img["enc_image_mask"].shape, device=dev, dtype=torch.float64) if mask_prob > 0.0 else None
    cap = caption_ids[:, :MAX_CAPTION_LEN].contiguous()
    abnormal = dialogs.get("abnormal")
    valid = (~abnormal.bool()).to(torch.int32) if abnormal is not None else None
    rows = ops.dialog_rows(cap, ques.contiguous(), ans.contiguous(), ppl.float().contiguous(), T, Ud, params["select_data"],
                           params["threshold"], mask_prob, valid=valid, u_tok=u_tok)
    feats = img["enc_image_feat"]
    if mask_prob > 0.0:
        feats = image_noise(feats, img["enc_image_mask"], u_img.to(dev), mask_prob)
    names = (("enc_input_ids", "enc_ids"), ("enc_segments", "enc_seg"), ("enc_sep_indices", "enc_sep"), ("enc_mlm_labels", "enc_mlm"),
             ("enc_att_mask", "enc_att"), ("dec_input_ids", "dec_ids"), ("dec_att_mask", "dec_att"), ("dec_labels", "dec_labels"))
    out = {k: rows[src].unsqueeze(2) for k, src in names}
    out["enc_hist_len"] = rows["enc_hist_len"].unsqueeze(2)
    out["enc_next_sentence_labels"] = torch.full((B, R, 1), -1, dtype=torch.long, device=dev)
    out["enc_image_feat"], out["enc_image_loc"], out["enc_image_mask"] = feats, img["enc_image_loc"], img["enc_image_mask"]
    if dialogs.get("soft_ids") is not None:
        sid, slp = align_soft_labels(dialogs["soft_ids"], dialogs["soft_logp"], dialogs["soft_tgt"], rows["dec_labels"])
        out["dec_soft_ids"], out["dec_soft_logp"] = sid.unsqueeze(2), slp.unsqueeze(2)
    return out
