"""Masked-LM fill-in of the `random_token` text attack (utils/text_attack.py:30-56, evaluate_gen_attack.py:209-226).

The reference keeps a pretrained `BertForMaskedLM` next to the dialog model and replaces the [MASK] tokens of a context by the
arg-max token of its logits.  Here that model is a degenerate configuration of the package's own encoder: with
`v_biattention_id = t_biattention_id = []` and `v_num_hidden_layers = 0` the encoder schedule is the N text layers alone
(config.encoder_schedule), and embeddings + text layers + cls.predictions (transform, decoder tied to the word table, bias) are
BertForMaskedLM under the same sub-module names.  `MaskedLMFiller` owns such an encoder-only model, maps a BertForMaskedLM
state dict into it, and runs `VisualDialogEncoder.predict_masked` -- the arg-max over the vocabulary happens on the device, in
the bf16 engine without the [n, vocab] logits ever being stored (csrc/vocab_argmax.hip).

Parameters the checkpoint does not cover keep their initial values and reach nothing that is returned: the type-extension table
(segment ids stay below type_vocab_size), sep_embeddings, the image embedding of the one dummy region (it runs; no text layer
reads it), the poolers, the NSP and region heads.
"""
import json
import os
import tempfile

import torch

# sizes of the vision side of the text-only model: one dummy region, as small as the kernels' alignment rules allow
_DUMMY_V = dict(v_feature_size=64, v_hidden_size=64, v_num_attention_heads=1, v_intermediate_size=64, v_target_size=64,
                bi_hidden_size=64, bi_num_attention_heads=1, v_num_hidden_layers=0, v_biattention_id=[], t_biattention_id=[])
_BERT_KEYS = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "hidden_act",
              "max_position_embeddings", "type_vocab_size", "initializer_range")


def text_only_config(config):
    """The encoder configuration (a dict) of the text-only model for a BERT configuration `config`: a dict, or any object
    with BertConfig's attributes (transformers' BertConfig, this package's).  layer_norm_eps must be the 1e-12 the engine's
    LayerNorms use."""
    get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    out = {}
    for k in _BERT_KEYS:
        v = get(k)
        if v is not None:
            out[k] = v
    eps = get("layer_norm_eps", 1e-12)
    if abs(float(eps) - 1e-12) > 1e-18:
        raise NotImplementedError("layer_norm_eps=%r: the encoder's LayerNorms use 1e-12 (BERT's value)" % (eps,))
    if out.get("hidden_size") and out.get("num_attention_heads"):
        if out["hidden_size"] % out["num_attention_heads"] or out["hidden_size"] // out["num_attention_heads"] not in (32, 64, 128):
            raise NotImplementedError("hidden_size %d over %d heads: the attention kernels implement head sizes 32, 64 and 128 "
                                      "(bert-base: 64)" % (out["hidden_size"], out["num_attention_heads"]))
    out.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
               v_attention_probs_dropout_prob=0.0, v_hidden_act="gelu")
    out.update(_DUMMY_V)
    return out


_LAYER = (("attention.self.query", "attention.self.query"), ("attention.self.key", "attention.self.key"),
          ("attention.self.value", "attention.self.value"), ("attention.output.dense", "attention.output.dense"),
          ("attention.output.LayerNorm", "attention.output.LayerNorm"), ("intermediate.dense", "intermediate.dense"),
          ("output.dense", "output.dense"), ("output.LayerNorm", "output.LayerNorm"))


def _ln_names(sd, prefix):
    """(weight key, bias key) of a LayerNorm in `sd`: LayerNorm.weight / bias, or the legacy gamma / beta."""
    if prefix + ".weight" in sd or prefix + ".gamma" not in sd:
        return prefix + ".weight", prefix + ".bias"
    return prefix + ".gamma", prefix + ".beta"


def map_bert_mlm_state_dict(sd, num_layers):
    """BertForMaskedLM state dict -> ({key of VisualDialogEncoder.state_dict(): tensor}, [ignored keys]).  Raises KeyError
    naming a missing required key, ValueError naming `cls.predictions.decoder.weight` / `.decoder.bias` when they are present
    and differ from the word table / `cls.predictions.bias` (the package's head is tied: an untied checkpoint cannot be
    represented)."""
    out, used = {}, set()

    def take(src, dst):
        if src not in sd:
            raise KeyError("BertForMaskedLM state dict: required key %r is missing" % src)
        out["bert_pretrained." + dst] = sd[src]
        used.add(src)

    def take_ln(src, dst):
        w, b = _ln_names(sd, src)
        take(w, dst + ".weight")
        take(b, dst + ".bias")

    for name in ("word_embeddings", "position_embeddings", "token_type_embeddings"):
        take("bert.embeddings.%s.weight" % name, "bert.embeddings.%s.weight" % name)
    take_ln("bert.embeddings.LayerNorm", "bert.embeddings.LayerNorm")
    for i in range(num_layers):
        for src, dst in _LAYER:
            s, d = "bert.encoder.layer.%d.%s" % (i, src), "bert.encoder.layer.%d.%s" % (i, dst)
            if src.endswith("LayerNorm"):
                take_ln(s, d)
            else:
                take(s + ".weight", d + ".weight")
                take(s + ".bias", d + ".bias")
    take("cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.weight")
    take("cls.predictions.transform.dense.bias", "cls.predictions.transform.dense.bias")
    take_ln("cls.predictions.transform.LayerNorm", "cls.predictions.transform.LayerNorm")
    take("cls.predictions.bias", "cls.predictions.bias")
    word = sd["bert.embeddings.word_embeddings.weight"]
    for key, ref in (("cls.predictions.decoder.weight", word), ("cls.predictions.decoder.bias", sd["cls.predictions.bias"])):
        if key in sd:
            if sd[key].shape != ref.shape or not torch.equal(sd[key].to(ref.dtype).cpu(), ref.cpu()):
                raise ValueError("BertForMaskedLM state dict: %r is not tied (it differs from %s); the masked-LM head of this "
                                 "package is tied" % (key, "the word table" if key.endswith("weight") else "cls.predictions.bias"))
            used.add(key)
    return out, sorted(k for k in sd if k not in used)


class MaskedLMFiller(object):
    """BertForMaskedLM as a text-only VisualDialogEncoder (model 'enc_only_a', eval mode) with the fill rule of
    TextAttack.random_token_attack on top.  `config`: a BERT configuration (dict or object); `precision`: 'bf16' or 'fp32'."""

    def __init__(self, config, device, precision="bf16", mask_token_id=103):
        from .modules import VisualDialogEncoder
        self.device = torch.device(device)
        self.mask_token_id = int(mask_token_id)
        self.enc_config = text_only_config(config)
        d = tempfile.mkdtemp(prefix="gstvd_mlm_")
        path = os.path.join(d, "enc.json")
        try:
            with open(path, "w") as f:
                json.dump(self.enc_config, f)
            self.params = dict(model_enc_config=path, gpu_ids=[self.device.index or 0], model="enc_only_a", mode="vd_eval_val",
                               batch_size=1, device=self.device, amd_precision=precision)
            self.model = VisualDialogEncoder(self.params)
        finally:
            if os.path.exists(path):
                os.remove(path)
            os.rmdir(d)
        self.model.eval()
        self.model.to(self.device)
        self._dummy = {}

    def load_bert_mlm_state_dict(self, sd):
        """Load a BertForMaskedLM state dict (see map_bert_mlm_state_dict for the refusals) -> the ignored keys
        (`bert.embeddings.position_ids`, a pooler, ...)."""
        mapped, ignored = map_bert_mlm_state_dict(sd, self.enc_config["num_hidden_layers"])
        own = self.model.state_dict()
        for k, v in mapped.items():
            if own[k].shape != v.shape:
                raise ValueError("BertForMaskedLM state dict: %r has shape %s, the configuration needs %s"
                                 % (k[len("bert_pretrained."):], tuple(v.shape), tuple(own[k].shape)))
        merged = dict(own)
        merged.update(mapped)
        merged["bert_pretrained.cls.predictions.decoder.weight"] = mapped["bert_pretrained.bert.embeddings.word_embeddings.weight"]
        self.model.load_state_dict(merged, strict=True)      # in-place copies: an engine's flat views (and shadow version) follow
        return ignored

    def _image(self, B):
        if B not in self._dummy:
            c = self.enc_config
            self._dummy[B] = (torch.zeros(B, 1, c["v_feature_size"], device=self.device), torch.zeros(B, 1, 5, device=self.device),
                              torch.ones(B, 1, device=self.device))
        return self._dummy[B]

    def host_rows(self, input_ids):
        """Flat indices (int64, host) of the positions of host tensor `input_ids` equal to the mask token: no device round trip."""
        return (input_ids.reshape(-1).cpu() == self.mask_token_id).nonzero().view(-1)

    def predict(self, input_ids, token_type_ids=None, attention_mask=None, rows=None, image=None):
        """The multi-row form: arg-max token and its logit at every [MASK] position of input_ids [B, T], all rows in one pass
        -> (flat positions [n], token ids [n], logits [n]).  `rows`: the flat positions, when the caller has them on the host.
        `image`: (features, boxes, mask) in place of the dummy region (nothing returned depends on it)."""
        ids = input_ids.to(self.device)
        B = ids.shape[0]
        if rows is None:
            rows = (ids.reshape(-1) == self.mask_token_id).nonzero().view(-1)
        rows = rows.to(self.device, torch.int64)
        feats, loc, vmask = image if image is not None else self._image(B)
        seg = None if token_type_ids is None else token_type_ids.to(self.device)
        att = None if attention_mask is None else attention_mask.to(self.device)
        idx, val = self.model.predict_masked(ids, feats, loc, token_type_ids=seg, attention_mask=att, image_attention_mask=vmask,
                                             rows=rows, mask_token_id=self.mask_token_id)
        return rows, idx, val

    def fill(self, input_ids, token_type_ids, attention_mask, rows=None):
        """The rule of TextAttack.random_token_attack: only row 0 of input_ids [B, T] is read; its positions equal to the mask
        token receive the masked-LM's arg-max token there; the result is that row repeated B times ([B, T] int64 on the
        filler's device).  No mask position: row 0 repeated unchanged.  `rows`: the mask positions of row 0 (indices < T), from
        a caller that has the ids on the host.
        Unlike the reference, which writes the predictions into a view of the caller's tensor (nothing downstream reads it),
        the caller's `input_ids` is NOT modified."""
        B = input_ids.shape[0]
        row0 = input_ids[:1].to(self.device, copy=True)
        seg = None if token_type_ids is None else token_type_ids[:1]
        att = None if attention_mask is None else attention_mask[:1]
        rows, idx, _ = self.predict(row0, seg, att, rows=rows)
        if rows.numel():
            row0.view(-1).index_copy_(0, rows, idx)
        return row0.repeat(B, 1)
