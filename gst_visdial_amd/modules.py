"""Host-side mirror of the reference's module API for the enc_dec_a path and for the enc_only_a model (ranking and training).

`VisualDialogEncoder`, `VisualDialogDecoder`, `EncoderDecoderModel`, `VLFusion` keep the constructor and
forward signatures, return conventions and the `state_dict()` key layout of

    models/visual_dialog_encoder.py:7-76, models/visual_dialog_decoder.py:18-86,
    models/visual_dialog_model.py:8-135  (+ the parameter tree of models/vilbert_dialog.py)

so that the reference's scripts (train_gen.py:200-202,293; evaluate_gen.py:177-186; generate.py:60-77) can
build, alias (`decoder.decoder.bert.embeddings = encoder.bert_pretrained.bert.embeddings`), load checkpoints
into and call them unchanged.  The sub-modules below are *parameter holders only* (their forward raises):
all arithmetic runs in `engine.Engine` through the HIP C ABI.  There is no CPU execution path.
"""
import torch
from torch import nn

from .config import BertConfig, DecoderConfig


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("gst_visdial_amd parameter holder: compute runs in engine.Engine via the HIP C ABI, "
                           "call EncoderDecoderModel / VisualDialogEncoder / VisualDialogDecoder instead")


class Linear(_Holder):
    def __init__(self, n_in, n_out, bias=True, std=0.02):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n_out, n_in).normal_(0.0, std))
        self.bias = nn.Parameter(torch.zeros(n_out)) if bias else None


class Embedding(_Holder):
    def __init__(self, n, dim, std=0.02):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, dim).normal_(0.0, std))


class LayerNorm(_Holder):
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class BertEmbeddingsDialog(_Holder):
    """Parameters of models/vilbert_dialog.py:298-322 (the unused sinusoid table is not built)."""

    def __init__(self, cfg):
        super().__init__()
        H, s = cfg.hidden_size, cfg.initializer_range
        self.word_embeddings = Embedding(cfg.vocab_size, H, s)
        self.position_embeddings = Embedding(cfg.max_position_embeddings, H, s)
        self.token_type_embeddings = Embedding(cfg.type_vocab_size, H, s)
        self.token_type_embeddings_extension = Embedding(10, H, s)
        self.sep_embeddings = Embedding(50, H, s)
        self.LayerNorm = LayerNorm(H)


class _SelfAttention(_Holder):
    def __init__(self, hidden, std):
        super().__init__()
        self.query, self.key, self.value = Linear(hidden, hidden, std=std), Linear(hidden, hidden, std=std), Linear(hidden, hidden, std=std)


class _AttnOutput(_Holder):
    def __init__(self, n_in, n_out, std):
        super().__init__()
        self.dense = Linear(n_in, n_out, std=std)
        self.LayerNorm = LayerNorm(n_out)


class _Attention(_Holder):
    def __init__(self, hidden, std):
        super().__init__()
        self.self = _SelfAttention(hidden, std)
        self.output = _AttnOutput(hidden, hidden, std)


class _Intermediate(_Holder):
    def __init__(self, hidden, inter, std):
        super().__init__()
        self.dense = Linear(hidden, inter, std=std)


class _Layer(_Holder):
    """BertLayer / BertImageLayer parameter tree (vilbert_dialog.py:465-476, 592-603)."""

    def __init__(self, hidden, inter, std, cross=False):
        super().__init__()
        self.attention = _Attention(hidden, std)
        if cross:
            self.crossattention = _Attention(hidden, std)
        self.intermediate = _Intermediate(hidden, inter, std)
        self.output = _AttnOutput(inter, hidden, std)


class _BiAttention(_Holder):
    def __init__(self, cfg):
        super().__init__()
        s, Hb = cfg.initializer_range, cfg.bi_hidden_size
        self.query1, self.key1, self.value1 = (Linear(cfg.v_hidden_size, Hb, std=s) for _ in range(3))
        self.query2, self.key2, self.value2 = (Linear(cfg.hidden_size, Hb, std=s) for _ in range(3))


class _BiOutput(_Holder):
    def __init__(self, cfg):
        super().__init__()
        s, Hb = cfg.initializer_range, cfg.bi_hidden_size
        self.dense1 = Linear(Hb, cfg.v_hidden_size, std=s)
        self.LayerNorm1 = LayerNorm(cfg.v_hidden_size)
        self.q_dense1 = Linear(Hb, cfg.v_hidden_size, std=s)      # unused by the reference (vilbert_dialog.py:722)
        self.dense2 = Linear(Hb, cfg.hidden_size, std=s)
        self.LayerNorm2 = LayerNorm(cfg.hidden_size)
        self.q_dense2 = Linear(Hb, cfg.hidden_size, std=s)        # unused by the reference (:729)


class _ConnectionLayer(_Holder):
    """BertConnectionLayer parameter tree (vilbert_dialog.py:746-757)."""

    def __init__(self, cfg):
        super().__init__()
        s = cfg.initializer_range
        self.biattention = _BiAttention(cfg)
        self.biOutput = _BiOutput(cfg)
        self.v_intermediate = _Intermediate(cfg.v_hidden_size, cfg.v_intermediate_size, s)
        self.v_output = _AttnOutput(cfg.v_intermediate_size, cfg.v_hidden_size, s)
        self.t_intermediate = _Intermediate(cfg.hidden_size, cfg.intermediate_size, s)
        self.t_output = _AttnOutput(cfg.intermediate_size, cfg.hidden_size, s)


class _TwoStreamEncoder(_Holder):
    def __init__(self, cfg):
        super().__init__()
        s = cfg.initializer_range
        self.layer = nn.ModuleList([_Layer(cfg.hidden_size, cfg.intermediate_size, s) for _ in range(cfg.num_hidden_layers)])
        self.v_layer = nn.ModuleList([_Layer(cfg.v_hidden_size, cfg.v_intermediate_size, s) for _ in range(cfg.v_num_hidden_layers)])
        self.c_layer = nn.ModuleList([_ConnectionLayer(cfg) for _ in range(len(cfg.v_biattention_id))])


class _ImageEmbeddings(_Holder):
    def __init__(self, cfg):
        super().__init__()
        s = cfg.initializer_range
        self.image_embeddings = Linear(cfg.v_feature_size, cfg.v_hidden_size, std=s)
        self.image_location_embeddings = Linear(5, cfg.v_hidden_size, std=s)
        self.LayerNorm = LayerNorm(cfg.v_hidden_size)


class _Pooler(_Holder):
    def __init__(self, n_in, n_out, std):
        super().__init__()
        self.dense = Linear(n_in, n_out, std=std)


class _BertModel(_Holder):
    """BertModel parameter tree (vilbert_dialog.py:1310-1323)."""

    def __init__(self, cfg):
        super().__init__()
        self.embeddings = BertEmbeddingsDialog(cfg)
        self.v_embeddings = _ImageEmbeddings(cfg)
        self.encoder = _TwoStreamEncoder(cfg)
        self.t_pooler = _Pooler(cfg.hidden_size, cfg.bi_hidden_size, cfg.initializer_range)       # dead in enc_dec
        self.v_pooler = _Pooler(cfg.v_hidden_size, cfg.bi_hidden_size, cfg.initializer_range)     # dead in enc_dec


class _HeadTransform(_Holder):
    def __init__(self, hidden, std):
        super().__init__()
        self.dense = Linear(hidden, hidden, std=std)
        self.LayerNorm = LayerNorm(hidden)


class _LMPredictionHead(_Holder):
    def __init__(self, cfg, tied_weight):
        super().__init__()
        self.transform = _HeadTransform(cfg.hidden_size, cfg.initializer_range)
        self.decoder = Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        self.decoder.weight = tied_weight                      # tied to the word embedding (vilbert_dialog.py:991)
        self.bias = nn.Parameter(torch.zeros(cfg.vocab_size))


class _ImagePredictionHead(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.transform = _HeadTransform(cfg.v_hidden_size, cfg.initializer_range)
        self.decoder = Linear(cfg.v_hidden_size, cfg.v_target_size, std=cfg.initializer_range)


class _PreTrainingHeads(_Holder):
    """cls.* of BertForMultiModalPreTraining (vilbert_dialog.py:1017-1024): dead compute in enc_dec mode
    (outputs discarded at :1485-1487); kept only so checkpoints load with strict key matching."""

    def __init__(self, cfg, tied_weight):
        super().__init__()
        self.predictions = _LMPredictionHead(cfg, tied_weight)
        self.bi_seq_relationship = Linear(cfg.bi_hidden_size, 2, std=cfg.initializer_range)
        self.imagePredictions = _ImagePredictionHead(cfg)


class BertForMultiModalPreTraining(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.bert = _BertModel(cfg)
        self.cls = _PreTrainingHeads(cfg, self.bert.embeddings.word_embeddings.weight)


class _GenerationLMHead(_Holder):
    """BertGenerationOnlyLMHead (visual_dialog_decoder.py:326-343): `decoder.weight` starts tied to the decoder's
    own word embedding and stays a separate parameter once the embedding module is replaced by the encoder's;
    `bias` and `decoder.bias` are one parameter under two names."""

    def __init__(self, tied_weight):
        super().__init__()
        V, H = tied_weight.shape
        self.decoder = Linear(H, V)
        self.decoder.weight = tied_weight
        self.bias = nn.Parameter(torch.zeros(V))
        self.decoder.bias = self.bias


class _GenerationStack(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(cfg.hidden_size, cfg.intermediate_size, cfg.initializer_range, cross=True)
                                    for _ in range(cfg.num_hidden_layers)])


class BertGenerationEncoder(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.embeddings = BertEmbeddingsDialog(cfg)
        self.encoder = _GenerationStack(cfg)


class BertForSequenceGeneration(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.bert = BertGenerationEncoder(cfg)
        self.lm_head = _GenerationLMHead(self.bert.embeddings.word_embeddings.weight)

    def _reorder_cache(self, past, beam_idx):   # exists in the reference (visual_dialog_decoder.py:177-181), never called
        return tuple(tuple(s.index_select(0, beam_idx) for s in layer) for layer in past)


class VLFusion(_Holder):
    """models/visual_dialog_model.py:123-135."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.fc_l = Linear(config.hidden_size, config.hidden_size)
        self.fc_v = Linear(config.v_hidden_size, config.hidden_size)


class DecoderOutput(object):
    """The fields of transformers' Seq2SeqLMOutput the reference reads (visual_dialog_model.py:72)."""

    def __init__(self, loss, logits):
        self.loss, self.logits = loss, logits
        self.past_key_values = self.decoder_hidden_states = self.decoder_attentions = self.cross_attentions = None


def _check_master_current(engine, what):
    """state_dict() of the model OR of one of its sub-modules (train_gen.py:346-357 saves `model.module.encoder` /
    `.decoder` state dicts separately in some forks): refused while a sharded optimizer holds stale fp32 masters here."""
    pipe = getattr(engine, "pipe", None) if engine is not None else None
    if pipe is not None and hasattr(pipe, "check_master_current"):
        pipe.check_master_current(what)


class VisualDialogEncoder(nn.Module):
    """models/visual_dialog_encoder.py:7-76.  `params` is held by reference and re-read on every call.

    model = 'enc_dec_*': the encoder half of an EncoderDecoderModel (hidden states out).
    model = 'enc_only_a': the discriminative model of evaluate_disc.py / train_disc.py.  The module owns an encoder-only engine.
    Under an eval mode `forward` returns the reference's 7-tuple with `seq_relationship_score` [B, 2] fp32 in place 3 and None
    everywhere else -- including `prediction_scores_t`, the MLM logits over all B*T tokens (6 GB at 200 x 256 x 30522), which
    the reference computes and its only caller discards (evaluate_disc.py:79): deliberately not computed here.
    Under a mode containing 'train' (params['mode'] decides the branch, as in the reference; the module's `.training` decides
    dropout) and with masked_lm_labels, next_sentence_label, image_label and image_target all given, it returns
    (lm_loss [1], img_loss [1], nsp_loss [1], seq_relationship_score, None, None, None): the three unscaled losses of
    models/vilbert_dialog.py:1496-1510, differentiable -- `loss.backward()` fills `.grad` of every parameter but
    sep_embeddings and q_dense* (Engine.disc_step).  A train-mode call without those four labels, and a module left in
    training state under an eval mode, raise."""

    def __init__(self, params):
        super().__init__()
        self.params = params
        self.config = BertConfig.from_json_file(params["model_enc_config"])
        self.config.__dict__["cur_device"] = params["gpu_ids"][0]
        self.config.__dict__["model_arch"] = params["model"]
        self.config.__dict__["mode"] = params["mode"]
        self.config.validate()
        self.model_arch = params["model"]
        if "enc_dec" not in self.model_arch and self.model_arch != "enc_only_a":
            raise NotImplementedError("gst_visdial_amd implements the enc_dec_* generative path and the discriminative "
                                      "enc_only_a model only (model=%r)" % self.model_arch)
        # the reference calls from_pretrained('bert-base-uncased') (network); here weights come from
        # load_state_dict / a checkpoint, with BERT-style N(0, 0.02) init as the starting point
        self.bert_pretrained = BertForMultiModalPreTraining(self.config)
        self._engine_owner = None
        self._engine = None

    @property
    def engine(self):
        """enc_only_a: the module's own encoder-only engine, built on first use (as EncoderDecoderModel.engine is)."""
        if self.model_arch != "enc_only_a":
            raise AttributeError("a VisualDialogEncoder of an enc_dec model runs on its EncoderDecoderModel's engine")
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self)
        return self._engine

    def state_dict(self, *args, **kwargs):
        if not kwargs.get("prefix") and not (len(args) > 1 and args[1]):      # (a parent's state_dict() has checked already)
            _check_master_current(getattr(self, "_standalone_engine", None), "model.encoder.state_dict()")
        return super().state_dict(*args, **kwargs)

    def _check_disc_inference(self):
        mode = self.params["mode"]
        if "train" in mode or self.training:
            raise NotImplementedError(
                "the ranking branch of the enc_only_a model (evaluate_disc.py) needs an eval mode and .eval(): mode=%r, "
                "module.training=%s.  The training branch of train_disc.py is forward(...) under a 'train' mode with "
                "masked_lm_labels, next_sentence_label, image_label and image_target" % (mode, self.training))

    def nsp_scores(self, input_ids, image_feat, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None):
        """enc_only_a: (seq_relationship_score [B, 2], softmax(score, 1)[:, 0] [B]), both fp32, the second straight from the
        head kernel -- what evaluate_disc.py:81-83 ranks the answer options by."""
        self._check_disc_inference()
        return self.engine.nsp_scores(image_feat, image_loc, image_attention_mask, input_ids, token_type_ids, attention_mask)

    def predict_masked(self, input_ids, image_feat, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None,
                       rows=None, mask_token_id=103):
        """enc_only_a, eval mode: the arg-max token of the model's own tied MLM head (cls.predictions) at the token positions
        `rows` -> (token ids [n] int64, their logits [n] fp32), in the order of `rows`; equal logits go to the smaller id.
        `rows`: flat indices into input_ids.view(-1) (int64, ascending), from a caller that has the ids on the host; None: the
        positions equal to `mask_token_id`, taken from the device tensor with `nonzero` (one host synchronisation), the
        convention of `token_rows` in forward.  No position: two empty tensors, nothing is launched for the head.  On the
        two-stream model this is the visually grounded fill-in; on a text-only config (mlm.MaskedLMFiller) BertForMaskedLM's."""
        self._check_disc_inference()
        if rows is None:
            rows = (input_ids.reshape(-1) == int(mask_token_id)).nonzero().view(-1)
        return self.engine.mlm_argmax(image_feat, image_loc, image_attention_mask, input_ids, token_type_ids, attention_mask, rows)

    def attention_maps(self, input_ids, image_feat, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None,
                       select=None, heads="all"):
        """The softmax probabilities of the encoder's attention sites, what the reference's BertModel returns under
        output_all_attention_masks=True (models/vilbert_dialog.py:806-912; the fifth output of the enc_only_a eval branch, :1519)
        -> attn_maps.AttentionMaps(t, v, c, layers): t[i] [B, nh, T, T], v[i] [B, nhv, R, R], c[i] = (probs1 [B, nhb, T, R] text
        queries over the regions, probs2 [B, nhb, R, T] region queries over the tokens), fp32 on the device.  `select`: None (every
        site) or a dict kind -> "all" / iterable of layer indices over "t", "v", "c"; `heads`: "all" or "mean" (the mean over the
        heads, no head dimension).  Eval only; the encoder runs eagerly, on the module's own engine (enc_only_a) or on the engine
        of the EncoderDecoderModel it belongs to."""
        from .engine import encoder_attention_maps, _owner_engine
        if self.model_arch == "enc_only_a":
            eng = self.engine
        else:
            eng = _owner_engine(self, "VisualDialogEncoder")
        return encoder_attention_maps(eng, input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask,
                                      select, heads)

    def forward(self, input_ids, image_feat, image_loc, sep_indices=None, token_type_ids=None, attention_mask=None,
                masked_lm_labels=None, next_sentence_label=None, image_attention_mask=None, image_label=None,
                image_target=None, token_rows=None, region_rows=None):
        """enc_only_a, train mode: `token_rows` / `region_rows` (not in the reference's signature, optional) are the flat indices
        of the tokens with masked_lm_labels != -1 and of the regions with image_label == 1, which a caller that still has the
        labels on the host passes along (evaluate_disc.forward_disc does).  Without them the two index lists are taken from
        the device tensors with `nonzero`: one host synchronisation each per call."""
        if self.model_arch == "enc_only_a" and "train" in self.params["mode"]:
            # train branch of models/visual_dialog_encoder.py:51-57
            if masked_lm_labels is None or next_sentence_label is None or image_label is None or image_target is None:
                raise NotImplementedError(
                    "the train branch of the enc_only_a model (train_disc.py) needs masked_lm_labels, next_sentence_label, "
                    "image_label and image_target; without them there is no loss to return (mode=%r)" % (self.params["mode"],))
            lm, img, nsp, score = self.engine.disc_step(image_feat, image_loc, image_attention_mask, input_ids, token_type_ids,
                                                        attention_mask, masked_lm_labels, next_sentence_label, image_label,
                                                        image_target, token_rows=token_rows, region_rows=region_rows)
            return (lm, img, nsp, score, None, None, None)
        if self.model_arch == "enc_only_a":
            # eval branch of models/visual_dialog_encoder.py:68-76; sep_indices / masked_lm_labels feed nothing in it
            score, _ = self.nsp_scores(input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask)
            return (None, None, None, score, None, None, None)
        from .engine import standalone_encoder_forward
        enc_t, enc_v = standalone_encoder_forward(self, input_ids, image_feat, image_loc, token_type_ids, attention_mask,
                                                  image_attention_mask)
        return (None, None, None, None, None, enc_t, enc_v)


class VisualDialogDecoder(nn.Module):
    """models/visual_dialog_decoder.py:18-86."""

    def __init__(self, params):
        super().__init__()
        self.params = params
        self.config = DecoderConfig.from_json_file(params["model_dec_config"])
        self.config.__dict__["cur_device"] = params["gpu_ids"][0]
        self.config.validate()
        self.decoder = BertForSequenceGeneration(self.config)

    def state_dict(self, *args, **kwargs):
        if not kwargs.get("prefix") and not (len(args) > 1 and args[1]):
            _check_master_current(getattr(self, "_standalone_engine", None), "model.decoder.state_dict()")
        return super().state_dict(*args, **kwargs)

    def _reorder_cache(self, past, beam_idx):
        return self.decoder._reorder_cache(past, beam_idx)

    def forward(self, decoder_input_ids=None, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                labels=None, use_cache=False, output_attentions=False, output_hidden_states=False, return_dict=True,
                loss_reduction=True):
        from .engine import standalone_decoder_forward
        loss, logits = standalone_decoder_forward(self, decoder_input_ids, attention_mask, encoder_hidden_states,
                                                  encoder_attention_mask, labels, loss_reduction)
        return DecoderOutput(loss, logits)


class EncoderDecoderModel(nn.Module):
    """models/visual_dialog_model.py:8-120: encoder -> VLFusion -> decoder (train/eval) or the 18-step sampling
    decode.  One `torch.autograd.Function` wraps the whole step, so `loss.backward()` runs the hand-written
    backward and fills `.grad` of every live parameter (and of `enc_image_features` when it requires grad)."""

    def __init__(self, params, encoder, decoder):
        super().__init__()
        self.params = params
        self.encoder = encoder
        self.decoder = decoder
        self.vlfusion = VLFusion(encoder.config)
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self)
            object.__setattr__(self.encoder, "_standalone_engine", self._engine)
            object.__setattr__(self.decoder, "_standalone_engine", self._engine)
        return self._engine

    def state_dict(self, *args, **kwargs):
        _check_master_current(self._engine, "model.state_dict()")
        return super().state_dict(*args, **kwargs)

    def _replicate_for_data_parallel(self):
        """nn.DataParallel(model, [0, 1, 2, 3]) (train_gen.py:295, README.md:89) replicates the module tree per device and runs the
        replicas in threads; the replicas would all drive ONE engine (one flat parameter buffer, one arena, one tape).  Refuse
        loudly instead: this framework scales as one process per GPU.  (`nn.DataParallel(model, [0])` never replicates.)"""
        from ._lib import GstvdError
        raise GstvdError(
            "gst_visdial_amd.EncoderDecoderModel cannot be replicated by nn.DataParallel over several device ids: it runs one "
            "process per GPU.  Keep nn.DataParallel(model, [local_gpu]) for the reference's `.module` access and launch N ranks "
            "(torchrun --nproc-per-node N train script) with gst_visdial_amd.pipeline.BackwardPipeline doing the gradient "
            "all-reduce over RCCL (INTEGRATION.md, 'Multi-GPU').")

    def inputs_only(self):
        """Context manager: the backward of a forward made inside it returns d loss / d enc_image_features only and leaves
        every parameter's `.grad` alone (Engine.inputs_only; the FGSM attack, attack.fgsm_features)."""
        return self.engine.inputs_only()

    def score_candidates(self, enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                         enc_attention_mask, dec_input_ids, dec_attention_mask, num_options):
        """Generative ranking scores of evaluate_gen.py:45-106 with one encoder pass per dialog round (see
        Engine.score_candidates).  Encoder tensors: one row per round; decoder tensors: num_options rows per round."""
        return self.engine.score_candidates(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids,
                                            enc_segments, enc_attention_mask, dec_input_ids, dec_attention_mask, num_options)

    def rank_loss(self, enc_image_features=None, enc_image_spatials=None, enc_image_mask=None, enc_input_ids=None, enc_segments=None,
                  enc_attention_mask=None, dec_input_ids=None, dec_attention_mask=None, relevance=None, num_options=None,
                  temperature=1.0):
        """Listwise candidate training (Engine.rank_step; rank_train.forward_rank): encoder tensors with one row per round,
        decoder tensors and `relevance` with num_options rows / values per round -> (loss, scores [rounds, num_options]).  The
        loss is differentiable like `forward`'s: `loss.backward()` fills `.grad` of every live parameter."""
        return self.engine.rank_step(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                     enc_attention_mask, dec_input_ids, dec_attention_mask, relevance, int(num_options),
                                     temperature=temperature)

    def beam_search(self, enc_image_features=None, enc_image_spatials=None, enc_image_mask=None, enc_input_ids=None,
                    enc_segments=None, enc_attention_mask=None, dec_input_ids=None, num_beams=5, length_penalty=1.0,
                    ngram_blocking_size=0, max_seq_len=18, **_):
        """Beam-search decoding of the answer (Engine.beam_search states the rule): the forward's encoder / decoder keywords ->
        (sequences [B, K, max_seq_len] int64, scores [B, K] fp32 = log-probability sum / len ** length_penalty), each row's K
        hypotheses best first.  n-gram blocking is not available with beams."""
        from ._lib import GstvdError
        if int(ngram_blocking_size or 0) > 0:
            raise GstvdError("beam search does not support ngram_blocking_size > 0 (a per-beam history needs the back-pointers); "
                             "use the sampling branch for n-gram blocking")
        return self.engine.beam_search(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                       enc_attention_mask, dec_input_ids, num_beams=int(num_beams),
                                       length_penalty=float(length_penalty), max_seq_len=int(max_seq_len))

    def sample_ranked(self, enc_image_features=None, enc_image_spatials=None, enc_image_mask=None, enc_input_ids=None,
                      enc_segments=None, enc_attention_mask=None, dec_input_ids=None, num_samples=4, length_penalty=1.0,
                      temperature=1.0, top_k=0, top_p=0.0, ngram_blocking_size=0, max_seq_len=18, uniforms=None, **_):
        """Sample-and-rank decoding of the answer (Engine.sample_ranked states the rule): the forward's encoder / decoder keywords
        -> (sequences [B, S, max_seq_len] int64, scores [B, S] fp32 = sum of the drawn tokens' log-probabilities / len **
        length_penalty, token_logp [B, S, max_seq_len] fp32), each row's S = num_samples samples best first."""
        from ._lib import GstvdError
        if _.get("num_beams") is not None and int(_["num_beams"]) > 1:
            raise GstvdError("num_samples and num_beams = %d exclude each other: sample-and-rank draws, beam search does not"
                             % int(_["num_beams"]))
        return self.engine.sample_ranked(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                         enc_attention_mask, dec_input_ids, num_samples=int(num_samples),
                                         length_penalty=float(length_penalty), temperature=temperature, top_k=top_k, top_p=top_p,
                                         ngram_blocking_size=ngram_blocking_size, max_seq_len=int(max_seq_len), uniforms=uniforms)

    def attention_maps(self, enc_image_features=None, enc_image_spatials=None, enc_image_mask=None, enc_image_target=None,
                       enc_image_label=None, enc_next_sentence_labels=None, enc_input_ids=None, enc_segments=None,
                       enc_sep_indices=None, enc_mlm_labels=None, enc_attention_mask=None, dec_input_ids=None,
                       dec_attention_mask=None, dec_labels=None, select=None, heads="all"):
        """The eval-mode teacher-forced forward with its attention maps -> ((loss, logits), maps): (loss, logits) as `forward`
        returns them, maps an attn_maps.ModelAttentionMaps -- maps.encoder as VisualDialogEncoder.attention_maps returns it,
        maps.decoder_self[i] [B, nh, U, U], maps.decoder_cross[i] [B, nh, U, R + T] (regions first), maps.layers.  `select`: None
        (every site) or a dict over "t", "v", "c", "decoder_self", "decoder_cross" -> "all" / iterable of layer indices (a missing
        key: none); `heads`: "all" or "mean".  Needs an 'eval' mode and .eval(); issued eagerly, without autograd."""
        from ._lib import GstvdError
        from . import attn_maps
        from .engine import model_attention_maps
        mode = self.params["mode"]
        if "train" in mode or "eval" not in mode or self.training:
            raise GstvdError("attention_maps(mode=%r, training=%s): %s" % (mode, self.training, attn_maps.ALLOWED))
        return model_attention_maps(self.engine, enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                    enc_attention_mask, dec_input_ids, dec_attention_mask, dec_labels, True, select, heads)

    def soft_labels(self, enc_image_features=None, enc_image_spatials=None, enc_image_mask=None, enc_image_target=None,
                    enc_image_label=None, enc_next_sentence_labels=None, enc_input_ids=None, enc_segments=None,
                    enc_sep_indices=None, enc_mlm_labels=None, enc_attention_mask=None, dec_input_ids=None,
                    dec_attention_mask=None, dec_labels=None, loss_reduction=True, top_k=8):
        """The teacher's side of the soft pseudo-labels: the eval-mode teacher-forced forward of any rows, without gradients ->
        (loss, logits, (ids [B, U, K], logp [B, U, K], labels [B, U])) with (loss, logits) as `forward` returns them and, per
        position, the K = top_k (1..16) most likely tokens (equal logits: the smaller id first) with their fp32 log-probabilities
        and the labels the pass was scored against.  Needs .eval() and a mode without 'train'."""
        from ._lib import GstvdError
        mode = self.params["mode"]
        if "train" in mode or self.training:
            raise GstvdError("soft_labels(mode=%r, training=%s): the teacher runs in eval mode (model.eval(), a mode without 'train')"
                             % (mode, self.training))
        with torch.no_grad():
            return self.engine.step(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                    enc_attention_mask, dec_input_ids, dec_attention_mask, dec_labels, loss_reduction,
                                    soft_top_k=int(top_k))

    def forward(self, enc_image_features=None, enc_image_spatials=None, enc_image_mask=None, enc_image_target=None,
                enc_image_label=None, enc_next_sentence_labels=None, enc_input_ids=None, enc_segments=None,
                enc_sep_indices=None, enc_mlm_labels=None, enc_attention_mask=None, dec_input_ids=None,
                dec_attention_mask=None, dec_labels=None, loss_reduction=True, dec_soft_ids=None, dec_soft_logp=None,
                distill_alpha=0.5, distill_temperature=1.0, **decoding_kwargs):
        """Train / eval modes with `dec_soft_ids` / `dec_soft_logp` [B, U, K] (the teacher's soft labels, `soft_labels` /
        `Engine.rescore_sampled(soft_top_k=K)`; ids < 0 in entry 0: the token has none): the loss is the mean over the kept tokens
        of (1 - a) * ce + a * tau^2 * KL(q || softmax(logits / tau)), a = distill_alpha on tokens with a soft label and 0 elsewhere,
        tau = distill_temperature, q = softmax of the K teacher log-probabilities / tau; differentiable like the plain loss.
        Without them nothing new is launched.
        Generation modes: `num_beams` = K > 1 among the decoding keywords decodes by beam search and returns each row's best
        hypothesis as LongTensor [B, 18] -- type and padding of the sampling branch.  `temperature`, `top_k` and `top_p` are
        accepted and ignored there (beam search ranks raw log-probabilities); `length_penalty` (default 1.0) is honoured;
        `ngram_blocking_size` > 0 with beams raises (a per-beam history needs the back-pointers).  `num_beams` absent or 1: the
        sampling branch, untouched.
        `num_samples` = S > 1 (1..8) among the decoding keywords draws S answers per row under the sampling keywords and returns
        the most likely one (`sample_ranked`, `length_penalty` default 1.0) as LongTensor [B, 18], the sampling branch's type
        and padding; together with `num_beams` > 1 it raises.  `num_samples` absent or 1: the sampling branch, untouched."""
        mode = self.params["mode"]
        if "train" in mode or "eval" in mode:
            soft = None if dec_soft_ids is None and dec_soft_logp is None else (dec_soft_ids, dec_soft_logp, distill_alpha,
                                                                                  distill_temperature)
            return self.engine.step(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                    enc_attention_mask, dec_input_ids, dec_attention_mask, dec_labels, loss_reduction, soft=soft)
        num_beams = decoding_kwargs.get("num_beams")
        num_samples = decoding_kwargs.get("num_samples")
        if num_samples is not None:
            if int(num_samples) != 1:                 # (out of range: Engine.sample_ranked refuses it)
                seqs, _, _ = self.sample_ranked(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                                enc_attention_mask, dec_input_ids, **decoding_kwargs)
                return seqs[:, 0].contiguous()
            decoding_kwargs = {k: v for k, v in decoding_kwargs.items() if k != "num_samples"}
        if num_beams is not None and int(num_beams) > 1:
            kw = dict(num_beams=int(num_beams), ngram_blocking_size=decoding_kwargs.get("ngram_blocking_size", 0))
            for k in ("length_penalty", "max_seq_len"):
                if k in decoding_kwargs:
                    kw[k] = decoding_kwargs[k]
            seqs, _ = self.beam_search(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                       enc_attention_mask, dec_input_ids, **kw)
            return seqs[:, 0].contiguous()
        if num_beams is not None:
            decoding_kwargs = {k: v for k, v in decoding_kwargs.items() if k != "num_beams"}
        return self.engine.sample(enc_image_features, enc_image_spatials, enc_image_mask, enc_input_ids, enc_segments,
                                  enc_attention_mask, dec_input_ids, **decoding_kwargs)
