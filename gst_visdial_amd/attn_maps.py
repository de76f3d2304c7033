"""Attention maps: the softmax probabilities of the attention sites, on request.

The reference collects them in BertEncoder.forward when `output_all_attention_masks=True` (models/vilbert_dialog.py:806-912): a
list per stream -- text self-attention, vision self-attention, and per connection layer the pair (text queries over the regions,
region queries over the tokens; :671-712).  The fused kernels here never store a probability, so a map is a launch of its own
(gstvd_attn_probs, csrc/attn_maps.hip) on the descriptor a site has just run, issued by Engine.attn when the site is selected.

Eval mode only: what dropout leaves of the probabilities in training is not offered.
"""
import collections
import contextlib

import torch

from ._lib import GstvdError

KINDS = ("t", "v", "c", "decoder_self", "decoder_cross")
ENCODER_KINDS = KINDS[:3]

AttentionMaps = collections.namedtuple("AttentionMaps", "t v c layers")
AttentionMaps.__doc__ = """Encoder maps in the reference's order: t[i] [B, nh, T, T], v[i] [B, nhv, R, R], c[i] = (probs1 [B, nhb, T, R],
probs2 [B, nhb, R, T]); fp32 on the device, without the head dimension under heads="mean".  `layers`: kind -> the layer indices
the lists hold, ascending."""

ModelAttentionMaps = collections.namedtuple("ModelAttentionMaps", "encoder decoder_self decoder_cross layers")
ModelAttentionMaps.__doc__ = """`encoder`: an AttentionMaps; decoder_self[i] [B, nh, U, U]; decoder_cross[i] [B, nh, U, R + T], regions
first.  `layers` covers all five kinds."""

ALLOWED = ("attention maps are taken in eval mode only: EncoderDecoderModel.attention_maps(...) under an 'eval' mode after "
           ".eval(), or VisualDialogEncoder.attention_maps(...); a module in training state, a 'train' mode, sample, beam_search, "
           "sample_ranked and score_candidates serve no request (train-mode post-dropout probabilities are not offered)")


def site_of_parameter(key):
    """The attention site whose scores a query / key parameter of the reference's state dict feeds, or None: "t<i>" / "v<i>" (text /
    vision self-attention), "c<i>::0" (connection layer i, text queries over the regions: query2 and key1), "c<i>::1" (region
    queries over the tokens: query1 and key2), "decoder_self<i>", "decoder_cross<i>".  Values, outputs and every other tensor: None."""
    parts = key.split(".")
    if len(parts) < 2 or parts[-2] not in ("query", "key", "query1", "key1", "query2", "key2"):
        return None
    leaf = parts[-2]
    for kind, tag in (("c_layer", "c"), ("v_layer", "v"), ("layer", None)):
        if kind in parts:
            i = int(parts[parts.index(kind) + 1])
            if tag == "c":
                return "c%d::%d" % (i, 0 if leaf in ("query2", "key1") else 1)
            if tag == "v":
                return "v%d" % i
            if "crossattention" in parts:
                return "decoder_cross%d" % i
            return ("decoder_self%d" if "decoder" in parts[:parts.index(kind)] else "t%d") % i
    return None


def layer_counts(enc_cfg, dec_cfg=None):
    """kind -> number of sites of that kind in a model of these configs."""
    n = dict(t=enc_cfg.num_hidden_layers, v=enc_cfg.v_num_hidden_layers, c=len(enc_cfg.v_biattention_id))
    n["decoder_self"] = n["decoder_cross"] = dec_cfg.num_hidden_layers if dec_cfg is not None else 0
    return n


def parse_select(select, counts, kinds=KINDS):
    """`select` of attention_maps -> {kind: ascending list of layer indices} over `kinds`.  None: every site.  Otherwise a dict
    with keys among `kinds`; a value is "all" or an iterable of layer indices (a missing key: none).  An unknown key, an index
    outside 0 .. count - 1, a repeated index or anything that is no integer raises GstvdError."""
    if select is None:
        return {k: list(range(counts[k])) for k in kinds}
    if not isinstance(select, dict):
        raise GstvdError("select must be None or a dict with keys among %s, got %r" % (", ".join(kinds), type(select).__name__))
    out = {k: [] for k in kinds}
    for k, v in select.items():
        if k not in kinds:
            raise GstvdError("select: unknown key %r (this call takes %s)" % (k, ", ".join(kinds)))
        if isinstance(v, str):
            if v != "all":
                raise GstvdError("select[%r]: %r is neither \"all\" nor an iterable of layer indices" % (k, v))
            out[k] = list(range(counts[k]))
            continue
        try:
            idx = list(v)
        except TypeError:
            raise GstvdError("select[%r]: %r is neither \"all\" nor an iterable of layer indices" % (k, v))
        for i in idx:
            if isinstance(i, bool) or not isinstance(i, int):
                raise GstvdError("select[%r]: layer index %r is not an integer" % (k, i))
            if not 0 <= i < counts[k]:
                raise GstvdError("select[%r]: layer index %d outside 0..%d" % (k, i, counts[k] - 1))
        if len(set(idx)) != len(idx):
            raise GstvdError("select[%r]: a layer index is given twice" % (k,))
        out[k] = sorted(idx)
    return out


def parse_heads(heads):
    if heads not in ("all", "mean"):
        raise GstvdError("heads must be \"all\" or \"mean\", got %r" % (heads,))
    return heads == "mean"


class MapRequest(object):
    """What an engine call is to capture: the selected layers per kind, the head mode, and -- after alloc() -- the output tensor
    of every selected site by its engine label."""

    def __init__(self, layers, head_mean):
        self.layers, self.head_mean, self.out = layers, bool(head_mean), {}

    def alloc(self, enc_cfg, dec_cfg, Bn, T, R, U, device):
        """The outputs, from torch's allocator (not the engine's arena, which the next call rewinds), before the forward."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise GstvdError("gst_visdial_amd runs on MI355X only; tensors are on %s (no CPU path)" % dev)
        c = enc_cfg

        def new(label, nh, Lq, Lk):
            shape = (Bn, Lq, Lk) if self.head_mean else (Bn, nh, Lq, Lk)
            self.out[label] = torch.empty(shape, dtype=torch.float32, device=dev)
        for i in self.layers.get("t", ()):
            new("t%d.attn" % i, c.num_attention_heads, T, T)
        for i in self.layers.get("v", ()):
            new("v%d.attn" % i, c.v_num_attention_heads, R, R)
        for i in self.layers.get("c", ()):
            new("c%d.attn1" % i, c.bi_num_attention_heads, T, R)      # text queries over the regions (probs1)
            new("c%d.attn2" % i, c.bi_num_attention_heads, R, T)      # region queries over the tokens (probs2)
        for i in self.layers.get("decoder_self", ()):
            new("d%d.attn" % i, dec_cfg.num_attention_heads, U, U)
        for i in self.layers.get("decoder_cross", ()):
            new("d%d.xattn" % i, dec_cfg.num_attention_heads, U, R + T)
        self.pending = set(self.out)
        return self

    def encoder_maps(self):
        L, o = self.layers, self.out
        return AttentionMaps([o["t%d.attn" % i] for i in L["t"]], [o["v%d.attn" % i] for i in L["v"]],
                             [(o["c%d.attn1" % i], o["c%d.attn2" % i]) for i in L["c"]],
                             {k: list(L[k]) for k in ENCODER_KINDS})

    def model_maps(self):
        L, o = self.layers, self.out
        return ModelAttentionMaps(self.encoder_maps(), [o["d%d.attn" % i] for i in L["decoder_self"]],
                                  [o["d%d.xattn" % i] for i in L["decoder_cross"]], {k: list(L[k]) for k in KINDS})

    def check_complete(self):
        if self.pending:
            raise GstvdError("internal: attention sites selected but never reached: %s" % ", ".join(sorted(self.pending)))


@contextlib.contextmanager
def capture(engine, req):
    """The engine serves `req` for the calls made inside."""
    if engine._maps is not None:
        raise GstvdError("an attention-map request is already being served by this engine")
    engine._maps = req
    try:
        yield req
    finally:
        engine._maps = None
