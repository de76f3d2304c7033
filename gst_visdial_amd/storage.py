"""Storage of the engine: where parameters, gradients and activations live on the device.

  * parameters live in ONE flat fp32 buffer `P` (forward order), gradients in one flat fp32 buffer `G`,
    bf16 shadow weights (throughput mode) in one flat bf16 buffer `S`; the nn.Parameters are views.
    Q/K/V (and the co-attention / cross-attention K,V of all decoder layers) are laid out contiguously
    so each projection group is ONE GEMM, and a data-parallel all-reduce is a handful of large slices;
  * activations come from a bump arena that is rewound every step -> static addresses (hipGraph friendly),
    no allocator traffic; nothing of size [Lq, Lk] is ever stored (attention saves only LSE).

Pure layout code: no kernel schedule in here (that is engine.py).
"""
import torch

from . import ops
from .config import encoder_schedule
from ._lib import GstvdError


def _round_up(x, m):
    return (x + m - 1) // m * m


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


class Act(object):
    """An activation [M, N] in the arena plus (during backward) its gradient."""
    __slots__ = ("t", "g", "M", "N", "gelu_aux", "bias_done", "prod", "dgrad_done", "req")

    def __init__(self, t, M, N):
        self.t, self.g, self.M, self.N = t, None, M, N
        self.gelu_aux, self.bias_done = None, False
        self.prod, self.dgrad_done = None, False      # the Linear that produced it (input, weight, K_in, need_dx); see _ln_bwd
        # False: the activation does not depend on the image features (it comes from token ids and parameters alone), so the
        # inputs-only replay (Engine.inputs_only) needs no gradient for it.  Forward ops pass it on like autograd's requires_grad.
        self.req = True


class Arena(object):
    """Bump allocator over large device chunks; `reset()` rewinds, so a fixed call sequence gets fixed addresses
    (hipGraph friendly).  The request sequence of a step is identical from step to step, so the tensor views are
    memoised by sequence index: steady-state allocation is a list lookup, no tensor construction."""

    _ESZ = {torch.float32: 4, torch.bfloat16: 2, torch.int64: 8, torch.uint8: 1, torch.int32: 4}

    def __init__(self, device, chunk_bytes=1 << 28):
        self.device, self.chunk_bytes = device, chunk_bytes
        self.chunks, self.ci, self.off = [], 0, 0
        self.memo, self.seq = [], 0

    def reset(self):
        self.ci, self.off, self.seq = 0, 0, 0

    def rewind(self, mark):
        """Back to a position returned by `mark()` (decode loops reuse the same scratch every step)."""
        self.ci, self.off, self.seq = mark

    def mark(self):
        return (self.ci, self.off, self.seq)

    def alloc(self, numel, dtype, shape=None):
        nbytes = _round_up(numel * self._ESZ[dtype], 256)
        i = self.seq
        self.seq = i + 1
        if i < len(self.memo):
            m = self.memo[i]
            if m[0] == numel and m[1] is dtype and m[2] == shape and m[3] == self.ci and m[4] == self.off:
                self.ci, self.off = m[5], m[6]
                return m[7]
            del self.memo[i:]                 # the sequence diverged (different shapes): rebuild from here
        ci0, off0 = self.ci, self.off
        while True:
            if self.ci >= len(self.chunks):
                self.chunks.append(torch.empty(max(self.chunk_bytes, nbytes), dtype=torch.uint8, device=self.device))
            c = self.chunks[self.ci]
            if self.off + nbytes <= c.numel():
                out = c[self.off:self.off + nbytes].view(dtype)[:numel]
                if shape is not None:
                    out = out.view(shape)
                self.off += nbytes
                self.memo.append((numel, dtype, shape, ci0, off0, self.ci, self.off, out))
                return out
            self.ci, self.off = self.ci + 1, 0


class FlatParams(object):
    """Flat storage plan.  `slots[name] = (offset, shape)` are engine views (possibly fused groups of several
    nn.Parameters); every live nn.Parameter becomes a view of `P` and its `.grad` a view of `G`."""

    def __init__(self, model, precision):
        # `model`: an EncoderDecoderModel, or (encoder-only form) a VisualDialogEncoder of the discriminative enc_only arch
        self.enc_only = not hasattr(model, "decoder")
        encoder = model if self.enc_only else model.encoder
        enc_cfg = encoder.config
        bert = encoder.bert_pretrained.bert
        self.slots, self.items, self.pads = {}, [], []
        self.placed = {}
        self.off = 0
        H, Hv, Hb = enc_cfg.hidden_size, enc_cfg.v_hidden_size, enc_cfg.bi_hidden_size
        if self.enc_only:
            # no decoder slots; the MLM head of train_disc.py is tied to the word table (models/vilbert_dialog.py:991) the way the
            # enc_dec LM head is after train_gen.py:293, so the table gets the same row padding the head's GEMM needs
            dec_cfg = gen = None
            self.Vp = _round_up(enc_cfg.vocab_size, 64)
            lm_w = encoder.bert_pretrained.cls.predictions.decoder.weight
        else:
            dec_cfg = model.decoder.config
            gen = model.decoder.decoder
            V = dec_cfg.vocab_size
            self.Vp = _round_up(V, 64)
            lm_w = gen.lm_head.decoder.weight

        def place(name, params, shape=None, pad_rows_to=None):
            """Lay `params` out back to back under one fused slot `name`."""
            self.off = _round_up(self.off, 64)
            start = self.off
            for p in params:
                if id(p) in self.placed:
                    raise GstvdError("parameter shared between two fused groups: " + name)
                self.placed[id(p)] = self.off
                self.items.append((p, self.off))
                self.off += p.numel()
            if pad_rows_to is not None:
                cols = params[0].shape[1] if params[0].dim() == 2 else 1
                want = pad_rows_to * cols
                self.pads.append((self.off, start + want))
                self.off = start + want
            n = self.off - start
            if shape is None:
                shape = tuple(params[0].shape) if len(params) == 1 and pad_rows_to is None else (n,)
            self.slots[name] = (start, shape)

        def emb(prefix, mod):
            w = mod.word_embeddings.weight
            place(prefix + ".word", [w], shape=(self.Vp if w is lm_w else w.shape[0], w.shape[1]),
                  pad_rows_to=self.Vp if w is lm_w else None)
            place(prefix + ".pos", [mod.position_embeddings.weight])
            place(prefix + ".tt", [mod.token_type_embeddings.weight])
            place(prefix + ".tte", [mod.token_type_embeddings_extension.weight])
            place(prefix + ".ln.w", [mod.LayerNorm.weight])
            place(prefix + ".ln.b", [mod.LayerNorm.bias])

        def attn_out(p, lay):
            place(p + ".ao.w", [lay.attention.output.dense.weight]); place(p + ".ao.b", [lay.attention.output.dense.bias])
            place(p + ".ln1.w", [lay.attention.output.LayerNorm.weight]); place(p + ".ln1.b", [lay.attention.output.LayerNorm.bias])

        def ffn(p, inter_mod, out_mod, tag_i, tag_o, tag_ln):
            place(p + tag_i + ".w", [inter_mod.dense.weight]); place(p + tag_i + ".b", [inter_mod.dense.bias])
            place(p + tag_o + ".w", [out_mod.dense.weight]); place(p + tag_o + ".b", [out_mod.dense.bias])
            place(p + tag_ln + ".w", [out_mod.LayerNorm.weight]); place(p + tag_ln + ".b", [out_mod.LayerNorm.bias])

        def qkv(p, tag, q, k, v, hid_out, hid_in):
            place(p + tag + ".w", [q.weight, k.weight, v.weight], shape=(3 * hid_out, hid_in))
            place(p + tag + ".b", [q.bias, k.bias, v.bias], shape=(3 * hid_out,))

        def bert_layer(p, lay, hid):
            s = lay.attention.self
            qkv(p, ".qkv", s.query, s.key, s.value, hid, hid)
            attn_out(p, lay)
            ffn(p, lay.intermediate, lay.output, ".fi", ".fo", ".ln2")

        self.enc_emb = bert.embeddings
        self.dec_emb = None if self.enc_only else gen.bert.embeddings
        emb("emb", self.enc_emb)
        ve = bert.v_embeddings
        place("vemb.img.w", [ve.image_embeddings.weight]); place("vemb.img.b", [ve.image_embeddings.bias])
        place("vemb.loc.w", [ve.image_location_embeddings.weight]); place("vemb.loc.b", [ve.image_location_embeddings.bias])
        place("vemb.ln.w", [ve.LayerNorm.weight]); place("vemb.ln.b", [ve.LayerNorm.bias])
        self.marks = {}
        for kind, i in encoder_schedule(enc_cfg):
            self.marks[(kind, i)] = _round_up(self.off, 64)
            if kind == "t":
                bert_layer("t%d" % i, bert.encoder.layer[i], H)
            elif kind == "v":
                bert_layer("v%d" % i, bert.encoder.v_layer[i], Hv)
            else:
                c, p = bert.encoder.c_layer[i], "c%d" % i
                b = c.biattention
                qkv(p, ".qkv1", b.query1, b.key1, b.value1, Hb, Hv)
                qkv(p, ".qkv2", b.query2, b.key2, b.value2, Hb, H)
                o = c.biOutput
                place(p + ".d1.w", [o.dense1.weight]); place(p + ".d1.b", [o.dense1.bias])
                place(p + ".ln1.w", [o.LayerNorm1.weight]); place(p + ".ln1.b", [o.LayerNorm1.bias])
                place(p + ".d2.w", [o.dense2.weight]); place(p + ".d2.b", [o.dense2.bias])
                place(p + ".ln2.w", [o.LayerNorm2.weight]); place(p + ".ln2.b", [o.LayerNorm2.bias])
                ffn(p, c.v_intermediate, c.v_output, ".vfi", ".vfo", ".vln")
                ffn(p, c.t_intermediate, c.t_output, ".tfi", ".tfo", ".tln")
        if self.enc_only:
            # the three heads of BertPreTrainingHeads (models/vilbert_dialog.py:915-1055) are live here: NSP for ranking and
            # training, cls.predictions.* / cls.imagePredictions.* for training (Engine.disc_step); sep_embeddings and q_dense*
            # stay in the dead buffer, as in the enc_dec form
            cls = encoder.bert_pretrained.cls
            self.marks["nsp"] = _round_up(self.off, 64)
            place("pool.t.w", [bert.t_pooler.dense.weight]); place("pool.t.b", [bert.t_pooler.dense.bias])
            place("pool.v.w", [bert.v_pooler.dense.weight]); place("pool.v.b", [bert.v_pooler.dense.bias])
            place("nsp.w", [cls.bi_seq_relationship.weight]); place("nsp.b", [cls.bi_seq_relationship.bias])
            self.marks["mlm"] = _round_up(self.off, 64)
            tr = cls.predictions.transform
            place("mlm.tr.w", [tr.dense.weight]); place("mlm.tr.b", [tr.dense.bias])
            place("mlm.ln.w", [tr.LayerNorm.weight]); place("mlm.ln.b", [tr.LayerNorm.bias])
            if id(lm_w) in self.placed:
                self.slots["mlm.dec.w"] = self.slots["emb.word"]         # the tied decoder: an alias, one gradient slot
            else:
                place("mlm.dec.w", [lm_w], shape=(self.Vp, lm_w.shape[1]), pad_rows_to=self.Vp)
            place("mlm.b", [cls.predictions.bias], shape=(self.Vp,), pad_rows_to=self.Vp)
            self.marks["imgp"] = _round_up(self.off, 64)
            ip = cls.imagePredictions
            self.Cp = _round_up(ip.decoder.weight.shape[0], 64)
            place("imgp.tr.w", [ip.transform.dense.weight]); place("imgp.tr.b", [ip.transform.dense.bias])
            place("imgp.ln.w", [ip.transform.LayerNorm.weight]); place("imgp.ln.b", [ip.transform.LayerNorm.bias])
            place("imgp.dec.w", [ip.decoder.weight], shape=(self.Cp, Hv), pad_rows_to=self.Cp)
            place("imgp.dec.b", [ip.decoder.bias], shape=(self.Cp,), pad_rows_to=self.Cp)
            self._finish(model, precision)
            return
        self.marks["vlf"] = _round_up(self.off, 64)
        place("vlf.v.w", [model.vlfusion.fc_v.weight]); place("vlf.v.b", [model.vlfusion.fc_v.bias])
        place("vlf.l.w", [model.vlfusion.fc_l.weight]); place("vlf.l.b", [model.vlfusion.fc_l.bias])
        self.marks["dec"] = _round_up(self.off, 64)
        if self.dec_emb is not self.enc_emb:
            emb("demb", self.dec_emb)
        layers = gen.bert.encoder.layer
        Hd, L = dec_cfg.hidden_size, len(layers)
        kvw, kvb = [], []
        for lay in layers:
            cs = lay.crossattention.self
            kvw += [cs.key.weight, cs.value.weight]
            kvb += [cs.key.bias, cs.value.bias]
        place("dec.ckv.w", kvw, shape=(2 * L * Hd, Hd))
        place("dec.ckv.b", kvb, shape=(2 * L * Hd,))
        for i, lay in enumerate(layers):
            p = "d%d" % i
            self.marks[("d", i)] = _round_up(self.off, 64)
            s = lay.attention.self
            qkv(p, ".qkv", s.query, s.key, s.value, Hd, Hd)
            attn_out(p, lay)
            c = lay.crossattention
            place(p + ".cq.w", [c.self.query.weight]); place(p + ".cq.b", [c.self.query.bias])
            place(p + ".co.w", [c.output.dense.weight]); place(p + ".co.b", [c.output.dense.bias])
            place(p + ".ln2.w", [c.output.LayerNorm.weight]); place(p + ".ln2.b", [c.output.LayerNorm.bias])
            ffn(p, lay.intermediate, lay.output, ".fi", ".fo", ".ln3")
        self.marks["lm"] = _round_up(self.off, 64)
        if id(lm_w) in self.placed:
            wname = "emb.word" if lm_w is self.enc_emb.word_embeddings.weight else "demb.word"
            self.slots["lm.w"] = self.slots[wname]
        else:
            place("lm.w", [lm_w], shape=(self.Vp, lm_w.shape[1]), pad_rows_to=self.Vp)
        place("lm.b", [gen.lm_head.bias], shape=(self.Vp,), pad_rows_to=self.Vp)
        self._finish(model, precision)

    def _finish(self, model, precision):
        self.n_live = _round_up(self.off, 64)
        self.live = [p for p, _ in self.items]
        live_ids = set(id(p) for p in self.live)
        self.dead = [p for p in model.parameters() if id(p) not in live_ids]
        self.precision = precision
        self.P = self.G = self.S = self.D = None
        self.stale_guard = None       # callable -> True while fp32 masters of other ranks' shards are old (set by the engine)

    # -- materialise on the device the parameters currently live on ------------------------------------
    def materialize(self, device):
        P = torch.zeros(self.n_live, dtype=torch.float32, device=device)
        for p, off in self.items:
            P[off:off + p.numel()].copy_(p.data.reshape(-1))
        nd = sum(p.numel() for p in self.dead)
        D = torch.empty(max(nd, 1), dtype=torch.float32, device=device)
        o = 0
        for p in self.dead:
            D[o:o + p.numel()].copy_(p.data.reshape(-1))
            p.data = D[o:o + p.numel()].view(p.shape)
            o += p.numel()
        for p, off in self.items:
            p.data = P[off:off + p.numel()].view(p.shape)
        self.P, self.D = P, D
        # (encoder-only form: no gradient buffer, no gradient views until the first training call -- `ensure_grads`)
        self.G, self.grad_views = None, []
        if not self.enc_only:
            self.ensure_grads()
        self.S = torch.empty(self.n_live, dtype=torch.bfloat16, device=device) if self.precision == "bf16" else None
        self.ptrs = [(p, P[off:off + p.numel()].data_ptr()) for p, off in self.items]
        self.shadow_version = None
        self.device = device

    def ensure_grads(self):
        """The flat gradient buffer and the per-parameter views of it; -> True when this call made them."""
        if self.G is not None:
            return False
        self.G = torch.zeros(self.n_live, dtype=torch.float32, device=self.P.device)
        self.grad_views = [self.G[off:off + p.numel()].view(p.shape) for p, off in self.items]
        return True

    def is_materialized(self):
        if self.P is None:
            return False
        for p, ptr in self.ptrs:
            if p.data_ptr() != ptr:
                return False
        return True

    def version(self):
        return sum(p._version for p in self.live)

    def refresh_shadow(self, force=False):
        if self.S is None:
            return
        v = self.version()
        if force or v != self.shadow_version:
            if self.shadow_version is not None and self.stale_guard is not None and self.stale_guard():
                # sharded optimizer (pipeline.BackwardPipeline(shard_update=True)): P holds current master weights only for this
                # rank's shards, S holds the freshly GATHERED shadows of all of them -- a re-cast would replace other ranks' current
                # bf16 weights by this rank's old masters and the ranks would diverge silently
                raise GstvdError("a parameter was modified in place while the optimizer is sharded over the ranks: the bf16 shadow "
                                 "weights cannot be re-derived from this rank's fp32 masters (current only for its own shards).  "
                                 "Call pipe.sync_master() on EVERY rank before editing parameters.")
            ops.cast(self.P, self.S)
            self.shadow_version = v

    def fp32_read_ranges(self):
        """Sorted, disjoint flat ranges [x, y) whose fp32 values the forward reads directly (Engine.Pv: biases, LayerNorm gain /
        bias, the embedding tables, the image-location projection) -- everything in [0, n_live) that is not EXCLUSIVELY a GEMM
        weight (Engine.W: read from the bf16 shadow buffer in bf16 mode).  pipeline.BackwardPipeline(shard_update=True) gathers
        these in fp32; the GEMM weights only travel as bf16 shadows."""
        non_gemm = ("ln.w", "ln1.w", "ln2.w", "ln3.w", "vln.w", "tln.w", "vemb.loc.w", "nsp.w")
        by_start = {}
        for name, (off, shape) in self.slots.items():
            gemm = name.endswith(".w") and not name.endswith(non_gemm)
            by_start.setdefault((off, _numel(shape)), []).append(gemm)
        shadow_only = sorted(k for k, flags in by_start.items() if all(flags))      # (the tied LM head aliases an embedding table: not all)
        out, pos = [], 0
        for off, n in shadow_only:
            if off > pos:
                out.append((pos, off))
            pos = max(pos, off + n)
        if pos < self.n_live:
            out.append((pos, self.n_live))
        return out

    def view(self, buf, name):
        off, shape = self.slots[name]
        return buf[off:off + _numel(shape)].view(shape)
