"""Discriminative (enc_only) heads of the engine: the training step with the MLM, masked-region and NSP losses
(models/vilbert_dialog.py:1482-1514, train_disc.py) and the NSP ranking scores (evaluate_disc.py:79-83).  `DiscMixin` is the
discriminative half of `engine.Engine`; it uses the engine's op helpers, its encoder schedule and its tape replay.  Nothing on the
enc_dec path calls into this file."""
import torch

from . import ops
from ._lib import GstvdError


class DiscMixin(object):
    # ------------------------------------------------------------------------------------------ discriminative training
    def _scatter_grad(self, src, idx, x):
        """Rows idx of the gradient of activation `x` (+)= src (gstvd_rows_scatter).  The first writer zero-fills the rest."""
        first = x.g is None
        if first:
            x.g = self.buf(x.M, x.N)
        ops.rows_scatter(src, idx, x.g, accumulate=not first, M=x.M)

    def _gathered(self, x, idx, n):
        """Rows idx of activation `x` as a dense [n, N] activation; backward scatters its gradient into x's."""
        h = self.act(n, x.N)
        ops.rows_gather(x.t, idx, h.t, M=x.M)
        self.push(lambda: self._scatter_grad(h.g, idx, x))
        return h

    def _head_transform(self, h, p, H):
        """BertPredictionHeadTransform / BertImgPredictionHeadTransform (models/vilbert_dialog.py:943-977): Linear, erf-GELU,
        LayerNorm(1e-12).  The LayerNorm follows the GELU directly, so its backward yields d(GELU output): one multiply by the
        saved gelu' turns it into the d(pre-activation) that _lin_bwd expects."""
        a = self.lin(h, p + ".tr.w", p + ".tr.b", H, H, gelu=True)
        self.push(lambda: ops.rows_mul_(a.g, a.gelu_aux, a.M, H))       # backward: after the LayerNorm's, before the Linear's
        return self.ln(a, None, p + ".ln.w", p + ".ln.b", H, 0.0, None, 1e-12)

    def _mlm_head(self, xt, rows, labels):
        """cls.predictions on the `rows` (flat indices of the tokens with a label != -1) -> mean cross entropy (a view of the
        step's stats).  The decoder is the word table (tied) plus cls.predictions.bias."""
        c, n = self.enc_cfg, rows.numel()
        h = self._gathered(xt, rows, n)
        y = self._head_transform(h, "mlm", c.hidden_size)
        logits = self.lin(y, "mlm.dec.w", "mlm.b", self.flat.Vp, c.hidden_size)
        row_loss, lse, stats = self.vec(n), self.vec(n), self.vec(4)
        ops.ce_fwd(logits.t, labels, n, c.vocab_size, row_loss, lse, stats, ignore_index=-1)

        def seed():
            logits.g = self.buf(n, self.flat.Vp)
            ops.ce_bwd(logits.t, labels, lse, stats, self._seeds[0], True, n, c.vocab_size, logits.g, ignore_index=-1)
        self.push(seed)
        return stats[2:3]

    def _region_head(self, xv, rows, target):
        """cls.imagePredictions on the `rows` (flat indices of the regions with image_label == 1) -> the masked KL loss."""
        c, n = self.enc_cfg, rows.numel()
        C, Cp = c.v_target_size, self.flat.Cp
        h = self._gathered(xv, rows, n)
        y = self._head_transform(h, "imgp", c.v_hidden_size)
        scores = self.lin(y, "imgp.dec.w", "imgp.dec.b", Cp, c.v_hidden_size)
        row_loss, lse, stats = self.vec(n), self.vec(n), self.vec(4)
        ops.kl_fwd(scores.t, target, n, C, row_loss, lse, stats, target_row=rows)

        def seed():
            scores.g = self.buf(n, Cp)
            ops.kl_bwd(scores.t, target, lse, stats, self._seeds[1], True, n, C, scores.g, target_row=rows)
        self.push(seed)
        return stats[2:3]

    def _no_head(self, prefix):
        """A head without a single masked row: its loss is the reference's 0 / 0, nothing is launched for it, and backward leaves
        zeros in the gradient slots only it writes (the tied MLM decoder's slot belongs to the word table)."""
        def zero():
            word = self.flat.slots["emb.word"][0]
            for name, (off, _) in self.flat.slots.items():
                if name.startswith(prefix) and off != word:
                    g, acc = self.grad_slot(name)
                    if not acc:
                        g.zero_()
        self.push(zero)
        return torch.full((1,), float("nan"), dtype=torch.float32, device=self.flat.device)

    def _first_rows(self, Bn, L, dev):
        """Flat index of the first token / region of every batch row (cached: the same few shapes every step)."""
        key = (Bn, L, dev)
        if key not in self._first_idx:
            self._first_idx[key] = torch.arange(Bn, device=dev) * L
        return self._first_idx[key]

    def _nsp_train_head(self, xt, xv, I, labels, record):
        """Poolers, fusion, Dropout(0.1), cls.bi_seq_relationship and the soft-label loss in one launch (gstvd_nsp_train_fwd);
        backward: one launch down to the gradients in front of the two ReLUs, then the engine's own Linear backward."""
        c, Bn, dev = self.enc_cfg, I["B"], xt.t.device
        H, Hv, Hb = c.hidden_size, c.v_hidden_size, c.bi_hidden_size
        z = torch.empty(Bn, 2, dtype=torch.float32, device=dev)        # handed to the caller: not in the arena
        pt, pv = self.buf(Bn, Hb, torch.float32), self.buf(Bn, Hb, torch.float32)
        keep = self.arena.alloc(Bn * Hb, torch.uint8, (Bn, Hb))
        row_loss, stats = self.vec(Bn), self.vec(4)
        p = 0.1 if self.train else 0.0
        d = ops.nsp_train_desc(xt.t, I["T"], xv.t, I["R"], self.W["pool.t.w"], self.Pv["pool.t.b"], self.W["pool.v.w"],
                               self.Pv["pool.v.b"], self.Pv["nsp.w"], self.Pv["nsp.b"], labels, Bn, c.fusion_method, z, pt, pv, keep,
                               row_loss, stats, p=p, site=self.site("nsp.drop", 0.1, "rows", (Bn, Hb)), rng=self.rng)
        ops.nsp_train_fwd(d)
        if record:
            # the first token / region of every batch row, dense: the B operand of the two pooler weight gradients
            x0t = self._gathered(xt, self._first_rows(Bn, I["T"], dev), Bn)
            x0v = self._gathered(xv, self._first_rows(Bn, I["R"], dev), Bn)

            def bwd():
                dpt, dpv = self.act(Bn, Hb), self.act(Bn, Hb)
                dpt.g, dpv.g = dpt.t, dpv.t
                gw, aw = self.grad_slot("nsp.w")
                gb, ab = self.grad_slot("nsp.b")
                ops.nsp_train_bwd(d, self._seeds[2], gw, gb, dpt.g, dpv.g, aw, ab)
                self._lin_bwd(x0t, dpt, "pool.t.w", "pool.t.b", Hb, H, True)
                self._lin_bwd(x0v, dpv, "pool.v.w", "pool.v.b", Hb, Hv, True)
            self.push(bwd)
        return z, stats[2:3]

    def disc_step(self, feats, loc, img_mask, ids, segs, att_mask, mlm_labels, nsp_labels, img_label, img_target,
                  token_rows=None, region_rows=None, compact=True):
        """The train branch of the enc_only arch (models/vilbert_dialog.py:1482-1514): the two-stream encoder, then the MLM,
        masked-region and NSP heads with their losses -> (lm_loss [1], img_loss [1], nsp_loss [1], seq_relationship_score [B, 2]),
        the losses unscaled and differentiable (one autograd function; backward replays the tape as Engine.backward does).

        The MLM and region heads run on the masked rows only: `token_rows` / `region_rows` are the flat indices (int64, on the
        device, ascending) of the tokens with masked_lm_labels != -1 and of the regions with image_label == 1.  A caller that
        has the labels on the host passes them (no device sync); None: they are taken from the device labels with `nonzero`,
        one sync each.  No masked token / region: that loss is NaN (the reference's 0 / 0), nothing is launched for the head
        and its parameters get zero gradient.  `compact` False (measurements only): the MLM head runs on all B * T rows."""
        if not self.enc_only:
            raise GstvdError("disc_step belongs to the encoder-only engine of an enc_only VisualDialogEncoder")
        record = torch.is_grad_enabled()
        dev = ids.device
        self._begin(dev, record)
        if record and self.flat.ensure_grads():
            self._bind_views()
        dummy = ids.new_zeros(ids.shape[0], 1)
        I = self._inputs(feats, loc, img_mask, ids, segs, att_mask, dummy, None)
        Bn, T, R = I["B"], I["T"], I["R"]
        lab = mlm_labels.reshape(-1).to(dev, torch.int64).contiguous()
        if not compact:
            token_rows = torch.arange(Bn * T, device=dev) if bool((lab != -1).any()) else lab.new_zeros(0)
        elif token_rows is None:
            token_rows = (lab != -1).nonzero().view(-1)
        if region_rows is None:
            region_rows = (img_label.reshape(-1).to(dev) == 1).nonzero().view(-1)
        token_rows, region_rows = token_rows.to(dev, torch.int64).contiguous(), region_rows.to(dev, torch.int64).contiguous()
        target = img_target.reshape(Bn * R, -1).to(dev, torch.float32).contiguous()
        if target.shape[1] != self.enc_cfg.v_target_size:
            raise GstvdError("image_target has %d classes, the config's v_target_size is %d" % (target.shape[1], self.enc_cfg.v_target_size))
        nsp_lab = nsp_labels.reshape(Bn, 2).to(dev, torch.float32).contiguous()
        xt, xv = self.encoder(I)
        prev_scope, ops.Profiler.scope = ops.Profiler.scope, "heads"
        try:
            ops.Profiler.scope = "head.mlm"
            lm = self._mlm_head(xt, token_rows, lab[token_rows] if compact else lab) if token_rows.numel() else self._no_head("mlm.")
            ops.Profiler.scope = "head.img"
            img = self._region_head(xv, region_rows, target) if region_rows.numel() else self._no_head("imgp.")
            ops.Profiler.scope = "head.nsp"
            z, nsp = self._nsp_train_head(xt, xv, I, nsp_lab, record)
        finally:
            ops.Profiler.scope = prev_scope
        self.last = dict(enc_t=xt, enc_v=xv, token_rows=token_rows, region_rows=region_rows)
        if record:
            st = dict(I=I, tape=self.tape)
            lm, img, nsp = _DiscFn.apply(self.anchor, feats if I["feats_grad"] else None, self, st, lm, img, nsp)
            return lm, img, nsp, z
        return lm.clone(), img.clone(), nsp.clone(), z

    def disc_backward(self, st, seeds):
        """Backward of disc_step: `seeds` = the three upstream gradients (lm, img, nsp; [1] fp32 on the device) the heads start
        from; then the shared replay."""
        self._backward_begin()
        self._seeds = seeds
        try:
            return self._replay(st)
        finally:
            self._seeds = None

    # ------------------------------------------------------------------------------------------ discriminative ranking
    @torch.no_grad()
    def nsp_scores(self, feats, loc, img_mask, ids, segs, att_mask):
        """The eval branch of the enc_only arch (models/visual_dialog_encoder.py:68-74, vilbert_dialog.py:1400-1401,1482,1519):
        the two-stream encoder, then ONE launch (gstvd_nsp_head) for first-token gather, both poolers, the fusion, cls.
        bi_seq_relationship and the 2-way softmax.  -> (seq_relationship_score z [B, 2] fp32, prob0 [B] fp32 =
        softmax(z, 1)[:, 0], what evaluate_disc.py:81-83 ranks by).  The MLM / image prediction heads over all B*T tokens,
        whose outputs the reference's only caller discards (evaluate_disc.py:79), are not computed."""
        if not self.enc_only:
            raise GstvdError("nsp_scores belongs to the encoder-only engine of an enc_only VisualDialogEncoder")
        self._begin(ids.device, False, inference=True)
        dummy = ids.new_zeros(ids.shape[0], 1)
        I = self._inputs(feats, loc, img_mask, ids, segs, att_mask, dummy, None)
        xt, xv = self.encoder(I)
        Bn = I["B"]
        z = torch.empty(Bn, 2, dtype=torch.float32, device=ids.device)
        prob0 = torch.empty(Bn, dtype=torch.float32, device=ids.device)
        ops.nsp_head(xt.t, I["T"], xv.t, I["R"], self.W["pool.t.w"], self.Pv["pool.t.b"], self.W["pool.v.w"], self.Pv["pool.v.b"],
                     self.Pv["nsp.w"], self.Pv["nsp.b"], Bn, self.enc_cfg.fusion_method, z, prob0)
        self.last = dict(enc_t=xt, enc_v=xv)
        return z, prob0

    # ------------------------------------------------------------------------------------------ masked-LM fill-in
    @torch.no_grad()
    def mlm_argmax(self, feats, loc, img_mask, ids, segs, att_mask, rows):
        """Inference form of the MLM head (cls.predictions, models/vilbert_dialog.py:980-1003) at the flat token indices `rows`
        (int64 [n], into ids.view(-1)): the encoder, the gather of those rows, the head transform, then the arg-max over the
        vocabulary of the tied decoder's logits -> (idx [n] int64, val [n] fp32), equal logits to the smaller token id.  No tape,
        no dropout.  bf16 engine: the product and the arg-max are one kernel pair (gstvd_vocab_argmax), the [n, vocab] logits
        never exist; fp32 engine (or a width that kernel does not tile): the GEMM into [n, Vp] fp32 and gstvd_rows_argmax.
        n == 0: the encoder does not run either, two empty tensors come back."""
        if not self.enc_only:
            raise GstvdError("mlm_argmax belongs to the encoder-only engine of an enc_only VisualDialogEncoder")
        dev = ids.device
        rows = rows.to(dev, torch.int64).contiguous().view(-1)
        n = rows.numel()
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
        self._begin(dev, False, inference=True)
        dummy = ids.new_zeros(ids.shape[0], 1)
        I = self._inputs(feats, loc, img_mask, ids, segs, att_mask, dummy, None)
        xt, xv = self.encoder(I)
        c = self.enc_cfg
        prev_scope, ops.Profiler.scope = ops.Profiler.scope, "head.mlm"
        try:
            y = self._head_transform(self._gathered(xt, rows, n), "mlm", c.hidden_size)
            w, b, V = self.W["mlm.dec.w"], self.Pv["mlm.b"], c.vocab_size
            out = None
            if self.adt == torch.bfloat16:
                ws = self.arena.alloc(ops.vocab_argmax_ws_bytes(n, V), torch.uint8)
                out = ops.vocab_argmax_fused(y.t, w, b, V, n=n, ws=ws)
            if out is None:
                out = ops.vocab_argmax(y.t, w, b, V, n=n, logits=self.buf(n, self.flat.Vp, torch.float32), fused=False)
        finally:
            ops.Profiler.scope = prev_scope
        self.last = dict(enc_t=xt, enc_v=xv, token_rows=rows)
        return out


class _DiscFn(torch.autograd.Function):
    """The counterpart of engine._StepFn for Engine.disc_step: hands out the three losses, receives their three upstream gradients
    (train_disc.forward's coefficients and .mean() arrive through them; a loss the caller dropped arrives as zero)."""

    @staticmethod
    def forward(ctx, anchor, feats, engine, st, lm, img, nsp):
        engine._fn_enter(ctx, feats, st)
        return lm.clone(), img.clone(), nsp.clone()

    @staticmethod
    def backward(ctx, g_lm, g_img, g_nsp):
        seeds = [g.reshape(1).float().contiguous() for g in (g_lm, g_img, g_nsp)]
        return None, ctx.engine._fn_feats_grad(ctx, ctx.engine.disc_backward(ctx.st, seeds)), None, None, None, None, None
