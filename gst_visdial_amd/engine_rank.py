"""Listwise candidate training of the generative model: `RankMixin.rank_step` trains on what `score_candidates` ranks by.  The
`group` answer candidates of a dialog round share ONE encoder pass and ONE cross-attention K/V projection, forward and backward;
the loss is the cross entropy between the softmax of the candidates' sequence log-likelihoods and the round's normalised dense
relevance.  Not in the reference, which ships the dense annotations and the NDCG metric but no trainer
that uses them.  `RankMixin` is a part of `engine.Engine`; it uses the engine's forward schedule, its loss plumbing and its tape
replay.  The decoder's cross-attention backward of such a step is gstvd_attn_group_bwd (Engine._attn_bwd)."""
import torch

from . import ops
from ._lib import GstvdError


class RankMixin(object):
    def rank_step(self, feats, loc, img_mask, ids, segs, att_mask, dec_ids, dec_mask, relevance, group, temperature=1.0):
        """Encoder-side tensors have E rows (one per dialog round), decoder-side tensors E * group rows ordered [round, candidate],
        `relevance` E * group values >= 0.  -> (loss, scores [E, group]):
            score_i = sum_u [tgt != 0] log softmax(logits)[i, u, tgt], tgt = dec_ids shifted left   (score_candidates' value)
            t = relevance / sum(relevance) per round,  p = softmax(scores / temperature) over the round
            loss = mean over the rounds with sum(relevance) > 0 of  -sum_i t_i log p_i   (0 when no round counts)
        The forward is score_candidates' with recording on and dropout as the module's mode says; `loss.backward()` fills `.grad`
        of every live parameter (accumulating onto kept ones) and of the image features when they require grad, as after `step`.
        The caller's `dec_ids` stays as it is (the decoder reads the eos -> pad masked copy)."""
        dc = self.dec_cfg
        if self.enc_only:
            raise GstvdError("rank_step belongs to the engine of an EncoderDecoderModel")
        self._refuse_maps("rank_step")
        if self._inputs_only:
            raise GstvdError("rank_step under inputs_only(): the listwise step returns parameter gradients; inputs_only() serves `step`")
        if torch.cuda.is_current_stream_capturing():
            raise GstvdError("rank_step under a stream capture: the listwise step is issued eagerly")
        if self.pipe is not None:
            raise GstvdError("rank_step with an attached BackwardPipeline: the listwise step runs on one GPU without the pipeline")
        E, rows, group = ids.shape[0], dec_ids.shape[0], int(group)
        if group < 1 or rows != E * group:
            raise GstvdError("rank_step: %d decoder rows for %d encoder rows x %d candidates" % (rows, E, group))
        if relevance.numel() != rows:
            raise GstvdError("rank_step: %d relevance values for %d candidates" % (relevance.numel(), rows))
        if not float(temperature) > 0.0:
            raise GstvdError("rank_step: temperature must be positive, got %r" % (temperature,))
        record = torch.is_grad_enabled()
        dev = ids.device
        self._begin(dev, record)
        dec_in = dec_ids.masked_fill(dec_ids == dc.eos_token_id, dc.pad_token_id)
        I = self._inputs(feats, loc, img_mask, ids, segs, att_mask, dec_in, dec_mask)
        xt, xv = self.encoder(I)
        enc = self.fusion(xt, xv, I)
        y, logits = self.decoder(enc, I, self._cross_kv(enc), kv_group=group)
        U = I["U"]
        tgt = dec_ids.new_zeros(dec_ids.shape)
        tgt[:, :-1] = dec_ids[:, 1:]
        ce = self._ce(logits, tgt, rows, U)[2]
        rel = relevance.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        ids_c = dec_ids.contiguous()
        scores = torch.empty(E, group, dtype=torch.float32, device=dev)      # handed to the caller: not in the arena
        p, round_loss, g_tok, stats = self.vec(rows), self.vec(E), self.vec(rows * U), self.vec(4)
        ops.rank_loss(logits.t, ce["lse"], ids_c, rel, E, group, U, 1.0 / float(temperature), scores, p, round_loss, g_tok, stats[:3])
        self.last = dict(enc_t=xt, enc_v=xv, enc=enc, dec_hidden=y, logits=logits, lse=ce["lse"], rank_p=p, rank_round_loss=round_loss,
                         rank_stats=stats)
        if record:
            st = dict(ce, I=I, logits=logits, tape=self.tape, g_tok=g_tok)
            return _RankFn.apply(self.anchor, feats if I["feats_grad"] else None, self, st, stats[2]), scores
        return stats[2].clone(), scores

    def rank_backward(self, st, gloss):
        """Backward of rank_step: the per-token upstream gradients the loss launch left, times the upstream scalar, through the
        per-row cross-entropy backward; then the shared replay."""
        self._backward_begin()
        logits = st["logits"]
        logits.g = self.buf(st["Md"], self.flat.Vp)
        g = st["g_tok"]
        if gloss is not None:
            g = g * gloss.reshape(1).to(device=g.device, dtype=torch.float32)
        ops.ce_bwd_rows(logits.t, st["lab"], st["lse"], g, st["Md"], st["V"], logits.g, ignore_index=st["pad"])
        return self._replay(st)


class _RankFn(torch.autograd.Function):
    """The counterpart of engine._StepFn for Engine.rank_step."""

    @staticmethod
    def forward(ctx, anchor, feats, engine, st, loss_raw):
        engine._fn_enter(ctx, feats, st)
        return loss_raw.clone()

    @staticmethod
    def backward(ctx, gloss):
        return None, ctx.engine._fn_feats_grad(ctx, ctx.engine.rank_backward(ctx.st, gloss)), None, None, None
