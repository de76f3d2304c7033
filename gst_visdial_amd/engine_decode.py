"""Answer decoding of the engine (models/visual_dialog_model.py:74-120, generate.py:183-211): one token per row and step
through the decoder stack against per-layer K/V caches, in three modes -- `sample`, `beam_search`, `sample_ranked` -- that run
through ONE driver (`_decode`: eager first call, then the captured hipGraph form of the loop), and the perplexity re-score of
the sampled answer.  `DecodeMixin` is the decode half of `engine.Engine`; it uses the engine's op helpers and schedule."""
import collections

import torch

from . import ops
from . import _lib as _libmod
from .storage import Act
from ._lib import GstvdError, EPI_GELU


class _Session(object):
    """One decode call's state on fixed addresses.  An eager call builds one on the caller's tensors and drops it; a captured one
    owns clones of the inputs and is kept in `Engine._decode_sessions`.
      ins            the seven tensors the kernels read: (feats, loc, img_mask, ids, segs, att_mask, dec_ids)
      bufs           the mode's buffers by name (all time-major): the ids `cur`, the mode's scores, the call's uniforms `u`, the
                     n-gram history `hist`
      st             `_decode_plan`'s state: encoder inputs, cross K/V, caches, the arena mark -- what `rescore_sampled` reuses
      ret            what the mode's loop returned
      g_enc, g_dec   the captured graphs of the encoder side and of the whole token loop; None on an eager call"""

    def __init__(self, ins, bufs):
        self.ins, self.bufs, self.st, self.ret, self.g_enc, self.g_dec = ins, bufs, None, None, None, None

    def refresh(self, ins, u=None):
        for dst, src in zip(self.ins, ins):
            if dst is not None:
                dst.copy_(src)
        if u is not None:
            self.bufs["u"].copy_(u)


# What the three decode modes differ in.  reorder: a second set of self-attention caches (`_decode_plan`); keeps_state: the call
# leaves `_last_decode` for `rescore_sampled`; buffers(Bn, K, L0, max_seq_len, dev) -> dict of static tensors; hist(h, K) -> the
# n-gram history of the decoder rows from the B dialogs' `h` (None: the mode bans nothing); loop(engine, one_token, session, L0,
# max_seq_len, K, P): the whole token loop on the session's buffers, free of host synchronisation -- eager issue and graph capture
# run this same code.
_Mode = collections.namedtuple("_Mode", "name reorder keeps_state buffers hist loop")


def _sample_buffers(Bn, K, L0, max_seq_len, dev):
    return dict(cur=torch.zeros(L0 + max_seq_len, Bn, dtype=torch.long, device=dev))      # time-major (see _sampling_step)


def _sample_loop(eng, one_token, s, L0, max_seq_len, K, P):
    """Every decoder position's stack and, from position L0 - 1 on (earlier ones only consume the given prefix), its sampling
    step: filters, softmax, draw, append.  Returns the last logits."""
    cur, u, hist = s.bufs["cur"], s.bufs["u"], s.bufs["hist"]
    cur[:L0] = s.ins[6].t()
    for t in range(L0 + max_seq_len - 1):
        logits = one_token(cur[t], t)
        if t >= L0 - 1:
            eng._sampling_step(logits, cur, t + 1, hist, P, u[t - (L0 - 1)])
    return logits


def _beam_buffers(Bn, K, L0, max_seq_len, dev):
    """Static state of a beam call: the time-major id buffer, the ping-pong (score, done) pairs, one parent row per generated
    position, the step kernel's workspace and the state in front of the first step (s[b,0] = 0, s[b,j>0] = -inf)."""
    init = torch.full((Bn, K), -float("inf"), dtype=torch.float32, device=dev)
    init[:, 0] = 0.0
    return dict(cur=torch.zeros(L0 + max_seq_len, Bn * K, dtype=torch.long, device=dev),
                score=[torch.zeros(Bn, K, dtype=torch.float32, device=dev) for _ in range(2)],
                done=[torch.zeros(Bn, K, dtype=torch.int32, device=dev) for _ in range(2)],
                parent=torch.zeros(max_seq_len, Bn, K, dtype=torch.int32, device=dev),
                ws=ops.beam_workspace(Bn, K, dev), init=init)


def _beam_loop(eng, one_token, s, L0, max_seq_len, K, P):
    """The prefix positions feed all K rows of a dialog alike; from position L0 - 1 on every token step is followed by the beam
    step (gstvd_beam_step: token row t + 1 of the id buffer, parents, the other (score, done) pair) and, while another token step
    follows, by the reorder of the self-attention caches into the OTHER cache set, which the next token step then appends to and
    reads.  K = 1 keeps one cache set (its only parent is itself).  Returns the index of the final (score, done) pair."""
    dc, bufs, dec_ids = eng.dec_cfg, s.bufs, s.ins[6]
    cur, score, done = bufs["cur"], bufs["score"], bufs["done"]
    Bn = dec_ids.shape[0]
    cur[:L0] = dec_ids.t()[:, :, None].expand(L0, Bn, K).reshape(L0, Bn * K)
    score[0].copy_(bufs["init"])
    done[0].zero_()
    steps, cset = L0 + max_seq_len - 1, 0
    H, Umax = dc.hidden_size, s.st["Umax"]
    for t in range(steps):
        logits = one_token(cur[t], t, cset)
        if t < L0 - 1:
            continue
        g = t - (L0 - 1)
        ops.beam_step(logits, score[g & 1], done[g & 1], score[(g + 1) & 1], done[(g + 1) & 1], bufs["parent"][g], cur, t + 1,
                      bufs["ws"], dc.eos_token_id, dc.pad_token_id)
        if K > 1 and t + 1 < steps:
            sets = s.st["QKVc"]
            ops.beam_reorder([a.t.view(Bn * K, Umax, 3 * H) for a in sets[cset]],
                             [a.t.view(Bn * K, Umax, 3 * H) for a in sets[1 - cset]], bufs["parent"][g], t, H)
            cset = 1 - cset
    return max_seq_len & 1


def _ranked_buffers(Bn, S, L0, max_seq_len, dev):
    return dict(cur=torch.zeros(L0 + max_seq_len, Bn * S, dtype=torch.long, device=dev),
                lp=torch.zeros(max_seq_len, Bn * S, dtype=torch.float32, device=dev))


def _ranked_loop(eng, one_token, s, L0, max_seq_len, S, P):
    """The prefix goes to all S rows of a dialog alike; from position L0 - 1 on every token step is followed by ONE launch
    (gstvd_sample_topk_scored) that draws token row t + 1 of the time-major id buffer `cur` and writes the drawn ids'
    log-probabilities into row t - (L0 - 1) of the time-major buffer `lp`.  Returns the last logits."""
    cur, lp, u, hist, dec_ids = s.bufs["cur"], s.bufs["lp"], s.bufs["u"], s.bufs["hist"], s.ins[6]
    Bn = dec_ids.shape[0]
    cur[:L0] = dec_ids.t()[:, :, None].expand(L0, Bn, S).reshape(L0, Bn * S)
    for t in range(L0 + max_seq_len - 1):
        logits = one_token(cur[t], t)
        if t >= L0 - 1:
            g = t - (L0 - 1)
            ops.sample_topk_scored(logits, P["temperature"], P["top_k"], u[g], cur[t + 1], lp[g], None,
                                   ngram=(hist, cur, t + 1, P["ngram"]) if P["ngram"] > 0 else None, top_p=P["top_p"])
    return logits


_SAMPLE = _Mode("sample", True, True, _sample_buffers, lambda h, K: h, _sample_loop)
_BEAM = _Mode("beam", True, False, _beam_buffers, None, _beam_loop)
_RANKED = _Mode("ranked", False, True, _ranked_buffers, lambda h, S: h.repeat_interleave(S, 0), _ranked_loop)


class DecodeMixin(object):
    def _decode_plan(self, ins, L0, max_seq_len, beams=1, reorder=True):
        """Builds the two device programs of a decode call on the engine's arena: `encode()` (encoder, VLFusion, the
        cross-attention K/V of all decoder layers -- once per call) and `one_token(tok, t)` (ONE token per row through
        the decoder stack at position t, its self-attention K/V appended to the per-layer caches) -> fp32 logits [B, V].
        `ins` = (feats, loc, img_mask, ids, segs, att_mask, dec_ids) are the tensors the kernels read.
        beams = K > 1 (beam_search): B * K decoder rows over the B encoder rows -- cross-attention with kv_group = K -- and a
        SECOND set of self-attention caches; `one_token(tok, t, cset)` appends to and reads set `cset` (st["QKVc"][cset]).
        reorder=False (sample_ranked: K independent rows per dialog, nothing is ever permuted): the K rows per dialog over ONE
        cache set of B * K rows."""
        feats, loc, img_mask, ids, segs, att_mask, dec_ids = ins
        dc = self.dec_cfg
        st = {}

        def encode():
            self._begin(ids.device, False, inference=True)
            I = self._inputs(feats, loc, img_mask, ids, segs, att_mask, dec_ids, None)
            xt, xv = self.encoder(I)
            enc = self.fusion(xt, xv, I)
            Bn = I["B"]
            L, H = dc.num_hidden_layers, dc.hidden_size
            st["I"], st["Bn"], st["S"] = I, Bn, I["R"] + I["T"]
            st["kv"] = self._cross_kv(enc)                                       # cross K/V of all layers, once
            Umax = L0 + max_seq_len
            st["Umax"] = Umax
            # per-layer cache of the fused Q|K|V rows, [B, Umax, 3H]: the QKV GEMM of position t writes its output rows straight
            # into cache[:, t] (row stride Umax*3H), attention reads K / V from the same rows -- no append copies
            Dn = Bn * beams
            sets = [[Act(self.buf(Dn * Umax, 3 * H), Dn * Umax, 3 * H) for _ in range(L)] for _ in range(2 if beams > 1 and reorder else 1)]
            st["QKVc"] = sets if len(sets) == 2 else sets[0]
            st["mark"] = self.arena.mark()

        def one_token(tok, t, cset=0):
            I, Bn, S, kv, QKVc, Umax = st["I"], st["Bn"] * beams, st["S"], st["kv"], st["QKVc"], st["Umax"]
            if beams > 1 and reorder:
                QKVc = QKVc[cset]
            V, Vp = dc.vocab_size, self.flat.Vp
            L, H, nh, eps = dc.num_hidden_layers, dc.hidden_size, dc.num_attention_heads, dc.layer_norm_eps
            d = H // nh
            prefix = "emb" if self.flat.dec_emb is self.flat.enc_emb else "demb"
            self.arena.rewind(st["mark"])
            y = self.embed(prefix, tok.contiguous(), None, Bn, 1, dc, pos_offset=t)
            # bf16: the three LayerNorms of a layer are folded into the Linears that read them (gstvd_gemv_ln) and the residual
            # adds into the epilogues of the Linears in front of them -- 8 launches per layer instead of 11.  `pre` = the
            # rows whose LayerNorm (parameters `lnp`) the next Linear still has to apply.
            fuse = (self.adt is torch.bfloat16 and Bn <= 16 and H <= 1024
                    and bool(self.model.params.get("amd_decode_fuse_ln", True)))       # (the switch exists for the parity test)
            I_ = dc.intermediate_size
            pre, lnp = None, None
            for i in range(L):
                p = "d%d" % i
                rows_t = QKVc[i].t.view(Bn, Umax, 3 * H)[:, t]                     # [Bn, 3H] view, row stride Umax * 3H
                if pre is None:
                    ops.gemm(y.t, self.W[p + ".qkv.w"], rows_t, Bn, 3 * H, H, bias=self.Pv[p + ".qkv.b"])
                else:
                    y = self.act(Bn, H)
                    ops.gemv_ln(pre.t, self.W[p + ".qkv.w"], rows_t, Bn, 3 * H, H, self.Pv[lnp + ".w"], self.Pv[lnp + ".b"], eps,
                                y_out=y.t, bias=self.Pv[p + ".qkv.b"])
                qkv = Act(rows_t, Bn, 3 * H)
                ctx = self.attn((qkv, 0), (QKVc[i], H), (QKVc[i], 2 * H), Bn, nh, 1, t + 1, d, None, False, -10000.0, 0.0,
                                kv_bstride=Umax)
                if fuse:
                    pre1, y1, q = self.act(Bn, H), self.act(Bn, H), self.act(Bn, H)
                    ops.gemm(ctx.t, self.W[p + ".ao.w"], pre1.t, Bn, H, H, bias=self.Pv[p + ".ao.b"], addend=y.t)
                    ops.gemv_ln(pre1.t, self.W[p + ".cq.w"], q.t, Bn, H, H, self.Pv[p + ".ln1.w"], self.Pv[p + ".ln1.b"], eps,
                                y_out=y1.t, bias=self.Pv[p + ".cq.b"])
                    ctx = self.attn((q, 0), (kv, 2 * i * H), (kv, (2 * i + 1) * H), Bn, nh, 1, S, d, I["emask"], False, -1e9, 0.0,
                                    kv_group=beams)
                    pre2, y2, a, aux = self.act(Bn, H), self.act(Bn, H), self.act(Bn, I_), self.buf(Bn, I_)
                    ops.gemm(ctx.t, self.W[p + ".co.w"], pre2.t, Bn, H, H, bias=self.Pv[p + ".co.b"], addend=y1.t)
                    ops.gemv_ln(pre2.t, self.W[p + ".fi.w"], a.t, Bn, I_, H, self.Pv[p + ".ln2.w"], self.Pv[p + ".ln2.b"], eps,
                                y_out=y2.t, bias=self.Pv[p + ".fi.b"], aux=aux, epi=EPI_GELU)
                    pre = self.act(Bn, H)
                    ops.gemm(a.t, self.W[p + ".fo.w"], pre.t, Bn, H, I_, bias=self.Pv[p + ".fo.b"], addend=y2.t)
                    lnp = p + ".ln3"
                    continue
                ao = self.lin(ctx, p + ".ao.w", p + ".ao.b", H, H)
                y1 = self.ln(ao, y, p + ".ln1.w", p + ".ln1.b", H, 0.0, None, eps)
                q = self.lin(y1, p + ".cq.w", p + ".cq.b", H, H)
                ctx = self.attn((q, 0), (kv, 2 * i * H), (kv, (2 * i + 1) * H), Bn, nh, 1, S, d, I["emask"], False, -1e9, 0.0,
                                kv_group=beams)
                co = self.lin(ctx, p + ".co.w", p + ".co.b", H, H)
                y2 = self.ln(co, y1, p + ".ln2.w", p + ".ln2.b", H, 0.0, None, eps)
                a = self.lin(y2, p + ".fi.w", p + ".fi.b", dc.intermediate_size, H, gelu=True)
                fo = self.lin(a, p + ".fo.w", p + ".fo.b", H, dc.intermediate_size)
                y = self.ln(fo, y2, p + ".ln3.w", p + ".ln3.b", H, 0.0, None, eps)
            if pre is not None:
                # (the LM head keeps LayerNorm + Linear as two launches: 1908 workgroups of the LN-in kernel, each holding
                # gamma / beta in registers, stream the 47 MB of vocabulary weights at a quarter of the plain kernel's rate)
                y = self.ln(pre, None, lnp + ".w", lnp + ".b", H, 0.0, None, eps)
            return self.lin(y, "lm.w", "lm.b", Vp, H).t[:, :V]         # [Bn, V] view of the arena (row stride Vp), activation dtype

        return encode, one_token, st

    def _sampling_step(self, logits, cur, pos, hist, P, u_row):
        """One step of models/visual_dialog_model.py:96-108 on static buffers: cur[pos] <- the token drawn from `logits`
        (temperature, n-gram ban against `hist`, top-k / top-p, softmax, inverse-CDF draw from the uniforms `u_row`).
        `cur` is the TIME-MAJOR id buffer [L0 + max_seq_len, B]: position t of all rows is one contiguous row, which the next
        token step's embedding reads as it is.  Free of host synchronisation and of generator state, so the token graph
        captures it together with the decoder stack."""
        from . import decoding
        if self._fused_sampling(P, logits.shape[-1]):
            # the n-gram ban (utils/decoding_utils.py:38-77) runs inside the sampling launch: `hist` and the time-major id buffer
            # are all it needs (round 4 built a [B, V + 1] mask with ten torch launches per token: +2 ms per questioner decode)
            ops.sample_topk(logits, P["temperature"], P["top_k"], u_row, cur[pos], None,
                            ngram=(hist, cur, pos, P["ngram"]) if P["ngram"] > 0 else None, top_p=P["top_p"])
            return
        last = logits.float() / P["temperature"]
        last = decoding.batch_ngram_blocking(last, hist, cur[:pos].t(), ngram_size=P["ngram"])
        last = decoding.batch_top_k_top_p_sampling(last, top_k=P["top_k"], top_p=P["top_p"])
        prob = torch.softmax(last, dim=-1)
        cur[pos] = decoding.draw_from_uniform(prob, u_row).view(-1)

    def _decode_issue(self, mode, ins, L0, max_seq_len, K, P, u, static):
        """Issues one decode call of `mode` on `ins` -> its _Session.  The ONLY function that opens decode captures.
        static=False: eagerly, on the caller's tensors and uniforms; counts `decode_lib_calls_per_token` over the token loop.
        static=True: the hipGraph form (generate.py's loop calls with the same shapes and settings batch after batch): clones of
        the inputs, a static uniform buffer, one captured graph for `encode` (and the n-gram history) and ONE for the whole token
        loop -- every position's decoder stack AND its tail (sampling step / beam step and cache reorder), so that nothing of the
        loop is issued from the host at replay (round 1-2 replayed one graph per position and ran ~25 small torch kernels per
        step eagerly in between: the loop was bound by host issue).  Nothing executes; one garbage collection for both captures,
        the loop graph in the encoder graph's pool.  Both ways run the same `mode.loop`."""
        if static:
            ins = tuple(x.clone() if x is not None else None for x in ins)
        ids, segs = ins[3], ins[4]
        s = _Session(ins, mode.buffers(ids.shape[0], K, L0, max_seq_len, ids.device))
        if u is not None:
            s.bufs["u"] = torch.zeros_like(u) if static else u
        encode, one_token, s.st = self._decode_plan(ins, L0, max_seq_len, beams=K, reorder=mode.reorder)

        def head():
            encode()
            if mode.hist is not None:
                s.bufs["hist"] = mode.hist(ids * (segs == 0).long(), K)

        def loop():
            s.ret = mode.loop(self, one_token, s, L0, max_seq_len, K, P)

        if not static:
            head()
            calls0 = _libmod.N_CALLS[0]
            loop()
            self.decode_lib_calls_per_token = (_libmod.N_CALLS[0] - calls0) / float(L0 + max_seq_len - 1)
            return s
        from .graph import capture, gc_quiet
        with gc_quiet():
            s.g_enc = torch.cuda.CUDAGraph()
            with capture(s.g_enc):
                head()
            s.g_dec = torch.cuda.CUDAGraph()
            with capture(s.g_dec, pool=s.g_enc.pool(), quiesce=False):
                loop()
        return s

    def _decode(self, mode, tensors, max_seq_len, finish, K=1, P=None, key=(), uniforms=None, graph=True):
        """The driver of `sample`, `beam_search` and `sample_ranked`: K decoder rows per dialog, P the sampling settings (None: the
        mode draws nothing), `key` what else tells two sessions of the mode apart, `finish(session)` forms the call's results and
        `self.last` from the session's buffers.  With params['amd_decode_graph'] (default on) and `graph`, the first call with a
        signature issues eagerly -- which also initialises every lazily built table / attribute / arena chunk -- and is then
        captured; later calls refresh the session's static tensors and replay its two graphs.  At most four sessions are kept."""
        feats, loc, img_mask, ids, segs, att_mask, dec_ids = tensors
        if segs is None:
            segs = torch.zeros_like(ids)
        ins = (feats, loc, img_mask, ids, segs, att_mask, dec_ids)
        L0, Bn, u = dec_ids.shape[1], ids.shape[0], None
        if P is not None and uniforms is None:
            # the call's randomness, drawn ONCE from torch's default CUDA generator (eagerly: no generator state inside the
            # captured graphs); every step then draws by inverse CDF -- the same distribution as the reference's
            # torch.multinomial (whose stream is device specific anyway), and the same ids from eager issue and graph replay
            u = torch.rand(max_seq_len, Bn * K, device=ids.device, dtype=torch.float32).clamp_min_(1e-12)
        elif P is not None:
            if uniforms.dim() != 2 or uniforms.shape[0] < max_seq_len or uniforms.shape[1] != Bn * K:
                raise GstvdError("uniforms must be [max_seq_len = %d, decoder rows = %d] (one draw per step and decoder row: batch "
                                 "times num_samples), got %s" % (max_seq_len, Bn * K, tuple(uniforms.shape)))
            u = uniforms.to(ids.device, torch.float32)[:max_seq_len].contiguous()
        sig = ((mode.name, L0, max_seq_len, K, tuple(sorted(P.items())) if P is not None else None) + tuple(key)
               + tuple((tuple(x.shape), x.dtype) if x is not None else None for x in ins))
        use_graph = graph and bool(self.model.params.get("amd_decode_graph", True))
        # parameters edited since the last call (load_state_dict, an optimizer step): the captured graphs read the flat
        # buffers / bf16 shadow, so bring those up to date OUTSIDE the graphs; a re-materialised buffer drops the sessions
        self.prepare(ids.device)
        s = self._decode_sessions.get(sig) if use_graph else None
        replayed = s is not None
        if replayed:
            s.refresh(ins, u)
            s.g_enc.replay()
            s.g_dec.replay()
        else:
            s = self._decode_issue(mode, ins, L0, max_seq_len, K, P, u, False)
        out = finish(s)
        if use_graph and not replayed:
            if len(self._decode_sessions) >= 4:
                self._decode_sessions.clear()
            self._decode_sessions[sig] = self._decode_issue(mode, ins, L0, max_seq_len, K, P, u, True)
        # (after the capture: capturing runs the Python side of encode() again -- which rewinds the arena bookkeeping and drops
        # this marker -- but executes nothing, so the eager call's encoder states are still what the arena holds.)  The encoder
        # side of a sampling call (B rows: cross-attention K/V of all layers, masks) stays valid in the arena until the next
        # engine call: `rescore_sampled` scores an answer against it without a second encoder pass.  Beam search leaves none:
        # its K rows per dialog are not a state rescore_sampled could score an answer against.
        self._last_decode = (s.st, Bn, self.arena) if mode.keeps_state else None
        return out

    def _decode_rows(self, name, arg, value):
        """The one range check of `num_beams` / `num_samples` (modules.py relies on it): K decoder rows per dialog, 1..ops.BEAM_MAX,
        over a vocabulary the fused step kernels hold."""
        K = int(value)
        if not 1 <= K <= ops.BEAM_MAX:
            raise GstvdError("%s: %s must be in 1..%d, got %r" % (name, arg, ops.BEAM_MAX, value))
        if self.dec_cfg.vocab_size > ops.SAMPLE_MAX_VOCAB:
            raise GstvdError("%s: vocabulary %d exceeds the kernel's %d" % (name, self.dec_cfg.vocab_size, ops.SAMPLE_MAX_VOCAB))
        return K

    @torch.no_grad()
    def sample(self, feats, loc, img_mask, ids, segs, att_mask, dec_ids, temperature=1.0, top_k=0, top_p=0.0,
               ngram_blocking_size=0, max_seq_len=18, uniforms=None, **_):
        """models/visual_dialog_model.py:74-120: 18 sampling steps (temperature, n-gram blocking, top-k / top-p, multinomial
        draw, [PAD] after the first [SEP]).  The reference re-runs the whole decoder on the growing prefix and re-projects
        the cross-attention K/V of all 37+T encoder states in all 12 layers at every step (use_cache=False); here the
        encoder, VLFusion and the cross K/V projection run once, and each step feeds ONE token per row through the stack,
        appending its self-attention K/V to a [B, Umax, H] cache per layer.  Same arithmetic, O(U) instead of O(U^2).
        From the second call with the same shapes and sampling settings on (params['amd_decode_graph'], default on) the
        device work is replayed from two captured hipGraphs (the encoder side; the whole token loop incl. its sampling
        steps): ~3000 launches per call leave the host.
        Token-id work (filters, n-gram ban, EOS fill) is integer-exact torch index plumbing (decoding.py), free of host syncs.
        Token t is drawn by inverse CDF from uniforms[t] ([max_seq_len, B] in (0, 1); drawn from torch's default generator when
        the caller passes none) instead of torch.multinomial (whose stream is device specific) -- the same rule the oracle
        applies to the reference, so sampled ids can be compared under real sampling."""
        self._refuse_maps("sample")
        from . import decoding
        if _.get("num_beams") is not None and int(_["num_beams"]) > 1:
            raise GstvdError("sample() draws one answer per row; num_beams = %d is beam search: call beam_search(...) or "
                             "model(..., num_beams=K)" % int(_["num_beams"]))
        dc, L0 = self.dec_cfg, dec_ids.shape[1]
        P = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), ngram=int(ngram_blocking_size))

        def finish(s):
            # (a replayed session's id buffer is overwritten by the next call: hand out a copy)
            cur = s.bufs["cur"].clone() if s.g_dec is not None else s.bufs["cur"]
            self.last = dict(decode_logits=s.ret.float())    # last position's raw logits (tests / debugging)
            return decoding.pad_after_eos(cur[L0:].t().contiguous(), dc.eos_token_id, dc.pad_token_id)

        # (a vocabulary beyond the fused kernel's takes the torch filters, eagerly step by step: no captured token graph)
        return self._decode(_SAMPLE, (feats, loc, img_mask, ids, segs, att_mask, dec_ids), max_seq_len, finish, P=P,
                            uniforms=uniforms, graph=self._fused_sampling(P, dc.vocab_size))

    @torch.no_grad()
    def beam_search(self, feats, loc, img_mask, ids, segs, att_mask, dec_ids, num_beams=5, length_penalty=1.0, max_seq_len=18):
        """Deterministic beam-search decoding of the answer -> (sequences [B, K, max_seq_len] int64, scores [B, K] fp32), the K
        hypotheses of every dialog row best first.  The reference has no beam search; this is the rule:

        Layout: B dialog rows, K = num_beams in 1..8; beam j of dialog b is decoder row b*K + j.  Encoder, VLFusion and the cross
        K/V projection run once on the B rows; cross-attention shares one encoder row among K decoder rows (kv_group = K).
        State: per beam an fp32 score s[b,j] (sum of token log-probabilities) and a flag done[b,j]; in front of the first
        generated position s[b,0] = 0, s[b,j>0] = -inf, nothing done.  The L0 prefix tokens of `dec_ids` go to all K rows alike.
        Step: a live beam j offers every v in [0, V) with score s[b,j] + logp_j[v], logp_j[v] = (z[v] - max z) - log sum exp(z -
        max z) in fp32 over the row's raw logits (temperature, top-k and top-p play no part); a done beam offers exactly one
        candidate, (j, PAD), with its score unchanged.  The K best candidates of the row become the new beams in order: higher
        score first, equal scores by smaller j, then smaller v; -inf sorts last under the same index rule.  New beam i records
        parent[b,i] = j, tok[b,i] = v, the score, and done = done_j or v == EOS.
        End: all max_seq_len steps always run (done beams are frozen, so the result equals stopping early and nothing depends on
        the host).  Sequences are the parents walked back from the last step; len = tokens up to and including the first EOS, or
        max_seq_len; final score = s / len ** length_penalty; hypotheses best first, ties to the smaller beam index; PAD follows
        the first EOS (decoding.pad_after_eos).

        The first call with a shape runs eagerly; from then on (params['amd_decode_graph'], default on) it replays two captured
        hipGraphs keyed by shapes, K and length_penalty: the encoder side, and the whole loop -- decoder stack, beam step
        (gstvd_beam_step) and cache reorder (gstvd_beam_reorder) at every position.  The back-trace and the final ordering are
        sync-free torch index work (decoding.beam_backtrace / beam_finalize).  A beam call leaves no decode state behind:
        `rescore_sampled` after it raises its "no decode state" error."""
        self._refuse_maps("beam_search")
        from . import decoding
        dc = self.dec_cfg
        K = self._decode_rows("beam_search", "num_beams", num_beams)
        if dc.num_hidden_layers > ops.BEAM_MAX_LAYERS:
            raise GstvdError("beam_search: at most %d decoder layers" % ops.BEAM_MAX_LAYERS)
        L0, Bn = dec_ids.shape[1], ids.shape[0]

        def finish(s):
            bufs, fin = s.bufs, s.ret
            tok = bufs["cur"][L0:].view(max_seq_len, Bn, K)
            seqs = decoding.beam_backtrace(tok, bufs["parent"])
            out, scores, order = decoding.beam_finalize(seqs, bufs["score"][fin], dc.eos_token_id, dc.pad_token_id, length_penalty)
            # (what the step kernel decided, unsorted, for tests / debugging: tokens and parents per step, summed log-probabilities)
            self.last = dict(beam_tok=tok.clone(), beam_parent=bufs["parent"].clone(), beam_logp=bufs["score"][fin].clone(),
                             beam_order=order)
            return out, scores

        return self._decode(_BEAM, (feats, loc, img_mask, ids, segs, att_mask, dec_ids), max_seq_len, finish, K=K,
                            key=(float(length_penalty),))

    @torch.no_grad()
    def sample_ranked(self, feats, loc, img_mask, ids, segs, att_mask, dec_ids, num_samples=4, length_penalty=1.0, temperature=1.0,
                      top_k=0, top_p=0.0, ngram_blocking_size=0, max_seq_len=18, uniforms=None):
        """Sample-and-rank decoding of the answer -> (sequences [B, S, max_seq_len] int64, scores [B, S] fp32, token_logp
        [B, S, max_seq_len] fp32): S = num_samples in 1..8 independent draws per dialog row under the settings of `sample`, each
        with the model's log-probability of every drawn token, the S samples of a dialog best first.

        Layout: sample j of dialog b is decoder row b*S + j over encoder row b.  Encoder, VLFusion and the cross K/V projection
        run once on the B rows; cross-attention shares one encoder row among S decoder rows (kv_group = S); ONE set of
        self-attention caches of B*S rows -- the rows are independent, nothing is reordered.  The n-gram filter of row b*S + j
        reads the history of dialog b.
        Draw: the rule of `sample` (gstvd_sample_topk) from uniforms[t, b*S + j]; `uniforms` is [max_seq_len, B*S] in (0, 1), drawn
        once from torch's generator when absent.  With S = 1 and the same uniforms the ids are those of `sample`.
        Score: the same launch (gstvd_sample_topk_scored) writes the drawn token's log-probability under the row's RAW logits,
        (x[id] - max x) - log sum exp(x - max x) in fp32 -- temperature, bans, top-k and top-p play no part; this is the beam
        step's logp, so sampled and beam scores compare.  Positions after the first EOS are PAD with token_logp 0; len = tokens
        up to and including the first EOS, or max_seq_len; score = sum(token_logp) / len ** length_penalty; samples best first,
        ties to the smaller sample index (decoding.beam_finalize).  All max_seq_len steps always run: nothing asks the host.

        The first call with a shape runs eagerly; from then on (params['amd_decode_graph'], default on) it replays two captured
        hipGraphs keyed by shapes, S and the sampling settings.  One library call per token more than the decoder stack's, as in
        `sample`.  The encoder side of the call stays valid for the B best answers: `rescore_sampled(best)` works as after
        `sample` (encoder states and cross K/V have B rows)."""
        self._refuse_maps("sample_ranked")
        from . import decoding
        dc = self.dec_cfg
        S = self._decode_rows("sample_ranked", "num_samples", num_samples)
        L0, Bn = dec_ids.shape[1], ids.shape[0]
        P = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), ngram=int(ngram_blocking_size))

        def finish(s):
            self.last = dict(decode_logits=s.ret.float())
            out, scores, token_logp, order = decoding.rank_samples(s.bufs["cur"][L0:].view(max_seq_len, Bn, S).permute(1, 2, 0),
                                                                   s.bufs["lp"].view(max_seq_len, Bn, S).permute(1, 2, 0),
                                                                   dc.eos_token_id, dc.pad_token_id, length_penalty)
            self.last["sample_order"] = order
            return out, scores, token_logp

        return self._decode(_RANKED, (feats, loc, img_mask, ids, segs, att_mask, dec_ids), max_seq_len, finish, K=S, P=P,
                            uniforms=uniforms)

    @torch.no_grad()
    def _topk_soft(self, logits, ce, rows, U, top_k):
        """The teacher's soft labels of a teacher-forced pass: the top_k best tokens of every position with their log-probabilities
        (gstvd_topk_logp on the pass's logits, before the arena is rewound) -> (ids [rows, U, K] int64, logp [rows, U, K] fp32,
        labels [rows, U] int64), tensors of their own."""
        K = int(top_k)
        if not 1 <= K <= ops.DISTILL_MAX_K:
            raise GstvdError("soft_top_k = %d outside 1..%d" % (K, ops.DISTILL_MAX_K))
        ids, logp = ops.topk_logp(logits.t, ce["lse"], ce["Md"], ce["V"], K)
        return ids.view(rows, U, K), logp.view(rows, U, K), ce["lab"].view(rows, U).clone()

    def rescore_sampled(self, dec_ids, dec_mask=None, loss_reduction=False, soft_top_k=None):
        """The "ppl trick" of generate.py:183-211 fused onto the decode call that produced the answer: ONE teacher-forced
        decoder pass over `dec_ids` against the encoder states / cross-attention K/V that the last `sample()` call left in
        the arena (same context by construction: the answer was sampled from it) -- no second encoder run, no second K/V
        projection.  Same conventions as the reference's labels=None branch (visual_dialog_decoder.py:53-57): labels are
        the ids shifted left, `dec_ids` has [SEP] -> [PAD] in place.  Returns (loss, logits) like `step`; with soft_top_k = K
        also the pass's soft labels: (loss, logits, (ids [rows, U, K], logp [rows, U, K], labels [rows, U]))."""
        ld = self._last_decode
        if ld is None or ld[2] is not self.arena or ld[1] != dec_ids.shape[0]:
            raise GstvdError("rescore_sampled: no decode state of a matching sample() call to reuse")
        st = ld[0]
        self.arena.rewind(st["mark"])
        self.tape, self.rec, self.tag, self.train = [], False, "t", False
        self.main = torch.cuda.current_stream()
        labels = self._shift_labels(dec_ids)
        I = dict(st["I"])
        Bn, U = I["B"], dec_ids.shape[1]
        I["U"] = U
        I["dec_ids"] = dec_ids.contiguous().view(-1)
        I["dmask"] = dec_mask.float().contiguous() if dec_mask is not None else None
        _, logits = self.decoder(None, I, kv=st["kv"])
        loss, lv, ce = self._ce(logits, labels, Bn, U, loss_reduction)
        self._last_decode = None                  # the decode scratch behind the mark has been overwritten
        if soft_top_k is not None:
            return loss.clone(), lv.to(torch.float32, copy=True), self._topk_soft(logits, ce, Bn, U, soft_top_k)
        return loss.clone(), lv.to(torch.float32, copy=True)
