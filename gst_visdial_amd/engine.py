"""Execution engine of the enc_dec_a hot path on one MI355X.

Replaces, for the modules of `modules.py`, the eager PyTorch arithmetic of
    models/vilbert_dialog.py:324-912,1325-1427   (embeddings, two-stream encoder schedule)
    models/visual_dialog_model.py:24-72,123-135 (glue, VLFusion)
    models/visual_dialog_decoder.py:33-86,219-339 + transformers-4.16.2 BertEncoder (decoder, LM head, CE)
and autograd's backward of all of it (train_gen.py:324) by a fixed schedule of HIP kernels called through
the C ABI (`ops`).  Design points:

  * parameters, gradients and bf16 shadow weights live in flat buffers, activations in a bump arena that is rewound
    every step (storage.py: `FlatParams`, `Arena`, `Act`);
  * forward records a tape of backward closures; backward replays it in reverse.  Residual gradients are
    accumulated in the dgrad GEMM epilogue, GELU' in the dgrad epilogue, bias gradients come out of the
    LayerNorm backward partial sums; dropout masks are regenerated from (seed, step, site, index);
  * the 42 parameters that get no gradient in enc_dec mode (poolers, cls heads, q_dense*, sep_embeddings;
    models/vilbert_dialog.py:1400-1401,1482-1487) are never touched: their forward is dead compute in the
    reference and skipping it changes no output.

Numerics: precision 'fp32' runs every GEMM on the exact-fp32 MFMA (parity gate: logits within 1e-4 of the
oracle); 'bf16' stores activations/weights in bf16 with fp32 accumulation and fp32 LN/softmax/CE statistics.
The sampling decode (`sample`, `rescore_sampled`) is engine_decode.py; the discriminative (enc_only) heads -- `disc_step`,
`nsp_scores` -- are engine_disc.py.
"""
import contextlib
import os
import weakref

import torch

from . import attn_maps, ops
from .config import encoder_schedule
from .engine_decode import DecodeMixin
from .engine_disc import DiscMixin, _DiscFn       # noqa: F401  (_DiscFn: importable from here as before)
from .engine_rank import RankMixin, _RankFn       # noqa: F401
from .storage import Act, Arena, FlatParams
from ._lib import GstvdError, EPI_GELU, EPI_DGELU, LN_RESID, LN_EMBED, LN_IMAGE


EARLY_WGRAD = 1     # 0 (tests / tools patch the attribute): the final grouped weight-gradient launch waits for the embedding backward

_DEVICE_STREAMS = {}


def device_streams(device):
    """ONE (vision, auxiliary) stream pair per device for every engine of the process.  torch hands out pool streams
    round-robin over 32 slots; a pair per Engine meant that after ~16 models (a test session, a checkpoint sweep) new
    engines aliased older engines' streams and the capture stream."""
    key = torch.device(device).index
    if key is None:                     # an index-less 'cuda': the CURRENT device, not device 0
        key = torch.cuda.current_device()
    if key not in _DEVICE_STREAMS:
        _DEVICE_STREAMS[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
    return _DEVICE_STREAMS[key]


class Engine(DecodeMixin, DiscMixin, RankMixin):
    def __init__(self, model):
        # weak: the model owns the engine, not the other way round -- no reference cycle, so dropping the model frees the
        # flat buffers, the arena and any captured decode sessions by reference counting, not at some later GC pass
        if hasattr(model, "decoder"):
            self._setup(weakref.ref(model), model.encoder.config, model.decoder.config, model.params)
        else:
            # encoder-only form: `model` is a VisualDialogEncoder of the enc_only arch (evaluate_disc.py); the encoder schedule
            # is the same code, what follows it is `nsp_scores` instead of VLFusion + decoder
            self._setup(weakref.ref(model), model.config, None, model.params)

    def _setup(self, model_ref, enc_cfg, dec_cfg, params):
        self._model_ref = model_ref
        self.enc_only = dec_cfg is None
        self.enc_cfg, self.dec_cfg = enc_cfg, dec_cfg
        prec = params.get("amd_precision", "bf16")
        if prec not in ("bf16", "fp32"):
            raise GstvdError("params['amd_precision'] must be 'bf16' or 'fp32'")
        self.precision = prec
        self.adt = torch.bfloat16 if prec == "bf16" else torch.float32
        self.flat = None
        self.arena = None
        self.rng = None
        self._decode_sessions = {}
        self._last_decode = None
        self._early, self._early_fused = False, ()
        self.anchor = None
        self._emb_span_ok = {}
        self._first_idx, self._seeds = {}, None
        self.pipe = None               # BackwardPipeline (pipeline.py): slice-wise wgrad / all-reduce / AdamW on the aux stream
        self.tape, self.rec = [], False
        self.accumulate, self.written = False, set()
        self._maps = None               # attn_maps.MapRequest while attention maps are being captured (attn_maps.capture)
        self._inputs_only, self._io = False, False     # inputs_only(): asked for by the caller / in force during the running replay
        self.stats = {}
        self._validate = True
        self.use_streams = bool(params.get("amd_streams", True))
        # LayerNorm folded into the Linear next to it for latency-bound row counts (the decoder: csrc/gemm_rows.hip)
        self.fuse_ln = (prec == "bf16" and bool(params.get("amd_fuse_ln", True)) and os.environ.get("GSTVD_FUSE_LN", "1") != "0")
        self.tag = "t"

    @property
    def model(self):
        m = self._model_ref()
        if m is None:
            raise GstvdError("the EncoderDecoderModel this engine belonged to is gone")
        return m

    def __deepcopy__(self, memo):
        """copy.deepcopy(model) copies the module tree; the copy's `engine` attribute must serve the COPY, not stay bound
        (through the weak reference) to the original.  The owner is already in `memo` when its attributes are copied."""
        import copy
        orig = self._model_ref()
        owner = memo.get(id(orig))
        if owner is None:
            raise GstvdError("an Engine is copied with its EncoderDecoderModel (copy.deepcopy(model)), not on its own")
        # (the owner is still being filled in at this point: take the configs / params through `memo`, which hands out the
        # very objects the copied module tree gets)
        new = Engine.__new__(Engine)
        new._setup(weakref.ref(owner), copy.deepcopy(self.enc_cfg, memo), copy.deepcopy(self.dec_cfg, memo),
                   copy.deepcopy(orig.params, memo))      # (dec_cfg is None for the encoder-only form, and stays None)
        return new

    @staticmethod
    def _fused_sampling(P, vocab):
        """The fused sampling kernel covers the reference's settings (generate.py:138-141,177-180: top_k 7, top_p 0; BERT's
        30522-token vocabulary) and, since ABI 6, any top_k and top_p; only a vocabulary beyond one CU's LDS takes the torch-op
        form of the filters, issued eagerly step by step (no captured token graph).  (Defined on Engine, not in DecodeMixin, which
        reaches it through `self`: a test swaps it on this class.)"""
        return vocab <= ops.SAMPLE_MAX_VOCAB        # (any top_k, any top_p: both filters run inside the sampling launch since ABI 6)

    def close(self):
        """Drop captured decode sessions (hipGraphs + their private pool) now."""
        self._decode_sessions.clear()

    # ------------------------------------------------------------------------------------------ setup
    def prepare(self, device):
        """(Re)build the flat storage if the module tree / device changed (e.g. after `.to(device)` or the
        embedding aliasing of train_gen.py:293) and make sure the bf16 shadow weights are current."""
        if device.type != "cuda":
            raise GstvdError("gst_visdial_amd runs on MI355X only; tensors are on %s (no CPU path)" % device)
        ops.set_device(device)
        if self.enc_only:
            topo = (id(self.model.bert_pretrained.bert.embeddings),)
        else:
            gen = self.model.decoder.decoder
            topo = (id(gen.bert.embeddings), id(self.model.encoder.bert_pretrained.bert.embeddings), id(gen.lm_head.decoder.weight))
        if self.flat is None or self.flat.topo != topo:
            self.flat = FlatParams(self.model, self.precision)
            self.flat.topo = topo
            self.flat.stale_guard = lambda: self.pipe is not None and bool(getattr(self.pipe, "master_stale", False))
        if self.flat.is_materialized() and self.flat.device != device:
            # the parameters live (as views of the flat buffer) on one device and the inputs arrive on another: a replica of
            # nn.DataParallel(model, [0, 1, ...]) (train_gen.py:295, README.md:89) -- replicas would share this one engine
            raise GstvdError(
                "inputs on %s but the model's parameters are on %s: gst_visdial_amd runs one process per GPU.  "
                "nn.DataParallel(model, [0]) is fine; for N GPUs launch N ranks (torchrun --nproc-per-node N) and attach "
                "pipeline.BackwardPipeline for the gradient all-reduce (INTEGRATION.md, 'Multi-GPU')" % (device, self.flat.device))
        if not self.flat.is_materialized():
            self.flat.materialize(device)
            self._bind_views()
            self._decode_sessions.clear()         # captured graphs address the old buffers
        if self.arena is None or self.arena.device != device:
            self._decode_sessions.clear()
            self.arena = Arena(device)
            seed = int(self.model.params.get("amd_seed", 0))
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and self.model.params.get("amd_seed_per_rank", True):
                # one mask stream per data-parallel rank, like the per-device generators of the reference's DataParallel
                # replicas (train_gen.py:295); params['amd_seed_per_rank'] = False restores one shared stream
                seed = ops.rank_seed(seed, dist.get_rank())
            self.rng = ops.Rng(device, seed=seed)
            self.anchor = torch.zeros(1, device=device, requires_grad=True)
            self.side, self.aux = device_streams(device)
            self.aux_busy = False
            self.colsums = ops.ColsumBatch(device)
            self.wgrads = ops.GemmGroup(device, a_km=True, b_km=True)
        self.flat.refresh_shadow()

    def _bind_views(self):
        f = self.flat
        wbuf = f.S if self.precision == "bf16" else f.P
        self.W, self.Pv, self.Gv = {}, {}, {}
        for name in f.slots:
            self.Pv[name] = f.view(f.P, name)
            if f.G is not None:
                self.Gv[name] = f.view(f.G, name)
            self.W[name] = f.view(wbuf, name)

    # ------------------------------------------------------------------------------------------ helpers
    def buf(self, M, N, dtype=None):
        return self.arena.alloc(M * N, dtype or self.adt, (M, N))

    def vec(self, n, dtype=torch.float32):
        return self.arena.alloc(n, dtype)

    def act(self, M, N):
        return Act(self.buf(M, N), M, N)

    def site(self, label=None, p=0.0, kind=None, shape=None, **extra):
        """Next dropout site of the step.  Sites are numbered in issue order; `site_log[label]` keeps what a checker needs to
        regenerate the site's keep mask with gstvd_dropout_mask (tests: the oracle is run with exactly these masks)."""
        self._site += 1
        if label is not None and self.train:
            if label in self.site_log:
                raise GstvdError("internal: dropout site label used twice in one step: " + label)
            self.site_log[label] = dict(site=self._site, p=float(p), kind=kind, shape=shape, **extra)
        return self._site

    def grad_slot(self, name):
        g = self.Gv[name]
        off = self.flat.slots[name][0]
        acc = self.accumulate or (off in self.written)
        self.written.add(off)
        return g, acc

    def push(self, fn):
        if self.rec:
            sc = ops.Profiler.scope
            if sc is not None and ops.Profiler.active is not None:      # instrumented step: backward inherits the block label
                def scoped(fn=fn, sc=sc):
                    prev, ops.Profiler.scope = ops.Profiler.scope, sc
                    try:
                        fn()
                    finally:
                        ops.Profiler.scope = prev
                self.tape.append((self.tag, scoped))
            else:
                self.tape.append((self.tag, fn))

    def mark(self, key):
        if self.rec and self.pipe is not None:
            off = self.flat.marks[key]
            self.tape.append(("t", lambda: self._hook(off)))

    def _hook(self, off):
        """Backward reached flat offset `off`: every gradient at offset >= off has been produced or queued."""
        if self._io:
            return
        if self.pipe is not None and self.pipe.ready(off):
            self._emit(off)

    def _early_final_wgrads(self):
        """Single-slice pipeline with the fused update (the N = 1 default): every weight-gradient GEMM of the step is queued once
        backward reaches the encoder's text embedding -- what is left is that embedding's backward (scatter-adds, 33 us), and the
        column reductions of the LayerNorm / bias gradients (47 us): inputs of the REMAINDER AdamW pass, not of the grouped
        launch.  So the grouped launch starts here on the auxiliary stream and those two run beside it instead of in front of it
        (engine.EARLY_WGRAD = 0: the launch waits for them, as in rounds 4-5a; profiles/r05_early_wgrad_ab.txt)."""
        p = self.pipe
        if self._io or not self.use_streams or p is None or p.hi is None or p.slices or p.hi != self.flat.n_live or p.fuse_handle() is None:
            return
        if any(self.wgrads.pending_into(self.Gv[n]) for n in ("emb.word", "emb.pos", "emb.tt", "emb.tte") if n in self.Gv):
            return      # a queued GEMM writes a table the embedding's backward is about to add into (tied LM head): keep the order
        self._wait_for(self.aux, self.main, self.side)
        with torch.cuda.stream(self.aux):
            self._early_fused = self.wgrads.flush(fuse=p.fuse_handle())
        self._early = True
        self.aux_busy = True

    def _flush_wgrads(self):
        """The slice's queued weight gradients: -> (fused, direct).  N = 1: one launch that also applies AdamW (`fused` offsets).
        N > 1 with a bf16 payload: the launch writes the payload itself (`direct` ranges, pipeline.bf16_target)."""
        tgt = self.pipe.bf16_target()
        if tgt is not None:
            return (), self.wgrads.flush_direct_bf16(*tgt)
        return self.wgrads.flush(fuse=self.pipe.fuse_handle()), ()

    def _emit(self, off):
        """Hand the finished slice [off, pipe.hi) to the backward pipeline on the auxiliary stream."""
        if self.pipe.segmenter is not None:
            # Segmented capture (graph.SegmentedStep: the fall-back when a whole-step capture WITH its collectives is refused): the
            # slice's collective is issued eagerly BETWEEN two captured graphs, so the capture is cut here.  A capture can only end
            # with every forked stream joined into its origin: the vision stream joins, the slice's weight gradients and column
            # reductions run on the main stream (beside the backward chain they are zero-sum anyway), run_slice cuts, and the vision
            # stream is forked into the next capture at once -- its next tape entry may come before the next recorded dependency,
            # and a launch on a stream outside the capture would run at capture time instead of being captured.
            if self.use_streams:
                self._wait("t", "v")
                if self.aux_busy:
                    self._wait_for(self.main, self.aux)
                    self.aux_busy = False
            fused, direct = self._flush_wgrads()
            self.colsums.flush()
            self.pipe.run_slice(off, self.pipe.hi, fused=fused, direct=direct)
            if self.use_streams:
                self._wait("v", "t")
            return
        self._wait_for(self.aux, *((self.main, self.side) if self.use_streams else (self.main,)))
        if off == 0 and self.use_streams:
            # the last slice, after backward's last kernel: the main stream has nothing left to do, so the slice's column
            # reductions run there, beside its grouped weight-gradient launch on the auxiliary stream (which then waits for them).
            # (Round 3 measured cutting this slice into 2-6 parts so that AdamW of part j runs beside the weight gradients of part
            # j+1, also with the weight-gradient launch confined to 160-224 CUs: 13.73-14.01 ms against 13.72 ms, resp. +0.3 ms --
            # the two full-chip kernels do not share the chip profitably; profiles/r03_chunk_sweep.txt.  Not kept.)
            with torch.cuda.stream(self.aux):
                if self._early:
                    # the grouped launch is already running (see _early_final_wgrads); a GEMM queued after it (none in this model) goes plain
                    self._early = False
                    self.wgrads.flush()
                    fused, direct = self._early_fused, ()
                else:
                    fused, direct = self._flush_wgrads()
            # (issuing these reductions from the vision stream instead does not let the grouped launch start earlier:
            # 12.30 / 12.34 vs 12.31 / 12.35 ms, tools/attic/r05_s14.sh)
            self.colsums.flush()
            self._wait_for(self.aux, self.main)
            with torch.cuda.stream(self.aux):
                self.pipe.run_slice(off, self.pipe.hi, fused=fused, direct=direct)
        else:
            with torch.cuda.stream(self.aux):
                fused, direct = self._flush_wgrads()
                self.colsums.flush()
                self.pipe.run_slice(off, self.pipe.hi, fused=fused, direct=direct)
        self.aux_busy = True

    # -- two HIP streams: the vision stream's skinny (M = B*37) kernels run beside the text stream's --------------
    class _On(object):
        def __init__(self, eng, tag):
            self.eng, self.tag, self.ctx = eng, tag, None

        def __enter__(self):
            self.prev = self.eng.tag
            self.eng.tag = self.tag
            if self.eng.use_streams and self.tag == "v":
                self.ctx = torch.cuda.stream(self.eng.side)
                self.ctx.__enter__()

        def __exit__(self, *a):
            if self.ctx is not None:
                self.ctx.__exit__(*a)
            self.eng.tag = self.prev

    def on(self, tag):
        return Engine._On(self, tag)

    def _flush_aux(self):
        """Run the queued (decoder + LM head) weight-gradient group and column reductions on a third stream so they
        overlap the encoder's backward chain; joined back before the final flush."""
        if self._io:
            return
        self._wait_for(self.aux, self.main)
        with torch.cuda.stream(self.aux):
            self.wgrads.flush()
            self.colsums.flush()
        self.aux_busy = True

    def _stream_of(self, tag):
        return self.side if tag == "v" else self.main

    @staticmethod
    def _wait_for(dst, *srcs):
        """Stream `dst` waits for everything queued so far on the streams `srcs` (one event per source, in the given order)."""
        for src in srcs:
            ev = torch.cuda.Event()
            ev.record(src)
            dst.wait_event(ev)

    def _wait(self, waiter, waitee):
        """The same by stream tag ("t" = main, "v" = vision)."""
        self._wait_for(self._stream_of(waiter), self._stream_of(waitee))

    def sync(self, waiter, waitee):
        """Forward dependency (ops on `waiter` after this point read results of `waitee`); backward mirrors it."""
        if not self.use_streams:
            return
        self._wait(waiter, waitee)
        if self.rec:
            self.tape.append(("sync", (waitee, waiter)))

    # ------------------------------------------------------------------------------------------ ops
    def lin(self, x, w, b, N, K, gelu=False, need_dx=True):
        y = self.act(x.M, N)
        if gelu:
            u = self.buf(x.M, N)
            ops.gemm(x.t, self.W[w], y.t, x.M, N, K, bias=self.Pv[b], aux=u, epi=EPI_GELU)
            y.gelu_aux = u
        else:
            ops.gemm(x.t, self.W[w], y.t, x.M, N, K, bias=self.Pv[b])
        y.prod = (x, w, K, need_dx)
        y.req = x.req
        self.push(lambda: self._lin_bwd(x, y, w, b, N, K, need_dx))
        return y

    def ln_lin(self, x, res, g, b, H, p_pre, bias_name, eps, w, wb, N, gelu=False, mark=None):
        """y = LN(drop(x) + res); out = Linear_w(y) (+ GELU): ONE launch when the rows are few enough that every launch is
        latency bound (gstvd_gemm_ln_fwd; the decoder's ln1 -> cross-attention query, ln2 -> FFN up, ln3 -> next layer's
        QKV), else the two kernels.  `mark`: a pipeline watermark that belongs between the two (the LayerNorm's parameters
        sit in the previous layer's slice of the flat buffer, the Linear's in the next one's).  Returns (y, out)."""
        M = x.M
        if not (self.fuse_ln and res is not None and ops.gemm_ln_ok(M, N, H, self.adt)):
            y = self.ln(x, res, g, b, H, p_pre, bias_name, eps)
            if mark is not None:
                self.mark(mark)
            return y, self.lin(y, w, wb, N, H, gelu=gelu)
        y, out = self.act(M, H), self.act(M, N)
        kw = dict(mode=LN_RESID, dtype=ops.dt(x.t), M=M, H=H, gamma=self.Pv[g], beta=self.Pv[b],
                  mean=self.vec(M), rstd=self.vec(M), eps=eps, x=x.t, res=res.t, y=y.t,
                  p_pre=p_pre if self.train else 0.0, site_pre=self.site(g[:-2], p_pre, "rows", (M, H)), rng=self.rng)
        aux = self.buf(M, N) if gelu else None
        ops.gemm_ln_fwd(kw, self.W[w], out.t, N, bias=self.Pv[wb], aux=aux, epi=EPI_GELU if gelu else 0)
        out.gelu_aux = aux
        out.prod = (y, w, H, True)
        y.req = out.req = x.req or res.req
        self.push(lambda: self._ln_bwd(kw, x, res, y, g, b, H, bias_name))
        if mark is not None:
            self.mark(mark)
        self.push(lambda: self._lin_bwd(y, out, w, wb, N, H, True))
        return y, out

    def _lin_bwd(self, x, y, w, b, N, K, need_dx):
        dy, M = y.g, x.M      # for a GELU output y.g already holds d(pre-activation): its producer applied gelu'
        if not self._io:
            self._lin_param_grads(x, y, w, b, N, K, dy, M)
        elif not x.req:
            return                # inputs-only replay: the weight- and bias-gradient siblings of the dgrad are dropped, and so is a dgrad nothing needs
        if need_dx and not y.dgrad_done:          # (dgrad_done: the LayerNorm behind y ran it with its own backward, _ln_bwd)
            add = x.g
            if x.g is None:
                x.g = self.buf(M, K)
            ops.gemm(dy, self.W[w], x.g, M, K, N, b_km=True, addend=add, aux=x.gelu_aux,
                     epi=EPI_DGELU if x.gelu_aux is not None else 0)

    def _lin_param_grads(self, x, y, w, b, N, K, dy, M):
        gw, acc = self.grad_slot(w)
        if not y.bias_done and self.wgrads.colsum_capable(dy):
            # the bias gradient (column sums of dY) comes out of the weight-gradient launch itself: its producer waves sum the
            # dY tiles they stage anyway
            gb, accb = self.grad_slot(b)
            self.wgrads.add(dy, x.t, gw, N, K, M, acc, colsum_out=gb, colsum_acc=accb)
        else:
            self.wgrads.add(dy, x.t, gw, N, K, M, acc)   # deferred: all weight-gradient GEMMs run as one grouped launch
            if not y.bias_done:
                gb, accb = self.grad_slot(b)
                scratch = self.vec(((M + 63) // 64) * N)
                self.colsums.add_slabs(dy, M, N, scratch, gb, accb)

    def ln(self, x, res, g, b, H, p_pre, bias_name, eps=1e-12):
        M = x.M
        y = self.act(M, H)
        kw = dict(mode=LN_RESID, dtype=ops.dt(x.t), M=M, H=H, gamma=self.Pv[g], beta=self.Pv[b],
                  mean=self.vec(M), rstd=self.vec(M), eps=eps, x=x.t, res=res.t if res is not None else None, y=y.t,
                  p_pre=p_pre if self.train else 0.0, site_pre=self.site(g[:-2], p_pre, "rows", (M, H)), rng=self.rng)
        ops.ln_fwd(**kw)
        y.req = x.req or (res is not None and res.req)
        self.push(lambda: self._ln_bwd(kw, x, res, y, g, b, H, bias_name))
        return y

    def _colsums(self, partial, nblk, H, names):
        """Queue the reduction of LN-backward partials into up to three gradient slots (None = skip)."""
        outs, accs = [], []
        for n in names:
            if n is None:
                outs.append(None); accs.append(False)
            else:
                gv, a = self.grad_slot(n)
                outs.append(gv); accs.append(a)
        self.colsums.add(partial, outs, nblk, 3 * H, H, 3, accs)

    def _ln_bwd(self, kw, x, res, y, g, b, H, bias_name):
        M = x.M
        if self._io and not (x.req or (res is not None and res.req)):
            return              # nothing below it depends on the image features
        prod = x.prod
        # (prod[0] must be a third tensor: for LN(Linear(r) + r) the input gradient of the Linear and the residual gradient are the
        # SAME tensor's gradient -- the fused launch would hand one uninitialised buffer to both its `dres` column tile and its
        # dgrad addend/C, an intra-kernel race; such a site takes the two-launch path, which accumulates correctly)
        if (self.fuse_ln and prod is not None and prod[3] and res is not None and prod[0].N == prod[2]
                and prod[0] is not res and prod[0] is not x and ops.gemm_ln_ok(M, prod[2], H, self.adt)):
            # the LayerNorm's backward and the input gradient of the Linear that produced its input, one launch
            # (gstvd_gemm_ln_bwd): dx never travels through HBM between the two, one dependent launch less per sub-layer
            xin, w, Kin, _ = prod
            R = ops.gemm_ln_rows()
            nblk = (M + R - 1) // R
            partial = self.arena.alloc(nblk * 3 * H, torch.float32)
            if res.g is not None:
                raise GstvdError("internal: residual gradient written twice")
            res.g = self.buf(M, H)
            x.g = self.buf(M, H)
            add = xin.g
            if xin.g is None:
                xin.g = self.buf(M, Kin)
            ops.gemm_ln_bwd(kw, y.g, partial, nblk, self.W[w], xin.g, Kin, dres=res.g, dx=x.g, addend=add, aux=xin.gelu_aux,
                            epi=EPI_DGELU if xin.gelu_aux is not None else 0)
            x.dgrad_done = True
            if not self._io:        # (inputs-only: the launch is kept for its dx / dres / dgrad, its parameter partials are dropped)
                self._colsums(partial, nblk, H, [g, b, bias_name])
            x.bias_done = bias_name is not None
            return
        nblk = ops.ln_bwd_blocks(M, H, LN_RESID)
        partial = self.arena.alloc(nblk * 3 * H, torch.float32)
        if res is not None:
            if res.g is not None:
                raise GstvdError("internal: residual gradient written twice")
            res.g = self.buf(M, H)
        x.g = self.buf(M, H)
        ops.ln_bwd(kw, y.g, partial, dres=res.g if res is not None else None, dx=x.g, nblk=nblk)
        if not self._io:
            self._colsums(partial, nblk, H, [g, b, bias_name])
        x.bias_done = bias_name is not None

    def embed(self, prefix, ids, segs, Bn, T, cfg, pos_offset=0, label=None, p_drop=None):
        M, H = Bn * T, cfg.hidden_size
        if p_drop is None:
            p_drop = cfg.hidden_dropout_prob
        y = self.act(M, H)
        kw = dict(mode=LN_EMBED, dtype=ops.dt(y.t), M=M, H=H, gamma=self.Pv[prefix + ".ln.w"], beta=self.Pv[prefix + ".ln.b"],
                  mean=self.vec(M), rstd=self.vec(M), eps=1e-12, y=y.t, ids=ids, segs=segs, T=T,
                  type_vocab=cfg.type_vocab_size, word=self.Pv[prefix + ".word"], pos=self.Pv[prefix + ".pos"],
                  tt=self.Pv[prefix + ".tt"], tt_ext=self.Pv[prefix + ".tte"],
                  p_post=p_drop if self.train else 0.0, site_post=self.site(label, p_drop, "rows", (M, H)), rng=self.rng,
                  pos_offset=pos_offset)
        ops.ln_fwd(**kw)
        y.req = False           # token ids and tables only
        self.push(lambda: self._embed_bwd(kw, prefix, y, M, H))
        return y

    def _embed_bwd(self, kw, prefix, y, M, H):
        if self._io:
            return              # table and LayerNorm gradients only
        tabs, fresh = [], []
        for n in (".word", ".pos", ".tt", ".tte"):
            gv, acc = self.grad_slot(prefix + n)
            if not acc:
                fresh.append(n)
            elif self.wgrads.pending_into(gv):
                # the LM head tied to this table (FlatParams aliases lm.w onto it when train_gen.py:293 was not applied) has its
                # weight-gradient GEMM queued: run the queue now, in order, WITHOUT the fused update -- the scatter-add below is a
                # second contribution to the same slot, and a GEMM launched later would overwrite it
                self.wgrads.flush()
            tabs.append(gv)
        if len(fresh) == 4:
            # the four tables are laid out back to back (FlatParams.emb; alignment gaps and the word table's row padding belong to
            # no parameter): one fill instead of four dependent ones on the backward chain
            lo = self.flat.slots[prefix + ".word"][0]
            hi = self.flat.slots[prefix + ".tte"][0] + tabs[3].numel()
            ok = self._emb_span_ok.get((prefix, lo, hi))
            if ok is None:
                # no OTHER parameter's slot may start inside the span (its finished gradient would be wiped): checked against the
                # layout itself, once per layout, instead of against a size bound with a whole padded table of slack
                mine = set(prefix + n for n in (".word", ".pos", ".tt", ".tte"))
                own = set(self.flat.slots[n][0] for n in mine)
                ok = hi >= lo and all(not (lo <= off < hi) or off in own for name, (off, _) in self.flat.slots.items() if name not in mine)
                self._emb_span_ok[(prefix, lo, hi)] = ok
            if not ok:
                raise GstvdError("internal: embedding tables are not contiguous in the flat buffer")
            self.flat.G[lo:hi].zero_()
        else:
            for n, gv in zip((".word", ".pos", ".tt", ".tte"), tabs):
                if n in fresh:
                    gv.zero_()
        nblk = ops.ln_bwd_blocks(M)
        partial = self.arena.alloc(nblk * 4 * H, torch.float32)
        ops.ln_bwd(kw, y.g, partial, dword=tabs[0], dpos=tabs[1], dtt=tabs[2], dtt_ext=tabs[3])
        gw, aw = self.grad_slot(prefix + ".ln.w")
        gb, ab = self.grad_slot(prefix + ".ln.b")
        tt = tabs[2]                                   # zeroed above unless accumulating: rows 0/1 always add
        self.colsums.add(partial, (gw, gb, tt[0]), nblk, 4 * H, H, 3, (aw, ab, True))
        if tt.shape[0] > 1:
            self.colsums.add(partial[3 * H:], (tt[1], None, None), nblk, 4 * H, H, 1, (True, False, False))

    def img_embed(self, x, loc, cfg):
        M, H = x.M, cfg.v_hidden_size
        y = self.act(M, H)
        kw = dict(mode=LN_IMAGE, dtype=ops.dt(x.t), M=M, H=H, gamma=self.Pv["vemb.ln.w"], beta=self.Pv["vemb.ln.b"],
                  mean=self.vec(M), rstd=self.vec(M), eps=1e-12, x=x.t, y=y.t, loc=loc, w_loc=self.Pv["vemb.loc.w"],
                  b_loc=self.Pv["vemb.loc.b"], p_post=cfg.hidden_dropout_prob if self.train else 0.0,
                  site_post=self.site("vemb", cfg.hidden_dropout_prob, "rows", (M, H)), rng=self.rng)
        ops.ln_fwd(**kw)
        y.req = x.req
        self.push(lambda: self._img_embed_bwd(kw, x, y, loc, M, H))
        return y

    def _img_embed_bwd(self, kw, x, y, loc, M, H):
        nblk = ops.ln_bwd_blocks(M)
        partial = self.arena.alloc(nblk * 3 * H, torch.float32)
        x.g = self.buf(M, H)
        ops.ln_bwd(kw, y.g, partial, dres=x.g)
        if self._io:
            return
        self._colsums(partial, nblk, H, ["vemb.ln.w", "vemb.ln.b", "vemb.loc.b"])
        self._colsums(partial, nblk, H, [None, None, "vemb.img.b"])
        x.bias_done = True
        gw, acc = self.grad_slot("vemb.loc.w")
        ops.locgrad(x.g, loc, M, H, gw, acc)

    def attn(self, q, k, v, Bn, nh, Lq, Lk, d, key_mask, causal, neg, p, kv_group=1, kv_bstride=0, label=None):
        (qa, qc), (ka, kc), (va, vc) = q, k, v
        Hh = nh * d
        o = self.act(Bn * Lq, Hh)
        lse = self.vec(Bn * nh * Lq)
        # text self-attention in training: forward leaves the keep bits of its dropout draws (8 KB per head) for the one-pass
        # backward, which then reads a bit instead of hashing every draw a second time
        nbits = ops.attn_keep_bits_shape(Bn, nh, Lq, Lk, d, self.adt, causal, p if (self.train and self.rec) else 0.0) if kv_group == 1 else 0
        bits = self.arena.alloc(nbits, torch.int64) if nbits else None
        a = ops.attn_desc(qa.t[:, qc:qc + Hh], ka.t[:, kc:kc + Hh], va.t[:, vc:vc + Hh], o.t, lse, key_mask, Bn, nh, Lq, Lk, d,
                          causal=causal, mask_neg=neg, drop_p=p if self.train else 0.0,
                          site=self.site(label, p, "attn", (Bn, nh, Lq, (Lk + 3) // 4 * 4), Lk=Lk), rng=self.rng,
                          kv_group=kv_group, kv_bstride=kv_bstride, drop_bits=bits)
        ops.attn_fwd(a)
        if self._maps is not None and label in self._maps.out:
            # a selected site of an attention-map request: the probabilities of the descriptor just launched, on the site's stream
            ops.attn_probs(a, self._maps.out[label], self._maps.head_mean)
            self._maps.pending.discard(label)
        o.req = qa.req or ka.req or va.req
        self.push(lambda: self._attn_bwd(a, q, k, v, o, Bn, nh, Lq, Hh))
        return o

    def _attn_bwd(self, a, q, k, v, o, Bn, nh, Lq, Hh):
        if self._io and not o.req:
            return
        gs = []
        for (act, c) in (q, k, v):
            if act.g is None:
                act.g = self.buf(act.M, act.N)
            gs.append(act.g[:, c:c + Hh])
        delta = self.vec(Bn * nh * Lq)
        if a.kv_group > 1:      # rank_step's cross-attention: the query rows of a group share K / V, whose gradients are the group's sums
            ops.attn_group_bwd(a, o.g, gs[0], gs[1], gs[2], delta)
            return
        ops.attn_bwd(a, o.g, gs[0], gs[1], gs[2], delta)

    # ------------------------------------------------------------------------------------------ blocks
    def self_block(self, p, x, Bn, L, H, nh, key_mask, pa, ph, causal=False, inter=0):
        """QKV -> attention -> output dense -> dropout -> LN(+x)   (vilbert_dialog.py:380-431).  With `inter` the FFN's first
        Linear (+ GELU) is issued with the LayerNorm (ln_lin: one launch at the vision stream's row counts, the two kernels at
        the text stream's) and (x1, a) is returned for ffn_block(..., a=a)."""
        qkv = self.lin(x, p + ".qkv.w", p + ".qkv.b", 3 * H, H)
        ctx = self.attn((qkv, 0), (qkv, H), (qkv, 2 * H), Bn, nh, L, L, H // nh, key_mask, causal, -10000.0, pa, label=p + ".attn")
        ao = self.lin(ctx, p + ".ao.w", p + ".ao.b", H, H)
        if inter:
            return self.ln_lin(ao, x, p + ".ln1.w", p + ".ln1.b", H, ph, p + ".ao.b", 1e-12, p + ".fi.w", p + ".fi.b", inter, gelu=True)
        return self.ln(ao, x, p + ".ln1.w", p + ".ln1.b", H, ph, p + ".ao.b")

    def ffn_block(self, p, x, H, inter, ph, ti=".fi", to=".fo", tl=".ln2", a=None):
        """dense+GELU -> dense -> dropout -> LN(+x)   (vilbert_dialog.py:445-462); `a`: the first Linear's output when the caller
        issued it with the LayerNorm in front (ln_lin)."""
        if a is None:
            a = self.lin(x, p + ti + ".w", p + ti + ".b", inter, H, gelu=True)
        fo = self.lin(a, p + to + ".w", p + to + ".b", H, inter)
        return self.ln(fo, x, p + tl + ".w", p + tl + ".b", H, ph, p + to + ".b")

    def conn_layer(self, p, xv, xt, Bn, R, T, I):
        """BertConnectionLayer (vilbert_dialog.py:646-773): stream 1 = vision, 2 = text; ctx1 (text queries over
        vision keys) feeds the text branch, ctx2 the vision branch."""
        c = self.enc_cfg
        H, Hv, Hb, nh = c.hidden_size, c.v_hidden_size, c.bi_hidden_size, c.bi_num_attention_heads
        d = Hb // nh
        prev_scope, ops.Profiler.scope = ops.Profiler.scope, "coattn"
        try:
            return self._conn_layer(p, xv, xt, Bn, R, T, I, c, H, Hv, Hb, nh, d)
        finally:
            ops.Profiler.scope = prev_scope

    def _conn_layer(self, p, xv, xt, Bn, R, T, I, c, H, Hv, Hb, nh, d):
        with self.on("v"):
            qkv1 = self.lin(xv, p + ".qkv1.w", p + ".qkv1.b", 3 * Hb, Hv)
        qkv2 = self.lin(xt, p + ".qkv2.w", p + ".qkv2.b", 3 * Hb, H)
        self.sync("t", "v")
        self.sync("v", "t")
        ctx1 = self.attn((qkv2, 0), (qkv1, Hb), (qkv1, 2 * Hb), Bn, nh, T, R, d, I["vmask"], False, -10000.0,
                         c.v_attention_probs_dropout_prob, label=p + ".attn1")
        with self.on("v"):
            ctx2 = self.attn((qkv1, 0), (qkv2, Hb), (qkv2, 2 * Hb), Bn, nh, R, T, d, I["tmask"], False, -10000.0,
                             c.attention_probs_dropout_prob, label=p + ".attn2")
            hv = self.lin(ctx2, p + ".d1.w", p + ".d1.b", Hv, Hb)
            av, a = self.ln_lin(hv, xv, p + ".ln1.w", p + ".ln1.b", Hv, c.v_hidden_dropout_prob, p + ".d1.b", 1e-12,
                                p + ".vfi.w", p + ".vfi.b", c.v_intermediate_size, gelu=True)
            ov = self.ffn_block(p, av, Hv, c.v_intermediate_size, c.v_hidden_dropout_prob, ".vfi", ".vfo", ".vln", a=a)
        ht = self.lin(ctx1, p + ".d2.w", p + ".d2.b", H, Hb)
        at, a = self.ln_lin(ht, xt, p + ".ln2.w", p + ".ln2.b", H, c.hidden_dropout_prob, p + ".d2.b", 1e-12,
                            p + ".tfi.w", p + ".tfi.b", c.intermediate_size, gelu=True)
        ot = self.ffn_block(p, at, H, c.intermediate_size, c.hidden_dropout_prob, ".tfi", ".tfo", ".tln", a=a)
        return ov, ot

    def encoder(self, I):
        """BertModel.forward for enc_dec (vilbert_dialog.py:1325-1407); poolers / cls heads are dead and skipped."""
        c = self.enc_cfg
        Bn, T, R = I["B"], I["T"], I["R"]
        xt = self.embed("emb", I["ids"], I["segs"], Bn, T, c, label="emb.enc")
        if self.rec and self.pipe is not None and EARLY_WGRAD:
            self.tape.append(("t", self._early_final_wgrads))       # backward: runs just before this embedding's backward
        f = Act(I["feats"], Bn * R, c.v_feature_size)
        self.sync("v", "t")                   # fork: the vision stream starts once the inputs are staged
        with self.on("v"):
            g0 = self.lin(f, "vemb.img.w", "vemb.img.b", c.v_hidden_size, c.v_feature_size, need_dx=I["feats_grad"])
            xv = self.img_embed(g0, I["loc"], c)
        I["feats_act"] = f
        for kind, i in encoder_schedule(c):
            self.mark((kind, i))
            if kind == "t":
                p = "t%d" % i
                x1, a = self.self_block(p, xt, Bn, T, c.hidden_size, c.num_attention_heads, I["tmask"],
                                        c.attention_probs_dropout_prob, c.hidden_dropout_prob, inter=c.intermediate_size)
                xt = self.ffn_block(p, x1, c.hidden_size, c.intermediate_size, c.hidden_dropout_prob, a=a)
            elif kind == "v":
                p = "v%d" % i
                with self.on("v"):
                    x1, a = self.self_block(p, xv, Bn, R, c.v_hidden_size, c.v_num_attention_heads, I["vmask"],
                                            c.v_attention_probs_dropout_prob, c.v_hidden_dropout_prob, inter=c.v_intermediate_size)
                    xv = self.ffn_block(p, x1, c.v_hidden_size, c.v_intermediate_size, c.v_hidden_dropout_prob, a=a)
            else:
                xv, xt = self.conn_layer("c%d" % i, xv, xt, Bn, R, T, I)
        self.sync("t", "v")                   # join before VLFusion
        return xt, xv

    def fusion(self, xt, xv, I):
        """VLFusion (visual_dialog_model.py:131-135): cat(fc_v(h_v), fc_l(h_t)) along the sequence, dropout 0.1."""
        c = self.enc_cfg
        Bn, T, R = I["B"], I["T"], I["R"]
        S, H, Hv = R + T, c.hidden_size, c.v_hidden_size
        self.mark("vlf")
        enc = self.act(Bn * S, H)
        p = 0.1 if self.train else 0.0
        sv, st = self.site("vlf.v", 0.1, "rows", (Bn * R, H)), self.site("vlf.l", 0.1, "rows", (Bn * T, H))
        e3 = enc.t.view(Bn, S, H)
        ops.gemm(xv.t, self.W["vlf.v.w"], e3[:, :R], R, H, Hv, bias=self.Pv["vlf.v.b"], batch=Bn, sA=R * Hv, sC=S * H,
                 lda=Hv, ldc=H, drop_p=p, site=sv, rng=self.rng)
        ops.gemm(xt.t, self.W["vlf.l.w"], e3[:, R:], T, H, H, bias=self.Pv["vlf.l.b"], batch=Bn, sA=T * H, sC=S * H,
                 lda=H, ldc=H, drop_p=p, site=st, rng=self.rng)
        self.push(lambda: self._fusion_bwd(enc, xt, xv, Bn, R, T, H, Hv, p, sv, st))
        return enc

    def _fusion_bwd(self, enc, xt, xv, Bn, R, T, H, Hv, p, sv, st):
        yv, yt = self.act(Bn * R, H), self.act(Bn * T, H)
        yv.g, yt.g = yv.t, yt.t
        ops.vl_split(enc.g, Bn, R, T, H, yv.g, yt.g, p, sv, st, self.rng)
        self._lin_bwd(xv, yv, "vlf.v.w", "vlf.v.b", H, Hv, True)
        self._lin_bwd(xt, yt, "vlf.l.w", "vlf.l.b", H, H, True)

    def _cross_kv(self, enc):
        """The cross-attention K/V projection of ALL decoder layers over the encoder states: one GEMM, [rows, 2 * L * H]."""
        c = self.dec_cfg
        return self.lin(enc, "dec.ckv.w", "dec.ckv.b", 2 * c.num_hidden_layers * c.hidden_size, c.hidden_size)

    def decoder(self, enc, I, kv=None, kv_group=1):
        """BertGenerationEncoder + HF BertEncoder (self-attn -> cross-attn -> FFN, post-LN) + LM head.
        kv_group > 1 (inference): `kv_group` consecutive decoder rows attend to the same encoder row."""
        c = self.dec_cfg
        Bn, U, S = I["B"] * kv_group, I["U"], I["R"] + I["T"]
        H, nh, L = c.hidden_size, c.num_attention_heads, c.num_hidden_layers
        d = H // nh
        eps = c.layer_norm_eps
        self.mark("dec")
        if self.rec and self.use_streams and self.pipe is None:
            self.tape.append(("t", self._flush_aux))      # backward: the decoder's gradients are complete here
        kv_on_side = kv is None and self.use_streams
        if kv_on_side:
            # the cross-attention K/V of all layers (one 4688 x 18432 x 768 GEMM, 0.19 ms; its input gradient as much) goes
            # to the side stream, idle since the encoder joined: it runs beside the decoder's embedding and the first layer's
            # self-attention sub-layer, and in backward its input gradient beside what is left of the decoder's backward
            self.sync("v", "t")
            with self.on("v"):
                kv = self._cross_kv(enc)
        elif kv is None:
            kv = self._cross_kv(enc)
        shared = self.flat.dec_emb is self.flat.enc_emb
        # the embedding MODULE's own dropout: with the shared module of train_gen.py:293 that is the ENCODER config's
        # hidden_dropout_prob (vilbert_dialog.py:321), whoever calls it (tests/golden/tiny_train_dropout.npz)
        y = self.embed("emb" if shared else "demb", I["dec_ids"], None, Bn, U, c, label="emb.dec",
                       p_drop=self.enc_cfg.hidden_dropout_prob if shared else None)
        # Each of the three LayerNorms of a layer is issued together with the Linear that reads it (ln_lin: one launch at the
        # decoder's row counts) -- ln3 with the NEXT layer's QKV projection, hence `pend`; its backward runs with the input
        # gradient of the Linear in front of it (_ln_bwd).  8 launches per layer and direction instead of 11.
        pend = None                                   # (fo, y2, prefix) of the previous layer: its ln3 is still to be issued
        for i in range(L):
            p = "d%d" % i
            if pend is None:
                self.mark(("d", i))
                qkv = self.lin(y, p + ".qkv.w", p + ".qkv.b", 3 * H, H)
            else:
                fo_, y2_, pp = pend
                y, qkv = self.ln_lin(fo_, y2_, pp + ".ln3.w", pp + ".ln3.b", H, c.hidden_dropout_prob, pp + ".fo.b", eps,
                                     p + ".qkv.w", p + ".qkv.b", 3 * H, mark=("d", i))
            ctx = self.attn((qkv, 0), (qkv, H), (qkv, 2 * H), Bn, nh, U, U, d, I["dmask"], True, -10000.0,
                            c.attention_probs_dropout_prob, label=p + ".attn")
            ao = self.lin(ctx, p + ".ao.w", p + ".ao.b", H, H)
            y1, q = self.ln_lin(ao, y, p + ".ln1.w", p + ".ln1.b", H, c.hidden_dropout_prob, p + ".ao.b", eps,
                                p + ".cq.w", p + ".cq.b", H)
            if kv_on_side and i == 0:
                self.sync("t", "v")               # the first cross-attention needs the K/V projection
            ctx = self.attn((q, 0), (kv, 2 * i * H), (kv, (2 * i + 1) * H), Bn, nh, U, S, d, I["emask"], False, -1e9,
                            c.attention_probs_dropout_prob, kv_group=kv_group, label=p + ".xattn")
            co = self.lin(ctx, p + ".co.w", p + ".co.b", H, H)
            y2, a = self.ln_lin(co, y1, p + ".ln2.w", p + ".ln2.b", H, c.hidden_dropout_prob, p + ".co.b", eps,
                                p + ".fi.w", p + ".fi.b", c.intermediate_size, gelu=True)
            fo = self.lin(a, p + ".fo.w", p + ".fo.b", H, c.intermediate_size)
            pend = (fo, y2, p)
        if pend is not None:
            fo_, y2_, pp = pend
            y = self.ln(fo_, y2_, pp + ".ln3.w", pp + ".ln3.b", H, c.hidden_dropout_prob, pp + ".fo.b", eps)
        self.mark("lm")
        logits = self.lin(y, "lm.w", "lm.b", self.flat.Vp, H)
        return y, logits

    # ------------------------------------------------------------------------------------------ step
    def _inputs(self, feats, loc, img_mask, ids, segs, att_mask, dec_ids, dec_mask):
        dev = ids.device
        Bn, T = ids.shape
        R = feats.shape[1]
        c = self.enc_cfg
        if T > c.max_position_embeddings:
            raise GstvdError("sequence length %d exceeds max_position_embeddings" % T)
        if segs is None:
            segs = torch.zeros_like(ids)
        if self._validate:   # the reference asserts on device every call (vilbert_dialog.py:339); here: first call / on request
            if int(segs.max()) >= c.type_vocab_size + 10 or int(segs.min()) < 0:
                raise GstvdError("segment id out of range")
            if int(ids.max()) >= c.vocab_size or int(ids.min()) < 0 or int(dec_ids.max()) >= c.vocab_size or int(dec_ids.min()) < 0:
                raise GstvdError("token id out of range")
            self._validate = bool(self.model.params.get("amd_validate_inputs", False))
        I = dict(B=Bn, T=T, R=R, U=dec_ids.shape[1])
        I["ids"], I["segs"] = ids.contiguous().view(-1), segs.contiguous().view(-1)
        tm = att_mask if att_mask is not None else torch.ones(Bn, T, device=dev)
        vm = img_mask if img_mask is not None else torch.ones(Bn, R, device=dev)
        I["tmask"], I["vmask"] = tm.float().contiguous(), vm.float().contiguous()
        em = self.arena.alloc(Bn * (R + T), torch.float32, (Bn, R + T))
        em[:, :R].copy_(I["vmask"])
        em[:, R:].copy_(I["tmask"])
        I["emask"] = em
        I["dmask"] = dec_mask.float().contiguous() if dec_mask is not None else None
        I["dec_ids"] = dec_ids.contiguous().view(-1)
        f2 = feats.reshape(Bn * R, feats.shape[-1])
        if self.adt == torch.float32:
            I["feats"] = f2.float().contiguous()
        else:
            fb = self.buf(Bn * R, f2.shape[1])
            ops.cast(f2.float().contiguous(), fb)
            I["feats"] = fb
        I["loc"] = loc.reshape(Bn * R, 5).float().contiguous()
        I["feats_grad"] = bool(feats.requires_grad and torch.is_grad_enabled())
        return I

    def _refuse_maps(self, what):
        if self._maps is not None:
            raise GstvdError("%s under an attention-map request: %s" % (what, attn_maps.ALLOWED))

    def _begin(self, device, record, inference=False, maps_ok=False):
        """Start of every engine call.  `inference`: dropout off whatever the module's mode (the RNG still advances with it).
        `maps_ok`: the call is one that serves an attention-map request (eval-mode forward, the encoder alone)."""
        if self._maps is not None:
            if not maps_ok:
                self._refuse_maps("this engine call")
            if self.model.training or "train" in str(self.model.params.get("mode", "")):
                self._refuse_maps("a module in training state or a 'train' mode")
            if record:
                self._refuse_maps("a forward that records its backward (wrap the call in torch.no_grad())")
            if torch.cuda.is_current_stream_capturing():
                self._refuse_maps("a stream capture (the forward of a request is issued eagerly)")
        self.prepare(device)
        self._last_decode = None          # the arena is rewound: a previous decode call's encoder states are about to be overwritten
        self.arena.reset()
        self.tape, self.rec, self.tag = [], record, "t"
        self.main = torch.cuda.current_stream()
        self._site, self.site_log = 0, {}
        training = bool(self.model.training)
        self.train = training and not inference
        if training:
            self.rng.advance()

    def _shift_labels(self, dec_ids):
        """The reference's labels=None branch (visual_dialog_decoder.py:53-57): labels are the ids shifted left; then [SEP] becomes
        [PAD] in the CALLER's `dec_ids`, in place."""
        dc = self.dec_cfg
        labels = dec_ids.new_zeros(dec_ids.shape)
        labels[:, :-1] = dec_ids[:, 1:].clone()
        dec_ids.masked_fill_(dec_ids == dc.eos_token_id, dc.pad_token_id)
        return labels

    def _ce(self, logits, labels, rows, U, mean=True):
        """Cross-entropy of the LM head's `logits` ([rows * U, Vp] Act) against `labels` [rows, U], [PAD] ignored.
        -> (loss, logits[:, :, :V], ce): `loss` is the mean over the counted tokens or the per-token losses, and like the logits a
        VIEW of the arena (rewound by the next engine call: no-grad callers copy); `ce` holds what backward / scoring read."""
        dc = self.dec_cfg
        Md, V = rows * U, dc.vocab_size
        lab = labels.contiguous().view(-1)
        row_loss, lse, stats = self.vec(Md), self.vec(Md), self.vec(4)
        ops.ce_fwd(logits.t, lab, Md, V, row_loss, lse, stats, ignore_index=dc.pad_token_id)
        ce = dict(lab=lab, row_loss=row_loss, lse=lse, stats=stats, Md=Md, V=V, pad=dc.pad_token_id)
        return (stats[2] if mean else row_loss), logits.t.view(rows, U, self.flat.Vp)[:, :, :V], ce

    def _soft_labels(self, soft, dec_ids, loss_reduction):
        """Validation of `step`'s soft labels (dec_soft_ids, dec_soft_logp, alpha, temperature), before anything is launched ->
        None or a dict with the [B * U, K] tensors on the device."""
        if soft is None or (soft[0] is None and soft[1] is None):
            return None
        sid, slp, alpha, temperature = soft
        if sid is None or slp is None:
            raise GstvdError("dec_soft_ids and dec_soft_logp go together: both or neither")
        alpha, temperature = float(alpha), float(temperature)
        if not 0.0 <= alpha <= 1.0:
            raise GstvdError("distill_alpha = %r outside [0, 1]" % alpha)
        if not (temperature > 0.0 and temperature != float("inf")):
            raise GstvdError("distill_temperature = %r must be positive and finite" % temperature)
        Bn, U = dec_ids.shape
        if sid.dim() != 3 or tuple(sid.shape[:2]) != (Bn, U) or sid.shape != slp.shape or not 1 <= sid.shape[2] <= ops.DISTILL_MAX_K:
            raise GstvdError("dec_soft_ids / dec_soft_logp must both be [B = %d, U = %d, K <= %d], got %s and %s"
                             % (Bn, U, ops.DISTILL_MAX_K, tuple(sid.shape), tuple(slp.shape)))
        if not loss_reduction:
            raise GstvdError("soft labels with loss_reduction=False: the distillation loss is the mean over the kept tokens")
        if dec_ids.is_cuda and torch.cuda.is_current_stream_capturing():
            raise GstvdError("soft labels under a stream capture: the distillation step is issued eagerly")
        dev = dec_ids.device
        K = sid.shape[2]
        return dict(ids=sid.to(device=dev, dtype=torch.int64).contiguous().view(-1, K),
                    logp=slp.to(device=dev, dtype=torch.float32).contiguous().view(-1, K), alpha=alpha, temperature=temperature)

    def _distill(self, logits, ce, soft):
        """The distillation loss behind `_ce` on the same logits (gstvd_distill_fwd) -> the mean over the kept tokens; `ce` gains
        what the backward reads."""
        Md = ce["Md"]
        row_l, row_kd, lse_tau, stats = self.vec(Md), self.vec(Md), self.vec(Md), self.vec(4)
        ops.distill_fwd(logits.t, ce["lab"], soft["ids"], soft["logp"], Md, ce["V"], soft["alpha"], soft["temperature"], ce["row_loss"],
                        row_l, row_kd, lse_tau, stats, ignore_index=ce["pad"])
        ce.update(soft=soft, lse_tau=lse_tau, row_kd=row_kd, ce_stats=ce["stats"], stats=stats, row_loss=row_l, ce_row_loss=ce["row_loss"])
        return stats[2]

    def step(self, feats, loc, img_mask, ids, segs, att_mask, dec_ids, dec_mask, labels, loss_reduction=True, soft=None, soft_top_k=None):
        """EncoderDecoderModel.forward, train/eval branch -> (loss, logits).  `soft`: None or (dec_soft_ids [B, U, K],
        dec_soft_logp [B, U, K], alpha, temperature) -- the loss is then the distillation loss ("Soft
        pseudo-labels"); only the launch that fills the logits' gradient differs in its backward.  soft_top_k = K (the teacher's side,
        without gradients): -> (loss, logits, (ids [B, U, K], logp [B, U, K], labels [B, U]))."""
        record = torch.is_grad_enabled()
        soft = self._soft_labels(soft, dec_ids, loss_reduction)
        if soft_top_k is not None and (record or soft is not None or self.model.training):
            raise GstvdError("soft_top_k is the teacher's side: eval(), torch.no_grad() and no soft labels of its own")
        self._begin(ids.device, record, maps_ok=True)
        if labels is None:
            labels = self._shift_labels(dec_ids)
        I = self._inputs(feats, loc, img_mask, ids, segs, att_mask, dec_ids, dec_mask)
        if self._inputs_only and not (record and I["feats_grad"]):
            raise GstvdError("inputs_only(): the call needs enabled gradients and enc_image_features that require grad -- "
                             "d loss / d enc_image_features is all such a backward returns")
        xt, xv = self.encoder(I)
        enc = self.fusion(xt, xv, I)
        y, logits = self.decoder(enc, I)
        loss_raw, lv, ce = self._ce(logits, labels, I["B"], I["U"], loss_reduction)
        if soft_top_k is not None:                                     # (no-grad, eval: EncoderDecoderModel.soft_labels sees to it)
            return loss_raw.clone(), lv.to(torch.float32, copy=True), self._topk_soft(logits, ce, I["B"], I["U"], soft_top_k)
        if soft is not None:
            loss_raw = self._distill(logits, ce, soft)
        st = dict(ce, I=I, logits=logits, mean=bool(loss_reduction), tape=self.tape, inputs_only=self._inputs_only)
        self.last = dict(enc_t=xt, enc_v=xv, enc=enc, dec_hidden=y, logits=logits, lse=ce["lse"], row_loss=ce["row_loss"])
        if record:
            loss = _StepFn.apply(self.anchor, feats if I["feats_grad"] else None, self, st, loss_raw)
            return loss, lv
        return loss_raw.clone(), lv.to(torch.float32, copy=True)      # copies: the arena is rewound by the next engine call

    @contextlib.contextmanager
    def inputs_only(self):
        """For one forward / backward pair of `step`: the backward returns d loss / d enc_image_features and NOTHING else.  The
        tape keeps every launch that gradient depends on -- the same dgrad GEMMs, LayerNorm and attention backwards with the same
        operands, so the result is bit-identical to the full replay's -- and drops their siblings: weight gradients, bias and
        LayerNorm column sums, the embedding scatters, the location-projection gradient, and the backward of every activation
        that does not depend on the image features (Act.req: the text stream below the first connection layer, the decoder's
        embedding and its first self-attention sub-layer).  `p.grad`, the flat gradient buffer, `written` / `accumulate` and an
        attached BackwardPipeline are not touched.  What it is for: the FGSM attack of evaluate_gen_attack.py:101-131
        (attack.fgsm_features), which discards every parameter gradient."""
        prev, self._inputs_only = self._inputs_only, True
        try:
            yield self
        finally:
            self._inputs_only = prev

    def backward(self, st, gloss):
        """Replay the tape: fills the flat gradient buffer, assigns `.grad` views, returns d loss / d image features.
        `gloss`: the upstream gradient of the mean loss ([] / [1]) or, after loss_reduction=False, of the per-token losses
        ([B * U] or [B, U]; evaluate_gen_attack.py:126-130 arrives here as relevance[b] / U on every token of row b)."""
        flat = self.flat
        self._io = bool(st.get("inputs_only", False))       # as recorded by the forward, wherever backward() is called from
        try:
            if not self._io:
                self._backward_begin()
            logits = st["logits"]
            logits.g = self.buf(st["Md"], flat.Vp)
            if st.get("soft") is not None:
                gs = gloss.reshape(1).float().contiguous() if gloss is not None else None
                so = st["soft"]
                ops.distill_bwd(logits.t, st["lab"], so["ids"], so["logp"], st["lse"], st["lse_tau"], st["stats"], gs, st["Md"], st["V"],
                                so["alpha"], so["temperature"], logits.g, ignore_index=st["pad"])
            elif st["mean"]:
                gs = gloss.reshape(1).float().contiguous() if gloss is not None else None
                ops.ce_bwd(logits.t, st["lab"], st["lse"], st["stats"], gs, True, st["Md"], st["V"], logits.g, ignore_index=st["pad"])
            else:
                if gloss is None or gloss.numel() != st["Md"]:
                    raise GstvdError("backward of the per-token losses needs an upstream gradient of %d elements" % st["Md"])
                g = gloss.reshape(-1).to(device=logits.t.device, dtype=torch.float32).contiguous()
                ops.ce_bwd_rows(logits.t, st["lab"], st["lse"], g, st["Md"], st["V"], logits.g, ignore_index=st["pad"])
            return self._replay(st)
        finally:
            self._io = False

    def _backward_begin(self):
        """Start of every backward: gradient accumulation state (an optimizer that kept `.grad`), the deferred launches."""
        flat = self.flat
        have = [p.grad is not None for p in flat.live]
        self.accumulate = any(have)
        if self.accumulate:
            for p, gv in zip(flat.live, flat.grad_views):
                if p.grad is None:
                    gv.zero_()
                elif p.grad.data_ptr() != gv.data_ptr():
                    gv.copy_(p.grad)
        self.written = set()
        self._early = False
        self.colsums.reset()
        self.wgrads.reset()

    def _replay(self, st):
        """The tape in reverse on the two streams, the deferred weight-gradient / column-sum launches, the `.grad` views;
        -> d loss / d image features (or None).  Shared by the enc_dec step and the discriminative step."""
        flat = self.flat
        io = self._io
        self.main, self.tag = torch.cuda.current_stream(), "t"
        if self.pipe is not None and not io:
            self.pipe.begin()
        for tag, fn in reversed(st["tape"]):
            if tag == "sync":
                self._wait(*fn)
            elif tag == "v" and self.use_streams:
                with torch.cuda.stream(self.side):
                    fn()
            else:
                fn()
        if self.use_streams:
            self._wait("t", "v")
        if io:
            return self._feats_grad(st)         # no parameter gradient was queued or written: nothing to flush, `.grad` stays
        if self.pipe is not None:
            if self.pipe.hi > 0:
                self._emit(0)
            tail = self.pipe.end()
            if tail is not None:                       # communication stream (all-reduce + AdamW of the slices): join it here
                self.main.wait_event(tail)
        if self.aux_busy:
            self._wait_for(self.main, self.aux)
            self.aux_busy = False
        self.wgrads.flush()
        self.colsums.flush()
        stale = self.pipe.stale_grad_offsets() if self.pipe is not None else ()
        if stale:
            # the weight-gradient launch updated these weights in its epilogue and never stored dW: `.grad` stays None (a view
            # of the flat buffer would show an older step's bytes to gradient clipping / logging, and the next backward would
            # accumulate onto them); BackwardPipeline(keep_grads=True) materialises them
            for (p, off), gv in zip(flat.items, flat.grad_views):
                p.grad = None if off in stale else gv
        else:
            for p, gv in zip(flat.live, flat.grad_views):
                p.grad = gv
        return self._feats_grad(st)

    @staticmethod
    def _feats_grad(st):
        """d loss / d image features as an fp32 tensor of its own (not a view of the arena, which the next engine call rewinds:
        autograd keeps what it is handed as the leaf's `.grad`), or None."""
        fa = st["I"].get("feats_act")
        if st["I"]["feats_grad"] and fa is not None and fa.g is not None:
            return fa.g.to(torch.float32, copy=True)
        return None

    def _fn_enter(self, ctx, feats, st):
        """forward of the autograd bridges (_StepFn, _DiscFn): what their backward needs."""
        ctx.engine, ctx.st = self, st
        ctx.feats_shape = feats.shape if feats is not None else None

    @staticmethod
    def _fn_feats_grad(ctx, dfe):
        """... and the tail of their backward: the replay's feature gradient in the shape of the caller's tensor."""
        return dfe.view(ctx.feats_shape) if ctx.feats_shape is not None and dfe is not None else dfe

    # ------------------------------------------------------------------------------------------ candidate scoring
    @torch.no_grad()
    def score_candidates(self, feats, loc, img_mask, ids, segs, att_mask, dec_ids, dec_mask, group):
        """evaluate_gen.py:45-106 without the 100x redundancy: the `group` answer candidates of a dialog round share ONE
        encoder pass and ONE cross-attention K/V projection (the reference re-encodes the identical context per candidate).
        Encoder-side tensors have E rows (one per dialog round), decoder-side tensors E*group rows ordered
        [round, candidate].  Returns score[E*group] = sum_u [tgt != 0] log softmax(logits)[u, tgt], tgt = ids shifted left;
        the decoder input is the eos->pad masked copy, as visual_dialog_decoder.py:53-57 makes it."""
        dc = self.dec_cfg
        self._refuse_maps("score_candidates")
        E, rows = ids.shape[0], dec_ids.shape[0]
        if rows != E * group:
            raise GstvdError("score_candidates: %d decoder rows for %d encoder rows x %d candidates" % (rows, E, group))
        self._begin(ids.device, False, inference=True)
        dec_in = dec_ids.masked_fill(dec_ids == dc.eos_token_id, dc.pad_token_id)
        I = self._inputs(feats, loc, img_mask, ids, segs, att_mask, dec_in, dec_mask)
        xt, xv = self.encoder(I)
        enc = self.fusion(xt, xv, I)
        _, logits = self.decoder(enc, I, self._cross_kv(enc), kv_group=group)
        U = I["U"]
        tgt = dec_ids.new_zeros(dec_ids.shape)      # (not _shift_labels: the caller's `dec_ids` stays as it is, see `dec_in`)
        tgt[:, :-1] = dec_ids[:, 1:]
        ce = self._ce(logits, tgt, rows, U)[2]
        scores = torch.empty(rows, dtype=torch.float32, device=ids.device)
        ops.answer_scores(logits.t, ce["lse"], dec_ids.contiguous(), rows, U, scores)
        return scores


class _StepFn(torch.autograd.Function):
    """Bridges the hand-written backward into torch.autograd so `loss.backward()` (train_gen.py:324) and
    d loss / d enc_image_features (FGSM in evaluate_gen_attack.py:101-131) keep working."""

    @staticmethod
    def forward(ctx, anchor, feats, engine, st, loss_raw):
        engine._fn_enter(ctx, feats, st)
        return loss_raw.clone()

    @staticmethod
    def backward(ctx, gloss):
        return None, ctx.engine._fn_feats_grad(ctx, ctx.engine.backward(ctx.st, gloss)), None, None, None


# ---- stand-alone encoder / decoder calls (inference plumbing; no autograd) --------------------------------
def _owner_engine(module, kind):
    eng = getattr(module, "_standalone_engine", None)
    if eng is None:
        raise GstvdError("%s.forward outside an EncoderDecoderModel is not supported by the MI355X engine; "
                         "call EncoderDecoderModel(...) (the reference scripts only ever do that)" % kind)
    return eng


def standalone_encoder_forward(module, input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask):
    eng = _owner_engine(module, "VisualDialogEncoder")
    with torch.no_grad():
        eng._begin(input_ids.device, False, maps_ok=True)
        dummy = input_ids.new_zeros(input_ids.shape[0], 1)
        I = eng._inputs(image_feat, image_loc, image_attention_mask, input_ids, token_type_ids, attention_mask, dummy, None)
        xt, xv = eng.encoder(I)
        Bn = I["B"]
        return xt.t.view(Bn, I["T"], -1).float(), xv.t.view(Bn, I["R"], -1).float()


def standalone_decoder_forward(module, dec_ids, attention_mask, enc_hidden, enc_mask, labels, loss_reduction):
    """VisualDialogDecoder.forward on caller-supplied encoder states (models/visual_dialog_decoder.py:33-86), inference
    only: the training graph lives in EncoderDecoderModel's single autograd function.  Same conventions as the reference:
    labels=None -> labels are the ids shifted left and the caller's `decoder_input_ids` has [SEP] replaced by [PAD] in place."""
    eng = _owner_engine(module, "VisualDialogDecoder")
    if torch.is_grad_enabled() and (enc_hidden.requires_grad or module.training):
        raise GstvdError("VisualDialogDecoder.forward alone is inference only on the MI355X engine (eval() + torch.no_grad()); "
                         "train through EncoderDecoderModel(...)")
    with torch.no_grad():
        eng._begin(dec_ids.device, False, inference=True)
        if labels is None:
            labels = eng._shift_labels(dec_ids)
        Bn, S, H = enc_hidden.shape
        U = dec_ids.shape[1]
        if H != eng.dec_cfg.hidden_size:
            raise GstvdError("encoder_hidden_states width %d != decoder hidden size %d" % (H, eng.dec_cfg.hidden_size))
        enc = eng.act(Bn * S, H)
        enc.t.copy_(enc_hidden.reshape(Bn * S, H))
        em = enc_mask if enc_mask is not None else torch.ones(Bn, S, device=dec_ids.device)
        dm = attention_mask if attention_mask is not None else torch.ones(Bn, U, device=dec_ids.device)
        I = dict(B=Bn, T=S, R=0, U=U, emask=em.float().contiguous(), dmask=dm.float().contiguous(),
                 dec_ids=dec_ids.contiguous().view(-1))
        y, logits = eng.decoder(enc, I)
        loss, lv, _ = eng._ce(logits, labels, Bn, U, loss_reduction)
        return loss.clone(), lv.float()


def encoder_attention_maps(eng, input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask, select, heads):
    """VisualDialogEncoder.attention_maps on engine `eng` (the module's own encoder-only engine, or the engine of the
    EncoderDecoderModel it belongs to): the two-stream encoder alone, eagerly, with the selected maps -> attn_maps.AttentionMaps."""
    layers = attn_maps.parse_select(select, attn_maps.layer_counts(eng.enc_cfg), attn_maps.ENCODER_KINDS)
    req = attn_maps.MapRequest(layers, attn_maps.parse_heads(heads))
    req.alloc(eng.enc_cfg, None, input_ids.shape[0], input_ids.shape[1], image_feat.shape[1], 0, input_ids.device)
    with torch.no_grad(), attn_maps.capture(eng, req):
        eng._begin(input_ids.device, False, inference=True, maps_ok=True)
        dummy = input_ids.new_zeros(input_ids.shape[0], 1)
        I = eng._inputs(image_feat, image_loc, image_attention_mask, input_ids, token_type_ids, attention_mask, dummy, None)
        eng.encoder(I)                    # (its join before VLFusion orders the vision stream's map writes behind the caller's stream)
    req.check_complete()
    return req.encoder_maps()


def model_attention_maps(eng, feats, loc, img_mask, ids, segs, att_mask, dec_ids, dec_mask, labels, loss_reduction, select, heads):
    """EncoderDecoderModel.attention_maps: the eval-mode teacher-forced forward, eagerly, with the selected maps ->
    ((loss, logits), attn_maps.ModelAttentionMaps)."""
    layers = attn_maps.parse_select(select, attn_maps.layer_counts(eng.enc_cfg, eng.dec_cfg))
    req = attn_maps.MapRequest(layers, attn_maps.parse_heads(heads))
    req.alloc(eng.enc_cfg, eng.dec_cfg, ids.shape[0], ids.shape[1], feats.shape[1], dec_ids.shape[1], ids.device)
    with torch.no_grad(), attn_maps.capture(eng, req):
        out = eng.step(feats, loc, img_mask, ids, segs, att_mask, dec_ids, dec_mask, labels, loss_reduction)
    req.check_complete()
    return out, req.model_maps()
