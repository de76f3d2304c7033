"""Thin tensor-level wrappers over the C ABI (include/gstvd_hip.h).

torch is used only as the owner of device memory and of the HIP stream; every function here launches
a hand-written gfx950 kernel on `torch.cuda.current_stream()` and raises if the library is missing,
a tensor is not on the GPU, or the kernel returns a non-zero status.  No fallbacks.
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import F32, BF16, EPI_BIAS, EPI_ADD, EPI_GELU, EPI_DGELU, EPI_DROPOUT, LN_RESID, LN_EMBED, LN_IMAGE  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt(t):
    return _DT[t.dtype]


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise L.GstvdError("gst_visdial_amd ops need GPU tensors (got %s); there is no CPU path" % t.device)
    return t.data_ptr()


# The handle of the current HIP stream is needed by every library call (~330 per eagerly issued step).  The public route --
# torch.cuda.current_stream().cuda_stream -- builds a Stream object and resolves the device index through four Python layers:
# 2.55 us per call, 0.85 ms of host time per step (tools/host_profile.py, profiles/r06_host_profile.txt).  torch's own raw
# accessor returns the same handle in ~0.2 us; the engine tells this module which device it drives (one per process).
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_DEV_INDEX = None


def set_device(device):
    global _DEV_INDEX
    _DEV_INDEX = device.index if device.index is not None else torch.cuda.current_device()


def _stream():
    if _RAW_STREAM is not None and _DEV_INDEX is not None:
        return _RAW_STREAM(_DEV_INDEX)
    return torch.cuda.current_stream().cuda_stream


class Profiler(object):
    """Optional per-launch timing with HIP events on the launch stream (bench.py's kernel breakdown).
    Off by default; `with ops.Profiler() as p:` records (tag, flops, bytes, start, end) per wrapped call."""
    active = None
    scope = None          # label the engine sets around a block (e.g. "coattn"): carried by every record made inside it

    def __init__(self):
        self.records = []

    def __enter__(self):
        Profiler.active = self
        return self

    def __exit__(self, *a):
        Profiler.active = None

    def summary(self, by_shape=False, scope=None):
        """Aggregate by tag; `scope`: only the records made inside that engine block."""
        torch.cuda.synchronize()
        agg = {}
        for tag, flops, nbytes, e0, e1, detail, sc in self.records:
            if scope is not None and sc != scope:
                continue
            if by_shape and detail is not None:
                tag = "%s %s" % (tag, "x".join(str(d) for d in detail))
            a = agg.setdefault(tag, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            a["launches"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["flops"] += flops
            a["bytes"] += nbytes
        return agg


def _prof_begin():
    if Profiler.active is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(e0, tag, flops=0.0, nbytes=0.0, detail=None):
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    Profiler.active.records.append((tag, flops, nbytes, e0, e1, detail, Profiler.scope))


_KNAME = {}


def gemm_kernel_symbol(d, splits=1):
    """(Mangled) symbol of the device kernel the library launches for descriptor `d` -- asked of the library's own dispatch
    (gstvd_gemm_kernel_name), cached by everything the dispatch looks at."""
    key = (d.M, d.N, d.K, d.batch, d.dtype_in, d.dtype_out, d.a_kmajor, d.b_kmajor, splits, d.ldc % 8, d.epilogue & ~0)
    name = _KNAME.get(key)
    if name is None:
        buf = C.create_string_buffer(512)
        L.check("gstvd_gemm_kernel_name", L.load().gstvd_gemm_kernel_name(C.byref(d), splits, buf, 512))
        name = _KNAME[key] = buf.value.decode()
    return name


def rank_seed(seed, rank):
    """Dropout seed of data-parallel rank `rank`: every nn.DataParallel replica of the reference draws its masks from its own
    device's generator (train_gen.py:295), so ranks must not share a mask stream.  Rank 0 keeps `seed`."""
    return (int(seed) + int(rank) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF


class Rng:
    """Device-resident (seed, offset) pair read by every dropout site; graph-capture safe."""

    def __init__(self, device, seed=0):
        self.state = torch.tensor([seed, 0], dtype=torch.int64, device=device)

    def advance(self):
        lib = L.load()
        L.check("gstvd_rng_advance", lib.gstvd_rng_advance(self.state.data_ptr(), _stream()))

    def ptr(self):
        return self.state.data_ptr()


def gemm(A, B, C_out, M, N, K, *, a_km=False, b_km=False, bias=None, addend=None, aux=None, epi=0,
         alpha=1.0, lda=None, ldb=None, ldc=None, ldadd=None, ldaux=None, batch=1, sA=0, sB=0, sC=0, sAdd=0, sAux=0,
         drop_p=0.0, site=0, rng=None):
    """C[M,N] = epi(alpha * A(m,k) B(n,k)); see gstvd_gemm in include/gstvd_hip.h.  Leading dimensions
    default to the tensors' row strides."""
    lib = L.load()
    d = L.GemmDesc()
    d.A, d.B, d.C = _p(A), _p(B), _p(C_out)
    d.bias, d.addend, d.aux = _p(bias), _p(addend), _p(aux)
    d.M, d.N, d.K = M, N, K
    d.lda = A.stride(-2) if lda is None else lda
    d.ldb = B.stride(-2) if ldb is None else ldb
    d.ldc = C_out.stride(-2) if ldc is None else ldc
    d.ldadd = (addend.stride(-2) if addend is not None else 0) if ldadd is None else ldadd
    d.ldaux = (aux.stride(-2) if aux is not None else 0) if ldaux is None else ldaux
    d.batch, d.sA, d.sB, d.sC, d.sAdd, d.sAux = batch, sA, sB, sC, sAdd, sAux
    d.dtype_in, d.dtype_out = dt(A), dt(C_out)
    d.a_kmajor, d.b_kmajor = int(a_km), int(b_km)
    if bias is not None:
        epi |= EPI_BIAS
    if addend is not None:
        epi |= EPI_ADD
    if drop_p > 0:
        epi |= EPI_DROPOUT
    d.epilogue = epi
    d.alpha, d.dropout_p, d.site = alpha, drop_p, site
    d.rng = rng.ptr() if (rng is not None and drop_p > 0) else None
    e0 = _prof_begin()
    splits = splitk_plan(d.dtype_in, M, N, K, batch, a_km, b_km)
    if splits > 1:
        ws = _splitk_scratch(A.device)
        L.check("gstvd_gemm_splitk", lib.gstvd_gemm_splitk(C.byref(d), splits, ws.data_ptr(), ws.numel(), _stream()))
    else:
        L.check("gstvd_gemm", lib.gstvd_gemm(C.byref(d), _stream()))
    # profiling: the record is keyed by the symbol the library really launched (one per template instantiation)
    tag = ("gemm:" + gemm_kernel_symbol(d, splits)) if e0 is not None else None
    _prof_end(e0, tag, 2.0 * M * N * K * batch,
              float(batch) * ((M * K + N * K) * A.element_size() + M * N * C_out.element_size()), (M, N, K, batch))
    return C_out


def gemv_ln(A, B, C_out, M, N, K, gamma, beta, eps, y_out=None, bias=None, addend=None, aux=None, epi=0):
    """C[M <= 16, N] = epi(LayerNorm(A[M, K]; gamma, beta, eps) . B[N, K]^T), bf16 operands (gstvd_gemv_ln): the decode step's
    LayerNorm -> Linear pairs as one launch; y_out [M, K] bf16 (optional) receives the normalised rows."""
    lib = L.load()
    d = L.GemmDesc()
    d.A, d.B, d.C = _p(A), _p(B), _p(C_out)
    d.bias, d.addend, d.aux = _p(bias), _p(addend), _p(aux)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = A.stride(-2), B.stride(-2), C_out.stride(-2)
    d.ldadd = addend.stride(-2) if addend is not None else 0
    d.ldaux = aux.stride(-2) if aux is not None else 0
    d.batch, d.dtype_in, d.dtype_out, d.alpha = 1, dt(A), dt(C_out), 1.0
    if bias is not None:
        epi |= EPI_BIAS
    if addend is not None:
        epi |= EPI_ADD
    d.epilogue = epi
    e0 = _prof_begin()
    L.check("gstvd_gemv_ln", lib.gstvd_gemv_ln(C.byref(d), _p(gamma), _p(beta), float(eps), _p(y_out),
                                              y_out.stride(-2) if y_out is not None else 0, _stream()))
    _prof_end(e0, "gemv_ln", 2.0 * M * N * K, float((M * K + N * K) * 2 + M * N * C_out.element_size()), (M, N, K, 1))
    return C_out


SPLITK = 1                  # 0: never split (the reference path of the split-K test)
_SPLITK_WS = {}


def splitk_plan(dtype_in, M, N, K, batch, a_km, b_km):
    """Number of K splits for the 64x64-tile kernel (1 = plain launch).  Skinny and deep only: the tiles must leave
    most of the 256 CUs idle and each split must still run a ring's worth of K-tiles."""
    if not SPLITK or dtype_in != BF16 or batch != 1 or (a_km and not b_km):
        return 1
    if M <= 16 and not a_km and not b_km:
        return 1                                    # the skinny kernel of csrc/gemv.hip takes it (one launch, K split over waves)
    if M >= 256 and N >= 128 and ((M + 127) // 128) * ((N + 127) // 128) >= 96:
        return 1                                    # the 128 / 256 tile kernels take it
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    nkt = (K + 63) // 64
    s = min(256 // max(tiles, 1), nkt // 10, 8)
    return s if s >= 2 else 1


def _splitk_scratch(device):
    """Per-stream split-K scratch (launches on one stream never overlap): counters + 256 tile slots, zeroed once."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = torch.zeros(4096 + 256 * 64 * 64 * 4, dtype=torch.uint8, device=device)
        _SPLITK_WS[key] = ws
    return ws


# Tile placement of the grouped launches (xcd_block_map): 3 = per-XCD queues in ROUNDS of an XCD's 32 CUs with short-K fillers
# for the fused weight-gradient + AdamW launch, plain per-XCD queues of whole units (mode 1) for the unfused launch of the N > 1
# path.  0 = the library's own chunked order (rounds 1-4; tests compare against it).  Round 5's other candidates (staggered
# lead-in, 30-tile pieces) were measured and are gone: profiles/r05_group_order_ab.txt, r05_group_rounds_ab.txt.
GROUP_ORDER = 3
N_XCD = 8
XCD_CUS = 32                                # CUs of one XCD = workgroups of the 139 KB-LDS grouped kernels it runs at a time
GROUP_ORDER_MIN_TILES = 4 * N_XCD * 32      # a few rounds of the chip at least: below that the order is moot (tests lower it)


def xcd_block_map(shapes, tile, fused_epilogue, mode=1, unit_tiles=40):
    """Placement of a grouped launch's tiles (gstvd_gemm_grouped*'s block_map_dev): -> list of tile ids, one per workgroup, -1 =
    idle; entries b, b + 8, b + 16, ... are the queue of ONE XCD (workgroups are dealt to the eight XCDs round-robin).

    Why: a 256 x 256 weight-gradient tile streams two [K, 256] operand panels (K = the batch rows: 2 MB each at K = 4096) and the
    36 tiles of a [3072, 768] problem share 15 panels between them.  They only meet in an XCD's 4 MB L2 when they run on that XCD
    AT THE SAME TIME: the ~32 tiles an XCD has in flight must belong to the same problem(s) and walk K in step.  Rounds 1-4 dealt
    chunks of 8 tiles round-robin, so an XCD's 32 tiles were four chunks from four places of a table that mixes K = 400 / 592 /
    4096 problems: equal-K tiles drifted apart within a round or two and the launch fetched its operands 3.5x (r04_pmc_traffic).
    Here: (1) a problem (or, for the few large ones, a contiguous range of <= `unit_tiles` of its tiles) is a UNIT that goes to
    one XCD whole; (2) units are sorted into classes of equal K -- equal running time -- long K first, and dealt to the XCD
    with the least work so far (LPT), so every queue is long-K units back to back, then the short ones: tiles that start
    together finish together and the next 32 start together again; (3) mode 3: the queue is cut into ROUNDS (below).
    `shapes`: [(M, N, K)] per problem in table order; tile ids follow tile_off (problem after problem)."""
    T = tile
    if mode not in (1, 3):
        raise ValueError("xcd_block_map: mode 1 (queues of whole units) or 3 (rounds with short-K fillers)")
    rounds = mode == 3
    if rounds:
        unit_tiles = min(unit_tiles, XCD_CUS - 5)    # 27: a unit must fit one round of an XCD's CUs with room for a few fillers
    units = []                                   # (K, first tile id, number of tiles)
    gid = 0
    for (M, N, K) in shapes:
        nt = ((M + T - 1) // T) * ((N + T - 1) // T)
        parts = max(1, (nt + unit_tiles - 1) // unit_tiles)
        sizes = [nt // parts + (1 if i < nt % parts else 0) for i in range(parts)]
        t0 = gid
        for n in sizes:
            units.append((K, t0, n))
            t0 += n
        gid += nt
    epi = 30.0 if fused_epilogue else 9.0        # us per tile outside the K loop (fused: 1.7 MB of optimizer state per tile)

    def cost(K, n):
        return n * (epi + 5.0 + 0.76 * ((K + 31) // 32))

    kmax = max(u[0] for u in units)
    long_u = sorted([u for u in units if 2 * u[0] > kmax], key=lambda u: (-u[0], -u[2], u[1]))
    short_u = sorted([u for u in units if 2 * u[0] <= kmax], key=lambda u: (-u[0], -u[2], u[1]))
    load = [0.0] * N_XCD
    ql, qs = [[] for _ in range(N_XCD)], [[] for _ in range(N_XCD)]
    for group, dst in ((long_u, ql), (short_u, qs)):
        for u in group:
            x = min(range(N_XCD), key=lambda i: (load[i], i))
            dst[x].append(u)
            load[x] += cost(u[0], u[2])
    queues = []
    for x in range(N_XCD):
        q = []
        if rounds and ql[x]:
            # ROUNDS (round 5, second half): an XCD runs XCD_CUS = 32 of these workgroups at a time (139 KB of LDS: one per CU), and
            # equal-K tiles that start together finish together.  With the long units simply back to back, the window of 32 running
            # tiles slides across unit boundaries: the first few tiles of a 27- or 36-tile unit run a round earlier than the rest and
            # stream their operand panels alone.  Here the long units are packed into rounds of <= 32 tiles (first fit, largest
            # first), and the CUs a round leaves over are kept busy with SHORT-K tiles -- as many as fit into a long tile's time --
            # so that the next round's long tiles find all their CUs free at the same moment.
            shorts = [t for (_, t0, n) in qs[x] for t in range(t0, t0 + n)]
            t_long = cost(ql[x][0][0], 1)
            t_short = cost(qs[x][0][0], 1) if qs[x] else t_long
            per_slot = max(1, int(t_long / t_short))
            bins = []
            for u in sorted(ql[x], key=lambda u: (-u[2], -u[0], u[1])):
                for b in bins:
                    if b[0] + u[2] <= XCD_CUS:
                        b[0] += u[2]; b[1].append(u); break
                else:
                    bins.append([u[2], [u]])
            si = 0
            for nl, us in bins:
                for (_, t0, n) in us:
                    q.extend(range(t0, t0 + n))
                nf = min((XCD_CUS - nl) * per_slot, len(shorts) - si)
                q.extend(shorts[si:si + nf])
                si += nf
            q.extend(shorts[si:])
        else:
            for (_, t0, n) in ql[x] + qs[x]:
                q.extend(range(t0, t0 + n))
        queues.append(q)
    depth = max(len(q) for q in queues)
    out = [-1] * (depth * N_XCD)
    for x, q in enumerate(queues):
        out[x:x + len(q) * N_XCD:N_XCD] = q
    return out


class GemmGroup(object):
    """Deferred GEMMs that share dtypes / operand layouts, executed as ONE grouped launch (gstvd_gemm_grouped).
    The engine queues every weight-gradient GEMM of a backward pass here.  Device tables are cached by content
    (arena addresses are static from step to step), so steady state is a single launch with no host->device copy."""

    def __init__(self, device, a_km=True, b_km=True):
        self.device, self.a_km, self.b_km = device, a_km, b_km
        self.items, self.cache, self.keep = [], {}, []
        self.dtype_in = self.dtype_out = None
        self._caps = None

    def colsum_capable(self, A):
        """True when a grouped launch of this group can also produce bias[m] = sum_k A[k][m] (GSTVD_EPI_COLSUM): bf16 operands
        (the grouped kernel), k-major A, and the library says its grouped launch honours the flag."""
        if not (self.a_km and A.dtype == torch.bfloat16):
            return False
        if self._caps is None:
            self._caps = int(L.load().gstvd_gemm_group_caps())
        return bool(self._caps & 1)

    def add(self, A, B, C_out, M, N, K, accumulate, colsum_out=None, colsum_acc=False):
        di, do = dt(A), dt(C_out)
        if self.items and (di, do) != (self.dtype_in, self.dtype_out):
            self.flush()
        self.dtype_in, self.dtype_out = di, do
        self.keep.append((A, B, C_out, colsum_out))      # keep the operands alive until the launch
        cs = (_p(colsum_out), int(bool(colsum_acc))) if colsum_out is not None else (0, 0)
        self.items.append((_p(A), _p(B), _p(C_out), M, N, K, A.stride(-2), B.stride(-2), C_out.stride(-2), int(bool(accumulate))) + cs)

    def reset(self):
        self.items, self.keep = [], []

    def pending_into(self, C_out):
        """True when a queued problem writes the block that starts at C_out's address.  A NON-GEMM writer into the same gradient
        slot (the embedding scatter-add when the LM head is tied to the decoder's own word embedding) asks this before it
        accumulates: the queued GEMM would otherwise run later and overwrite what was added."""
        ptr = _p(C_out)
        return any(it[2] == ptr for it in self.items)

    @staticmethod
    def _overlapping(items):
        """Indices of queued problems whose C block shares bytes with another queued problem's (sorted sweep over [lo, hi))."""
        spans = sorted((it[2], it[2] + 4 * ((it[3] - 1) * it[8] + it[4]), i) for i, it in enumerate(items))
        bad, reach, owner = set(), -1, -1
        for lo, hi, i in spans:
            if lo < reach:
                bad.add(i); bad.add(owner)
            if hi > reach:
                reach, owner = hi, i
        return bad

    def flush_direct_bf16(self, G, Gb):
        """The N > 1 path with a bf16 gradient payload: every queued weight gradient that is the ONLY contribution to its weight
        this step is written by the launch ITSELF in bf16 into `Gb` (the flat bf16 buffer the slice's collective sends, indexed
        like the fp32 gradient buffer `G`) instead of in fp32 into G -- the fp32 store (4 B per weight) and the cast pass that would
        read it back (4 B) never happen; the rounding is the cast's (round to nearest even of the fp32 accumulator), so the payload
        is bit-identical.  The other problems (accumulating, or sharing their block with another writer: the tied LM head) stay
        fp32.  Two launches instead of one.  Returns the flat (offset, numel) ranges written in bf16, sorted."""
        if not self.items or self.dtype_in != BF16 or self.dtype_out != F32 or not (self.a_km and self.b_km):
            self.flush()
            return ()
        base, nG = G.data_ptr(), G.numel()
        shared = self._overlapping(self.items)
        direct, rest, keep_d, keep_r, ranges = [], [], [], [], []
        for i, (it, kp) in enumerate(zip(self.items, self.keep)):
            (a, b, c, M, N, K, lda, ldb, ldc, acc) = it[:10]
            off = (c - base) // 4
            if acc or i in shared or ldc != N or c < base or off + M * N > nG or (c - base) % 4 or off % 8:
                rest.append(it); keep_r.append(kp)
            else:
                direct.append(it[:2] + (Gb.data_ptr() + 2 * off,) + it[3:]); keep_d.append(kp)
                ranges.append((off, M * N))
        self.items, self.keep = rest, keep_r
        self.flush()
        if direct:
            self.items, self.keep, self.dtype_out = direct, keep_d, BF16
            try:
                self.flush()
            finally:
                self.dtype_out = F32
        return tuple(sorted(ranges))

    def flush(self, fuse=None):
        """Launch the queued problems.  `fuse` (optim.FusedAdamW.fuse_handle(), single-GPU training only): every queued weight
        gradient that is the ONLY contribution to its weight this step gets GSTVD_EPI_ADAMW -- the launch updates the weight in
        its epilogue (gstvd_gemm_grouped_adamw) instead of storing dW.  Returns the flat offsets of the weights updated that way
        (a tuple, empty without fusion): the caller's remainder pass must leave them alone."""
        if not self.items:
            return ()
        keep, self.keep = self.keep, []      # released when this call returns (after the launch is enqueued)
        fused = ()
        if fuse is not None and self.dtype_in == BF16 and self.dtype_out == F32 and self.a_km and self.b_km:
            items, fl = [], []
            # a weight is updated in the launch only when this problem is the ONLY contribution to it this step: not when it
            # accumulates, and not when another queued problem (accumulating or not) writes into the same block
            shared = self._overlapping(self.items)
            for i, it in enumerate(self.items):
                (a, b, c, M, N, K, lda, ldb, ldc, acc, cs_ptr, cs_acc) = it[:12]
                hp_addr, offs = (0, ()) if (acc or i in shared) else fuse.cover(c, M, N, ldc)
                fl.extend(offs)
                items.append(it[:12] + (hp_addr,))
            if fl:
                self.items, fused = items, tuple(fl)
            else:
                fuse = None
        else:
            fuse = None
        if self.dtype_in != BF16:            # fp32 parity mode: plain launches
            lib = L.load()
            for (a, b, c, M, N, K, lda, ldb, ldc, acc, cs_ptr, cs_acc) in [it[:12] for it in self.items]:
                if cs_ptr:
                    raise L.GstvdError("column sums ride on the grouped bf16 launch only")
                d = L.GemmDesc()
                d.A, d.B, d.C, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.batch = a, b, c, M, N, K, lda, ldb, ldc, 1
                d.dtype_in, d.dtype_out, d.a_kmajor, d.b_kmajor, d.alpha = self.dtype_in, self.dtype_out, int(self.a_km), int(self.b_km), 1.0
                if acc:
                    d.addend, d.ldadd, d.epilogue = c, ldc, EPI_ADD
                L.check("gstvd_gemm", lib.gstvd_gemm(C.byref(d), _stream()))
            self.items = []
            return ()
        key = tuple(self.items)
        hit = self.cache.get(key)
        if hit is None:
            arr = (L.GemmDesc * len(key))()
            offs, tiles, flops, nbytes = [], 0, 0.0, 0.0
            esz_in, esz_out = (2 if self.dtype_in == BF16 else 4), (2 if self.dtype_out == BF16 else 4)
            T = int(L.load().gstvd_gemm_group_tile())
            for d, it in zip(arr, key):
                (a, b, c, M, N, K, lda, ldb, ldc, acc, cs_ptr, cs_acc) = it[:12]
                d.A, d.B, d.C, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.batch = a, b, c, M, N, K, lda, ldb, ldc, 1
                d.dtype_in, d.dtype_out, d.a_kmajor, d.b_kmajor, d.alpha = self.dtype_in, self.dtype_out, int(self.a_km), int(self.b_km), 1.0
                if acc:
                    d.addend, d.ldadd, d.epilogue = c, ldc, EPI_ADD
                elif len(it) > 12 and it[12]:   # the weight's (lr, wd) pair: updated in the launch's epilogue
                    d.addend, d.epilogue = it[12], L.EPI_ADAMW
                if cs_ptr:                      # bias[m] (+)= sum_k A[k][m] out of the same launch
                    d.bias = cs_ptr
                    d.epilogue |= L.EPI_COLSUM | (L.EPI_COLSUM_ACC if cs_acc else 0)
                offs.append(tiles)
                tiles += ((M + T - 1) // T) * ((N + T - 1) // T)
                flops += 2.0 * M * N * K
                if len(it) > 12 and it[12]:
                    nbytes += esz_in * (M * K + K * N) + M * N * 26.0       # param / m / v in and out + bf16 shadow, no dW
                else:
                    nbytes += esz_in * (M * K + K * N) + esz_out * M * N * (2 if acc else 1)
            tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
            off = torch.tensor(offs, dtype=torch.int32).to(self.device)
            bmap = None
            if GROUP_ORDER and tiles >= GROUP_ORDER_MIN_TILES:
                # (rounds with fillers pay in the FUSED launch, whose tiles carry 50 us epilogues and which runs near the fabric's
                # rate: 13.50 -> 13.15 GB, -2.6 %; the plain launch of the N > 1 path is not bound by bytes and fetches less with
                # whole 36-tile units: 3.44 vs 3.86 GB stand-alone, profiles/r05_group_rounds_ab.txt)
                mode = 3 if fuse is not None else 1
                bm_host = xcd_block_map([(it[3], it[4], it[5]) for it in key], T, fuse is not None, mode)
                # the C side's contract -- every tile id exactly once, the rest idle (-1) -- is checked HERE, where the map is
                # made (once per cached table): an id out of range would compute a tile past its problem's extent
                if sorted(t for t in bm_host if t >= 0) != list(range(tiles)) or any(t < -1 for t in bm_host):
                    raise L.GstvdError("internal: block map is not a placement of the launch's %d tiles" % tiles)
                bmap = torch.tensor(bm_host, dtype=torch.int32).to(self.device)
            hit = (tab, off, len(key), tiles, flops, nbytes, bmap)
            if len(self.cache) > 64:
                self.cache.clear()
            self.cache[key] = hit
        tab, off, n, tiles, flops, nbytes, bmap = hit
        bm_ptr, bm_n = (bmap.data_ptr(), bmap.numel()) if bmap is not None else (None, 0)
        lib = L.load()
        e0 = _prof_begin()
        if fuse is not None:
            L.check("gstvd_gemm_grouped_adamw", lib.gstvd_gemm_grouped_adamw(tab.data_ptr(), off.data_ptr(), n, tiles, C.byref(fuse.desc()),
                                                                             bm_ptr, bm_n, _stream()))
            if e0 is not None:
                name = _KNAME.get("grouped_adamw")
                if name is None:
                    buf = C.create_string_buffer(512)
                    L.check("gstvd_gemm_grouped_adamw_kernel_name", lib.gstvd_gemm_grouped_adamw_kernel_name(buf, 512))
                    name = _KNAME["grouped_adamw"] = buf.value.decode()
                _prof_end(e0, "gemm:" + name, flops, nbytes, (n, tiles))
            self.items = []
            return fused
        L.check("gstvd_gemm_grouped", lib.gstvd_gemm_grouped(tab.data_ptr(), off.data_ptr(), n, tiles, self.dtype_in, self.dtype_out,
                                                             int(self.a_km), int(self.b_km), bm_ptr, bm_n, _stream()))
        if e0 is not None:
            key = ("grouped", self.dtype_in, self.dtype_out, self.a_km, self.b_km)
            name = _KNAME.get(key)
            if name is None:
                buf = C.create_string_buffer(512)
                L.check("gstvd_gemm_grouped_kernel_name", lib.gstvd_gemm_grouped_kernel_name(self.dtype_in, self.dtype_out, int(self.a_km),
                                                                                           int(self.b_km), buf, 512))
                name = _KNAME[key] = buf.value.decode()
            _prof_end(e0, "gemm:" + name, flops, nbytes, (n, tiles))
        self.items = []
        return ()


def _ln_desc(mode, dtype, M, H, gamma, beta, mean, rstd, eps, x=None, res=None, y=None, p_pre=0.0, p_post=0.0,
             site_pre=0, site_post=0, rng=None, ids=None, segs=None, T=0, type_vocab=2, word=None, pos=None, tt=None,
             tt_ext=None, loc=None, w_loc=None, b_loc=None, pos_offset=0):
    d = L.LnDesc()
    d.mode, d.dtype, d.M, d.H = mode, dtype, M, H
    d.x, d.ldx = _p(x), (x.stride(-2) if x is not None else 0)
    d.res, d.ldres = _p(res), (res.stride(-2) if res is not None else 0)
    d.gamma, d.beta, d.eps = _p(gamma), _p(beta), eps
    d.y, d.ldy = _p(y), (y.stride(-2) if y is not None else 0)
    d.mean, d.rstd = _p(mean), _p(rstd)
    d.p_pre, d.p_post, d.site_pre, d.site_post = p_pre, p_post, site_pre, site_post
    d.rng = rng.ptr() if (rng is not None and (p_pre > 0 or p_post > 0)) else None
    d.ids, d.segs, d.T, d.type_vocab = _p(ids), _p(segs), T, type_vocab
    d.word, d.pos, d.tt, d.tt_ext = _p(word), _p(pos), _p(tt), _p(tt_ext)
    d.loc, d.w_loc, d.b_loc = _p(loc), _p(w_loc), _p(b_loc)
    d.pos_offset = pos_offset
    return d


def ln_fwd(**kw):
    lib = L.load()
    d = _ln_desc(**kw)
    e0 = _prof_begin()
    L.check("gstvd_ln_fwd", lib.gstvd_ln_fwd(C.byref(d), _stream()))
    _prof_end(e0, "ln_fwd", 0.0, 3.0 * d.M * d.H * (2 if d.dtype == BF16 else 4), (d.M, d.H, d.mode))


def ln_bwd_blocks(M, H=None, mode=None):
    """Number of column-partial slabs the backward kernel writes for this geometry (size `partial` with it and pass it on)."""
    if H is None:
        return int(L.load().gstvd_ln_bwd_blocks(M))
    return int(L.load().gstvd_ln_bwd_blocks_for(M, H, mode))


def _ln_bwd_desc(fwd_kw, dy, partial, dres=None, dx=None, dword=None, dpos=None, dtt=None, dtt_ext=None, nblk=0):
    b = L.LnBwdDesc()
    b.f = _ln_desc(**fwd_kw)
    b.nblk = nblk
    b.dy, b.lddy = _p(dy), dy.stride(-2)
    b.dres, b.lddres = _p(dres), (dres.stride(-2) if dres is not None else 0)
    b.dx, b.lddx = _p(dx), (dx.stride(-2) if dx is not None else 0)
    b.partial = _p(partial)
    b.dword, b.dpos, b.dtt, b.dtt_ext = _p(dword), _p(dpos), _p(dtt), _p(dtt_ext)
    return b


def ln_bwd(fwd_kw, dy, partial, dres=None, dx=None, dword=None, dpos=None, dtt=None, dtt_ext=None, nblk=0):
    lib = L.load()
    b = _ln_bwd_desc(fwd_kw, dy, partial, dres, dx, dword, dpos, dtt, dtt_ext, nblk)
    e0 = _prof_begin()
    L.check("gstvd_ln_bwd", lib.gstvd_ln_bwd(C.byref(b), _stream()))
    _prof_end(e0, "ln_bwd", 0.0, 5.0 * b.f.M * b.f.H * (2 if b.f.dtype == BF16 else 4), (b.f.M, b.f.H, b.f.mode))


def ln_kernel_symbol(fwd_kw, bwd=None):
    """(Mangled) symbol of the device kernel ln_fwd(**fwd_kw) launches, or -- bwd: the dict of ln_bwd's other arguments -- the one
    ln_bwd(fwd_kw, **bwd) launches: asked of the library's own route decision (gstvd_ln_kernel_name), nothing is launched."""
    d = _ln_desc(**fwd_kw) if bwd is None else _ln_bwd_desc(fwd_kw, **bwd)
    buf = C.create_string_buffer(512)
    L.check("gstvd_ln_kernel_name", L.load().gstvd_ln_kernel_name(C.byref(d), int(bwd is not None), buf, 512))
    return buf.value.decode()


def colsum_partials(partial, nblk, nvec, H, out0, out1, out2, accumulate):
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_colsum_partials", lib.gstvd_colsum_partials(_p(partial), nblk, nvec, H, _p(out0), _p(out1), _p(out2),
                                                               int(accumulate), _stream()))
    _prof_end(e0, "colsum_partials", 0.0, 4.0 * nblk * nvec * H)


def colsum(x, M, N, out, scratch, accumulate):
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_colsum", lib.gstvd_colsum(_p(x), x.stride(-2), M, N, dt(x), _p(out), _p(scratch), scratch.numel(),
                                             int(accumulate), _stream()))
    _prof_end(e0, "colsum", 0.0, float(M) * N * x.element_size())


def colsum_slabs(x, M, N, scratch):
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_colsum_slabs", lib.gstvd_colsum_slabs(_p(x), x.stride(-2), M, N, dt(x), _p(scratch), scratch.numel(), _stream()))
    _prof_end(e0, "colsum_slabs", 0.0, float(M) * N * x.element_size())


class ColsumBatch(object):
    """Collects column reductions (LayerNorm-backward partials, bias-gradient slabs) and runs them in ONE launch.
    The device table is rebuilt only when the (static, arena-addressed) entry list changes."""

    def __init__(self, device):
        self.device = device
        self.entries = []            # (partial_ptr, (out0,out1,out2 ptrs), nblk, stride, H, nvec, (acc0,acc1,acc2))
        self.targets, self.keep = set(), []
        self.slabs, self.slab_dtype, self.slab_cache = [], None, {}
        self.cache = {}

    def add_slabs(self, x, M, N, scratch, out, accumulate):
        """out[c] (+)= sum_m x[m, c]: queue the 64-row slab stage and the final reduction (both batched at flush)."""
        nslab = (M + 63) // 64
        self.slabs.append((x.data_ptr(), scratch.data_ptr(), x.stride(-2), M, N))
        self.slab_dtype = dt(x)
        self.keep.append((x, scratch))
        self.add(scratch, (out, None, None), nslab, N, N, 1, (accumulate, False, False))

    def add(self, partial, outs, nblk, stride, H, nvec, accs):
        ptrs = [o.data_ptr() for o in outs if o is not None]
        if any(p in self.targets for p in ptrs):      # same output twice (shared embedding LayerNorm): keep launch order
            self.flush()
        self.keep.append((partial, outs))
        self.targets.update(ptrs)
        self.entries.append((partial.data_ptr(), tuple(o.data_ptr() if o is not None else 0 for o in outs), nblk, stride, H,
                             nvec, tuple(int(bool(a)) for a in accs)))

    def reset(self):
        self.entries, self.targets, self.keep, self.slabs = [], set(), [], []

    def _flush_slabs(self):
        key = tuple(self.slabs)
        hit = self.slab_cache.get(key)
        if hit is None:
            arr = (L.SlabEntry * len(key))()
            blk = 0
            for e, (xp, sp, ldx, M, N) in zip(arr, key):
                e.x, e.scratch, e.ldx, e.M, e.N, e.blk0 = xp, sp, ldx, M, N, blk
                blk += ((M + 63) // 64) * ((N + 255) // 256)
            hit = (torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device), len(key), blk)
            if len(self.slab_cache) > 64:
                self.slab_cache.clear()
            self.slab_cache[key] = hit
        tab, n, blocks = hit
        lib = L.load()
        e0 = _prof_begin()
        L.check("gstvd_colsum_slabs_batched", lib.gstvd_colsum_slabs_batched(tab.data_ptr(), n, blocks, self.slab_dtype, _stream()))
        _prof_end(e0, "colsum_slabs_batched", 0.0, 0.0)
        self.slabs = []

    def flush(self):
        if not self.entries:
            return
        if self.slabs:
            self._flush_slabs()
        key = tuple(self.entries)
        hit = self.cache.get(key)
        if hit is None:
            arr = (L.ColsumEntry * len(key))()
            blk = 0
            for e, (pp, outs, nblk, stride, H, nvec, accs) in zip(arr, key):
                e.partial = pp
                for j in range(3):
                    e.out[j] = outs[j] or None
                    e.accumulate[j] = accs[j]
                e.nblk, e.stride, e.H, e.nvec, e.blk0 = nblk, stride, H, nvec, blk
                blk += (nvec * H + 63) // 64
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            hit = (host.to(self.device), len(key), blk)
            if len(self.cache) > 64:
                self.cache.clear()
            self.cache[key] = hit
        tab, n, blocks = hit
        lib = L.load()
        e0 = _prof_begin()
        L.check("gstvd_colsum_batched", lib.gstvd_colsum_batched(tab.data_ptr(), n, blocks, _stream()))
        _prof_end(e0, "colsum_batched", 0.0, 0.0)
        self.entries, self.targets, self.keep = [], set(), []


def locgrad(dh, loc, M, H, dw_loc, accumulate):
    lib = L.load()
    L.check("gstvd_locgrad", lib.gstvd_locgrad(_p(dh), dh.stride(-2), _p(loc), M, H, dt(dh), _p(dw_loc), int(accumulate),
                                               _stream()))


KEEP_BITS = 1     # 0 (tests / tools patch the attribute): the backward hashes its dropout draws again (profiles/r05_attn_keep_bits_ab.txt)


def attn_keep_bits_shape(B, nh, Lq, Lk, d, dtype, causal, drop_p):
    """int64 element count of the keep-bit buffer that attn_desc(drop_bits=...) takes, or 0 when the shape's backward does not read
    one (the one-pass kernel's range: bf16, d = 64, no causal mask, 64 < keys <= 256, 64 <= queries <= 1024, dropout on)."""
    if not (KEEP_BITS and dtype == torch.bfloat16 and d == 64 and not causal and drop_p > 0 and 64 < Lk <= 256 and 64 <= Lq <= 1024):
        return 0
    return B * nh * ((Lq + 15) // 16) * ((Lk + 15) // 16) * 4


def attn_desc(Q, K, V, O, LSE, key_mask, B, nh, Lq, Lk, d, *, causal=False, mask_neg=-10000.0, scale=None, drop_p=0.0,
              site=0, rng=None, ldq=None, ldk=None, ldv=None, ldo=None, kv_group=1, q_bstride=0, kv_bstride=0, drop_bits=None):
    a = L.AttnDesc()
    a.Q, a.K, a.V, a.O, a.LSE, a.key_mask = _p(Q), _p(K), _p(V), _p(O), _p(LSE), _p(key_mask)
    a.ldq = Q.stride(-2) if ldq is None else ldq
    a.ldk = K.stride(-2) if ldk is None else ldk
    a.ldv = V.stride(-2) if ldv is None else ldv
    a.ldo = O.stride(-2) if ldo is None else ldo
    a.B, a.nh, a.Lq, a.Lk, a.d, a.causal, a.dtype = B, nh, Lq, Lk, d, int(causal), dt(Q)
    a.mask_neg = mask_neg
    a.scale = (1.0 / (d ** 0.5)) if scale is None else scale
    a.dropout_p, a.site = drop_p, site
    a.rng = rng.ptr() if (rng is not None and drop_p > 0) else None
    a.kv_group, a.q_bstride, a.kv_bstride = kv_group, q_bstride, kv_bstride
    if drop_bits is not None:
        need = B * nh * ((Lq + 15) // 16) * ((Lk + 15) // 16) * 4
        if drop_bits.dtype != torch.int64 or drop_bits.numel() < need or not drop_bits.is_contiguous():
            raise L.GstvdError("attn_desc: drop_bits must be a contiguous int64 tensor of >= %d elements" % need)
        a.drop_bits = _p(drop_bits)
    return a


def attn_kernel_symbol(a, bwd=False):
    """(Mangled) symbol of the device kernel gstvd_attn_fwd / gstvd_attn_bwd launch for descriptor `a` -- asked of the library's own
    route decision (gstvd_attn_kernel_name).  The two-part backward's answer ends in " dq_first=0" or " dq_first=1"."""
    buf = C.create_string_buffer(512)
    L.check("gstvd_attn_kernel_name", L.load().gstvd_attn_kernel_name(C.byref(a), int(bool(bwd)), buf, 512))
    return buf.value.decode()


def attn_fwd(a):
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_attn_fwd", lib.gstvd_attn_fwd(C.byref(a), _stream()))
    _prof_end(e0, "attn_fwd_d%d" % a.d, 4.0 * a.B * a.nh * a.Lq * a.Lk * a.d, 0.0, (a.B, a.nh, a.Lq, a.Lk))


def attn_probs(a, out, head_mean=False):
    """The attention map of descriptor `a` (gstvd_attn_probs): softmax(scale * Q K^T + mask) in fp32 into `out`, a contiguous
    fp32 tensor of B * nh * Lq * Lk elements, or of B * Lq * Lk with `head_mean` (the mean over the heads).  Reads Q, K and the
    key mask only; a descriptor with dropout or batch strides is refused."""
    n = a.B * (1 if head_mean else a.nh) * a.Lq * a.Lk
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n:
        raise L.GstvdError("attn_probs: `out` must be a contiguous fp32 tensor of %d elements" % n)
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_attn_probs", lib.gstvd_attn_probs(C.byref(a), _p(out), int(bool(head_mean)), _stream()))
    _prof_end(e0, "attn_probs_d%d" % a.d, 2.0 * 2.0 * a.B * a.nh * a.Lq * a.Lk * a.d, 4.0 * n, (a.B, a.nh, a.Lq, a.Lk))


def attn_bwd(a, dO, dQ, dK, dV, delta, lddo=None, lddq=None, lddk=None, lddv=None):
    lib = L.load()
    a.dO, a.dQ, a.dK, a.dV, a.delta = _p(dO), _p(dQ), _p(dK), _p(dV), _p(delta)
    a.lddo = dO.stride(-2) if lddo is None else lddo
    a.lddq = dQ.stride(-2) if lddq is None else lddq
    a.lddk = dK.stride(-2) if lddk is None else lddk
    a.lddv = dV.stride(-2) if lddv is None else lddv
    e0 = _prof_begin()
    L.check("gstvd_attn_bwd", lib.gstvd_attn_bwd(C.byref(a), _stream()))
    _prof_end(e0, "attn_bwd_d%d" % a.d, 14.0 * a.B * a.nh * a.Lq * a.Lk * a.d, 0.0, (a.B, a.nh, a.Lq, a.Lk))


def attn_group_bwd(a, dO, dQ, dK, dV, delta, lddo=None, lddq=None, lddk=None, lddv=None):
    """The backward of a grouped launch (gstvd_attn_group_bwd): `a` as attn_fwd left it with kv_group = G; dQ, delta per query
    row, dK / dV [B / G * Lk rows] written (not accumulated) as the sums over each group's query rows."""
    lib = L.load()
    a.dO, a.dQ, a.dK, a.dV, a.delta = _p(dO), _p(dQ), _p(dK), _p(dV), _p(delta)
    a.lddo = dO.stride(-2) if lddo is None else lddo
    a.lddq = dQ.stride(-2) if lddq is None else lddq
    a.lddk = dK.stride(-2) if lddk is None else lddk
    a.lddv = dV.stride(-2) if lddv is None else lddv
    e0 = _prof_begin()
    L.check("gstvd_attn_group_bwd", lib.gstvd_attn_group_bwd(C.byref(a), _stream()))
    _prof_end(e0, "attn_group_bwd_d%d" % a.d, 14.0 * a.B * a.nh * a.Lq * a.Lk * a.d, 0.0, (a.B, a.nh, a.Lq, a.Lk, a.kv_group))


def ce_fwd(logits, labels, M, V, row_loss, lse, stats, ignore_index=0):
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_ce_fwd", lib.gstvd_ce_fwd(_p(logits), logits.stride(-2), _p(labels), M, V, ignore_index, dt(logits),
                                             _p(row_loss), _p(lse), _p(stats), _stream()))
    _prof_end(e0, "ce_fwd", 0.0, float(M) * V * logits.element_size(), (M, V))


def ce_bwd(logits, labels, lse, stats, gscale, mean, M, V, dlogits, ignore_index=0):
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_ce_bwd", lib.gstvd_ce_bwd(_p(logits), logits.stride(-2), _p(labels), _p(lse), _p(stats), _p(gscale),
                                             int(mean), M, V, ignore_index, dt(logits), _p(dlogits), dlogits.stride(-2),
                                             _stream()))
    _prof_end(e0, "ce_bwd", 0.0, float(M) * V * (logits.element_size() + dlogits.element_size()), (M, V))


def ce_bwd_rows(logits, labels, lse, g, M, V, dlogits, ignore_index=0):
    """dlogits = g[row] * (softmax - onehot): the backward of the per-token losses (gstvd_ce_bwd_rows); g fp32 [M] on the device."""
    lib = L.load()
    if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != M:
        raise L.GstvdError("ce_bwd_rows: g must be a contiguous fp32 tensor of %d elements" % M)
    if dlogits.dtype != logits.dtype:
        raise L.GstvdError("ce_bwd_rows: logits and dlogits must share one dtype")
    e0 = _prof_begin()
    L.check("gstvd_ce_bwd_rows", lib.gstvd_ce_bwd_rows(_p(logits), logits.stride(-2), _p(labels), _p(lse), _p(g), M, V, ignore_index,
                                                       dt(logits), _p(dlogits), dlogits.stride(-2), _stream()))
    _prof_end(e0, "ce_bwd_rows", 0.0, float(M) * V * (logits.element_size() + dlogits.element_size()), (M, V))


DISTILL_MAX_K = 16             # entries of a soft label (gstvd_topk_logp / gstvd_distill_*)
TOPK_MAX_VOCAB = 32 * 1024     # a teacher row lives in 32 registers per thread


def _soft_pair(who, soft_ids, soft_logp, M):
    """The [M, K] soft labels of `M` logits rows, validated -> K."""
    if soft_ids.dtype != torch.int64 or soft_logp.dtype != torch.float32 or not soft_ids.is_contiguous() or not soft_logp.is_contiguous():
        raise L.GstvdError("%s: soft_ids (int64) and soft_logp (fp32) must be contiguous" % who)
    if soft_ids.dim() < 1 or soft_ids.shape != soft_logp.shape or soft_ids.numel() == 0 or soft_ids.numel() // soft_ids.shape[-1] != M:
        raise L.GstvdError("%s: soft_ids and soft_logp must both be [%d rows, K], got %s and %s"
                           % (who, M, tuple(soft_ids.shape), tuple(soft_logp.shape)))
    K = soft_ids.shape[-1]
    if not 1 <= K <= DISTILL_MAX_K:
        raise L.GstvdError("%s: K = %d outside 1..%d" % (who, K, DISTILL_MAX_K))
    return K


def _distill_scalars(who, alpha, temperature):
    alpha, temperature = float(alpha), float(temperature)
    if not 0.0 <= alpha <= 1.0:
        raise L.GstvdError("%s: alpha = %r outside [0, 1]" % (who, alpha))
    if not (temperature > 0.0 and temperature != float("inf")):
        raise L.GstvdError("%s: temperature = %r must be positive and finite" % (who, temperature))
    return alpha, 1.0 / temperature


def topk_logp(logits, lse, M, V, K, ids=None, logp=None):
    """(ids [M, K] int64, logp [M, K] fp32): the K best tokens of every row of logits [M, ld >= V] under (value descending, smaller
    id first) and their log-probabilities x[id] - lse[m] (gstvd_topk_logp); lse as ce_fwd saved it."""
    lib = L.load()
    K = int(K)
    if not 1 <= K <= DISTILL_MAX_K:
        raise L.GstvdError("topk_logp: K = %d outside 1..%d" % (K, DISTILL_MAX_K))
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() < M:
        raise L.GstvdError("topk_logp: lse must be a contiguous fp32 vector of at least %d entries" % M)
    ids = torch.empty(M, K, dtype=torch.int64, device=logits.device) if ids is None else ids
    logp = torch.empty(M, K, dtype=torch.float32, device=logits.device) if logp is None else logp
    _soft_pair("topk_logp", ids, logp, M)
    if ids.shape[-1] != K:
        raise L.GstvdError("topk_logp: outputs hold %d entries per row, K = %d" % (ids.shape[-1], K))
    e0 = _prof_begin()
    L.check("gstvd_topk_logp", lib.gstvd_topk_logp(_p(logits), logits.stride(-2), _p(lse), M, V, K, dt(logits), _p(ids), _p(logp), _stream()))
    _prof_end(e0, "topk_logp", 0.0, float(M) * V * logits.element_size(), (M, V, K))
    return ids, logp


def distill_fwd(logits, labels, soft_ids, soft_logp, M, V, alpha, temperature, ce_row_loss, row_loss, row_kd, lse_tau, stats,
                ignore_index=0):
    """The per-token loss (1 - a) * ce + a * tau^2 * KL(q || softmax(x / tau)) against the [M, K] soft labels and its stats
    (gstvd_distill_fwd), after ce_fwd on the same logits and labels (`ce_row_loss` is its row_loss)."""
    lib = L.load()
    K = _soft_pair("distill_fwd", soft_ids, soft_logp, M)
    alpha, inv_tau = _distill_scalars("distill_fwd", alpha, temperature)
    for name, t in (("ce_row_loss", ce_row_loss), ("row_loss", row_loss), ("row_kd", row_kd), ("lse_tau", lse_tau)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < M:
            raise L.GstvdError("distill_fwd: %s must be a contiguous fp32 vector of at least %d entries" % (name, M))
    e0 = _prof_begin()
    L.check("gstvd_distill_fwd", lib.gstvd_distill_fwd(_p(logits), logits.stride(-2), _p(labels), _p(soft_ids), _p(soft_logp), M, V, K,
                                                       ignore_index, alpha, inv_tau, dt(logits), _p(ce_row_loss), _p(row_loss),
                                                       _p(row_kd), _p(lse_tau), _p(stats), _stream()))
    _prof_end(e0, "distill_fwd", 0.0, float(M) * V * logits.element_size(), (M, V, K))


def distill_bwd(logits, labels, soft_ids, soft_logp, lse, lse_tau, stats, gscale, M, V, alpha, temperature, dlogits, ignore_index=0):
    """dlogits of distill_fwd's mean loss in one launch (gstvd_distill_bwd); a token without a soft label gets ce_bwd's row."""
    lib = L.load()
    K = _soft_pair("distill_bwd", soft_ids, soft_logp, M)
    alpha, inv_tau = _distill_scalars("distill_bwd", alpha, temperature)
    if dlogits.dtype != logits.dtype:
        raise L.GstvdError("distill_bwd: logits and dlogits must share one dtype")
    e0 = _prof_begin()
    L.check("gstvd_distill_bwd", lib.gstvd_distill_bwd(_p(logits), logits.stride(-2), _p(labels), _p(soft_ids), _p(soft_logp), _p(lse),
                                                       _p(lse_tau), _p(stats), _p(gscale), M, V, K, ignore_index, alpha, inv_tau,
                                                       dt(logits), _p(dlogits), dlogits.stride(-2), _stream()))
    _prof_end(e0, "distill_bwd", 0.0, float(M) * V * (logits.element_size() + dlogits.element_size()), (M, V, K))


def fgsm_step(x, g, eps, out=None):
    """out = x + eps * sign(g) over contiguous fp32 tensors of one size (gstvd_fgsm_step); `out` None: a new tensor, `out` may be x."""
    lib = L.load()
    if out is None:
        out = torch.empty_like(x)
    for t in (x, g, out):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != x.numel():
            raise L.GstvdError("fgsm_step: x, g and out must be contiguous fp32 tensors of one size")
    e0 = _prof_begin()
    L.check("gstvd_fgsm_step", lib.gstvd_fgsm_step(_p(x), _p(g), float(eps), _p(out), x.numel(), _stream()))
    _prof_end(e0, "fgsm_step", 0.0, 12.0 * x.numel(), (x.numel(),))
    return out


SAMPLE_MAX_TOP_K = 1 << 30 # (ABI 6: no limit any more -- k <= 16 walks the distinct values from the top, larger k bisects; top-p is in the kernel too)
SAMPLE_MAX_VOCAB = 31 * 1024   # a row of scaled logits lives in one CU's LDS (and 31 registers per thread)


SPECIAL_TOKEN_IDS = (0, 100, 101, 102, 103)      # utils/decoding_utils.py:38 (the default no reference caller overrides)


def _sample_desc(who, logits, temperature, top_k, u, out, banned, ngram, top_p):
    """The gstvd_sample_t of one sampling step, validated (`who` names the op in the messages)."""
    Bn, V = logits.shape
    d = L.SampleDesc()
    d.logits, d.ld, d.dtype, d.B, d.V, d.top_k, d.temperature = _p(logits), logits.stride(0), dt(logits), Bn, V, int(top_k), float(temperature)
    d.top_p = float(top_p)
    if u.dtype != torch.float32 or not u.is_contiguous() or u.numel() != Bn:
        raise L.GstvdError("%s: u must be a contiguous fp32 vector of B uniforms" % who)
    if out.dtype != torch.int64 or out.numel() != Bn or logits.stride(1) != 1:
        raise L.GstvdError("%s: out must hold B int64 ids; logits rows must be dense" % who)
    d.u, d.out, d.out_stride = _p(u), _p(out), (out.stride(0) if out.dim() else 1)
    if banned is not None:
        if banned.dtype not in (torch.bool, torch.uint8) or banned.stride(1) != 1 or banned.shape[1] < V:
            raise L.GstvdError("%s: banned must be bool / uint8 [B, >= V] with dense rows" % who)
        d.banned, d.banned_ld = _p(banned), banned.stride(0)
    if ngram is not None and int(ngram[3]) > 0:
        hist, ids_tm, cur_len, n = ngram[:4]
        special = tuple(ngram[4]) if len(ngram) > 4 else SPECIAL_TOKEN_IDS
        if hist.dtype != torch.int64 or ids_tm.dtype != torch.int64 or hist.stride(1) != 1 or ids_tm.stride(1) != 1 or hist.shape[0] != Bn:
            raise L.GstvdError("%s: hist [B, T] and ids_tm [L, B] must be int64 with dense rows" % who)
        if len(special) > 8 or ids_tm.shape[0] < cur_len:
            raise L.GstvdError("%s: at most 8 special ids; ids_tm must hold cur_len positions" % who)
        d.hist, d.hist_ld, d.hist_T, d.ngram = _p(hist), hist.stride(0), hist.shape[1], int(n)
        d.ids_tm, d.ids_stride, d.cur_len, d.n_special = _p(ids_tm), ids_tm.stride(0), int(cur_len), len(special)
        for i, t in enumerate(special):
            d.special[i] = int(t)
    return d


def sample_topk(logits, temperature, top_k, u, out, banned=None, ngram=None, top_p=0.0):
    """One sampling step (gstvd_sample_topk): out[b] <- inverse-CDF draw from softmax(top_p(top_k(logits / temperature, banned -> -inf))).
    top_p in (0, 1): nucleus filtering (utils/decoding_utils.py:22-34) inside the launch; 0 / >= 1: off.
    logits [B, V] fp32 / bf16 (row stride free); u [B] fp32 in (0, 1); out: int64 view with B elements (any stride, e.g. a
    column of the id buffer); banned: None or bool / uint8 [B, >= V].
    ngram = (hist [B, T] int64, ids_tm [L, B] int64 time-major, cur_len, n[, special ids]): the n-gram filter of
    utils/decoding_utils.py:38-77 inside the same launch (the row's last n-1 ids are ids_tm[cur_len-(n-1) : cur_len, b])."""
    lib = L.load()
    d = _sample_desc("sample_topk", logits, temperature, top_k, u, out, banned, ngram, top_p)
    L.check("gstvd_sample_topk", lib.gstvd_sample_topk(C.byref(d), _stream()))


def sample_topk_scored(logits, temperature, top_k, u, out, logp, banned=None, ngram=None, top_p=0.0):
    """`sample_topk` -- the same draw, the same ids -- and in the same launch (gstvd_sample_topk_scored) logp[b] <- the drawn id's
    log-probability under the row's RAW logits, (x[id] - max x) - log sum exp(x - max x) in fp32: temperature, bans and filters
    play no part in it (the definition `beam_step` uses).  logp: fp32 view with B elements (any positive stride, e.g. a row of a
    time-major buffer or a column), as `out` is."""
    lib = L.load()
    d = _sample_desc("sample_topk_scored", logits, temperature, top_k, u, out, banned, ngram, top_p)
    if (not isinstance(logp, torch.Tensor) or not logp.is_cuda or logp.dtype != torch.float32 or logp.dim() > 1
            or logp.numel() != logits.shape[0] or (logp.dim() == 1 and logp.numel() > 1 and logp.stride(0) < 1)):
        raise L.GstvdError("sample_topk_scored: logp must hold B fp32 values on the GPU (a vector or a strided column)")
    stride = logp.stride(0) if logp.dim() and logp.stride(0) > 0 else 1
    L.check("gstvd_sample_topk_scored", lib.gstvd_sample_topk_scored(C.byref(d), _p(logp), stride, _stream()))


def answer_scores(logits, lse, dec_ids, rows, U, scores):
    lib = L.load()
    L.check("gstvd_answer_scores", lib.gstvd_answer_scores(_p(logits), logits.stride(-2), _p(lse), _p(dec_ids), rows, U,
                                                           dt(logits), _p(scores), _stream()))


def rank_loss(logits, lse, dec_ids, relevance, E, G, U, inv_temperature, scores, p, round_loss, g_tok, stats):
    """The listwise loss head (gstvd_rank_loss): scores, p [E * G], round_loss [E], g_tok [E * G * U] and stats [3] are written,
    all contiguous fp32; g_tok is the upstream gradient ce_bwd_rows takes."""
    lib = L.load()
    for name, t, n in (("relevance", relevance, E * G), ("scores", scores, E * G), ("p", p, E * G), ("round_loss", round_loss, E),
                       ("g_tok", g_tok, E * G * U), ("stats", stats, 3), ("lse", lse, E * G * U)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise L.GstvdError("rank_loss: %s must be a contiguous fp32 tensor of %d elements" % (name, n))
    if dec_ids.dtype != torch.int64 or not dec_ids.is_contiguous() or dec_ids.numel() != E * G * U:
        raise L.GstvdError("rank_loss: dec_ids must be a contiguous int64 tensor of %d elements" % (E * G * U))
    e0 = _prof_begin()
    L.check("gstvd_rank_loss", lib.gstvd_rank_loss(_p(logits), logits.stride(-2), _p(lse), _p(dec_ids), _p(relevance), E, G, U,
                                                   float(inv_temperature), dt(logits), _p(scores), _p(p), _p(round_loss), _p(g_tok),
                                                   _p(stats), _stream()))
    _prof_end(e0, "rank_loss", 0.0, 0.0, (E, G, U))


BEAM_MAX = 8                   # beams per dialog row (gstvd_beam_step: K * K candidates fit one wave)
BEAM_MAX_LAYERS = 16           # layer pointers a gstvd_beam_reorder_t carries


def _beam_state(who, B, K, i32=(), f32=()):
    for ts, want in ((i32, torch.int32), (f32, torch.float32)):
        for t in ts:
            if not t.is_cuda:
                raise L.GstvdError("gst_visdial_amd ops need GPU tensors (got %s); there is no CPU path" % t.device)
            if t.dtype != want or t.numel() != B * K or not t.is_contiguous():
                raise L.GstvdError("%s: beam state is contiguous [B = %d, K = %d]: scores fp32, done / parent int32" % (who, B, K))


def beam_workspace(B, K, device):
    """The caller-owned workspace of `beam_step`: [B, K, K] pairs of (fp32 score, int32 token)."""
    return torch.empty(B * K * K * 2, dtype=torch.int32, device=device)


def beam_step(logits, score_in, done_in, score_out, done_out, parent, ids_tm, pos, workspace, eos, pad):
    """One beam-search step (gstvd_beam_step; the rule is stated in include/gstvd_hip.h and Engine.beam_search): logits
    [B*K, V] fp32 / bf16 (dense rows, row stride free) and the state in front of the step -- score_in fp32 [B, K], done_in int32
    [B, K] -- give the K best of every dialog row's candidates, in order: token -> ids_tm[pos, b*K + i] (the time-major int64 id
    buffer [positions, >= B*K]), parent int32 [B, K], score_out, done_out.  In and out state are different tensors; `workspace`
    from `beam_workspace`.  No host synchronisation."""
    lib = L.load()
    if score_in.dim() != 2:
        raise L.GstvdError("beam_step: score_in must be [B, K]")
    B, K = score_in.shape
    if not 1 <= K <= BEAM_MAX:
        raise L.GstvdError("beam_step: num_beams must be in 1..%d, got %d" % (BEAM_MAX, K))
    _beam_state("beam_step", B, K, i32=(done_in, done_out, parent), f32=(score_in, score_out))
    if not logits.is_cuda or logits.dim() != 2 or logits.shape[0] != B * K or logits.stride(1) != 1 or logits.dtype not in _DT:
        raise L.GstvdError("beam_step: logits must be fp32 / bf16 [B*K = %d, V] on the GPU with dense rows" % (B * K))
    V = logits.shape[1]
    if V > SAMPLE_MAX_VOCAB:
        raise L.GstvdError("beam_step: vocabulary %d exceeds the kernel's %d" % (V, SAMPLE_MAX_VOCAB))
    if (not ids_tm.is_cuda or ids_tm.dtype != torch.int64 or ids_tm.dim() != 2 or ids_tm.stride(1) != 1 or ids_tm.shape[1] < B * K
            or not 0 <= pos < ids_tm.shape[0]):
        raise L.GstvdError("beam_step: ids_tm must be int64 [positions > pos, >= B*K] time-major with dense rows")
    if score_in.data_ptr() == score_out.data_ptr() or done_in.data_ptr() == done_out.data_ptr():
        raise L.GstvdError("beam_step: in and out state must be different buffers")
    if not workspace.is_cuda or workspace.dtype != torch.int32 or workspace.numel() < 2 * B * K * K or not workspace.is_contiguous():
        raise L.GstvdError("beam_step: workspace must come from beam_workspace(B, K)")
    d = L.BeamStepDesc()
    d.logits, d.ld, d.dtype, d.B, d.K, d.V = _p(logits), logits.stride(0), dt(logits), B, K, V
    d.score_in, d.done_in, d.score_out, d.done_out, d.parent = _p(score_in), _p(done_in), _p(score_out), _p(done_out), _p(parent)
    d.ids_tm, d.ids_stride, d.positions, d.pos = _p(ids_tm), ids_tm.stride(0), ids_tm.shape[0], int(pos)
    d.workspace, d.eos, d.pad = _p(workspace), int(eos), int(pad)
    e0 = _prof_begin()
    L.check("gstvd_beam_step", lib.gstvd_beam_step(C.byref(d), _stream()))
    _prof_end(e0, "beam_step", 0.0, float(B * K * V * logits.element_size()), (B, K, V))


def beam_reorder(src, dst, parent, t, H):
    """dst[l][b*K + i, :t+1, H:3H] = src[l][b*K + parent[b, i], :t+1, H:3H] for every layer l in one launch (gstvd_beam_reorder).
    src / dst: lists (<= 16) of the per-layer fused Q|K|V caches [B*K, Umax, 3H] (contiguous, one dtype), src[l] is not dst[l];
    parent int32 [B, K].  Only the K | V columns of positions <= t are written."""
    lib = L.load()
    if parent.dim() != 2:
        raise L.GstvdError("beam_reorder: parent must be [B, K]")
    B, K = parent.shape
    _beam_state("beam_reorder", B, K, i32=(parent,))
    n = len(src)
    if not 1 <= K <= BEAM_MAX or not 1 <= n <= BEAM_MAX_LAYERS or len(dst) != n:
        raise L.GstvdError("beam_reorder: 1..%d beams and 1..%d layers, as many dst as src caches" % (BEAM_MAX, BEAM_MAX_LAYERS))
    shape, dtype = tuple(src[0].shape), src[0].dtype
    if len(shape) != 3 or shape[0] != B * K or shape[2] != 3 * H or dtype not in _DT or not 0 <= t < shape[1]:
        raise L.GstvdError("beam_reorder: caches are fp32 / bf16 [B*K = %d, Umax > t, 3H = %d], got %s" % (B * K, 3 * H, shape))
    d = L.BeamReorderDesc()
    for l in range(n):
        for c in (src[l], dst[l]):
            if not c.is_cuda or tuple(c.shape) != shape or c.dtype != dtype or not c.is_contiguous():
                raise L.GstvdError("beam_reorder: every cache must be a contiguous GPU tensor of one shape and dtype")
        if src[l].data_ptr() == dst[l].data_ptr():
            raise L.GstvdError("beam_reorder: src and dst must be two cache sets (a permutation cannot run in place)")
        d.src[l], d.dst[l] = _p(src[l]), _p(dst[l])
    d.parent, d.row_stride, d.ld = _p(parent), shape[1] * shape[2], shape[2]
    d.n_layers, d.B, d.K, d.H, d.Umax, d.t, d.dtype = n, B, K, H, shape[1], int(t), _DT[dtype]
    e0 = _prof_begin()
    L.check("gstvd_beam_reorder", lib.gstvd_beam_reorder(C.byref(d), _stream()))
    _prof_end(e0, "beam_reorder", 0.0, 2.0 * n * B * K * (t + 1) * 2 * H * src[0].element_size(), (n, B * K, t + 1, H))


def _rows_i64(who, name, t, cols=None, dtype=torch.int64):
    """A 2-D tensor of `dtype` with dense rows (row stride free) -- the layout the self-training entries take."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) \
            or (cols is not None and t.shape[1] != cols) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise L.GstvdError("%s: %s must be %s [rows, %s] with dense rows" % (who, name, str(dtype).replace("torch.", ""),
                                                                             "cols" if cols is None else cols))
    return t


def _flag_vec(who, name, t, B, dtype):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or t.numel() != B or not t.is_contiguous():
        raise L.GstvdError("%s: %s must be a contiguous %s vector of %d elements" % (who, name, str(dtype).replace("torch.", ""), B))
    return t


def context_append(ctx_ids, ctx_len, new_ids, sep_id, abnormal, full, segments=None, segment_value=0, att_mask=None, n_out=None):
    """`generate.append_to_context` for all rows in one launch, without a host synchronisation (gstvd_context_append; the rule is
    stated in include/gstvd_hip.h).  ctx_ids int64 [B, T], ctx_len int64 [B] and, when given, segments int64 [B, T] / att_mask
    fp32 [B, T] are updated in place from new_ids int64 [B, U]; a row that would overflow receives one [SEP] and abnormal[b] = 1;
    a row whose context is full already is left alone with abnormal[b] = full[b] = 1 (int32 [B]; the kernel only ever sets them:
    zero them in front of a loop, read `full` once behind it).  n_out int64 [B], when given, receives the tokens written per row."""
    who = "context_append"
    _rows_i64(who, "ctx_ids", ctx_ids)
    B, T = ctx_ids.shape
    _rows_i64(who, "new_ids", new_ids)
    if new_ids.shape[0] != B or new_ids.shape[1] < 1 or T < 1:
        raise L.GstvdError("%s: new_ids must be [B = %d, U >= 1] and T >= 1" % (who, B))
    _flag_vec(who, "ctx_len", ctx_len, B, torch.int64)
    _flag_vec(who, "abnormal", abnormal, B, torch.int32)
    _flag_vec(who, "full", full, B, torch.int32)
    if segments is not None and _rows_i64(who, "segments", segments, T).shape[0] != B:
        raise L.GstvdError("%s: segments must be [B, T]" % who)
    if att_mask is not None and _rows_i64(who, "att_mask", att_mask, T, torch.float32).shape[0] != B:
        raise L.GstvdError("%s: att_mask must be [B, T]" % who)
    if n_out is not None:
        _flag_vec(who, "n_out", n_out, B, torch.int64)
    d = L.ContextAppendDesc()
    d.ctx_ids, d.ld_ctx = _p(ctx_ids), ctx_ids.stride(0)
    d.segments, d.ld_seg = (_p(segments), segments.stride(0)) if segments is not None else (None, 0)
    d.att_mask, d.ld_att = (_p(att_mask), att_mask.stride(0)) if att_mask is not None else (None, 0)
    d.ctx_len, d.new_ids, d.ld_new = _p(ctx_len), _p(new_ids), new_ids.stride(0)
    d.B, d.T, d.U, d.sep_id, d.segment_value = B, T, new_ids.shape[1], int(sep_id), int(segment_value)
    d.n_out, d.abnormal, d.full = _p(n_out), _p(abnormal), _p(full)
    lib = L.load()
    L.check("gstvd_context_append", lib.gstvd_context_append(C.byref(d), _stream()))


DIALOG_MAX_SEP = 25            # max_sep_len of utils/data_utils.py:34 (no reference caller overrides it)
DIALOG_MAX_UTT = 64            # tokens of one utterance row the kernel's lanes cover (U, Lc)
_DIALOG_OUT = (("enc_ids", torch.int64, "T"), ("enc_seg", torch.int64, "T"), ("enc_mlm", torch.int64, "T"),
               ("enc_att", torch.float32, "T"), ("enc_sep", torch.int64, "S"), ("dec_ids", torch.int64, "Ud"),
               ("dec_labels", torch.int64, "Ud"), ("dec_att", torch.float32, "Ud"))


def dialog_rows(cap, ques, ans, ppl, T, Ud, select_data, threshold, mask_prob, valid=None, u_tok=None, cls=101, sep=102,
                mask=103, special=SPECIAL_TOKEN_IDS, S=DIALOG_MAX_SEP, out=None):
    """The student's train rows of B generated dialogs of R rounds in one launch (gstvd_dialog_rows; the rule -- the loader of
    dataloader/dataloader_cc12m_gen.py:104-248 on token ids -- is stated in include/gstvd_hip.h).
    cap int64 [B, Lc <= 64] (0-padded captions); ques, ans int64 [B, R, U <= 64] as the generation loop recorded them; ppl fp32
    [B, R]; valid int32 [B] or None (0: the dialog's labels are zeroed); u_tok fp32 [B, R, T], required when mask_prob > 0.
    Returns a dict: enc_ids, enc_seg, enc_mlm int64 [B, R, T], enc_att fp32 [B, R, T], enc_sep int64 [B, R, S], enc_hist_len int64
    [B, R], dec_ids, dec_labels int64 [B, R, Ud], dec_att fp32 [B, R, Ud].  `out`: a dict of caller-owned 2-D views [B * R, .] with
    dense rows (enc_* of one row stride, dec_* of one) and enc_hist_len [B * R] to write into instead (returned as it is)."""
    who = "dialog_rows"
    for name, t in (("ques", ques), ("ans", ans)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 3 or not t.is_contiguous():
            raise L.GstvdError("%s: %s must be a contiguous int64 [B, R, U] tensor" % (who, name))
    B, R, U = ques.shape
    T, Ud, S = int(T), int(Ud), int(S)
    if tuple(ans.shape) != (B, R, U):
        raise L.GstvdError("%s: ques and ans must share one shape [B, R, U]" % who)
    if R < 1 or 2 * R > S or 2 * R > 64:
        raise L.GstvdError("%s: %d rounds give %d separators, more than max_sep_len = %d allows (1 <= R, 2R <= S)" % (who, R, 2 * R, S))
    _rows_i64(who, "cap", cap)
    Lc = cap.shape[1]
    if cap.shape[0] != B or not 1 <= U <= DIALOG_MAX_UTT or not 1 <= Lc <= DIALOG_MAX_UTT or T < 2 or Ud < 3:
        raise L.GstvdError("%s: cap [B, Lc], 1 <= U, Lc <= %d, T >= 2 and Ud >= 3 (got U %d, Lc %d, T %d, Ud %d)"
                           % (who, DIALOG_MAX_UTT, U, Lc, T, Ud))
    if not isinstance(ppl, torch.Tensor) or ppl.dtype != torch.float32 or tuple(ppl.shape) != (B, R) or not ppl.is_contiguous():
        raise L.GstvdError("%s: ppl must be a contiguous fp32 [B, R] tensor" % who)
    if valid is not None:
        _flag_vec(who, "valid", valid, B, torch.int32)
    special = tuple(int(t) for t in special)
    if len(special) > 8:
        raise L.GstvdError("%s: at most 8 special ids" % who)
    mask_prob, threshold = float(mask_prob), float(threshold)
    if u_tok is None and mask_prob > 0.0:
        raise L.GstvdError("%s: mask_prob = %g needs u_tok, one uniform per row position [B, R, T]" % (who, mask_prob))
    if u_tok is not None and (not isinstance(u_tok, torch.Tensor) or u_tok.dtype != torch.float32 or tuple(u_tok.shape) != (B, R, T)
                              or not u_tok.is_contiguous()):
        raise L.GstvdError("%s: u_tok must be a contiguous fp32 [B, R, T = %d] tensor" % (who, T))
    dims = dict(T=T, S=S, Ud=Ud)
    if out is None:
        if not ques.is_cuda:
            _p(ques)
        o = {k: torch.empty(B * R, dims[c], dtype=dtp, device=ques.device) for k, dtp, c in _DIALOG_OUT}
        o["enc_hist_len"] = torch.empty(B * R, dtype=torch.int64, device=ques.device)
    else:
        o = out
        for k, dtp, c in _DIALOG_OUT:
            if _rows_i64(who, "out[%s]" % k, o[k], dims[c], dtp).shape[0] != B * R:
                raise L.GstvdError("%s: out[%s] must have B * R = %d rows" % (who, k, B * R))
        _flag_vec(who, "out[enc_hist_len]", o["enc_hist_len"], B * R, torch.int64)
        for grp in (("enc_ids", "enc_seg", "enc_mlm", "enc_att"), ("dec_ids", "dec_labels", "dec_att")):
            if len(set(o[k].stride(0) for k in grp)) != 1:
                raise L.GstvdError("%s: %s must share one row stride" % (who, ", ".join(grp)))
    d = L.DialogRowsDesc()
    d.cap, d.ld_cap, d.ques, d.ans, d.ld_utt = _p(cap), cap.stride(0), _p(ques), _p(ans), U
    d.ppl, d.valid, d.u_tok, d.ld_u = _p(ppl), _p(valid), _p(u_tok), T
    d.enc_ids, d.enc_seg, d.enc_mlm, d.enc_att, d.ld_enc = _p(o["enc_ids"]), _p(o["enc_seg"]), _p(o["enc_mlm"]), _p(o["enc_att"]), o["enc_ids"].stride(0)
    d.enc_sep, d.ld_sep, d.enc_hist_len = _p(o["enc_sep"]), o["enc_sep"].stride(0), _p(o["enc_hist_len"])
    d.dec_ids, d.dec_labels, d.dec_att, d.ld_dec = _p(o["dec_ids"]), _p(o["dec_labels"]), _p(o["dec_att"]), o["dec_ids"].stride(0)
    d.mask_prob, d.threshold, d.cls, d.sep, d.mask = mask_prob, threshold, int(cls), int(sep), int(mask)
    for i, t in enumerate(special):
        d.special[i] = t
    d.B, d.R, d.U, d.Lc, d.T, d.S, d.Ud, d.n_special, d.select_data = B, R, U, Lc, T, S, Ud, len(special), int(bool(select_data))
    lib = L.load()
    L.check("gstvd_dialog_rows", lib.gstvd_dialog_rows(C.byref(d), _stream()))
    if out is not None:
        return o
    res = {k: o[k].view(B, R, dims[c]) for k, _, c in _DIALOG_OUT}
    res["enc_hist_len"] = o["enc_hist_len"].view(B, R)
    return res


DISC_MAX_OPTIONS = 100         # options of a round gstvd_disc_rows covers (two ballots)
_DISC_OUT = (("tokens", torch.int64, "T"), ("segments", torch.int64, "T"), ("mask", torch.int64, "T"), ("att", torch.float32, "T"),
             ("sep_indices", torch.int64, "S"))
_DISC_VEC = (("hist_len", torch.int64, 1), ("neg_option", torch.int32, 1), ("nsp_labels", torch.float32, 2))


def disc_rows(cap, ques, ans, opts, gt_index, row_dialog, row_round, row_slot, T, tot_rounds, num_options, train, mask_prob=0.0,
              u_tok=None, u_neg=None, dense_scores=None, cls=101, sep=102, mask=103, S=DIALOG_MAX_SEP, out=None):
    """N rows of the discriminative model from token-id pools in one launch (gstvd_disc_rows; the rule -- the loader of
    dataloader/dataloader_visdial_disc.py on token ids -- is stated in include/gstvd_hip.h).
    Pools, int64 and 0-padded: cap [D, Lc <= 64] (dense rows), ques / ans [D, R, U <= 64], opts [D, R, O <= 100, U] (row stride
    free, everything else dense), gt_index [D, R]; dense_scores float64 [D, R, O] or None.  row_dialog / row_round / row_slot
    int32 [N].  `train`: False -- slot k is option k of the eval order (ground truth first); True -- slot 0 is the ground-truth
    answer, any other slot a negative drawn with u_neg fp32 [N].  u_tok fp32 [N, T] (dense rows), required when mask_prob > 0.
    Returns a dict: tokens, segments, mask int64 [N, T], att fp32 [N, T], sep_indices int64 [N, S], hist_len int64 [N], neg_option
    int32 [N] and, in train mode, nsp_labels fp32 [N, 2].  `out`: a dict of caller-owned tensors to write into instead (the four
    [N, T] arrays 2-D views of one row stride, sep_indices a 2-D view, the rest contiguous)."""
    who = "disc_rows"
    for name, t, nd in (("ques", ques, 3), ("ans", ans, 3), ("opts", opts, 4), ("gt_index", gt_index, 2)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != nd:
            raise L.GstvdError("%s: %s must be an int64 tensor of %d dimensions" % (who, name, nd))
    D, R, U = ques.shape
    O = opts.shape[2]
    T, S, train = int(T), int(S), bool(train)
    if tuple(ans.shape) != (D, R, U) or tuple(opts.shape) != (D, R, O, U) or tuple(gt_index.shape) != (D, R):
        raise L.GstvdError("%s: ques / ans [D, R, U], opts [D, R, O, U] and gt_index [D, R] do not belong together: %s %s %s %s"
                           % (who, tuple(ques.shape), tuple(ans.shape), tuple(opts.shape), tuple(gt_index.shape)))
    _rows_i64(who, "cap", cap)
    if not (ques.is_contiguous() and ans.is_contiguous() and gt_index.is_contiguous()):
        raise L.GstvdError("%s: ques, ans and gt_index must be contiguous" % who)
    so = opts.stride()
    if D * R * O > 0 and ((U > 1 and so[3] != 1) or so[2] < U or (O > 1 and so[1] != O * so[2]) or (R > 1 and so[0] != R * O * so[2])):
        raise L.GstvdError("%s: opts must have dense rows of one stride (got strides %s)" % (who, so))
    Lc = cap.shape[1]
    if cap.shape[0] != D or D < 1 or not 1 <= U <= DIALOG_MAX_UTT or not 1 <= Lc <= DIALOG_MAX_UTT or T < 2:
        raise L.GstvdError("%s: cap [D >= 1, Lc], 1 <= U, Lc <= %d and T >= 2 (got D %d, U %d, Lc %d, T %d)"
                           % (who, DIALOG_MAX_UTT, D, U, Lc, T))
    if R < 1 or 2 * R + 1 > S or S > 64:
        raise L.GstvdError("%s: %d rounds give %d separators, more than max_sep_len = %d allows (2R + 1 <= S <= 64)" % (who, R, 2 * R + 1, S))
    tot_rounds, num_options = int(tot_rounds), int(num_options)
    if not 2 <= num_options <= O <= DISC_MAX_OPTIONS or tot_rounds < 1:
        raise L.GstvdError("%s: 2 <= num_options <= O <= %d and tot_rounds >= 1 (got num_options %d, O %d, tot_rounds %d)"
                           % (who, DISC_MAX_OPTIONS, num_options, O, tot_rounds))
    if not isinstance(row_dialog, torch.Tensor) or row_dialog.dim() != 1:
        raise L.GstvdError("%s: row_dialog must be an int32 vector" % who)
    N = row_dialog.numel()
    for name, t in (("row_dialog", row_dialog), ("row_round", row_round), ("row_slot", row_slot)):
        _flag_vec(who, name, t, N, torch.int32)
    mask_prob = float(mask_prob)
    if u_tok is None and mask_prob > 0.0:
        raise L.GstvdError("%s: mask_prob = %g needs u_tok, one uniform per row position [N, T]" % (who, mask_prob))
    if u_tok is not None and _rows_i64(who, "u_tok", u_tok, T, torch.float32).shape[0] != N:
        raise L.GstvdError("%s: u_tok must be fp32 [N = %d, T = %d]" % (who, N, T))
    if train:
        if u_neg is None:
            raise L.GstvdError("%s: train mode needs u_neg, one uniform per row [N]" % who)
        _flag_vec(who, "u_neg", u_neg, N, torch.float32)
    if dense_scores is not None and (not isinstance(dense_scores, torch.Tensor) or dense_scores.dtype != torch.float64
                                     or tuple(dense_scores.shape) != (D, R, O) or not dense_scores.is_contiguous()):
        raise L.GstvdError("%s: dense_scores must be a contiguous float64 [D, R, O] tensor" % who)
    dims = dict(T=T, S=S)
    vec = [v for v in _DISC_VEC if train or v[0] != "nsp_labels"]
    if out is None:
        _p(ques)
        o = {k: torch.empty(N, dims[c], dtype=dtp, device=ques.device) for k, dtp, c in _DISC_OUT}
        for k, dtp, w in vec:
            o[k] = torch.empty((N,) if w == 1 else (N, w), dtype=dtp, device=ques.device)
    else:
        o = out
        for k, dtp, c in _DISC_OUT:
            if _rows_i64(who, "out[%s]" % k, o[k], dims[c], dtp).shape[0] != N:
                raise L.GstvdError("%s: out[%s] must have N = %d rows" % (who, k, N))
        for k, dtp, w in vec:
            t = o[k]
            if not isinstance(t, torch.Tensor) or t.dtype != dtp or tuple(t.shape) != ((N,) if w == 1 else (N, w)) or not t.is_contiguous():
                raise L.GstvdError("%s: out[%s] must be a contiguous %s tensor of %d x %d" % (who, k, str(dtp).replace("torch.", ""), N, w))
        if len(set(o[k].stride(0) for k in ("tokens", "segments", "mask", "att"))) != 1:
            raise L.GstvdError("%s: tokens, segments, mask and att must share one row stride" % who)
    d = L.DiscRowsDesc()
    d.cap, d.ld_cap, d.ques, d.ans, d.ld_utt = _p(cap), max(cap.stride(0), Lc), _p(ques), _p(ans), U
    d.opts, d.ld_opt, d.gt_index, d.dense_scores = _p(opts), max(so[2], U), _p(gt_index), _p(dense_scores)
    d.row_dialog, d.row_round, d.row_slot = _p(row_dialog), _p(row_round), _p(row_slot)
    d.u_tok, d.ld_u, d.u_neg = _p(u_tok), (max(u_tok.stride(0), T) if u_tok is not None else 0), _p(u_neg) if train else None
    d.tokens, d.segments, d.mask, d.att = _p(o["tokens"]), _p(o["segments"]), _p(o["mask"]), _p(o["att"])
    d.ld_row, d.sep_indices, d.ld_sep = max(o["tokens"].stride(0), T), _p(o["sep_indices"]), max(o["sep_indices"].stride(0), S)
    d.hist_len, d.neg_option, d.nsp_labels = _p(o["hist_len"]), _p(o["neg_option"]), _p(o["nsp_labels"]) if train else None
    d.mask_prob, d.cls, d.sep, d.mask_id, d.N = mask_prob, int(cls), int(sep), int(mask), N
    d.D, d.R, d.O, d.U, d.Lc, d.T, d.S = D, R, O, U, Lc, T, S
    d.tot_rounds, d.num_options, d.train = tot_rounds, num_options, int(train)
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_disc_rows", lib.gstvd_disc_rows(C.byref(d), _stream()))
    _prof_end(e0, "disc_rows", 0.0, N * (T * 28.0 + S * 8.0), (N, T))
    return o


GEN_MODES = {"eval": L.GEN_EVAL, "test": L.GEN_TEST, "train_a": L.GEN_TRAIN_A, "train_q": L.GEN_TRAIN_Q}
_GEN_ENC = (("tokens", torch.int64, "T"), ("segments", torch.int64, "T"), ("mlm", torch.int64, "T"), ("att", torch.float32, "T"),
            ("sep_indices", torch.int64, "S"))
_GEN_DEC = (("dec_ids", torch.int64, "Ud"), ("dec_att", torch.float32, "Ud"), ("dec_labels", torch.int64, "Ud"))


def gen_rows(cap, ques, ans, opts, gt_index, mode, T, Ud, enc_rows=None, dec_rows=None, num_options=None, mask_prob=0.0, u_tok=None,
             cls=101, sep=102, mask=103, S=DIALOG_MAX_SEP, out=None):
    """Encoder and decoder rows of the generative model from token-id pools in one launch (gstvd_gen_rows; the rule -- the loader
    of dataloader/dataloader_visdial_gen.py on token ids -- is stated in include/gstvd_hip.h).
    Pools, int64 and 0-padded: cap [D, Lc <= 64] (dense rows), ques / ans [D, R, U <= 64], opts [D, Ro, O <= 100, U] with Ro = R or
    1 (row stride free, everything else dense), gt_index [D, R].  `mode`: "eval" (slot k is option k of the eval order, ground
    truth first), "test" (slot k is option k; gt_index may be None), "train_a" / "train_q" (the target is the answer / the
    question, the slot is 0; opts and gt_index may be None).  enc_rows: (dialog, round) int32 [n_enc] or None; dec_rows: (dialog,
    round, slot) int32 [n_dec] or None.  u_tok fp32 [n_enc, T] (dense rows), required when mask_prob > 0.
    Returns a dict: with encoder rows tokens, segments, mlm int64 [n_enc, T], att fp32 [n_enc, T], sep_indices int64 [n_enc, S],
    hist_len int64 [n_enc]; with decoder rows dec_ids int64 [n_dec, Ud], dec_att fp32 [n_dec, Ud], dec_option int32 [n_dec] and, in
    the train modes, dec_labels int64 [n_dec, Ud].  `out`: a dict of caller-owned tensors to write into instead (the four [n_enc, T]
    arrays 2-D views of one row stride, the [n_dec, Ud] arrays of one, sep_indices a 2-D view, the rest contiguous)."""
    who = "gen_rows"
    if mode not in GEN_MODES:
        raise L.GstvdError("%s: mode must be one of %s (got %r)" % (who, sorted(GEN_MODES), mode))
    train = mode in ("train_a", "train_q")
    need = [("ques", ques, 3), ("ans", ans, 3)] + ([] if train else [("opts", opts, 4)]) + ([("gt_index", gt_index, 2)] if mode == "eval" else [])
    for name, t, nd in need:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != nd:
            raise L.GstvdError("%s: %s must be an int64 tensor of %d dimensions" % (who, name, nd))
    if train:
        opts = gt_index = None
    elif mode == "test":
        gt_index = None
    D, R, U = ques.shape
    T, Ud, S = int(T), int(Ud), int(S)
    if tuple(ans.shape) != (D, R, U) or (gt_index is not None and tuple(gt_index.shape) != (D, R)):
        raise L.GstvdError("%s: ques / ans [D, R, U] and gt_index [D, R] do not belong together: %s %s %s"
                           % (who, tuple(ques.shape), tuple(ans.shape), None if gt_index is None else tuple(gt_index.shape)))
    _rows_i64(who, "cap", cap)
    if not (ques.is_contiguous() and ans.is_contiguous() and (gt_index is None or gt_index.is_contiguous())):
        raise L.GstvdError("%s: ques, ans and gt_index must be contiguous" % who)
    Lc = cap.shape[1]
    if cap.shape[0] != D or D < 1 or not 1 <= U <= DIALOG_MAX_UTT or not 1 <= Lc <= DIALOG_MAX_UTT or T < 2 or Ud < 3:
        raise L.GstvdError("%s: cap [D >= 1, Lc], 1 <= U, Lc <= %d, T >= 2 and Ud >= 3 (got D %d, U %d, Lc %d, T %d, Ud %d)"
                           % (who, DIALOG_MAX_UTT, D, U, Lc, T, Ud))
    if R < 1 or 2 * R > S or S > 64:
        raise L.GstvdError("%s: %d rounds give %d separators, more than max_sep_len = %d allows (2R <= S <= 64)" % (who, R, 2 * R, S))
    Ro = O = 0
    so = (0, 0, U, 1)
    if opts is not None:
        Ro, O = opts.shape[1], opts.shape[2]
        if opts.shape[0] != D or opts.shape[3] != U or Ro not in (R, 1):
            raise L.GstvdError("%s: opts must be [D, R or 1, O, U] = [%d, %d or 1, O, %d] (got %s)" % (who, D, R, U, tuple(opts.shape)))
        so = opts.stride()
        # the kernel addresses row ((d * Ro + round) * O + c) * stride: the dialog stride counts whenever D > 1, also for Ro == 1
        if D * Ro * O > 0 and ((U > 1 and so[3] != 1) or so[2] < U or (O > 1 and so[1] != O * so[2])
                               or (D > 1 and so[0] != Ro * O * so[2])):
            raise L.GstvdError("%s: opts must have dense rows of one stride (got strides %s)" % (who, so))
        num_options = O if num_options is None else int(num_options)
        if not 2 <= num_options <= O <= DISC_MAX_OPTIONS:
            raise L.GstvdError("%s: 2 <= num_options <= O <= %d (got num_options %d, O %d)" % (who, DISC_MAX_OPTIONS, num_options, O))
    lists = []
    for name, rows, width in (("enc_rows", enc_rows, 2), ("dec_rows", dec_rows, 3)):
        if rows is None:
            lists.append(((None,) * width, 0))
            continue
        if len(rows) != width or not isinstance(rows[0], torch.Tensor) or rows[0].dim() != 1:
            raise L.GstvdError("%s: %s must be %d int32 vectors of one length" % (who, name, width))
        n = rows[0].numel()
        for i, t in enumerate(rows):
            _flag_vec(who, "%s[%d]" % (name, i), t, n, torch.int32)
        lists.append((tuple(rows), n))
    (enc_l, n_enc), (dec_l, n_dec) = lists
    mask_prob = float(mask_prob)
    if u_tok is None and mask_prob > 0.0:
        raise L.GstvdError("%s: mask_prob = %g needs u_tok, one uniform per row position [n_enc, T]" % (who, mask_prob))
    if u_tok is not None and _rows_i64(who, "u_tok", u_tok, T, torch.float32).shape[0] != n_enc:
        raise L.GstvdError("%s: u_tok must be fp32 [n_enc = %d, T = %d]" % (who, n_enc, T))
    dims = dict(T=T, S=S, Ud=Ud)
    enc_out = _GEN_ENC if n_enc else ()
    dec_out = tuple(v for v in _GEN_DEC if train or v[0] != "dec_labels") if n_dec else ()
    vec = ((("hist_len", torch.int64, n_enc),) if n_enc else ()) + ((("dec_option", torch.int32, n_dec),) if n_dec else ())
    if out is None:
        _p(ques)
        o = {k: torch.empty(n_enc if c != "Ud" else n_dec, dims[c], dtype=dtp, device=ques.device) for k, dtp, c in enc_out + dec_out}
        for k, dtp, n in vec:
            o[k] = torch.empty(n, dtype=dtp, device=ques.device)
    else:
        o = out
        for k, dtp, c in enc_out + dec_out:
            n = n_dec if c == "Ud" else n_enc
            if _rows_i64(who, "out[%s]" % k, o[k], dims[c], dtp).shape[0] != n:
                raise L.GstvdError("%s: out[%s] must have %d rows" % (who, k, n))
        for k, dtp, n in vec:
            _flag_vec(who, "out[%s]" % k, o[k], n, dtp)
        for grp in (tuple(k for k, _, c in enc_out if c == "T"), tuple(k for k, _, _ in dec_out)):
            if grp and len(set(o[k].stride(0) for k in grp)) != 1:
                raise L.GstvdError("%s: %s must share one row stride" % (who, ", ".join(grp)))
    d = L.GenRowsDesc()
    d.cap, d.ld_cap, d.ques, d.ans, d.ld_utt = _p(cap), max(cap.stride(0), Lc), _p(ques), _p(ans), U
    d.opts, d.ld_opt, d.gt_index = _p(opts), max(so[2], U), _p(gt_index)
    d.enc_dialog, d.enc_round = _p(enc_l[0]), _p(enc_l[1])
    d.u_tok, d.ld_u = _p(u_tok), (max(u_tok.stride(0), T) if u_tok is not None else 0)
    if n_enc:
        d.tokens, d.segments, d.mlm, d.att = _p(o["tokens"]), _p(o["segments"]), _p(o["mlm"]), _p(o["att"])
        d.ld_row, d.sep_indices, d.ld_sep = max(o["tokens"].stride(0), T), _p(o["sep_indices"]), max(o["sep_indices"].stride(0), S)
        d.hist_len = _p(o["hist_len"])
    d.dec_dialog, d.dec_round, d.dec_slot = _p(dec_l[0]), _p(dec_l[1]), _p(dec_l[2])
    if n_dec:
        d.dec_ids, d.dec_att, d.ld_dec, d.dec_option = _p(o["dec_ids"]), _p(o["dec_att"]), max(o["dec_ids"].stride(0), Ud), _p(o["dec_option"])
        d.dec_labels = _p(o["dec_labels"]) if train else None
    d.mask_prob, d.cls, d.sep, d.mask_id, d.n_enc, d.n_dec = mask_prob, int(cls), int(sep), int(mask), n_enc, n_dec
    d.D, d.R, d.Ro, d.O, d.U, d.Lc, d.T, d.S, d.Ud = D, R, Ro, O, U, Lc, T, S, Ud
    d.num_options, d.mode = (num_options if opts is not None else 0), GEN_MODES[mode]
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_gen_rows", lib.gstvd_gen_rows(C.byref(d), _stream()))
    _prof_end(e0, "gen_rows", 0.0, n_enc * (T * 28.0 + S * 8.0) + n_dec * Ud * 12.0, (n_enc + n_dec, T))
    return o


RANK_MAX_OPTIONS = L.RANK_MAX_OPTIONS      # options of a list gstvd_rank_metrics covers (a lane owns options i and i + 64)
RANK_ACC_SLOTS = L.RANK_ACC_SLOTS          # int64 slots of its accumulator: the counts, the bits of the float64 ndcg sum, hist[0..128]
RANK_N_SPARSE, RANK_N_GT_SKIPPED, RANK_N_NDCG, RANK_N_NDCG_EMPTY = L.RANK_N_SPARSE, L.RANK_N_GT_SKIPPED, L.RANK_N_NDCG, L.RANK_N_NDCG_EMPTY
RANK_N_REL_SKIPPED, RANK_N_CALLS, RANK_NDCG_SUM, RANK_HIST = L.RANK_N_REL_SKIPPED, L.RANK_N_CALLS, L.RANK_NDCG_SUM, L.RANK_HIST


def rank_metrics(scores, gt_index=None, relevance=None, rel_index=None, discounts=None, ranks=None, gt_rank=None, ndcg=None, acc=None):
    """Ranks, ground-truth ranks, NDCG ratios and accumulator additions of L score lists of O <= 128 options in one call without a
    host synchronisation (gstvd_rank_metrics; the rule -- the stable descending sort, the sequential float64 NDCG sums, the
    add-only accumulator -- is stated in include/gstvd_hip.h).
    scores fp32 [L, O] (dense rows, row stride free); gt_index int64 [L]; relevance fp32 [n_rel, O] (dense rows); rel_index int32 [L]
    (-1: no relevance row; None: row l, n_rel == L); discounts fp32 [>= O] = log2(arange(O) + 2) computed on the host, required with
    relevance.  Outputs are caller-owned and each optional: ranks int64 [L, O] (dense rows), gt_rank int32 [L] (needs gt_index),
    ndcg fp32 [L] (required with relevance), acc int64 [RANK_ACC_SLOTS] (added to).  Returns a dict of the outputs written."""
    who = "rank_metrics"
    _rows_i64(who, "scores", scores, None, torch.float32)
    n, O = scores.shape
    if n < 1 or not 1 <= O <= RANK_MAX_OPTIONS:
        raise L.GstvdError("%s: scores must be [L >= 1, 1 <= O <= %d] (got %d x %d)" % (who, RANK_MAX_OPTIONS, n, O))
    if gt_index is not None:
        _flag_vec(who, "gt_index", gt_index, n, torch.int64)
    if gt_rank is not None:
        if gt_index is None:
            raise L.GstvdError("%s: gt_rank needs gt_index" % who)
        _flag_vec(who, "gt_rank", gt_rank, n, torch.int32)
    n_rel = 0
    if relevance is not None:
        n_rel = _rows_i64(who, "relevance", relevance, O, torch.float32).shape[0]
        if discounts is None:
            raise L.GstvdError("%s: relevance needs discounts, fp32 log2(arange(O) + 2) computed on the host" % who)
        if not isinstance(discounts, torch.Tensor) or discounts.dtype != torch.float32 or discounts.dim() != 1 \
                or discounts.numel() < O or not discounts.is_contiguous():
            raise L.GstvdError("%s: discounts must be a contiguous float32 vector of at least O = %d elements" % (who, O))
        if ndcg is None:
            raise L.GstvdError("%s: relevance needs ndcg, the fp32 [L] output of the ratios" % who)
        if rel_index is not None:
            _flag_vec(who, "rel_index", rel_index, n, torch.int32)
        elif n_rel != n:
            raise L.GstvdError("%s: without rel_index, relevance must have one row per list (L = %d, got %d rows)" % (who, n, n_rel))
        if n_rel < 1:
            raise L.GstvdError("%s: relevance must have at least one row" % who)
    elif ndcg is not None or rel_index is not None:
        raise L.GstvdError("%s: ndcg and rel_index need relevance" % who)
    if ndcg is not None:
        _flag_vec(who, "ndcg", ndcg, n, torch.float32)
    if ranks is not None and tuple(_rows_i64(who, "ranks", ranks, O, torch.int64).shape) != (n, O):
        raise L.GstvdError("%s: ranks must be int64 [L = %d, O = %d]" % (who, n, O))
    if acc is not None:
        _flag_vec(who, "acc", acc, RANK_ACC_SLOTS, torch.int64)
    for name, t in (("gt_index", gt_index), ("relevance", relevance), ("rel_index", rel_index), ("discounts", discounts), ("ranks", ranks),
                    ("gt_rank", gt_rank), ("ndcg", ndcg), ("acc", acc)):
        if t is not None and t.device != scores.device:
            raise L.GstvdError("%s: %s lives on %s, scores on %s" % (who, name, t.device, scores.device))
    d = L.RankMetricsDesc()
    d.scores, d.ld_scores, d.gt_index = _p(scores), max(scores.stride(0), O), _p(gt_index)
    d.relevance, d.ld_rel, d.n_rel = _p(relevance), (max(relevance.stride(0), O) if relevance is not None else 0), n_rel
    d.rel_index, d.discounts, d.n_discounts = _p(rel_index), _p(discounts), (discounts.numel() if discounts is not None else 0)
    d.ranks, d.ld_ranks = _p(ranks), (max(ranks.stride(0), O) if ranks is not None else 0)
    d.gt_rank, d.ndcg, d.acc, d.L, d.O = _p(gt_rank), _p(ndcg), _p(acc), n, O
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_rank_metrics", lib.gstvd_rank_metrics(C.byref(d), _stream()))
    _prof_end(e0, "rank_metrics", 0.0, n * O * (4.0 + (8.0 if ranks is not None else 0.0)), (n, O))
    return {k: v for k, v in (("ranks", ranks), ("gt_rank", gt_rank), ("ndcg", ndcg), ("acc", acc)) if v is not None}


GAUSS_MAX_D, GAUSS_FIT_SLAB = L.GAUSS_MAX_D, L.GAUSS_FIT_SLAB
_GAUSS_DTYPE = {torch.float16: L.F16, torch.float32: L.F32}


def _gauss_feats(who, feats, min_rows):
    """The feature matrix of the in-domain filter: fp16 or fp32 [rows, D], dense rows (row stride free), D % 16 == 0, 16 <= D <= 1024."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
        raise L.GstvdError("%s: feats must be a 2-D tensor [rows, D]" % who)
    if feats.dtype not in _GAUSS_DTYPE:
        raise L.GstvdError("%s: feats must be float16 or float32 (got %s)" % (who, str(feats.dtype).replace("torch.", "")))
    n, D = feats.shape
    if D % 16 or not 16 <= D <= GAUSS_MAX_D:
        raise L.GstvdError("%s: D must be a multiple of 16 in [16, %d] (got %d)" % (who, GAUSS_MAX_D, D))
    if n < min_rows:
        raise L.GstvdError("%s: feats must have at least %d row%s (got %d)" % (who, min_rows, "s" if min_rows > 1 else "", n))
    if feats.stride(1) != 1 or (n > 1 and feats.stride(0) < D):
        raise L.GstvdError("%s: feats must have dense rows (element stride 1, row stride >= D)" % who)
    if not feats.is_cuda:
        raise L.GstvdError("%s: feats lives on %s; gst_visdial_amd ops need GPU tensors, there is no CPU path" % (who, feats.device))
    return n, D


def _gauss_f64(who, name, t, shape, device):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise L.GstvdError("%s: %s must be a contiguous float64 tensor of shape %s" % (who, name, list(shape)))
    if t.device != device:
        raise L.GstvdError("%s: %s lives on %s, feats on %s" % (who, name, t.device, device))
    return t


def gauss_fit_ws_bytes(N, D):
    """Bytes of workspace gauss_fit needs for N rows of D features."""
    need = L.load().gstvd_gauss_fit_ws_bytes(N, D)
    if need < 0:
        raise L.GstvdError("gauss_fit_ws_bytes: N = %d, D = %d is outside the rule (N in [2, 2^28], D %% 16 == 0, 16 <= D <= %d)"
                           % (N, D, GAUSS_MAX_D))
    return need


def gauss_fit(feats, mean=None, cov=None, workspace=None):
    """Mean float64 [D] and covariance float64 [D, D] of the rows of feats (fp16 or fp32 [N >= 2, D]) in two launches, no host
    synchronisation (gstvd_gauss_fit; the rule -- two passes, float64 sums in a fixed order, fact = 1/(N-1) applied once, the lower
    tiles mirrored -- is stated in include/gstvd_hip.h).  mean, cov and workspace (uint8, >= gauss_fit_ws_bytes(N, D)) are
    caller-owned when given, allocated here otherwise.  Returns (mean, cov)."""
    who = "gauss_fit"
    n, D = _gauss_feats(who, feats, 2)
    if n > (1 << 28):
        raise L.GstvdError("%s: at most 2^28 rows (got %d)" % (who, n))
    dev = feats.device
    mean = torch.empty(D, dtype=torch.float64, device=dev) if mean is None else _gauss_f64(who, "mean", mean, (D,), dev)
    cov = torch.empty(D, D, dtype=torch.float64, device=dev) if cov is None else _gauss_f64(who, "cov", cov, (D, D), dev)
    need = gauss_fit_ws_bytes(n, D)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 \
            or not workspace.is_contiguous() or workspace.numel() < need:
        raise L.GstvdError("%s: workspace must be a contiguous uint8 vector of at least %d bytes" % (who, need))
    elif workspace.device != dev:
        raise L.GstvdError("%s: workspace lives on %s, feats on %s" % (who, workspace.device, dev))
    d = L.GaussFitDesc()
    d.x, d.ldx, d.N, d.mean, d.cov = _p(feats), max(feats.stride(0), D), n, _p(mean), _p(cov)
    d.workspace, d.workspace_bytes, d.D, d.dtype = _p(workspace), workspace.numel(), D, _GAUSS_DTYPE[feats.dtype]
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_gauss_fit", lib.gstvd_gauss_fit(C.byref(d), _stream()))
    _prof_end(e0, "gauss_fit", float(n) * D * (D + 64), 2.0 * n * D * feats.element_size(), (n, D))
    return mean, cov


def gauss_pack_w(w):
    """The lower triangle of W = L^-1 (float64 [D, D], any device; done once per fit, on the host) in the operand order
    gstvd_gauss_logprob reads: block row t of 16 rows, then K-step s < 4 t + 4, then column c of the step, then row r --
    packed[128 t (t + 1) + 64 s + 16 c + r] = W[16 t + r, 4 s + c].  Returns a CPU float64 vector."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float64 or w.dim() != 2 or w.shape[0] != w.shape[1] \
            or w.shape[0] % 16 or not 16 <= w.shape[0] <= GAUSS_MAX_D:
        raise L.GstvdError("gauss_pack_w: w must be float64 [D, D], D a multiple of 16 in [16, %d]" % GAUSS_MAX_D)
    w = w.detach().cpu()
    return torch.cat([w[16 * t:16 * t + 16, :16 * t + 16].t().contiguous().reshape(-1) for t in range(w.shape[0] // 16)])


def gauss_logprob(feats, mean, w, klog2pi, half_log_det, out=None, threshold=None, keep=None, n_kept=None):
    """out[m] = (-0.5 * (klog2pi + |W (feats[m] - mean)|^2)) - half_log_det in float64, one launch (gstvd_gauss_logprob; rule in
    include/gstvd_hip.h).  feats fp16 or fp32 [M >= 1, D]; mean float64 [D]; w the packed lower triangle of W (gauss_pack_w) on the
    device; the two constants are Python floats.  With a threshold: keep uint8 [M] receives out[m] >= threshold (a NaN score is
    never kept) and the int64 [1] counter n_kept is added to; both optional.  A NaN or Inf feature gives a NaN or Inf score and does
    not raise.  Returns out."""
    who = "gauss_logprob"
    M, D = _gauss_feats(who, feats, 1)
    if M > 0x7fffffff:
        raise L.GstvdError("%s: at most 2^31 - 1 rows (got %d)" % (who, M))
    dev = feats.device
    _gauss_f64(who, "mean", mean, (D,), dev)
    _gauss_f64(who, "w", w, (128 * (D // 16) * (D // 16 + 1),), dev)
    out = torch.empty(M, dtype=torch.float64, device=dev) if out is None else _gauss_f64(who, "out", out, (M,), dev)
    if threshold is None and (keep is not None or n_kept is not None):
        raise L.GstvdError("%s: keep and n_kept need a threshold" % who)
    if keep is not None:
        _flag_vec(who, "keep", keep, M, torch.uint8)
    if n_kept is not None:
        _flag_vec(who, "n_kept", n_kept, 1, torch.int64)
    for name, t in (("keep", keep), ("n_kept", n_kept)):
        if t is not None and t.device != dev:
            raise L.GstvdError("%s: %s lives on %s, feats on %s" % (who, name, t.device, dev))
    d = L.GaussLogprobDesc()
    d.x, d.ldx, d.M, d.mean, d.w_packed = _p(feats), max(feats.stride(0), D), M, _p(mean), _p(w)
    d.klog2pi, d.half_log_det, d.threshold = float(klog2pi), float(half_log_det), float(threshold) if threshold is not None else 0.0
    d.out, d.keep, d.n_kept, d.D, d.dtype = _p(out), _p(keep), _p(n_kept), D, _GAUSS_DTYPE[feats.dtype]
    lib = L.load()
    e0 = _prof_begin()
    L.check("gstvd_gauss_logprob", lib.gstvd_gauss_logprob(C.byref(d), _stream()))
    _prof_end(e0, "gauss_logprob", float(M) * D * (D + 16), float(M) * D * feats.element_size(), (M, D))
    return out


FUSION = {"mul": 0, "sum": 1}


def _nsp_fwd_desc(who, d, xt, t_rows, xv, v_rows, wt, bt, wv, bv, wn, bn, B, fusion, z, own_fp32, own_names=""):
    """Validates the operands the NSP head's two forms share and fills the leading fields gstvd_nsp_head_t and gstvd_nsp_train_t
    have in common into descriptor `d`.  `who` prefixes the error messages; `own_fp32`: the caller's further fp32 operands,
    `own_names` what the message calls them."""
    if fusion not in FUSION:
        raise L.GstvdError("%s: fusion_method must be 'mul' or 'sum', got %r" % (who, fusion))
    Hb = wt.shape[0]
    if wt.dtype != xt.dtype or wv.dtype != xt.dtype or xv.dtype != xt.dtype:
        raise L.GstvdError("%s: activations and pooler weights must share one dtype" % who)
    for t in (bt, bv, wn, bn, z) + tuple(own_fp32):
        if t.dtype != torch.float32:
            raise L.GstvdError("%s: biases, the classifier%s and the outputs are fp32" % (who, own_names))
    if xt.shape[0] < B * t_rows or xv.shape[0] < B * v_rows or z.shape[0] < B \
            or z.stride(-1) != 1 or xt.stride(-1) != 1 or xv.stride(-1) != 1 or wt.stride(-1) != 1 or wv.stride(-1) != 1 \
            or wn.stride(-1) != 1 or bt.numel() != Hb or bv.numel() != Hb or wv.shape[0] != Hb or tuple(wn.shape) != (2, Hb) \
            or bn.numel() != 2:
        raise L.GstvdError("%s: operand shapes do not match" % who)
    d.xt, d.ldt, d.t_rows = _p(xt), xt.stride(0), t_rows
    d.xv, d.ldv, d.v_rows = _p(xv), xv.stride(0), v_rows
    d.wt, d.ldwt, d.wv, d.ldwv = _p(wt), wt.stride(0), _p(wv), wv.stride(0)
    d.bt, d.bv, d.wn, d.ldwn, d.bn = _p(bt), _p(bv), _p(wn), wn.stride(0), _p(bn)
    d.z, d.ldz = _p(z), z.stride(0)
    d.B, d.H, d.Hv, d.Hb = B, wt.shape[1], wv.shape[1], Hb
    d.dtype, d.fusion = dt(xt), FUSION[fusion]
    return d


def nsp_head(xt, t_rows, xv, v_rows, wt, bt, wv, bv, wn, bn, B, fusion, z, prob0):
    """NSP scores of the enc_only model in one launch (gstvd_nsp_head): row 0 of every batch row of the encoder's final
    activations xt [B * t_rows, H] / xv [B * v_rows, Hv] (read in place, row strides taken from the tensors) -> poolers
    wt [Hb, H], wv [Hb, Hv] (dtype of the activations) with fp32 biases -> `fusion` ('mul' | 'sum') -> wn [2, Hb], bn [2] in
    fp32 -> z [B, 2] fp32 and prob0 [B] fp32 = softmax(z, 1)[:, 0]."""
    lib = L.load()
    d = _nsp_fwd_desc("nsp_head", L.NspHeadDesc(), xt, t_rows, xv, v_rows, wt, bt, wv, bv, wn, bn, B, fusion, z, (prob0,))
    if prob0.shape[0] < B or prob0.stride(0) != 1:
        raise L.GstvdError("nsp_head: operand shapes do not match")
    d.prob0 = _p(prob0)
    e0 = _prof_begin()
    buf = C.create_string_buffer(256) if e0 is not None else None
    if buf is not None:
        d.kernel_name, d.kernel_name_len = C.addressof(buf), 256
    L.check("gstvd_nsp_head", lib.gstvd_nsp_head(C.byref(d), _stream()))
    if e0 is not None:          # keyed by the symbol the call itself reports having launched
        H, Hv, Hb = d.H, d.Hv, d.Hb
        _prof_end(e0, "nsp_head:" + buf.value.decode(), 2.0 * B * Hb * (H + Hv + 2),
                  float(Hb * (H + Hv) * wt.element_size() + B * (H + Hv) * xt.element_size() + B * 12), (B, H, Hv, Hb))
    return z, prob0


def _i64_index(idx, n):
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous() or idx.numel() != n or n <= 0:
        raise L.GstvdError("row index: a contiguous int64 vector with one entry per compacted row (at least one) is needed")


def rows_gather(src, idx, dst, M=None):
    """dst[i, :] = src[idx[i], :] (gstvd_rows_gather): src [>= M, H] with any row stride, dst [n, H]."""
    lib = L.load()
    n, H = dst.shape
    _i64_index(idx, n)
    if src.dtype != dst.dtype or src.shape[1] != H or src.stride(1) != 1 or dst.stride(1) != 1:
        raise L.GstvdError("rows_gather: source and destination must share dtype and width, with dense rows")
    M = src.shape[0] if M is None else M
    e0 = _prof_begin()
    L.check("gstvd_rows_gather", lib.gstvd_rows_gather(_p(src), src.stride(0), M, _p(idx), n, H, dt(src), _p(dst), dst.stride(0), _stream()))
    _prof_end(e0, "rows_gather", 0.0, 2.0 * n * H * src.element_size(), (n, H))
    return dst


def rows_scatter(src, idx, dst, accumulate, M=None):
    """dst[idx[i], :] (=|+=) src[i, :] (gstvd_rows_scatter), idx distinct.  accumulate False: the first writer of `dst` -- rows
    [0, M) that no index names are zero filled."""
    lib = L.load()
    n, H = src.shape
    _i64_index(idx, n)
    if src.dtype != dst.dtype or dst.shape[1] != H or src.stride(1) != 1 or dst.stride(1) != 1:
        raise L.GstvdError("rows_scatter: source and destination must share dtype and width, with dense rows")
    M = dst.shape[0] if M is None else M
    e0 = _prof_begin()
    L.check("gstvd_rows_scatter", lib.gstvd_rows_scatter(_p(src), src.stride(0), _p(idx), n, H, dt(src), _p(dst), dst.stride(0), M,
                                                         int(bool(accumulate)), _stream()))
    _prof_end(e0, "rows_scatter", 0.0, float((3 * n if accumulate else 2 * n + M) * H * src.element_size()), (n, H))
    return dst


def _argmax_out(who, n, device, idx, val):
    idx = torch.empty(n, dtype=torch.int64, device=device) if idx is None else idx
    val = torch.empty(n, dtype=torch.float32, device=device) if val is None else val
    if (idx.dtype != torch.int64 or val.dtype != torch.float32 or idx.numel() < n or val.numel() < n
            or not idx.is_contiguous() or not val.is_contiguous()):
        raise L.GstvdError("%s: idx (int64) and val (fp32) must be contiguous vectors of at least %d entries" % (who, n))
    return idx, val


def rows_argmax(logits, V, n=None, idx=None, val=None):
    """(idx [n] int64, val [n] fp32): per row of logits [n, ld >= V] (fp32 or bf16) the largest of columns 0..V-1 and its column,
    equal values to the smaller column (gstvd_rows_argmax).  n == 0: nothing is launched."""
    lib = L.load()
    n = logits.shape[0] if n is None else n
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < V or logits.shape[0] < n:
        raise L.GstvdError("rows_argmax: logits must be [>= %d, >= %d] with dense rows" % (n, V))
    idx, val = _argmax_out("rows_argmax", n, logits.device, idx, val)
    if n == 0:
        return idx[:0], val[:0]
    e0 = _prof_begin()
    L.check("gstvd_rows_argmax", lib.gstvd_rows_argmax(_p(logits), logits.stride(0), n, V, dt(logits), _p(idx), _p(val), _stream()))
    _prof_end(e0, "rows_argmax", 0.0, float(n) * V * logits.element_size(), (n, V))
    return idx[:n], val[:n]


def vocab_argmax_ws_bytes(n, V):
    return int(L.load().gstvd_vocab_argmax_ws_bytes(n, V))


def vocab_argmax_fused(x, w, bias, V, n=None, idx=None, val=None, ws=None):
    """The fused form alone (gstvd_vocab_argmax): x [n, H] bf16, w [>= V, H] bf16, bias fp32 [>= V] -> (idx, val), or None when the
    library answers GSTVD_E_UNSUPPORTED (dtype, H) -- the caller then takes the GEMM + rows_argmax route.  `ws`: a uint8 workspace
    of at least vocab_argmax_ws_bytes(n, V) bytes (None: allocated here)."""
    lib = L.load()
    n = x.shape[0] if n is None else n
    H = x.shape[1]
    if w.shape[1] != H or w.shape[0] < V or bias.numel() < V or bias.dtype != torch.float32 or x.stride(1) != 1 or w.stride(1) != 1:
        raise L.GstvdError("vocab_argmax: x [n, H], w [>= V, H] with dense rows and an fp32 bias of >= V entries are needed")
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        return None
    idx, val = _argmax_out("vocab_argmax", n, x.device, idx, val)
    if n == 0:
        return idx[:0], val[:0]
    need = vocab_argmax_ws_bytes(n, V)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    e0 = _prof_begin()
    rc = lib.gstvd_vocab_argmax(_p(x), x.stride(0), _p(w), w.stride(0), _p(bias), n, V, H, dt(x), _p(ws), ws.numel() * ws.element_size(),
                                _p(idx), _p(val), _stream())
    if rc == -5:            # GSTVD_E_UNSUPPORTED: not an error, the other route exists
        return None
    L.check("gstvd_vocab_argmax", rc)
    _prof_end(e0, "vocab_argmax", 2.0 * n * V * H, float(V) * H * 2, (n, V, H))
    return idx[:n], val[:n]


def vocab_argmax(x, w, bias, V, n=None, logits=None, ws=None, fused=True):
    """Arg-max over v < V of x . w[v] + bias[v] -> (idx [n] int64, val [n] fp32), ties to the smaller v.  bf16 operands with a
    width the fused kernel tiles: gstvd_vocab_argmax, no [n, V] buffer.  Anything else (fp32 operands: the fp32-precision path),
    or `fused` False (measurements): gstvd_gemm into `logits` ([n, >= round_up(V, 4)] fp32; None: allocated here) and
    gstvd_rows_argmax.  Both are HIP kernels of this library; n == 0 launches nothing."""
    n = x.shape[0] if n is None else n
    if n == 0:
        return (torch.empty(0, dtype=torch.int64, device=x.device), torch.empty(0, dtype=torch.float32, device=x.device))
    if fused:
        out = vocab_argmax_fused(x, w, bias, V, n=n, ws=ws)
        if out is not None:
            return out
    N = (V + 3) // 4 * 4                    # gstvd_gemm writes whole 4-column groups; rows_argmax never reads columns >= V
    if w.shape[0] < N or bias.numel() < N:
        raise L.GstvdError("vocab_argmax: the GEMM route needs the table and the bias padded to %d rows (a multiple of 4)" % N)
    if logits is None:
        logits = torch.empty(n, N, dtype=torch.float32, device=x.device)
    gemm(x, w, logits, n, N, x.shape[1], bias=bias)
    return rows_argmax(logits, V, n=n)


def rows_mul_(x, a, M, N):
    """x[:M, :N] *= a[:M, :N] in place (gstvd_rows_mul)."""
    lib = L.load()
    if x.dtype != a.dtype:
        raise L.GstvdError("rows_mul_: operands must share one dtype")
    e0 = _prof_begin()
    L.check("gstvd_rows_mul", lib.gstvd_rows_mul(_p(x), x.stride(-2), _p(a), a.stride(-2), M, N, dt(x), _stream()))
    _prof_end(e0, "rows_mul", 0.0, 3.0 * M * N * x.element_size(), (M, N))


def kl_fwd(scores, target, rows, C, row_loss, lse, stats, target_row=None, labels=None):
    """Masked-region loss (gstvd_kl_fwd): scores [rows, >= C] fp32 / bf16, target fp32 [*, >= C] (row i of the scores belongs to
    target row target_row[i], or i)."""
    lib = L.load()
    if target.dtype != torch.float32 or target.stride(-1) != 1 or scores.stride(-1) != 1:
        raise L.GstvdError("kl_fwd: the target is fp32, rows dense")
    e0 = _prof_begin()
    L.check("gstvd_kl_fwd", lib.gstvd_kl_fwd(_p(scores), scores.stride(-2), _p(target), target.stride(-2), _p(target_row), _p(labels),
                                             rows, C, dt(scores), _p(row_loss), _p(lse), _p(stats), _stream()))
    _prof_end(e0, "kl_fwd", 0.0, float(rows) * C * (3 * scores.element_size() + 4), (rows, C))


def kl_bwd(scores, target, lse, stats, gscale, mean, rows, C, dscores, target_row=None, labels=None):
    lib = L.load()
    if dscores.dtype != scores.dtype or dscores.stride(-1) != 1:
        raise L.GstvdError("kl_bwd: the gradient has the scores' dtype, rows dense")
    e0 = _prof_begin()
    L.check("gstvd_kl_bwd", lib.gstvd_kl_bwd(_p(scores), scores.stride(-2), _p(target), target.stride(-2), _p(target_row), _p(labels),
                                             _p(lse), _p(stats), _p(gscale), int(mean), rows, C, dt(scores), _p(dscores),
                                             dscores.stride(-2), _stream()))
    _prof_end(e0, "kl_bwd", 0.0, float(rows) * C * (2 * scores.element_size() + 8), (rows, C))


def nsp_train_desc(xt, t_rows, xv, v_rows, wt, bt, wv, bv, wn, bn, labels, B, fusion, z, pt, pv, keep, row_loss, stats, p=0.0,
                   site=0, rng=None):
    """Descriptor of the NSP head in training form (gstvd_nsp_train_t), forward half; nsp_train_bwd fills in the rest.  Operands
    as ops.nsp_head; labels [B, 2] fp32 (soft), pt / pv [B, Hb] fp32 and keep [B, Hb] uint8 are written for backward."""
    d = _nsp_fwd_desc("nsp_train", L.NspTrainDesc(), xt, t_rows, xv, v_rows, wt, bt, wv, bv, wn, bn, B, fusion, z,
                      (labels, pt, pv, row_loss, stats), ", the labels")
    if tuple(labels.shape) != (B, 2) or labels.stride(1) != 1 or keep.dtype != torch.uint8 or row_loss.numel() < B or stats.numel() < 3 \
            or any(tuple(t.shape) != (B, d.Hb) or not t.is_contiguous() for t in (pt, pv, keep)):
        raise L.GstvdError("nsp_train: operand shapes do not match")
    d.labels, d.ldl = _p(labels), labels.stride(0)
    d.pt, d.pv, d.keep, d.row_loss, d.stats = _p(pt), _p(pv), _p(keep), _p(row_loss), _p(stats)
    d.p, d.site = float(p), int(site)
    d.rng = rng.ptr() if (rng is not None and p > 0) else None
    d._keep = (xt, xv, wt, bt, wv, bv, wn, bn, labels, z, pt, pv, keep, row_loss, stats)
    return d


def nsp_train_fwd(d):
    lib = L.load()
    e0 = _prof_begin()
    buf = C.create_string_buffer(256) if e0 is not None else None
    if buf is not None:
        d.kernel_name, d.kernel_name_len = C.addressof(buf), 256
    L.check("gstvd_nsp_train_fwd", lib.gstvd_nsp_train_fwd(C.byref(d), _stream()))
    d.kernel_name, d.kernel_name_len = None, 0
    if e0 is not None:
        _prof_end(e0, "nsp_train_fwd:" + buf.value.decode(), 2.0 * d.B * d.Hb * (d.H + d.Hv + 2), 0.0, (d.B, d.H, d.Hv, d.Hb))


def nsp_train_bwd(d, gscale, dwn, dbn, dpt, dpv, acc_w=False, acc_b=False):
    """Backward of gscale[0] * (mean soft-label loss) of descriptor `d` (after nsp_train_fwd): dwn [2, Hb], dbn [2] fp32 (=|+=),
    dpt / dpv [B, Hb] in the activations' dtype = the gradients in front of the two pooler ReLUs."""
    lib = L.load()
    if dwn.dtype != torch.float32 or dbn.dtype != torch.float32 or tuple(dwn.shape) != (2, d.Hb) or dbn.numel() != 2 \
            or dwn.stride(1) != 1 or dpt.dtype != dpv.dtype or _DT[dpt.dtype] != d.dtype or tuple(dpt.shape) != (d.B, d.Hb) \
            or tuple(dpv.shape) != (d.B, d.Hb) or dpt.stride(1) != 1 or dpv.stride(1) != 1 or dpt.stride(0) != dpv.stride(0):
        raise L.GstvdError("nsp_train_bwd: operand shapes do not match")
    d.gscale, d.dwn, d.lddwn, d.dbn = _p(gscale), _p(dwn), dwn.stride(0), _p(dbn)
    d.dpt, d.dpv, d.lddp = _p(dpt), _p(dpv), dpt.stride(0)
    d.acc_w, d.acc_b = int(bool(acc_w)), int(bool(acc_b))
    e0 = _prof_begin()
    L.check("gstvd_nsp_train_bwd", lib.gstvd_nsp_train_bwd(C.byref(d), _stream()))
    _prof_end(e0, "nsp_train_bwd", 8.0 * d.B * d.Hb, 14.0 * d.B * d.Hb, (d.B, d.Hb))


def vl_split(d_enc, B, R, T, H, d_v, d_t, p, site_v, site_t, rng):
    lib = L.load()
    L.check("gstvd_vl_split", lib.gstvd_vl_split(_p(d_enc), B, R, T, H, dt(d_enc), _p(d_v), _p(d_t), p, site_v, site_t,
                                                 rng.ptr() if (rng is not None and p > 0) else None, _stream()))


def cast(src, dst, n=None):
    lib = L.load()
    n = src.numel() if n is None else n
    L.check("gstvd_cast", lib.gstvd_cast(_p(src), dt(src), _p(dst), dt(dst), n, _stream()))
    return dst


class CastRanges(object):
    """A fixed list of ranges [(start, length)] of two flat buffers with the same indexing, uploaded once (gstvd_cast_ranges)."""

    def __init__(self, ranges, device):
        self.ranges = [(int(a), int(n)) for a, n in ranges if n > 0]
        if any(a % 4 for a, _ in self.ranges):
            raise L.GstvdError("cast_ranges: range starts must be multiples of 4 elements")
        blk0, b = [], 0
        for _, n in self.ranges:
            blk0.append(b)
            b += (n + 1023) // 1024
        blk0.append(b)
        self.blocks, self.elems = b, sum(n for _, n in self.ranges)
        flat = [v for r in self.ranges for v in r]
        self.tab = torch.tensor(flat, dtype=torch.int64).to(device) if flat else None
        self.blk0 = torch.tensor(blk0, dtype=torch.int32).to(device)

    def run(self, src, dst):
        """dst[e] = bf16(src[e]) over the ranges; src fp32, dst bf16, both indexed alike."""
        if not self.ranges:
            return
        lib = L.load()
        L.check("gstvd_cast_ranges", lib.gstvd_cast_ranges(_p(src), _p(dst), self.tab.data_ptr(), self.blk0.data_ptr(), len(self.ranges),
                                                           self.blocks, _stream()))


def scale_(x, factor):
    lib = L.load()
    L.check("gstvd_scale", lib.gstvd_scale(_p(x), _p(factor), x.numel(), _stream()))


def dropout_mask(n, p, site, rng, device):
    lib = L.load()
    out = torch.empty(n, dtype=torch.float32, device=device)
    L.check("gstvd_dropout_mask", lib.gstvd_dropout_mask(_p(out), n, p, site, rng.ptr(), _stream()))
    return out


def adamw(param, grad, m, v, shadow, seg_end, hp, step, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0, begin=0, end=None,
          grad_origin=0):
    """Fused AdamW over flat elements [begin, end) of the buffers.  `grad` is the flat fp32 gradient buffer, or a bf16
    tensor holding flat elements [grad_origin, grad_origin + grad.numel()) (the all-reduced compressed slice)."""
    lib = L.load()
    n = param.numel() if end is None else end
    e0 = _prof_begin()
    if grad.dtype == torch.bfloat16:
        if grad_origin + grad.numel() < n:
            raise ValueError("bf16 gradient slice does not cover [begin, end)")
        L.check("gstvd_adamw_bf16grad", lib.gstvd_adamw_bf16grad(_p(param), _p(grad), grad_origin, _p(m), _p(v), _p(shadow), n,
                                                                 _p(seg_end), _p(hp), seg_end.numel(), beta1, beta2, eps, _p(step),
                                                                 grad_scale, begin, _stream()))
    else:
        L.check("gstvd_adamw", lib.gstvd_adamw(_p(param), _p(grad), _p(m), _p(v), _p(shadow), n, _p(seg_end), _p(hp),
                                               seg_end.numel(), beta1, beta2, eps, _p(step), grad_scale, begin, _stream()))
    _prof_end(e0, "adamw", 0.0, (n - begin) * (30.0 if shadow is not None else 28.0))


def adamw_blocks(param, grad, m, v, shadow, seg_end, hp, step, blocks, seg_skip, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0,
                 begin=0, end=None):
    """AdamW on the listed 1024-element blocks (int32 device tensor of absolute block indices), clipped to [begin, end), leaving
    the segments flagged in `seg_skip` (uint8 device tensor, one per segment) alone: the remainder behind a weight-gradient
    launch that updated its weights itself (GemmGroup.flush(fuse=...)).  An empty list launches nothing."""
    lib = L.load()
    if blocks.numel() == 0:          # (an empty tensor has no address to pass; the entry point would launch nothing either)
        return
    n = param.numel() if end is None else end
    e0 = _prof_begin()
    L.check("gstvd_adamw_blocks", lib.gstvd_adamw_blocks(_p(param), _p(grad), _p(m), _p(v), _p(shadow), n, _p(seg_end), _p(hp),
                                                         seg_end.numel(), beta1, beta2, eps, _p(step), grad_scale, begin, _p(blocks),
                                                         blocks.numel(), _p(seg_skip), _stream()))
    _prof_end(e0, "adamw", 0.0, blocks.numel() * 1024 * (30.0 if shadow is not None else 28.0))


def gemm_ln_rows():
    """Rows per block of the LayerNorm-folded GEMMs (their backward writes one [3][H] partial slab per block)."""
    return int(L.load().gstvd_gemm_ln_rows_per_block())


def _gemm_desc_noA(B, C_out, M, N, K, b_km, bias, addend, aux, epi):
    d = L.GemmDesc()
    d.A, d.B, d.C = None, _p(B), _p(C_out)
    d.bias, d.addend, d.aux = _p(bias), _p(addend), _p(aux)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = 0, B.stride(-2), C_out.stride(-2)
    d.ldadd = addend.stride(-2) if addend is not None else 0
    d.ldaux = aux.stride(-2) if aux is not None else 0
    d.batch, d.dtype_in, d.dtype_out, d.alpha = 1, dt(B), dt(C_out), 1.0
    d.a_kmajor, d.b_kmajor = 0, int(b_km)
    if bias is not None:
        epi |= EPI_BIAS
    if addend is not None:
        epi |= EPI_ADD
    d.epilogue = epi
    return d


def gemm_ln_fwd(ln_kw, B, C_out, N, *, b_km=False, bias=None, addend=None, aux=None, epi=0):
    """C[M, N] = epi(LN(ln_kw) . B^T) in ONE launch (gstvd_gemm_ln_fwd); also writes ln_kw['y'] / mean / rstd as ln_fwd would.
    Raises GstvdError(GSTVD_E_UNSUPPORTED) for shapes outside the kernel's range -- callers check `gemm_ln_ok` first."""
    lib = L.load()
    ld = _ln_desc(**ln_kw)
    d = _gemm_desc_noA(B, C_out, ld.M, N, ld.H, b_km, bias, addend, aux, epi)
    e0 = _prof_begin()
    L.check("gstvd_gemm_ln_fwd", lib.gstvd_gemm_ln_fwd(C.byref(d), C.byref(ld), _stream()))
    _prof_end(e0, "gemm_ln_fwd", 2.0 * ld.M * N * ld.H, float(3 * ld.M * ld.H * 2 + N * ld.H * 2 + ld.M * N * C_out.element_size()),
              (ld.M, N, ld.H, 1))
    return C_out


def gemm_ln_bwd(ln_kw, dy, partial, nblk, B, C_out, N, *, dres=None, dx=None, b_km=True, addend=None, aux=None, epi=0):
    """C[M, N] = epi(dx . B) with dx = the LayerNorm backward of ln_kw under dy, in ONE launch (gstvd_gemm_ln_bwd); also writes
    dres, dx and the [nblk, 3, H] column partials (nblk = ceil(M / gemm_ln_rows()))."""
    lib = L.load()
    b = L.LnBwdDesc()
    b.f = _ln_desc(**ln_kw)
    b.nblk = nblk
    b.dy, b.lddy = _p(dy), dy.stride(-2)
    b.dres, b.lddres = _p(dres), (dres.stride(-2) if dres is not None else 0)
    b.dx, b.lddx = _p(dx), (dx.stride(-2) if dx is not None else 0)
    b.partial = _p(partial)
    d = _gemm_desc_noA(B, C_out, b.f.M, N, b.f.H, b_km, None, addend, aux, epi)
    e0 = _prof_begin()
    L.check("gstvd_gemm_ln_bwd", lib.gstvd_gemm_ln_bwd(C.byref(d), C.byref(b), _stream()))
    _prof_end(e0, "gemm_ln_bwd", 2.0 * b.f.M * N * b.f.H, float(5 * b.f.M * b.f.H * 2 + N * b.f.H * 2 + b.f.M * N * C_out.element_size()),
              (b.f.M, N, b.f.H, 1))
    return C_out


LN_FOLD_MAX_H = 768


def gemm_ln_ok(M, N, H, dtype):
    """Shapes the engine gives to the LayerNorm-folded GEMMs (csrc/gemm_rows.hip): bf16, H = K a multiple of 64 up to
    ops.LN_FOLD_MAX_H = 768 (the decoder's sites), up to 640 rows (beyond that the plain kernels' larger tiles win), at least
    five 128-column tiles.  The kernel itself takes H up to 1024 since round 5 (the vision stream's width; LN_FOLD_MAX_H = 1024
    sends its 36 sites there): bit-identical, but an 80 KB / 512-thread workgroup does not fit beside the text stream's
    workgroups the way the 48 KB 64-tile GEMM + the LayerNorm kernel do -- 12.35 -> 12.66 ms per step
    (profiles/r05_ln_fold_vision_ab.txt), so the default keeps the vision sites on the separate kernels."""
    if not (dtype == torch.bfloat16 and H % 64 == 0 and H <= LN_FOLD_MAX_H and M <= 640 and N >= 640 and N % 8 == 0):
        return False
    # one round of the chip: two workgroups (16 rows x 128 columns) fit a CU; beyond 512 the second round doubles the launch
    # (N = 3072 at 400 rows: 22 us forward / 38 us backward against 23 / 26 us for the two separate kernels)
    return ((M + 15) // 16) * ((N + 127) // 128) <= 512


# ---- coreference text attack: nearest neighbours by cosine, id-level substitution --------------------------------------------
COS_TOPK_ROUTES = {"many": L.COS_TOPK_MANY, "few": L.COS_TOPK_FEW}
COS_TOPK_CENSUS = {"many": 0, "few": 0}      # launches per route so far (the tests' census that both routes ran)
SUBSEQ_MAX_PIECES = 16


def cos_topk_route(n, V):
    """The route gstvd_cos_topk takes for n source rows when none is forced: "many" or "few"."""
    return "many" if L.load().gstvd_cos_topk_route(n, V) == L.COS_TOPK_MANY else "few"


def cos_topk_ws_bytes(n, V, K):
    return int(L.load().gstvd_cos_topk_ws_bytes(n, V, K))


def cos_topk(ehat, src=None, K=10, threshold=0.5, route=None, V=None, D=None, idx=None, val=None, ws=None):
    """(idx int32 [n, K], val fp32 [n, K]): per source row the K best targets t != src[r] of the unit rows ehat[:V, :D] (fp32,
    dense rows, row stride a multiple of 4) with dot >= threshold, larger value first, then the smaller index; unused slots
    idx -1 / val 0 (gstvd_cos_topk; the rule is stated in include/gstvd_hip.h).  src int32 [n] on the device, or None: every row of
    the table is a source.  threshold None or -inf: no cut.  route None (chosen from n), "many" or "few": both return the same
    bits.  idx / val / ws (uint8, at least cos_topk_ws_bytes(n, V, K) bytes, "few" only): the caller's buffers, else allocated."""
    lib = L.load()
    if not isinstance(ehat, torch.Tensor) or ehat.dtype != torch.float32 or ehat.dim() != 2 or ehat.stride(1) != 1:
        raise L.GstvdError("cos_topk: ehat must be fp32 [V, D] with dense rows")
    V = ehat.shape[0] if V is None else int(V)
    D = ehat.shape[1] if D is None else int(D)
    if not (1 <= V <= ehat.shape[0]) or not (1 <= D <= ehat.shape[1]):
        raise L.GstvdError("cos_topk: V = %d, D = %d do not lie inside ehat %s" % (V, D, tuple(ehat.shape)))
    if src is None:
        n = V
    else:
        if src.dtype != torch.int32 or src.dim() != 1 or not src.is_contiguous():
            raise L.GstvdError("cos_topk: src must be a contiguous int32 vector")
        n = src.numel()
    K = int(K)
    if route not in (None, "many", "few"):
        raise L.GstvdError("cos_topk: route must be None, 'many' or 'few' (got %r)" % (route,))
    idx = torch.empty(n, K, dtype=torch.int32, device=ehat.device) if idx is None else idx
    val = torch.empty(n, K, dtype=torch.float32, device=ehat.device) if val is None else val
    if (idx.dtype != torch.int32 or val.dtype != torch.float32 or tuple(idx.shape) != (n, K) or tuple(val.shape) != (n, K)
            or not idx.is_contiguous() or not val.is_contiguous()):
        raise L.GstvdError("cos_topk: idx (int32) and val (fp32) must be contiguous [%d, %d]" % (n, K))
    if n == 0:
        return idx, val
    name = route if route is not None else cos_topk_route(n, V)
    nbytes = 0
    if name == "few":
        need = cos_topk_ws_bytes(n, V, K)
        if ws is None:
            ws = torch.empty(max(need, 8), dtype=torch.uint8, device=ehat.device)
        nbytes = ws.numel() * ws.element_size()
    else:
        ws = None
    thr = float("-inf") if threshold is None else float(threshold)
    e0 = _prof_begin()
    L.check("gstvd_cos_topk", lib.gstvd_cos_topk(_p(ehat), ehat.stride(0) if ehat.shape[0] > 1 else max(ehat.stride(0), D), V, D,
                                                 _p(src), n, K, thr, COS_TOPK_ROUTES[name], _p(ws), nbytes, _p(idx), _p(val),
                                                 _stream()))
    _prof_end(e0, "cos_topk_" + name, 2.0 * n * V * D, float(V) * D * 4, (n, V, D, K))
    COS_TOPK_CENSUS[name] += 1
    return idx, val


def pack_substitutions(plans, device):
    """The CSR form gstvd_subseq_replace reads, from `plans`: per row a list of (utterance, a ids, b ids).  Checked on the host:
    1 <= len(a), len(b) <= 16 and a non-negative utterance.  -> (row_ptr int32 [n + 1], subs int32 [S, 4], pieces int64) on
    `device`."""
    row_ptr, subs, pieces = [0], [], []
    for r, plan in enumerate(plans):
        for u, a, b in plan:
            a, b = [int(x) for x in a], [int(x) for x in b]
            if int(u) < 0 or not (1 <= len(a) <= SUBSEQ_MAX_PIECES) or not (1 <= len(b) <= SUBSEQ_MAX_PIECES):
                raise L.GstvdError("subseq_replace: row %d: utterance %r with %d -> %d pieces (an utterance >= 0 and 1..%d pieces "
                                   "on either side are needed)" % (r, u, len(a), len(b), SUBSEQ_MAX_PIECES))
            subs.append([int(u), len(pieces), len(a), len(b)])
            pieces.extend(a + b)
        row_ptr.append(len(subs))
    return (torch.tensor(row_ptr, dtype=torch.int32).to(device),
            torch.tensor(subs, dtype=torch.int32).reshape(-1, 4).to(device),
            torch.tensor(pieces, dtype=torch.int64).to(device))


def subseq_replace(ids, plans, cls=101, sep=102, pad=0, cont=None, out=None, n_replaced=None, segments=None, sep_indices=None,
                   att_mask=None, start_seg=None):
    """(out_ids int64 [n, T], n_replaced int32 [n]): the substitutions of `plans` applied to the context rows ids int64 [n, T], one
    launch, one workgroup per row (gstvd_subseq_replace; the rule is stated in include/gstvd_hip.h).  plans: per row a list of
    (utterance, a ids, b ids), or what pack_substitutions returned.  cont: uint8 [vocab] on the device, 1 for a "##" piece (None:
    no word-boundary condition).  segments int64 [n, T], sep_indices int64 [n, max_sep], att_mask fp32 [n, T]: written when given,
    recomputed from out_ids; start_seg int64 [n] (row stride free): each row's first segment (None: 0).  ids is never written."""
    who = "subseq_replace"
    lib = L.load()
    _rows_i64(who, "ids", ids)
    n, T = ids.shape
    row_ptr, subs, pieces = plans if isinstance(plans, tuple) else pack_substitutions(plans, ids.device)
    if row_ptr.dtype != torch.int32 or row_ptr.numel() != n + 1 or subs.dtype != torch.int32 or pieces.dtype != torch.int64 \
            or not (row_ptr.is_contiguous() and subs.is_contiguous() and pieces.is_contiguous()) or subs.numel() % 4:
        raise L.GstvdError("%s: row_ptr int32 [%d], subs int32 [S, 4] and pieces int64 are needed" % (who, n + 1))
    out = torch.empty(n, T, dtype=torch.int64, device=ids.device) if out is None else _rows_i64(who, "out", out, T)
    n_replaced = torch.empty(n, dtype=torch.int32, device=ids.device) if n_replaced is None else _flag_vec(who, "n_replaced", n_replaced, n, torch.int32)
    if out.shape[0] != n:
        raise L.GstvdError("%s: out must be [%d, %d]" % (who, n, T))
    if n == 0:
        return out, n_replaced
    d = L.SubseqReplaceDesc()
    d.ids, d.ld_ids, d.out_ids, d.ld_out, d.n_replaced = _p(ids), max(ids.stride(0), T), _p(out), max(out.stride(0), T), _p(n_replaced)
    d.row_ptr, d.subs, d.pieces = _p(row_ptr), (_p(subs) if subs.numel() else None), (_p(pieces) if pieces.numel() else None)
    d.n_subs, d.n_pieces = subs.numel() // 4, pieces.numel()
    if cont is not None:
        if cont.dtype != torch.uint8 or cont.dim() != 1 or not cont.is_contiguous() or cont.numel() < 1:
            raise L.GstvdError("%s: cont must be a contiguous uint8 vector over the vocabulary" % who)
        d.cont, d.n_vocab = _p(cont), cont.numel()
    d.cls, d.sep, d.pad = int(cls), int(sep), int(pad)
    if segments is not None:
        if _rows_i64(who, "segments", segments, T).shape[0] != n:
            raise L.GstvdError("%s: segments must be [n, T]" % who)
        d.segments, d.ld_seg = _p(segments), max(segments.stride(0), T)
    if att_mask is not None:
        if _rows_i64(who, "att_mask", att_mask, T, torch.float32).shape[0] != n:
            raise L.GstvdError("%s: att_mask must be [n, T]" % who)
        d.att_mask, d.ld_att = _p(att_mask), max(att_mask.stride(0), T)
    if sep_indices is not None:
        if _rows_i64(who, "sep_indices", sep_indices).shape[0] != n:
            raise L.GstvdError("%s: sep_indices must be [n, max_sep]" % who)
        d.sep_indices, d.ld_sep, d.max_sep = _p(sep_indices), max(sep_indices.stride(0), sep_indices.shape[1]), sep_indices.shape[1]
    if start_seg is not None:
        if start_seg.dtype != torch.int64 or start_seg.dim() != 1 or start_seg.numel() != n:
            raise L.GstvdError("%s: start_seg must be int64 [n]" % who)
        d.start_seg, d.ld_start = _p(start_seg), start_seg.stride(0)
    d.n, d.T = n, T
    e0 = _prof_begin()
    L.check("gstvd_subseq_replace", lib.gstvd_subseq_replace(C.byref(d), _stream()))
    _prof_end(e0, "subseq_replace", 0.0, 16.0 * n * T, (n, T))
    return out, n_replaced
