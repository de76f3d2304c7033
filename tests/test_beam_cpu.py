"""Beam-search decoding, the part that needs no GPU: the C ABI of the two new entry points against its ctypes mirror, their
argument checks, the host-side back-trace / final ordering on hand-made steps, and the refusals of the public interface."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS, PAD = 102, 0


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            for x in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(","):
                names.append(re.sub(r"\[\d+\]$", "", x.strip().lstrip("*").strip()))
    return names


def _lib():
    from gst_visdial_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib, _lib.load()


def test_header_bindings_and_library_agree_on_the_beam_entry_points():
    from gst_visdial_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    for fn, desc in (("gstvd_beam_step", _lib.BeamStepDesc), ("gstvd_beam_reorder", _lib.BeamReorderDesc)):
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s_t\s*\*" % (fn, fn), hdr)
        assert fn in _lib.SIGNATURES
        assert _struct_fields(hdr, fn + "_t") == [f[0] for f in desc._fields_]
    # the fixed array of 16 layer pointers, in the header and in the mirror
    assert re.search(r"const void\* src\[16\]; void\* dst\[16\];", hdr)
    assert _lib.BeamReorderDesc.src.size == 16 * 8 and _lib.BeamReorderDesc.dst.size == 16 * 8
    src = open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "beam.hip")).read()
    assert "getenv" not in src and "hipMalloc" not in src and "Synchronize" not in src


def test_entry_points_refuse_null_descriptors_and_abi_stays_9():
    _, lib = _lib()
    assert lib.gstvd_abi_version() == 9
    assert lib.gstvd_beam_step(None, None) == -4           # GSTVD_E_NULL, before anything touches a device
    assert lib.gstvd_beam_reorder(None, None) == -4


def test_entry_points_refuse_bad_descriptors_before_any_launch():
    import ctypes as C
    L, lib = _lib()
    d = L.BeamStepDesc()
    assert lib.gstvd_beam_step(C.byref(d), None) == -4      # null pointers inside
    for f in ("logits", "score_in", "done_in", "done_out", "parent", "ids_tm", "workspace"):
        setattr(d, f, 0x1000)
    d.score_out = 0x2000
    d.done_out = 0x2000
    d.ld, d.dtype, d.B, d.V, d.ids_stride, d.positions, d.pos = 40000, 0, 2, 600, 64, 4, 1
    for K in (0, 9):
        d.K = K
        assert lib.gstvd_beam_step(C.byref(d), None) == -2  # GSTVD_E_SHAPE
    d.K, d.V = 5, 31 * 1024 + 1
    assert lib.gstvd_beam_step(C.byref(d), None) == -5      # GSTVD_E_UNSUPPORTED: the sampler's vocabulary limit
    d.V, d.pos = 600, 4
    assert lib.gstvd_beam_step(C.byref(d), None) == -2      # position outside the id buffer
    d.pos, d.score_out = 1, d.score_in
    assert lib.gstvd_beam_step(C.byref(d), None) == -2      # in-place state
    r = L.BeamReorderDesc()
    r.parent = 0x1000
    r.n_layers = 17
    assert lib.gstvd_beam_reorder(C.byref(r), None) == -2
    r.n_layers = 2
    assert lib.gstvd_beam_reorder(C.byref(r), None) == -4   # a null layer pointer
    for l in range(2):
        r.src[l], r.dst[l] = 0x10000, 0x20000
    r.B, r.K, r.H, r.Umax, r.t, r.dtype, r.ld, r.row_stride = 2, 5, 64, 7, 7, 1, 192, 7 * 192
    assert lib.gstvd_beam_reorder(C.byref(r), None) == -2   # t outside the cache
    r.t, r.H, r.ld, r.row_stride = 3, 60, 180, 7 * 180
    assert lib.gstvd_beam_reorder(C.byref(r), None) == -3   # GSTVD_E_ALIGN: 120-byte column blocks
    r.H, r.ld, r.row_stride = 64, 192, 7 * 192
    r.dst[1] = r.src[1]
    assert lib.gstvd_beam_reorder(C.byref(r), None) == -2   # one cache set: a permutation cannot run in place


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from gst_visdial_amd import ops
    from gst_visdial_amd._lib import GstvdError
    B, K, V = 2, 3, 50
    s, dn = torch.zeros(B, K), torch.zeros(B, K, dtype=torch.int32)
    ids = torch.zeros(4, B * K, dtype=torch.long)
    ws = torch.zeros(2 * B * K * K, dtype=torch.int32)
    with pytest.raises(GstvdError):
        ops.beam_step(torch.zeros(B * K, V), s, dn, s.clone(), dn.clone(), dn.clone(), ids, 1, ws, EOS, PAD)
    with pytest.raises(GstvdError):
        ops.beam_step(torch.zeros(B * K, V), torch.zeros(B, 9), dn, s.clone(), dn.clone(), dn.clone(), ids, 1, ws, EOS, PAD)
    c = [torch.zeros(B * K, 7, 3 * 64)]
    with pytest.raises(GstvdError):
        ops.beam_reorder(c, [torch.zeros_like(c[0])], dn, 3, 64)
    with pytest.raises(GstvdError):
        ops.beam_reorder(c, c, dn, 9, 64)


# ---- back-trace and final ordering on hand-made steps ---------------------------------------------------------------------------
def _run(tok, parent, scores, lp):
    from gst_visdial_amd import decoding
    tok, parent = torch.tensor(tok)[:, None], torch.tensor(parent, dtype=torch.int32)[:, None]      # [steps, B = 1, K]
    seqs = decoding.beam_backtrace(tok, parent)
    return seqs, decoding.beam_finalize(seqs, torch.tensor([scores]), EOS, PAD, lp)


def test_backtrace_follows_crossing_parents_and_a_frozen_beam():
    # step 0: beams (7, 8, 9) all from beam 0; step 1: the parents CROSS (new 0 <- old 2, new 1 <- old 0, new 2 <- old 1) and
    # new beam 1 ends; step 2-3: beam 1 is frozen (PAD, its own parent), the other two swap places once more
    tok = [[7, 8, 9], [11, EOS, 13], [21, PAD, 23], [31, PAD, 33]]
    parent = [[0, 0, 0], [2, 0, 1], [2, 1, 0], [0, 1, 2]]
    seqs, (out, final, order) = _run(tok, parent, [-4.0, -3.0, -8.0], 0.0)
    assert seqs[0].tolist() == [[8, 13, 21, 31], [7, EOS, PAD, PAD], [9, 11, 23, 33]]
    assert order.tolist() == [[1, 0, 2]] and final.tolist() == [[-3.0, -4.0, -8.0]]
    assert out[0].tolist() == [[7, EOS, PAD, PAD], [8, 13, 21, 31], [9, 11, 23, 33]]
    assert seqs.dtype == torch.int64 and out.dtype == torch.int64


def test_length_penalty_flips_the_winner_and_pads_after_the_first_eos():
    # beam 0: 4 tokens without EOS, log-probability -4.4; beam 1: EOS at the second token (len 2), -2.4, then junk that must go
    tok = [[5, 6], [7, EOS], [8, 55], [9, EOS]]
    parent = [[0, 0], [0, 1], [0, 1], [0, 1]]
    _, (out0, f0, o0) = _run(tok, parent, [-4.4, -2.4], 0.0)
    assert o0.tolist() == [[1, 0]] and torch.equal(f0, torch.tensor([[-2.4, -4.4]]))     # length_penalty 0: the sums themselves
    assert out0[0, 0].tolist() == [6, EOS, PAD, PAD]
    _, (out1, f1, o1) = _run(tok, parent, [-4.4, -2.4], 1.0)
    assert o1.tolist() == [[0, 1]]                                   # -4.4 / 4 = -1.1 beats -2.4 / 2 = -1.2
    assert torch.allclose(f1, torch.tensor([[-1.1, -1.2]]))
    assert out1[0].tolist() == [[5, 7, 8, 9], [6, EOS, PAD, PAD]]


def test_an_exact_tie_goes_to_the_smaller_beam_index():
    tok = [[5, 6, 7], [8, 9, 10]]
    parent = [[0, 0, 0], [0, 1, 2]]
    _, (out, final, order) = _run(tok, parent, [-3.0, -2.0, -2.0], 1.0)
    assert order.tolist() == [[1, 2, 0]] and final.tolist() == [[-1.0, -1.0, -1.5]]
    assert out[0].tolist() == [[6, 9], [7, 10], [5, 8]]
    _, (_, _, order) = _run(tok, parent, [-2.0, -2.0, -2.0], 0.0)
    assert order.tolist() == [[0, 1, 2]]


# ---- the public interface refuses before any device work ------------------------------------------------------------------------
def _cpu_model():
    from gst_visdial_amd import selfcheck
    model, params, cfg = selfcheck.build_tiny_model("fp32", "cpu", mode="vd_gen_val")
    g = selfcheck.load_npz("tiny_train.npz")
    kw = selfcheck.golden_batch(g, "cpu")
    kw["dec_input_ids"] = torch.full((kw["enc_input_ids"].shape[0], 1), 101, dtype=torch.long)
    kw["dec_labels"] = None
    return model.eval(), kw


def test_beams_with_ngram_blocking_and_sampling_with_beams_are_refused_before_any_device_call():
    from gst_visdial_amd import _lib
    from gst_visdial_amd._lib import GstvdError
    model, kw = _cpu_model()
    calls = _lib.N_CALLS[0]
    with pytest.raises(GstvdError, match="ngram_blocking_size"):
        model(num_beams=3, ngram_blocking_size=2, **kw)
    with pytest.raises(GstvdError, match="num_beams"):
        model.beam_search(num_beams=9, **{k: v for k, v in kw.items() if k not in ("dec_attention_mask", "dec_labels")})
    with pytest.raises(GstvdError, match="beam search"):
        model.engine.sample(kw["enc_image_features"], kw["enc_image_spatials"], kw["enc_image_mask"], kw["enc_input_ids"],
                            kw["enc_segments"], kw["enc_attention_mask"], kw["dec_input_ids"], num_beams=3)
    assert _lib.N_CALLS[0] == calls and model.engine.flat is None and model.engine.arena is None
