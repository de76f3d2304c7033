"""Sample-and-rank decoding, the part that needs no GPU: the refusals of the public interface before any device call, the ranking
and finalising rule on hand-made tensors, and the new entry point in header, bindings and library."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS, PAD = 102, 0


def _cpu_model():
    from gst_visdial_amd import selfcheck
    model, params, cfg = selfcheck.build_tiny_model("fp32", "cpu", mode="vd_gen_val")
    g = selfcheck.load_npz("tiny_train.npz")
    kw = selfcheck.golden_batch(g, "cpu")
    kw["dec_input_ids"] = torch.full((kw["enc_input_ids"].shape[0], 1), 101, dtype=torch.long)
    kw.pop("dec_labels"), kw.pop("dec_attention_mask")
    return model.eval(), kw


def test_refusals_come_before_any_device_call():
    from gst_visdial_amd import _lib
    from gst_visdial_amd._lib import GstvdError
    model, kw = _cpu_model()
    calls = _lib.N_CALLS[0]
    for S in (0, 9, -1):
        with pytest.raises(GstvdError, match="num_samples"):
            model(num_samples=S, **kw)
        with pytest.raises(GstvdError, match="num_samples"):
            model.sample_ranked(num_samples=S, **kw)
        with pytest.raises(GstvdError, match="num_samples"):
            model.engine.sample_ranked(kw["enc_image_features"], kw["enc_image_spatials"], kw["enc_image_mask"], kw["enc_input_ids"],
                                       kw["enc_segments"], kw["enc_attention_mask"], kw["dec_input_ids"], num_samples=S)
    with pytest.raises(GstvdError, match="num_beams"):
        model(num_samples=3, num_beams=2, **kw)
    with pytest.raises(GstvdError, match="num_beams"):
        model.sample_ranked(num_samples=3, num_beams=2, **kw)
    for shape in ((18, 3), (18, 10), (17, 9), (18 * 9,), (18, 3, 3)):           # [max_seq_len, B * S] = [18, 9] is wanted
        with pytest.raises(GstvdError, match="uniforms"):
            model.sample_ranked(num_samples=3, uniforms=torch.full(shape, 0.5), **kw)
        with pytest.raises(GstvdError, match="uniforms"):
            model(num_samples=3, uniforms=torch.full(shape, 0.5), **kw)
    assert _lib.N_CALLS[0] == calls and model.engine.flat is None and model.engine.arena is None


def _rank(seqs, logp, lp):
    from gst_visdial_amd import decoding
    return decoding.rank_samples(torch.tensor([seqs]), torch.tensor([logp]), EOS, PAD, lp)


def test_ranking_sums_to_the_first_eos_and_pads_behind_it():
    # sample 0: no EOS (len 4); sample 1: EOS at position 1 (len 2), junk behind it that must go; sample 2: EOS at position 0 (len 1)
    seqs = [[5, 6, 7, 8], [9, EOS, 55, EOS], [EOS, 3, 4, 5]]
    logp = [[-1.0, -1.0, -1.0, -1.5], [-0.5, -2.0, -7.0, -9.0], [-2.0, -3.0, -3.0, -3.0]]
    out, scores, tl, order = _rank(seqs, logp, 0.0)
    assert order.tolist() == [[2, 1, 0]] and scores.tolist() == [[-2.0, -2.5, -4.5]]
    assert out[0].tolist() == [[EOS, PAD, PAD, PAD], [9, EOS, PAD, PAD], [5, 6, 7, 8]]
    assert tl[0].tolist() == [[-2.0, 0.0, 0.0, 0.0], [-0.5, -2.0, 0.0, 0.0], [-1.0, -1.0, -1.0, -1.5]]
    assert out.dtype == torch.int64 and scores.dtype == tl.dtype == torch.float32
    out, scores, tl, order = _rank(seqs, logp, 1.0)                              # -4.5 / 4, -2.5 / 2, -2 / 1
    assert order.tolist() == [[0, 1, 2]] and scores.tolist() == [[-1.125, -1.25, -2.0]]
    assert out[0, 0].tolist() == [5, 6, 7, 8] and tl[0, 2].tolist() == [-2.0, 0.0, 0.0, 0.0]
    out, scores, tl, order = _rank(seqs, logp, 2.0)                              # -4.5 / 16, -2.5 / 4, -2 / 1
    assert order.tolist() == [[0, 1, 2]] and scores.tolist() == [[-0.28125, -0.625, -2.0]]


def test_an_exact_tie_goes_to_the_smaller_sample_index_and_infinities_do_not_poison_the_padding():
    seqs = [[5, EOS, 1], [6, 7, EOS], [8, EOS, 2]]
    logp = [[-1.0, -1.0, -float("inf")], [-1.0, -1.0, -1.0], [-0.5, -1.5, float("nan")]]
    out, scores, tl, order = _rank(seqs, logp, 1.0)
    assert scores.tolist() == [[-1.0, -1.0, -1.0]] and order.tolist() == [[0, 1, 2]]
    assert bool(torch.isfinite(tl).all()) and tl[0, 0].tolist() == [-1.0, -1.0, 0.0]
    out, scores, tl, order = _rank(seqs, logp, 0.0)
    assert order.tolist() == [[0, 2, 1]] and scores.tolist() == [[-2.0, -2.0, -3.0]]
    assert out[0].tolist() == [[5, EOS, PAD], [8, EOS, PAD], [6, 7, EOS]]


def test_header_bindings_and_library_agree_on_the_scored_entry_point():
    import ctypes as C
    from gst_visdial_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    assert re.search(r"\bint\s+gstvd_sample_topk_scored\s*\(\s*const\s+gstvd_sample_t\s*\*\s*a,\s*float\s*\*\s*logp,\s*int64_t\s+logp_stride,"
                     r"\s*gstvd_stream_t\s+s\)", hdr)
    res, args = _lib.SIGNATURES["gstvd_sample_topk_scored"]
    assert res is C.c_int32 and args == [C.POINTER(_lib.SampleDesc), C.c_void_p, C.c_int64, C.c_void_p]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    assert lib.gstvd_abi_version() == 9
    assert lib.gstvd_sample_topk_scored(None, None, 1, None) == -4              # GSTVD_E_NULL, before anything touches a device
    d = _lib.SampleDesc()
    assert lib.gstvd_sample_topk_scored(C.byref(d), 0x1000, 1, None) == -4      # null pointers inside
    d.logits, d.u, d.out = 0x1000, 0x2000, 0x3000
    d.ld, d.dtype, d.B, d.V, d.top_k, d.temperature, d.out_stride = 600, 0, 2, 600, 7, 1.0, 1
    assert lib.gstvd_sample_topk_scored(C.byref(d), None, 1, None) == -4        # logp == NULL
    for stride in (0, -1):
        assert lib.gstvd_sample_topk_scored(C.byref(d), 0x4000, stride, None) == -2     # GSTVD_E_SHAPE
    d.temperature = 0.0
    assert lib.gstvd_sample_topk_scored(C.byref(d), 0x4000, 1, None) == -2      # ... after everything gstvd_sample_topk refuses
    d.temperature, d.V, d.ld = 1.0, 31 * 1024 + 1, 40000
    assert lib.gstvd_sample_topk_scored(C.byref(d), 0x4000, 1, None) == -5
    src = open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "sample.hip")).read()
    assert "getenv" not in src and "hipMalloc" not in src and "Synchronize" not in src
    from gst_visdial_amd import ops
    assert callable(ops.sample_topk_scored)
