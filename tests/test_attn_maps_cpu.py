"""CPU side of the attention maps: the fixture tests/golden/tiny_attn_maps.npz checks itself (shapes, row sums, masked zeros, the
peakedness condition of tools/make_golden_attn_maps.py), the `select` / `heads` parsers and their errors, the refusal of CPU
tensors, the entry point in the header and in the ctypes table -- and the checks of tests/exact_attn_maps.py proved against a
stand-in written in torch, and against deliberately wrong stand-ins, before tests/test_attn_maps_exact_gpu.py points them at the
HIP kernel."""
import os
import re

import pytest
import torch

import exact_attn_maps as M
from conftest import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MEAN_ROWMAX, MAX_ENTRY = 0.3, 0.97


@pytest.fixture(scope="module")
def fx():
    return load_npz("tiny_attn_maps.npz")


# ------------------------------------------------------------------------------------------ the entry point
def test_attn_probs_is_declared_in_the_header_and_in_the_ctypes_table():
    from gst_visdial_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gstvd_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gstvd_attn_probs\s*\(\s*const\s+gstvd_attn_t\s*\*\s*a\s*,\s*float\s*\*\s*P\s*,\s*int32_t\s+head_mean\s*,\s*gstvd_stream_t\s+s\s*\)\s*;", src)
    assert "gstvd_attn_probs" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gstvd_attn_probs"][1]) == 4


def test_cpu_tensors_raise():
    from gst_visdial_amd import ops, attn_maps, _lib
    from gst_visdial_amd._lib import GstvdError
    q = torch.zeros(2 * 16, 64)
    with pytest.raises(GstvdError, match="GPU tensors"):
        ops.attn_desc(q, q, None, None, None, None, 2, 2, 16, 16, 32, ldv=0, ldo=0)
    a = _lib.AttnDesc()                                   # a descriptor as such: the call under test is attn_probs
    a.B, a.nh, a.Lq, a.Lk, a.d = 2, 2, 16, 16, 32
    with pytest.raises(GstvdError, match="GPU tensors"):
        ops.attn_probs(a, torch.zeros(2 * 2 * 16 * 16))
    with pytest.raises(GstvdError, match="contiguous fp32 tensor of 1024 elements"):
        ops.attn_probs(a, torch.zeros(7))
    req = attn_maps.MapRequest(dict(t=[0], v=[], c=[]), False)
    with pytest.raises(GstvdError):
        req.alloc(None, None, 2, 16, 7, 0, torch.device("cpu"))


# ------------------------------------------------------------------------------------------ select / heads
COUNTS = dict(t=4, v=2, c=2, decoder_self=2, decoder_cross=2)


def test_select_parser():
    from gst_visdial_amd.attn_maps import parse_select, parse_heads, KINDS, ENCODER_KINDS
    full = parse_select(None, COUNTS)
    assert full == {k: list(range(COUNTS[k])) for k in KINDS}
    assert parse_select(None, COUNTS, ENCODER_KINDS) == {k: list(range(COUNTS[k])) for k in ENCODER_KINDS}
    got = parse_select({"c": "all", "t": (3, 0), "decoder_cross": iter([1])}, COUNTS)
    assert got == dict(t=[0, 3], v=[], c=[0, 1], decoder_self=[], decoder_cross=[1])
    assert parse_select({}, COUNTS) == {k: [] for k in KINDS}
    assert parse_heads("all") is False and parse_heads("mean") is True


@pytest.mark.parametrize("bad", [{"x": "all"}, {"t": [4]}, {"t": [-1]}, {"v": "some"}, {"c": [0, 0]}, {"t": [1.0]}, {"t": [True]}, {"t": 3},
                                 ["t"], "all"])
def test_select_parser_errors(bad):
    from gst_visdial_amd.attn_maps import parse_select
    from gst_visdial_amd._lib import GstvdError
    with pytest.raises(GstvdError):
        parse_select(bad, COUNTS)


def test_select_parser_refuses_decoder_kinds_for_the_encoder_alone_and_unknown_head_modes():
    from gst_visdial_amd.attn_maps import parse_select, parse_heads, ENCODER_KINDS
    from gst_visdial_amd._lib import GstvdError
    with pytest.raises(GstvdError):
        parse_select({"decoder_self": "all"}, COUNTS, ENCODER_KINDS)
    for h in ("max", None, 0):
        with pytest.raises(GstvdError):
            parse_heads(h)


def test_site_of_parameter():
    from gst_visdial_amd.attn_maps import site_of_parameter as site
    assert site("bert_pretrained.bert.encoder.layer.3.attention.self.query.weight") == "t3"
    assert site("encoder.bert_pretrained.bert.encoder.layer.0.attention.self.key.bias") == "t0"
    assert site("bert_pretrained.bert.encoder.v_layer.1.attention.self.key.weight") == "v1"
    assert site("bert_pretrained.bert.encoder.c_layer.0.biattention.query2.weight") == "c0::0"
    assert site("bert_pretrained.bert.encoder.c_layer.0.biattention.key1.bias") == "c0::0"
    assert site("bert_pretrained.bert.encoder.c_layer.1.biattention.query1.weight") == "c1::1"
    assert site("bert_pretrained.bert.encoder.c_layer.1.biattention.key2.weight") == "c1::1"
    assert site("decoder.decoder.bert.encoder.layer.1.attention.self.query.weight") == "decoder_self1"
    assert site("decoder.decoder.bert.encoder.layer.0.crossattention.self.key.weight") == "decoder_cross0"
    for other in ("bert_pretrained.bert.encoder.layer.3.attention.self.value.weight", "bert_pretrained.bert.encoder.c_layer.0.biattention.value1.bias",
                  "bert_pretrained.bert.encoder.layer.0.attention.output.dense.weight", "vlfusion.fc_l.weight", "query"):
        assert site(other) is None


# ------------------------------------------------------------------------------------------ the fixture
def fixture_maps(fx, prefix):
    return {k: v for k, v in fx.items() if k.startswith(prefix) and "::in::" not in k and "::factor::" not in k}


def test_fixture_shapes_and_row_sums(fx):
    B, T, R, U = 3, 24, 7, 9
    want = {}
    want.update({"enc::t%d" % i: (B, 2, T, T) for i in range(4)})
    want.update({"enc::v%d" % i: (B, 3, R, R) for i in range(2)})
    for i in range(2):
        want["enc::c%d::0" % i], want["enc::c%d::1" % i] = (B, 4, T, R), (B, 4, R, T)
        want["dec::self%d" % i], want["dec::cross%d" % i] = (B, 2, U, U), (B, 2, U, R + T)
    got = dict(fixture_maps(fx, "enc::"), **fixture_maps(fx, "dec::"))
    assert {k: tuple(v.shape) for k, v in got.items()} == want
    disc = fixture_maps(fx, "disc::")
    Td = fx["disc::in::ids"].shape[1]
    assert len(disc) == 10 and tuple(disc["disc::t3"].shape) == (2, 2, Td, Td) and tuple(disc["disc::c1::1"].shape) == (2, 4, R, Td)
    for k, v in dict(got, **disc).items():
        assert v.dtype == torch.float32
        assert float((v.double().sum(-1) - 1).abs().max()) < 1e-5, k
    assert (float(fx["factor"]), float(fx["factor_cross"])) == (8.0, 11.5)
    sites = sorted(k[len("disc::factor::"):] for k in fx if k.startswith("disc::factor::"))
    assert sites == sorted(k[len("disc::"):] for k in disc)          # one factor per enc_only_a site
    assert all(float(fx["disc::factor::" + s]) * 16 == int(float(fx["disc::factor::" + s]) * 16) > 0 for s in sites)


def test_fixture_masked_entries_are_zero(fx):
    tm, vm, dm = fx["in::enc_attention_mask"], fx["in::enc_image_mask"], fx["in::dec_attention_mask"]
    assert int((tm == 0).sum()) == 20 and int((vm == 0).sum()) == 2 and bool((vm[2, -2:] == 0).all())
    for i in range(4):
        assert bool((fx["enc::t%d" % i][(tm == 0)[:, None, None, :].expand(-1, 2, 24, -1)] == 0).all())
    for i in range(2):
        assert bool((fx["enc::v%d" % i][(vm == 0)[:, None, None, :].expand(-1, 3, 7, -1)] == 0).all())
        assert bool((fx["enc::c%d::0" % i][(vm == 0)[:, None, None, :].expand(-1, 4, 24, -1)] == 0).all())
        assert bool((fx["enc::c%d::1" % i][(tm == 0)[:, None, None, :].expand(-1, 4, 7, -1)] == 0).all())
        upper = torch.triu(torch.ones(9, 9, dtype=torch.bool), 1)
        dead = upper[None, None] | (dm == 0)[:, None, None, :]
        assert bool((fx["dec::self%d" % i][dead.expand(-1, 2, -1, -1)] == 0).all())
        em = torch.cat([vm, tm], 1)
        assert bool((fx["dec::cross%d" % i][(em == 0)[:, None, None, :].expand(-1, 2, 9, -1)] == 0).all())


def test_fixture_is_peaked(fx):
    """The generator's condition, restated: mean row maximum >= 0.3 and largest entry <= 0.97 over the rows with at least two
    allowed keys (the decoder's first causal row has one), for EVERY recorded map (tools/make_golden_attn_maps.py, FACTORS)."""
    dm = fx["in::dec_attention_mask"]
    allowed = (torch.tril(torch.ones(9, 9, dtype=torch.bool))[None] & (dm != 0)[:, None, :])[:, None]
    n = 0
    for prefix in ("enc::", "dec::", "disc::"):
        for k, v in fixture_maps(fx, prefix).items():
            rows = (allowed.sum(-1) >= 2).expand(v.shape[:-1]) if k.startswith("dec::self") else torch.ones(v.shape[:-1], dtype=torch.bool)
            mrm, top = float(v.max(-1).values[rows].mean()), float(v[rows].max())
            assert top <= MAX_ENTRY, (k, top)
            assert mrm >= MIN_MEAN_ROWMAX, (k, mrm)
            n += 1
    assert n == 24


# ------------------------------------------------------------------------------------------ the exact checks against a stand-in
class Torch(object):
    """gstvd_attn_probs in torch, fp32, on the CPU.  `wrong`: a deliberate mistake the checks must catch."""

    def __init__(self, wrong=None):
        self.device, self.wrong = torch.device("cpu"), wrong

    def run(self, p, scale=None, drop_p=0.0, q_bstride=0, kv_bstride=0):
        c = p.c
        if self.wrong == "accepts":
            drop_p = q_bstride = kv_bstride = 0
        if drop_p != 0 or q_bstride != 0 or kv_bstride != 0:
            raise RuntimeError("gstvd_attn_probs failed: GSTVD_E_UNSUPPORTED")
        scale = M.A.scale32(c.d) if scale is None else scale
        Q = p.Q.unflatten(-1, (c.nh, c.d)).float()
        K = p.K.unflatten(-1, (c.nh, c.d)).float().repeat_interleave(c.kv_group, 0)
        _, add = M.additive_mask(c, p.km, self.device)
        if self.wrong == "mask_twice" and c.causal and p.km is not None:
            add = add + torch.where((p.km == 0).repeat_interleave(c.kv_group, 0)[:, None, None, :] & (add != 0), torch.tensor(c.neg), torch.tensor(0.0))
        s = torch.einsum("bqhd,bkhd->bhqk", Q, K) * scale + add
        if self.wrong == "last_key":
            s[..., -1] = s[..., -1] - 1000.0
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        P = e * (1.0 / e.sum(-1, keepdim=True))
        if self.wrong == "uniform":
            al = M.A.allowed_keys(c, p.km, self.device).expand_as(P).float()
            al = al + (al.sum(-1, keepdim=True) == 0).float()
            P = al / al.sum(-1, keepdim=True)
        if c.mean:
            P = M.head_mean_rule(P, c.nh) if self.wrong != "mean_order" else P.flip(1).double().mean(1).float()
        out = P.reshape(-1)
        if self.wrong == "short":
            out = out[:-1]
            p.P[:-1].copy_(out)
            return
        p.P.copy_(out)
        if self.wrong == "overrun":
            p.wins["P"].flat[p.wins["P"].offset + p.P.numel()] = 0.0


SMALL = [c for c in M.CASES if c.B * c.nh * c.Lq * c.Lk <= 40000 and c.d == 32]


@pytest.mark.parametrize("c", SMALL, ids=[c.id for c in SMALL])
def test_checks_pass_on_the_torch_stand_in(c):
    be, seed = Torch(), M.CASES.index(c)
    M.check_onehot(be, c, seed)
    M.check_uniform(be, c, seed)
    M.check_integer_scores(be, c, seed)
    if c.Lk > 16:
        M.check_invariances(be, c, seed)


def test_refusals_on_the_stand_in_and_a_stand_in_that_accepts():
    c = M.case("f32", 32, 17, 70)

    def refused(fn):
        with pytest.raises(Exception, match="GSTVD_E_UNSUPPORTED"):
            fn()
    M.check_refusals(Torch(), c, refused)
    with pytest.raises(BaseException):
        M.check_refusals(Torch("accepts"), c, refused)


@pytest.mark.parametrize("wrong,check", [("uniform", "integer"), ("uniform", "onehot"), ("last_key", "uniform"), ("last_key", "integer"),
                                         ("short", "onehot"), ("overrun", "uniform"), ("mean_order", "integer")])
def test_checks_catch_wrong_stand_ins(wrong, check):
    c = M.case("f32", 32, 17, 70, mean=wrong == "mean_order", mask="holes")
    fn = dict(integer=M.check_integer_scores, onehot=M.check_onehot, uniform=M.check_uniform)[check]
    with pytest.raises(AssertionError):
        fn(Torch(wrong), c, 1 if wrong == "overrun" else 0)
