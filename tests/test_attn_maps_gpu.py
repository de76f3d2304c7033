"""Attention maps through the public interface on a real MI355X: EncoderDecoderModel.attention_maps and
VisualDialogEncoder.attention_maps against tests/golden/tiny_attn_maps.npz (tools/make_golden_attn_maps.py: the reference's own
output_all_attention_masks=True maps for the encoder, float64 maps from its hooked query / key Linears for the decoder), on the
fp32 and the bf16 engine.  The weights are those of tests/golden/tiny_state.npz with the query / key tensors scaled by the factors
the fixture records."""
import pytest
import torch

from conftest import load_npz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32_GATE = 1e-4            # the project's fp32 gate: of the map's maximum
# Largest |map - fixture| / max(fixture map) of the bf16 engine, measured on an MI355X ("Attention maps"): over
# the 14 maps of the enc-dec model (the second decoder cross-attention map) and over the 10 maps of the enc_only_a encoder; the
# tests allow twice that.
BF16_MAPS_MEASURED = 1.79e-2
BF16_DISC_MAPS_MEASURED = 3.93e-2
KEYWORDS = ("enc_image_features", "enc_image_spatials", "enc_image_mask", "enc_input_ids", "enc_segments", "enc_attention_mask",
            "dec_input_ids", "dec_attention_mask", "dec_labels")


@pytest.fixture(scope="module")
def fx():
    return load_npz("tiny_attn_maps.npz")


def scaled(sd, fx, disc=False):
    """The state dict with its query / key tensors scaled as the fixture's generator scaled them: per site for the enc_only_a
    state, by `factor_cross` under crossattention and `factor` elsewhere for the enc-dec state."""
    from gst_visdial_amd.attn_maps import site_of_parameter
    out = {}
    for k, v in sd.items():
        site = site_of_parameter(k)
        f = 1.0
        if site is not None:
            f = float(fx["disc::factor::" + site]) if disc else float(fx["factor_cross"]) if site.startswith("decoder_cross") else float(fx["factor"])
        out[k] = v * f
    return out


def batch(fx):
    return {k: fx["in::" + k].clone().to(DEV) for k in KEYWORDS}


class Run(object):
    """One engine precision: the model, a plain forward, the full maps call, a plain forward after it."""

    def __init__(self, precision, fx):
        from gst_visdial_amd.selfcheck import build_tiny_model
        self.model, self.params, _ = build_tiny_model(precision, DEV, mode="vd_eval_val")
        self.model.load_state_dict(scaled(load_npz("tiny_state.npz"), fx), strict=True)
        self.model.eval()
        with torch.no_grad():
            self.plain = self.forward(fx)
            self.out, self.maps = self.model.attention_maps(**batch(fx))
            self.out = tuple(x.clone() for x in self.out)
            self.states_maps = self.states()
            self.plain_after = self.forward(fx)
        torch.cuda.synchronize()

    def states(self):
        last = self.model.engine.last
        return last["enc_t"].t.clone(), last["enc_v"].t.clone()

    def forward(self, fx):
        loss, logits = self.model(**batch(fx))
        return (loss.clone(), logits.clone()) + self.states()


_RUNS = {}


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def run(request, fx):
    if request.param not in _RUNS:
        _RUNS[request.param] = Run(request.param, fx)
    return request.param, _RUNS[request.param]


def named(maps):
    """fixture key -> tensor, for a ModelAttentionMaps (or an AttentionMaps under `prefix`)."""
    out = {}
    enc = maps.encoder if hasattr(maps, "encoder") else maps
    for i, p in zip(enc.layers["t"], enc.t):
        out["t%d" % i] = p
    for i, p in zip(enc.layers["v"], enc.v):
        out["v%d" % i] = p
    for i, (p1, p2) in zip(enc.layers["c"], enc.c):
        out["c%d::0" % i], out["c%d::1" % i] = p1, p2
    if hasattr(maps, "encoder"):
        out = {"enc::" + k: v for k, v in out.items()}
        for i, p in zip(maps.layers["decoder_self"], maps.decoder_self):
            out["dec::self%d" % i] = p
        for i, p in zip(maps.layers["decoder_cross"], maps.decoder_cross):
            out["dec::cross%d" % i] = p
    return out


def worst(got, fx, prefix=""):
    w = {}
    for k, v in got.items():
        ref = fx[prefix + k].to(v.device)
        assert v.dtype == torch.float32 and v.is_cuda and tuple(v.shape) == tuple(ref.shape), k
        assert bool(torch.isfinite(v).all()), k
        w[k] = float((v.double() - ref.double()).abs().max() / ref.double().max())
    return w


def test_every_map_matches_the_fixture(run, fx):
    prec, r = run
    got = named(r.maps)
    assert len(got) == 14 and r.maps.layers == dict(t=[0, 1, 2, 3], v=[0, 1], c=[0, 1], decoder_self=[0, 1], decoder_cross=[0, 1])
    w = worst(got, fx)
    for k in sorted(w):
        print("%s engine: %-14s |map - fixture| / max %.3e" % (prec, k, w[k]))
    print("%s engine: largest over the 14 maps %.3e" % (prec, max(w.values())))
    bound = FP32_GATE if prec == "fp32" else 2.0 * BF16_MAPS_MEASURED
    assert max(w.values()) <= bound, (max(w.values()), bound)


def test_row_sums_and_exact_zeros(run, fx):
    prec, r = run
    got = named(r.maps)
    tm, vm, dm = (fx["in::" + k].to(DEV) for k in ("enc_attention_mask", "enc_image_mask", "dec_attention_mask"))
    em = torch.cat([vm, tm], 1)
    for k, v in got.items():
        rs = float((v.double().sum(-1) - 1).abs().max())
        assert rs <= 1e-5, (k, rs)                   # (at most 31 keys)
    upper = torch.triu(torch.ones(9, 9, dtype=torch.bool, device=DEV), 1)

    def zeros(k, dead):
        v = got[k]
        bad = int((v[dead.expand_as(v)] != 0).sum())
        assert bad == 0 and bool(dead.any()), "%s: %d masked entries are not exactly 0" % (k, bad)
    for i in range(4):
        zeros("enc::t%d" % i, (tm == 0)[:, None, None, :])                     # padded text keys
    for i in range(2):
        zeros("enc::v%d" % i, (vm == 0)[:, None, None, :])                     # the image-padded regions of row 2
        zeros("enc::c%d::0" % i, (vm == 0)[:, None, None, :])
        zeros("enc::c%d::1" % i, (tm == 0)[:, None, None, :])
        zeros("dec::self%d" % i, upper[None, None] | (dm == 0)[:, None, None, :])   # the upper triangle and the pad keys
        zeros("dec::cross%d" % i, (em == 0)[:, None, None, :])
    assert bool((vm[2, -2:] == 0).all()) and float(got["enc::v0"][2, :, :, -2:].abs().max()) == 0.0


def test_forward_and_encoder_states_are_bit_identical_with_and_without_a_request(run):
    prec, r = run
    names = ("loss", "logits", "encoder text states", "encoder vision states")
    for n, a, b in zip(names, r.plain, r.out + r.states_maps):
        assert torch.equal(a, b), "%s: a maps call changes %s" % (prec, n)
    for n, a, b in zip(names, r.plain, r.plain_after):
        assert torch.equal(a, b), "%s: %s differs after a maps call" % (prec, n)
    assert r.model.engine._maps is None


def test_select_subsets_equal_the_full_call_bit_for_bit(run, fx):
    prec, r = run
    full = named(r.maps)
    sel = {"t": [3, 1], "c": "all", "decoder_cross": (1,)}
    with torch.no_grad():
        out, maps = r.model.attention_maps(select=sel, **batch(fx))
    assert maps.layers == dict(t=[1, 3], v=[], c=[0, 1], decoder_self=[], decoder_cross=[1])
    got = named(maps)
    assert sorted(got) == ["dec::cross1", "enc::c0::0", "enc::c0::1", "enc::c1::0", "enc::c1::1", "enc::t1", "enc::t3"]
    assert maps.encoder.v == [] and maps.decoder_self == []
    for k, v in got.items():
        assert torch.equal(v, full[k]), k
    assert torch.equal(out[1], r.plain[1])
    with torch.no_grad():
        _, none = r.model.attention_maps(select={}, **batch(fx))
    assert named(none) == {}


def test_head_mean_equals_the_per_head_maps_reduced_by_the_rule(run, fx):
    prec, r = run
    with torch.no_grad():
        _, maps = r.model.attention_maps(heads="mean", **batch(fx))
    got, full = named(maps), named(r.maps)
    assert sorted(got) == sorted(full)
    for k, v in got.items():
        p = full[k]
        acc = p[:, 0].clone()
        for h in range(1, p.shape[1]):
            acc = acc + p[:, h]
        want = acc * (torch.ones((), dtype=torch.float32, device=DEV) / p.shape[1])
        assert tuple(v.shape) == (p.shape[0],) + tuple(p.shape[2:]) and torch.equal(v, want), k


def test_the_encoder_alone_gives_the_same_maps(run, fx):
    """VisualDialogEncoder.attention_maps of an enc-dec model's encoder: the stand-alone route on the model's engine."""
    prec, r = run
    b = batch(fx)
    with torch.no_grad():
        maps = r.model.encoder.attention_maps(b["enc_input_ids"], b["enc_image_features"], b["enc_image_spatials"],
                                              token_type_ids=b["enc_segments"], attention_mask=b["enc_attention_mask"],
                                              image_attention_mask=b["enc_image_mask"])
    got, full = named(maps), named(r.maps)
    assert len(got) == 10 and maps.layers == dict(t=[0, 1, 2, 3], v=[0, 1], c=[0, 1])
    for k, v in got.items():
        assert torch.equal(v, full["enc::" + k]), k
    from gst_visdial_amd._lib import GstvdError
    with pytest.raises(GstvdError):
        r.model.encoder.attention_maps(b["enc_input_ids"], b["enc_image_features"], b["enc_image_spatials"], select={"decoder_self": "all"})


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_enc_only_maps_match_the_fixture(prec, fx):
    from gst_visdial_amd.selfcheck import build_tiny_disc_encoder
    enc, params, dfx = build_tiny_disc_encoder(prec, None)
    enc.load_state_dict(scaled({k[len("state::"):]: v for k, v in dfx.items() if k.startswith("state::")}, fx, disc=True), strict=True)
    enc = enc.to(DEV).eval()
    d = {k: fx["disc::in::" + k].to(DEV) for k in ("ids", "seg", "att", "image_feat", "image_loc", "image_mask")}
    args = (d["ids"], d["image_feat"], d["image_loc"])
    kw = dict(token_type_ids=d["seg"], attention_mask=d["att"], image_attention_mask=d["image_mask"])
    with torch.no_grad():
        score0, _ = enc.nsp_scores(*args, **kw)
        score0 = score0.clone()
        maps = enc.attention_maps(*args, **kw)
        score1, _ = enc.nsp_scores(*args, **kw)
    got = named(maps)
    assert len(got) == 10
    w = worst(got, fx, "disc::")
    print("%s enc_only_a engine: largest |map - fixture| / max over the 10 maps %.3e" % (prec, max(w.values())))
    assert max(w.values()) <= (FP32_GATE if prec == "fp32" else 2.0 * BF16_DISC_MAPS_MEASURED)
    assert torch.equal(score0, score1)
    from gst_visdial_amd._lib import GstvdError
    enc.train()
    with pytest.raises(GstvdError, match="eval"):
        enc.attention_maps(*args, **kw)
    enc.eval()
    params["mode"] = "vd_train"
    with pytest.raises(GstvdError, match="eval"):
        enc.attention_maps(*args, **kw)


def test_training_state_train_mode_and_decode_calls_raise(run, fx):
    from gst_visdial_amd import attn_maps
    from gst_visdial_amd._lib import GstvdError
    prec, r = run
    m, b = r.model, batch(fx)
    m.train()
    try:
        with pytest.raises(GstvdError, match="eval mode only"):
            m.attention_maps(**b)
    finally:
        m.eval()
    r.params["mode"] = "vd_train"
    try:
        with pytest.raises(GstvdError, match="eval mode only"):
            m.attention_maps(**b)
    finally:
        r.params["mode"] = "vd_eval_val"
    with pytest.raises(GstvdError):
        m.attention_maps(heads="max", **b)
    with pytest.raises(GstvdError):
        m.attention_maps(select={"t": [4]}, **b)
    # the decode calls and candidate scoring serve no request
    eng = m.engine
    req = attn_maps.MapRequest(attn_maps.parse_select(None, attn_maps.layer_counts(eng.enc_cfg, eng.dec_cfg)), False)
    enc_kw = {k: b[k] for k in KEYWORDS[:6]}
    start = b["dec_input_ids"][:, :1].contiguous()
    r.params["mode"] = "vd_generate"
    try:
        with attn_maps.capture(eng, req), torch.no_grad():
            with pytest.raises(GstvdError, match="^sample under an attention-map request"):
                m(dec_input_ids=start, **enc_kw)
            with pytest.raises(GstvdError, match="^beam_search under an attention-map request"):
                m.beam_search(dec_input_ids=start, num_beams=2, **enc_kw)
            with pytest.raises(GstvdError, match="^sample_ranked under an attention-map request"):
                m.sample_ranked(dec_input_ids=start, num_samples=2, **enc_kw)
            with pytest.raises(GstvdError, match="^score_candidates under an attention-map request"):
                m.score_candidates(b["enc_image_features"], b["enc_image_spatials"], b["enc_image_mask"], b["enc_input_ids"],
                                   b["enc_segments"], b["enc_attention_mask"], b["dec_input_ids"], b["dec_attention_mask"], 1)
    finally:
        r.params["mode"] = "vd_eval_val"
    assert eng._maps is None and req.out == {}
    with torch.no_grad():
        after = r.forward(fx)
    for a, c in zip(r.plain, after):
        assert torch.equal(a, c)
