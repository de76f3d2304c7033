"""Fixture of the attention maps: tests/golden/tiny_attn_maps.npz, modelled on tools/make_golden_mlm_fill.py.

Runs in the build container only.  It imports the reference tree through oracle.ref_harness and copies none of its text.

    python tools/make_golden_attn_maps.py

Inputs: oracle.make_golden.make_inputs() -- B 3, T 24, R 7, U 9, ragged text (24 / 17 / 11 tokens), row 2 with two image-padded
regions, answers of 5 / 3 / 7 tokens.  Weights: tests/golden/tiny_state.npz with every state-dict tensor that has a key component
in {query, key, query1, key1, query2, key2} multiplied by a factor (weights and biases alike; the fixture records the factors, not
a second state dict).  At the tiny initialisation the maps are indistinguishable from uniform (mean row maximum 0.066 over 24 text
keys, against 1 / 24 = 0.042): a kernel that returned 1 / n would pass.  PEAKEDNESS: for every map recorded, the mean row
maximum is at least MIN_MEAN_ROWMAX and the largest entry at most MAX_ENTRY, asserted here; if the committed state needs another
factor to meet that, change the factor, not the bounds.

FACTORS.  One factor does not meet the condition at every site of the committed states:
  * FACTOR 8 for the encoder's sites and the decoder's self-attention of tiny_state (encoder maps: mean row maximum 0.32-0.54,
    largest entry 0.75-0.96);
  * FACTOR_CROSS 11.5 for its tensors under `crossattention`: at 8 the cross-attention maps over 31 keys stay flat (mean row
    maximum 0.15), at 12 the second layer's largest entry passes 0.97, and the vision maps saturate above 8;
  * one factor PER SITE for the state of tests/golden/tiny_disc.npz, whose layers differ too much for any one factor (at 1.125
    the last text layer is flat, mean row maximum 0.12, where the first connection layer is at 0.969).  A site's factor scales
    the two tensors (and biases) that form its scores -- query / key of a self-attention layer, query2 / key1 of a connection
    layer's text-over-regions map, query1 / key2 of its regions-over-text map (attn_maps.site_of_parameter) -- so the ten
    factors are independent knobs.  They are found here, deterministically, by disc_factors(): sites in DISC_ORDER (an earlier
    site changes the inputs of a later one), two passes, a bisection on the mean row maximum towards DISC_TARGET, then down
    until the largest entry is under DISC_TOP, rounded to multiples of 1 / 16; recorded as disc::factor::<site>.
  * Rows with ONE allowed key (the first query under the causal mask) are 1.0 whatever the weights are: the condition is taken
    over the rows with at least two allowed keys, which is every row of an encoder map.

What is recorded (fp32):
  * in::*        the batch; factor, factor_cross
  * enc::t<i> [3, 2, 24, 24], enc::v<i> [3, 3, 7, 7], enc::c<i>::0 [3, 4, 24, 7], enc::c<i>::1 [3, 4, 7, 24]: what the reference's own
    bert_pretrained.bert(..., output_all_attention_masks=True) returns (models/vilbert_dialog.py:806-912), in its order;
  * dec::self<i> [3, 2, 9, 9], dec::cross<i> [3, 2, 9, 31] (regions first): the installed transformers returns None for
    output_attentions through the reference's BertGenerationEncoder, so the query / key Linears of attention.self and
    crossattention.self of every decoder layer are hooked during the reference model's own forward and the map is formed as
    softmax(Q K^T / sqrt(d) + mask) in float64 with the extended / inverted masks the harness handed the decoder stack; the
    value Linear and the attention module's output are hooked as well, and P V is asserted to equal that output within 1e-6, which
    pins the reconstruction to what the reference computed;
  * loss, logits: the reference's (loss, logits) of that forward;
  * disc::in::*, disc::t<i>, disc::v<i>, disc::c<i>::0/1: the same for the enc_only_a encoder of tests/golden/tiny_disc.npz (its
    own per-site factors, disc::factor::<site>), 2 rows: the fifth output of the eval branch of BertForMultiModalPreTraining.forward (:1519).
"""
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                   # noqa: E402
from oracle.make_golden import make_inputs                             # noqa: E402
from gst_visdial_amd.selfcheck import write_npz, load_npz, GOLDEN      # noqa: E402
from gst_visdial_amd.attn_maps import site_of_parameter              # noqa: E402

FACTOR = 8.0                   # the encoder's sites and the decoder's self-attention
FACTOR_CROSS = 11.5            # the decoder's cross-attention (key component "crossattention")
DISC_ORDER = ("t0", "t1", "v0", "c0::0", "c0::1", "t2", "v1", "c1::0", "c1::1", "t3")      # tiny_disc: its sites, earlier layers first
DISC_TARGET, DISC_TOP = 0.42, 0.94                                                          # aimed at, inside the two bounds
SCALED = ("query", "key", "query1", "key1", "query2", "key2")
MIN_MEAN_ROWMAX, MAX_ENTRY = 0.3, 0.97
FAILED = []                    # maps that miss the peakedness condition (all are listed before the generator gives up)


def scale_state(sd, site_factors=None):
    """The state dict with its query / key tensors scaled: by the factor of their site (tiny_disc), else by FACTOR_CROSS under
    `crossattention` and FACTOR elsewhere (tiny_state)."""
    out, n = {}, 0
    for k, v in sd.items():
        site = site_of_parameter(k)
        if site is None:
            out[k] = v
            continue
        assert any(c in SCALED for c in k.split("."))
        out[k] = v * (site_factors[site] if site_factors is not None else FACTOR_CROSS if site.startswith("decoder_cross") else FACTOR)
        n += 1
    assert n == sum(1 for k in sd if any(c in SCALED for c in k.split("."))) > 0
    return out


def peaked(name, p, allowed=None):
    """The peakedness condition of one recorded map.  `allowed` [.., Lq, Lk] bool (the decoder's maps): rows with ONE allowed key
    -- the first query under the causal mask -- are 1.0 there whatever the weights are, so no factor could bring them under
    MAX_ENTRY; the condition is taken over the rows with at least two allowed keys (every row of an encoder map)."""
    p = p.double()
    rs = p.sum(-1)
    assert bool(((rs - 1).abs() < 1e-5).all()), name
    rows = torch.ones(p.shape[:-1], dtype=torch.bool) if allowed is None else (allowed.sum(-1) >= 2).expand(p.shape[:-1])
    assert bool(rows.any())
    mrm, top = p.max(-1).values[rows].mean().item(), p[rows].max().item()
    print("%-16s %-18s mean row maximum %.3f, largest entry %.3f (%d of %d rows with two or more allowed keys)"
          % (name, tuple(p.shape), mrm, top, int(rows.sum()), rows.numel()))
    if not (mrm >= MIN_MEAN_ROWMAX and top <= MAX_ENTRY):
        FAILED.append(name)
    return p.float()


def disc_factors(maps_of):
    """One factor per site of the tiny_disc state (see FACTORS).  maps_of(factors) -> {site: map}."""
    def stats(f, site):
        p = maps_of(f)[site].double()
        return p.max(-1).values.mean().item(), p.max().item()

    def bisect(f, site, which, goal):
        lo, hi = 1.0 / 16, 64.0
        for _ in range(24):
            mid = math.sqrt(lo * hi)
            if stats(dict(f, **{site: mid}), site)[which] < goal:
                lo = mid
            else:
                hi = mid
        return max(1, round(lo * 16)) / 16.0
    f = {s: 1.0 for s in DISC_ORDER}
    for _ in range(2):
        for site in DISC_ORDER:
            f[site] = bisect(f, site, 0, DISC_TARGET)
            if stats(f, site)[1] > DISC_TOP:
                f[site] = bisect(f, site, 1, DISC_TOP)
    return f


def record_encoder(out, prefix, maps):
    t, v, c = maps
    for i, p in enumerate(t):
        out["%st%d" % (prefix, i)] = peaked("%st%d" % (prefix, i), p)
    for i, p in enumerate(v):
        out["%sv%d" % (prefix, i)] = peaked("%sv%d" % (prefix, i), p)
    for i, pair in enumerate(c):
        for j, p in enumerate(pair):
            out["%sc%d::%d" % (prefix, i, j)] = peaked("%sc%d::%d" % (prefix, i, j), p)
    return len(t), len(v), len(c)


def main():
    enc_cfg, dec_cfg = RH.write_tiny_configs(tempfile.mkdtemp(prefix="gstvd_maps_"))
    model, _ = RH.build_reference_model(enc_cfg, dec_cfg, mode="vd_eval_val", seed=0)
    model.load_state_dict(scale_state(load_npz("tiny_state.npz")), strict=True)
    model.eval()
    b = make_inputs()
    out = {"in::" + k: v for k, v in b.items()}
    out["factor"] = np.asarray(FACTOR, dtype=np.float64)
    out["factor_cross"] = np.asarray(FACTOR_CROSS, dtype=np.float64)

    # ---- encoder maps: the reference's own flag ------------------------------------------------------------------------------
    bert = model.encoder.bert_pretrained.bert
    with torch.no_grad():
        res = bert(b["enc_input_ids"], b["enc_image_features"], b["enc_image_spatials"], token_type_ids=b["enc_segments"],
                   attention_mask=b["enc_attention_mask"], image_attention_mask=b["enc_image_mask"], output_all_attention_masks=True)
    n = record_encoder(out, "enc::", res[4])
    assert n == (4, 2, 2), n
    p1, p2 = res[4][2][0]
    assert p1.shape == (3, 4, 24, 7) and p2.shape == (3, 4, 7, 24)          # (text queries over regions, region queries over tokens)

    # ---- decoder maps: hooks on the reference model's own forward ------------------------------------------------------------------
    stack = model.decoder.decoder.bert.encoder
    got, hooks = {}, []

    def keep(name):
        def hook(mod, args, output):
            got[name] = (output[0] if isinstance(output, tuple) else output).detach().double()
        return hook

    def masks(mod, args, kwargs):
        got["self_mask"] = kwargs["attention_mask"].detach().double()
        got["cross_mask"] = kwargs["encoder_attention_mask"].detach().double()
    hooks.append(stack.register_forward_pre_hook(masks, with_kwargs=True))
    for i, layer in enumerate(stack.layer):
        for kind, att in (("self", layer.attention.self), ("cross", layer.crossattention.self)):
            for w in ("query", "key", "value"):
                hooks.append(getattr(att, w).register_forward_hook(keep("%s%d.%s" % (kind, i, w))))
            hooks.append(att.register_forward_hook(keep("%s%d.out" % (kind, i))))
    dec_ids = b["dec_input_ids"].clone()
    with torch.no_grad():
        loss, logits = model(enc_image_features=b["enc_image_features"], enc_image_spatials=b["enc_image_spatials"],
                             enc_image_mask=b["enc_image_mask"], enc_input_ids=b["enc_input_ids"], enc_segments=b["enc_segments"],
                             enc_attention_mask=b["enc_attention_mask"], dec_input_ids=dec_ids,
                             dec_attention_mask=b["dec_attention_mask"], dec_labels=b["dec_labels"])
    for h in hooks:
        h.remove()
    assert torch.equal(dec_ids, b["dec_input_ids"])
    out.update(loss=loss.detach().reshape(1), logits=logits.detach())
    nh = RH.TINY_DEC_CFG["num_attention_heads"]
    d = RH.TINY_DEC_CFG["hidden_size"] // nh

    def heads(x):
        return x.view(x.shape[0], x.shape[1], nh, d).permute(0, 2, 1, 3)
    for i in range(len(stack.layer)):
        for kind, mask in (("self", got["self_mask"]), ("cross", got["cross_mask"])):
            q, k, v = (heads(got["%s%d.%s" % (kind, i, w)]) for w in ("query", "key", "value"))
            p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + mask, -1)
            ctx = (p @ v).permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], nh * d)
            err = (ctx - got["%s%d.out" % (kind, i)]).abs().max().item()
            print("decoder layer %d %s-attention: |P V - module output| max %.2e" % (i, kind, err))
            assert err < 1e-6
            out["dec::%s%d" % (kind, i)] = peaked("dec::%s%d" % (kind, i), p, mask > -1.0)
    assert out["dec::self0"].shape == (3, 2, 9, 9) and out["dec::cross0"].shape == (3, 2, 9, 31)

    # ---- the enc_only_a eval branch's fifth output ---------------------------------------------------------------------------------
    fx = load_npz("tiny_disc.npz")
    params = dict(model_enc_config=enc_cfg, model_dec_config=dec_cfg, gpu_ids=[0], model="enc_only_a", mode="vd_eval_val",
                  batch_size=1, device=torch.device("cpu"))
    enc = RH._install_shims()["E"].VisualDialogEncoder(params)
    enc.eval()
    disc_sd = {k[len("state::"):]: v for k, v in fx.items() if k.startswith("state::")}
    Td = fx["in::tokens"].shape[-1]
    d_in = dict(ids=fx["in::tokens"].reshape(-1, Td)[[0, 37]].clone(), seg=fx["in::segments"].reshape(-1, Td)[[0, 37]].clone(),
                att=fx["attention_mask"][[0, 37]].clone().float(), image_feat=fx["in::image_feat"][[0, 1]].clone(),
                image_loc=fx["in::image_loc"][[0, 1]].clone(), image_mask=fx["in::image_mask"][[0, 1]].clone())

    def disc_maps(factors):
        enc.load_state_dict(scale_state(disc_sd, factors), strict=True)
        with torch.no_grad():
            res = enc.bert_pretrained(d_in["ids"], d_in["image_feat"], d_in["image_loc"], token_type_ids=d_in["seg"],
                                      attention_mask=d_in["att"], image_attention_mask=d_in["image_mask"], output_all_attention_masks=True)
        assert len(res) == 5
        return res[4]

    def by_site(factors):
        t, v, c = disc_maps(factors)
        m = {"t%d" % i: p for i, p in enumerate(t)}
        m.update({"v%d" % i: p for i, p in enumerate(v)})
        m.update({"c%d::%d" % (i, j): p for i, pair in enumerate(c) for j, p in enumerate(pair)})
        return m
    factors = disc_factors(by_site)
    assert sorted(factors) == sorted(set(filter(None, map(site_of_parameter, disc_sd))))
    print("tiny_disc factors:", ", ".join("%s %.4g" % (s_, factors[s_]) for s_ in DISC_ORDER))
    out.update({"disc::in::" + k: v for k, v in d_in.items()})
    out.update({"disc::factor::" + k: np.asarray(v, dtype=np.float64) for k, v in factors.items()})
    record_encoder(out, "disc::", disc_maps(factors))

    assert not FAILED, "not peaked enough / saturated: %s -- change the factors, not the bounds" % ", ".join(FAILED)
    files = write_npz(os.path.join(GOLDEN, "tiny_attn_maps.npz"), {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v))
                                                                  for k, v in out.items()})
    print("wrote", [(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
