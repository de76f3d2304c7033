"""Generate the full-configuration fixtures by importing and running the REAL reference on CPU.

Run only in the build container:  python oracle/make_golden_full.py
(the reference's Python never travels; only the arrays written here do).

The full bert-base model (config/bert_base_6layer_6conect_{enc,dec}.json) has 435 M parameters: its state dict cannot be
stored.  Instead the reference model is loaded with a state dict that `synthetic_state()` regenerates from a seed, so that
tests/test_oracle_vs_reference.py can rebuild the same weights and check the oracle against the recorded outputs without
the reference tree.

Fixtures written:
  full_cfg_state.json  {"enc": {...}, "dec": {...}, "state": [[name, shape, index of the key it is tied to or -1], ...]}:
                       the two model config dicts and the reference's 861 state-dict keys in order (tied keys share one
                       tensor in the reference model and one generated tensor here)
  full_ref.npz         eval()-mode outputs of the reference on `full_batch()` under that state: loss and the logits
                       [2, 25, 30522], one array "logits/u" [2, 30522] per answer position u (6 MB in all: stored in
                       numbered parts of less than 1 MiB, gst_visdial_amd.selfcheck.write_npz)
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402
from gst_visdial_amd.selfcheck import write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
STATE_SEED = 1


def synthetic_state(spec, seed=STATE_SEED):
    """The state dict described by `spec` (full_cfg_state.json "state"), regenerated from `seed`: weights N(0, 0.02) as
    BERT's own init draws them, LayerNorm weights 1 + N(0, 0.1) and biases N(0, 0.02) so that none of them is trivial."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    keys = [k for k, _, _ in spec]
    for name, shape, tied in spec:
        if tied >= 0:
            sd[name] = sd[keys[tied]]
            continue
        x = torch.randn(shape, generator=g)
        if "LayerNorm" in name and name.endswith(".weight"):
            sd[name] = x.mul_(0.1).add_(1.0)
        else:
            sd[name] = x.mul_(0.02)
    return sd


def full_batch():
    """Two rows at T = 48 (one padded from position 30), 37 regions, answer length 25."""
    g = torch.Generator().manual_seed(5)
    B, T, R, U = 2, 48, 37, 25
    ids = torch.randint(1000, 30000, (B, T), generator=g)
    ids[:, 0] = 101
    ids[1, 30:] = 0
    seg = (torch.arange(T)[None] // 7 % 2).expand(B, T).contiguous()
    att = (ids != 0).float()
    feats = torch.randn(B, R, 2048, generator=g).abs()
    loc = torch.rand(B, R, 5, generator=g)
    im = torch.ones(B, R)
    dec_ids = torch.zeros(B, U, dtype=torch.long)
    dec_ids[:, 0] = 101
    dec_ids[:, 1:6] = torch.randint(1000, 30000, (B, 5), generator=g)
    labels = torch.zeros(B, U, dtype=torch.long)
    labels[:, :5] = dec_ids[:, 1:6]
    labels[:, 5] = 102
    datt = torch.zeros(B, U)
    datt[:, :7] = 1
    return dict(enc_input_ids=ids, enc_segments=seg, enc_attention_mask=att, enc_image_features=feats,
                enc_image_spatials=loc, enc_image_mask=im, dec_input_ids=dec_ids, dec_attention_mask=datt, dec_labels=labels)


def main():
    e = rh.REFERENCE_ROOT + "/config/bert_base_6layer_6conect_enc.json"
    d = rh.REFERENCE_ROOT + "/config/bert_base_6layer_6conect_dec.json"
    model, params = rh.build_reference_model(e, d, seed=1)
    model.eval()
    ref_sd = model.state_dict()
    first = {}
    spec = []
    for i, (k, v) in enumerate(ref_sd.items()):
        tied = first.setdefault(v.data_ptr(), i)
        spec.append([k, list(v.shape), tied if tied != i else -1])
    sd = synthetic_state(spec)
    model.load_state_dict(sd, strict=True)
    for k, v in model.state_dict().items():        # tied keys: one tensor in the model, one generated tensor in `sd`
        assert torch.equal(v, sd[k]), k
    b = full_batch()
    with torch.no_grad():
        loss, logits = model(enc_image_features=b["enc_image_features"], enc_image_spatials=b["enc_image_spatials"],
                             enc_image_mask=b["enc_image_mask"], enc_input_ids=b["enc_input_ids"], enc_segments=b["enc_segments"],
                             enc_sep_indices=None, enc_mlm_labels=None, enc_attention_mask=b["enc_attention_mask"],
                             dec_input_ids=b["dec_input_ids"].clone(), dec_attention_mask=b["dec_attention_mask"],
                             dec_labels=b["dec_labels"])
    with open(os.path.join(OUT, "full_cfg_state.json"), "w") as f:
        json.dump({"enc": json.load(open(e)), "dec": json.load(open(d)), "state": spec}, f, indent=0)
    out = {"loss": loss.detach().numpy()}
    out.update(("logits/%d" % u, logits[:, u].detach().contiguous().numpy()) for u in range(logits.shape[1]))
    write_npz(os.path.join(OUT, "full_ref.npz"), out)
    print("full config: %d keys, %d parameters, loss %.6f, logits %s" % (len(spec), sum(v.numel() for v in ref_sd.values()),
                                                                         loss.item(), tuple(logits.shape)))


if __name__ == "__main__":
    main()
