"""The oracle against the reference at the full bert-base configuration (config/bert_base_6layer_6conect_{enc,dec}.json),
through fixtures that oracle/make_golden_full.py recorded by running the reference: the reference's 861 state-dict keys,
loaded with weights that oracle.make_golden_full.synthetic_state() regenerates from a seed, and its loss and logits on
full_batch()."""
import json
import os

import torch

from conftest import GOLDEN, load_npz
from oracle import make_golden_full as mf
from oracle import vd_oracle as O


def test_full_config_forward_matches_reference():
    with open(os.path.join(GOLDEN, "full_cfg_state.json")) as f:
        fx = json.load(f)
    ref = load_npz("full_ref.npz")
    enc_cfg, dec_cfg, spec = fx["enc"], fx["dec"], fx["state"]
    assert len(spec) == 861
    sd = mf.synthetic_state(spec)
    b = mf.full_batch()
    with torch.no_grad():
        out = O.model_forward(sd, enc_cfg, dec_cfg, b)
    logits = torch.stack([ref["logits/%d" % u] for u in range(out["logits"].shape[1])], 1)
    assert logits.shape == out["logits"].shape == (2, 25, 30522)
    assert (out["logits"] - logits).abs().max().item() < 1e-4
    assert abs(out["loss"].item() - ref["loss"].item()) < 1e-5
