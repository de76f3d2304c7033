"""CPU-side checks of the self-training glue: the module imports, the header declares and _lib binds the two entry points, and
argument errors are raised before any device call (there is no GPU in the CPU suite)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gstvd_context_append", "gstvd_dialog_rows")


def test_selftrain_imports_and_exposes_the_two_calls():
    from gst_visdial_amd import selftrain, ops
    assert callable(selftrain.generate_dialogs) and callable(selftrain.dialog_train_batch)
    assert callable(ops.context_append) and callable(ops.dialog_rows)
    assert selftrain.MAX_CAPTION_LEN == 38 and ops.DIALOG_MAX_SEP == 25


def test_header_declares_and_lib_binds_both_entries():
    from gst_visdial_amd import _lib
    src = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s_t\s*\*" % (name, name), src), name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i32 and len(args) == 2
    assert _lib.ABI_VERSION == 9                                 # entries added, no signature changed
    import ctypes as C
    d = _lib.DialogRowsDesc
    assert d.mask_prob.size == 8 and d.threshold.size == 8 and dict((f[0], f[1]) for f in d._fields_)["mask_prob"] is C.c_double
    assert "dialog.hip" in open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "Makefile")).read()


def test_library_exports_both_entries():
    from gst_visdial_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name)


def _dialogs(B=2, R=3, U=18):
    return dict(questions=torch.full((B, R, U), 200, dtype=torch.long), answers=torch.full((B, R, U), 201, dtype=torch.long),
                ppl=torch.ones(B, R), abnormal=torch.zeros(B, dtype=torch.bool))


def _image(B=2):
    return dict(enc_image_feat=torch.zeros(B, 37, 8), enc_image_loc=torch.zeros(B, 37, 5), enc_image_mask=torch.ones(B, 37))


PARAMS = dict(select_data=1, threshold=50.0, mask_prob=0.15, max_seq_len=32, max_utt_len=25)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from gst_visdial_amd import selftrain, ops, _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a device call was reached"))
    cap = torch.full((2, 8), 150, dtype=torch.long)
    # 2R > 25 separators
    with pytest.raises(_lib.GstvdError, match="separators"):
        selftrain.dialog_train_batch(_dialogs(R=13), cap, _image(), PARAMS)
    d = _dialogs(R=13)
    with pytest.raises(_lib.GstvdError, match="separators"):
        ops.dialog_rows(cap, d["questions"], d["answers"], d["ppl"], 32, 25, 1, 50.0, 0.0)
    # mask noise without uniforms, drawing forced off
    with pytest.raises(_lib.GstvdError, match="u_tok"):
        selftrain.dialog_train_batch(_dialogs(), cap, _image(), PARAMS, u_tok=False)
    d = _dialogs()
    with pytest.raises(_lib.GstvdError, match="u_tok"):
        ops.dialog_rows(cap, d["questions"], d["answers"], d["ppl"], 32, 25, 1, 50.0, 0.15, u_tok=None)
    # CPU tensors: there is no CPU path
    with pytest.raises(_lib.GstvdError, match="GPU tensors"):
        selftrain.dialog_train_batch(_dialogs(), cap, _image(), dict(PARAMS, mask_prob=0.0))
    with pytest.raises(_lib.GstvdError, match="GPU tensors"):
        ops.dialog_rows(cap, d["questions"], d["answers"], d["ppl"], 32, 25, 1, 50.0, 0.0)
    ids, ln = torch.zeros(2, 32, dtype=torch.long), torch.zeros(2, dtype=torch.long)
    flags = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.GstvdError, match="GPU tensors"):
        ops.context_append(ids, ln, d["questions"][:, 0], 102, flags, flags.clone())
    with pytest.raises(_lib.GstvdError, match="GPU tensors"):
        selftrain.generate_dialogs(None, None, dict(enc_input_ids=ids, enc_segments=ids.clone(), enc_input_len=ln), num_rounds=1)
    # shapes the kernel's lanes do not cover
    with pytest.raises(_lib.GstvdError):
        ops.dialog_rows(torch.zeros(2, 65, dtype=torch.long), d["questions"], d["answers"], d["ppl"], 32, 25, 1, 50.0, 0.0)
    with pytest.raises(_lib.GstvdError):
        ops.dialog_rows(cap, d["questions"], d["answers"], d["ppl"], 32, 2, 1, 50.0, 0.0)


def test_image_noise_is_the_reference_rule_in_float64():
    from gst_visdial_amd.selftrain import image_noise
    p = 0.15
    u = torch.tensor([[0.1349999, 0.135, 0.1350001, 0.14, 0.15, 0.0, 0.9, 0.01]], dtype=torch.float64)
    mask = torch.tensor([[1., 1., 1., 1., 1., 1., 1., 0.]])
    feats = torch.ones(1, 8, 3)
    want = []
    for i in range(8):                                           # utils/data_utils.py:89-101, the lines restated
        prob = float(u[0, i])
        zero = False
        if mask[0, i] != 0 and prob < p:
            prob /= p
            zero = prob < 0.9
        want.append(0.0 if zero else 1.0)
    got = image_noise(feats, mask, u, p)
    assert got[0, :, 0].tolist() == want and want[0] == 0.0 and want[5] == 0.0 and want[3] == 1.0 and want[7] == 1.0
    assert torch.equal(feats, torch.ones(1, 8, 3))              # a new tensor: the caller's features are left alone
