"""In-domain filter, what needs no GPU: the header's declarations, the ctypes binding and the descriptor fields agree (no ABI bump);
ops.gauss_fit / ops.gauss_logprob and InDomainFilter refuse bad arguments by name before anything is launched; CPU tensors
raise; the documents name the feature and its two departures."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gstvd_gauss_fit_ws_bytes", "gstvd_gauss_fit", "gstvd_gauss_w_packed_elems", "gstvd_gauss_logprob")
CTYPE = {"const void*": C.c_void_p, "void*": C.c_void_p, "double*": C.c_void_p, "const double*": C.c_void_p, "uint8_t*": C.c_void_p,
         "int64_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}


def struct_fields(hdr, name):
    """(type, field) pairs of `typedef struct { ... } name;` in declaration order."""
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(.*?[\s*])(\w+)$", decl)
            out.append((m.group(1).replace(" *", "*").strip(), m.group(2)))
    return out


def test_entry_points_are_declared_bound_and_described_without_an_abi_bump():
    from gst_visdial_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gstvd_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 9 and "GSTVD_F16 = 2" in hdr and _lib.F16 == 2
    assert "GSTVD_GAUSS_MAX_D = %d" % _lib.GAUSS_MAX_D in hdr and "GSTVD_GAUSS_FIT_SLAB = %d" % _lib.GAUSS_FIT_SLAB in hdr
    for cname, cls in (("gstvd_gauss_fit_t", _lib.GaussFitDesc), ("gstvd_gauss_logprob_t", _lib.GaussLogprobDesc)):
        want = struct_fields(hdr, cname)
        assert [f for _, f in want] == [f for f, _ in cls._fields_], cname
        for (ctype, field), (_, bound) in zip(want, cls._fields_):
            assert CTYPE[ctype] is bound, (cname, field, ctype)
    assert _lib.SIGNATURES["gstvd_gauss_fit"][1][0]._type_ is _lib.GaussFitDesc
    assert _lib.SIGNATURES["gstvd_gauss_logprob"][1][0]._type_ is _lib.GaussLogprobDesc
    mk = open(os.path.join(ROOT, "gst_visdial_amd", "csrc", "Makefile")).read()
    assert "indomain.hip" in mk
    expect = open(os.path.join(ROOT, "tools", "kernel_resources.expect")).read()
    for k in ("gauss_colsum_kernel 0", "gauss_syrk_kernel 0", "gauss_logprob_kernel 0"):
        assert k in expect, k


def test_documents_name_the_feature_and_its_departures():
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "InDomainFilter" in readme and "In-domain image filter" in design
    for needle in ("InDomainFilter", "gstvd_gauss_fit", "gstvd_gauss_logprob", "clip_in_domain_filtering.py", "validate_args", "-threshold"):
        assert needle in integ, needle
    assert "bench_indomain.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "indomain.txt" in open(os.path.join(ROOT, "profiles", "README.md")).read()


def test_ops_refuse_bad_arguments_by_name_and_cpu_tensors():
    from gst_visdial_amd import ops
    from gst_visdial_amd._lib import GstvdError
    ok = torch.zeros(40, 32, dtype=torch.float16)
    for bad, word in ((torch.zeros(40, 32, dtype=torch.bfloat16), "float16 or float32"), (torch.zeros(40, 32, dtype=torch.float64), "float16 or float32"),
                      (torch.zeros(40, 24), "multiple of 16"), (torch.zeros(40, 1040), "multiple of 16"), (torch.zeros(40, 0), "multiple of 16"),
                      (torch.zeros(32), "2-D"), (torch.zeros(1, 32), "at least 2 rows"), (torch.zeros(40, 64)[:, ::2], "dense rows"),
                      ([[0.0] * 32] * 4, "2-D tensor")):
        with pytest.raises(GstvdError, match=word):
            ops.gauss_fit(bad)
    with pytest.raises(GstvdError, match="GPU tensors"):
        ops.gauss_fit(ok)
    mean, w = torch.zeros(32, dtype=torch.float64), torch.zeros(128 * 2 * 3, dtype=torch.float64)
    with pytest.raises(GstvdError, match="GPU tensors"):
        ops.gauss_logprob(ok, mean, w, 1.0, 0.0)
    with pytest.raises(GstvdError, match="at least 1 row"):
        ops.gauss_logprob(ok[:0], mean, w, 1.0, 0.0)
    with pytest.raises(GstvdError, match="multiple of 16"):
        ops.gauss_logprob(torch.zeros(4, 24), mean, w, 1.0, 0.0)
    with pytest.raises(GstvdError, match="gauss_pack_w"):
        ops.gauss_pack_w(torch.zeros(24, 24, dtype=torch.float64))
    with pytest.raises(GstvdError, match="gauss_pack_w"):
        ops.gauss_pack_w(torch.zeros(32, 32))


def test_filter_refuses_use_before_a_fit_and_a_state_that_is_not_one_fit():
    from gst_visdial_amd.indomain import InDomainFilter
    from gst_visdial_amd._lib import GstvdError
    f = InDomainFilter(device="cpu")
    for call in (lambda: f.log_prob(torch.zeros(2, 32)), lambda: f.select(torch.zeros(2, 32), 0.0), f.n_kept, f.state_dict,
                 lambda: f.score_batches([], [])):
        with pytest.raises(GstvdError, match="fit"):
            call()
    good = {"mean": torch.zeros(32, dtype=torch.float64), "cov": torch.eye(32, dtype=torch.float64),
            "w_packed": torch.zeros(128 * 2 * 3, dtype=torch.float64), "half_log_det": torch.tensor(0.0, dtype=torch.float64)}
    with pytest.raises(GstvdError, match="missing 'cov'"):
        f.load_state_dict({k: v for k, v in good.items() if k != "cov"})
    with pytest.raises(GstvdError, match="one fit"):
        f.load_state_dict(dict(good, w_packed=torch.zeros(5, dtype=torch.float64)))
    f.load_state_dict(good)                                     # a CPU-resident state loads; scoring it still needs the device
    with pytest.raises(GstvdError, match="GPU tensors"):
        f.log_prob(torch.zeros(2, 32))
    with pytest.raises(GstvdError, match="CPU|cpu|GPU"):
        InDomainFilter(device="cpu").fit(torch.zeros(40, 32))
