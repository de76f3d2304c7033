"""Exact layer of the sampling tests on a real MI355X (tests/exact_sample.py): every case of the table through
ops.sample_topk -- one launch of at most 64 copies of a row with chosen uniforms, ids compared with the float64 kept set (exactly
at the midpoints and ends, to the two neighbours of a step, bit-predictable on tie rows), every window checked, the launch repeated.
The harness itself is proved on the CPU by tests/test_exact_sample_harness_cpu.py.

Premises that only the hardware can confirm -- __expf(0) == 1 (tie rows) and a correctly rounded fp32 division by the temperature
(division-tie rows) -- are what those cases assert."""
import ctypes as C

import pytest
import torch

import exact_sample as X

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    def __init__(self):
        self.device = torch.device(DEV, torch.cuda.current_device())

    def sample(self, *a, **kw):
        ops().sample_topk(*a, **kw)


@pytest.mark.parametrize("c", X.CASES, ids=[c.id for c in X.CASES])
def test_every_probe_draws_the_token_the_float64_reference_names(c):
    X.run_case(Gpu(), c)


def test_premise_expf_of_zero_is_one():
    X.premise_case(Gpu())


def test_an_all_banned_row_returns_id_zero():
    X.all_banned_case(Gpu())
    X.all_banned_case(Gpu(), V=30522, dtype="f32")


def _launch():
    be = Gpu()
    row = X.BY_ID["iter-v97-f32-k7-T1-mid"].row
    return be, X.Launch(be, row, X.probes(row, "mid")[0])


def test_refusals_of_the_wrapper_come_before_any_launch():
    be, L = _launch()
    o, B = ops(), L.B
    out, u, lg = L.out.view[:, 0], L.u.vector(), L.logits.view
    for kw in (dict(u=u.double()), dict(u=u[:B - 1]), dict(u=torch.zeros(2 * B, device=be.device)[::2]), dict(out=out.int()), dict(out=out[:B - 1]),
               dict(banned=torch.zeros(B, 96, dtype=torch.bool, device=be.device)), dict(banned=torch.zeros(B, 97, dtype=torch.int32, device=be.device)),
               dict(banned=torch.zeros(B, 2 * 97, dtype=torch.bool, device=be.device)[:, ::2])):
        a = dict(u=u, out=out, banned=None)
        a.update(kw)
        with pytest.raises(Exception, match="sample_topk"):
            o.sample_topk(lg, 1.0, 7, a["u"], a["out"], a["banned"])
    L.assert_windows("refusals")
    assert bool((out == X.CANARY[torch.int64]).all())                  # nothing was launched


def test_refusals_of_the_entry_point():
    be, L = _launch()
    o = ops()
    out, u, lg = L.out.view[:, 0], L.u.vector(), L.logits.view
    for (T, k, p) in ((0.0, 7, 0.0), (-1.0, 7, 0.0), (float("nan"), 7, 0.0), (1.0, -1, 0.0), (1.0, 7, -0.25), (1.0, 7, float("nan"))):
        with pytest.raises(Exception, match="GSTVD_E_SHAPE"):
            o.sample_topk(lg, T, k, u, out, None, top_p=p)
    wide = torch.zeros(2, 31745, device=be.device)
    with pytest.raises(Exception, match="GSTVD_E_UNSUPPORTED"):
        o.sample_topk(wide, 1.0, 7, u[:2].contiguous(), torch.zeros(2, dtype=torch.int64, device=be.device))
    # ld < V and null pointers: only the C entry can be asked
    from gst_visdial_amd import _lib as Lb
    lib = Lb.load()

    def desc(**over):
        d = Lb.SampleDesc()
        d.logits, d.ld, d.dtype, d.B, d.V, d.top_k, d.temperature = lg.data_ptr(), lg.stride(0), o.dt(lg), L.B, 97, 7, 1.0
        d.u, d.out, d.out_stride = u.data_ptr(), out.data_ptr(), out.stride(0)
        for k_, v in over.items():
            setattr(d, k_, v)
        return d

    def rc(d):
        try:
            Lb.check("gstvd_sample_topk", lib.gstvd_sample_topk(C.byref(d), None))
        except Exception as e:
            return str(e)
        return "accepted"

    assert "GSTVD_E_SHAPE" in rc(desc(ld=96))
    for name in ("logits", "u", "out"):
        assert "GSTVD_E_NULL" in rc(desc(**{name: None}))
    assert "GSTVD_E_NULL" in rc(desc(ngram=2, hist=None, ids_tm=None))
    L.assert_windows("refusals")
    assert bool((out == X.CANARY[torch.int64]).all())
