"""The exact GEMM harness (tests/exact_gemm.py) proved on the CPU: a stand-in "kernel" written in torch runs the same windows,
reference and assertions as tests/test_gemm_exact_gpu.py.  The correct stand-in passes every assertion; each deliberately wrong
one -- the subtle errors a tolerance relative to the tensor's maximum cannot see -- fails the assertion that is there to catch it.
This is the evidence that the GPU tests would fail if a kernel were subtly wrong, obtained without doing anything wrong on a GPU."""
import os

import pytest
import torch

import exact_gemm as E

DEV = "cpu"


def standin(p, mask=None, bug=None, scratch=None):
    """epi(alpha * A B) the way a tiled kernel computes it: fp32 accumulation in 64-deep K chunks, fp32 epilogue, one rounding
    at the store -- written into p.C's window.  `bug` plants one defect."""
    c = p.c
    a_km, b_km = E.LAYOUTS[c.lay]
    M, N, K = c.M, c.N, c.K
    A, B = p.A.view3.float(), p.B.view3.float()
    if bug == "read_pad_a":                  # the A tile is fetched one column too wide: the pad column meets a non-zero B element
        assert not a_km and p.A.ld > K and c.batch == 1
        A = torch.as_strided(p.A.flat, (1, M, K + 1), (p.A.stride, p.A.ld, 1), p.A.offset).float()
        B = torch.cat([B, torch.ones(B.shape[0], 1, K) if b_km else torch.ones(B.shape[0], N, 1)], dim=1 if b_km else 2)
        K = K + 1
    A = A.transpose(1, 2) if a_km else A                      # [batch, M, K]
    B = B if b_km else B.transpose(1, 2)                      # [batch or 1, K, N]
    acc = torch.zeros(c.batch, M, N)
    for k0 in range(0, K, 64):
        part = A[:, :, k0:k0 + 64] @ B[:, k0:k0 + 64]
        acc += part
        if bug == "partial_twice" and k0 == 64:               # one element's (small: it nearly cancels) partial of one K chunk added twice
            m, n = divmod(int(part[0].abs().masked_fill(part[0] == 0, 1e9).argmin()), N)
            acc[0, m, n] += part[0, m, n]
    if bug == "drop_product":                                 # one product missing from one element
        m, n = M // 2, N // 2
        k = int(torch.nonzero(A[0, m] * B[0, :, n])[-1])
        acc[0, m, n] -= A[0, m, k] * B[0, k, n]
    v = acc * c.alpha
    if p.bias is not None:
        b = p.bias.vector().clone()
        if bug == "bias_shift":                               # one 16-column block reads its bias one column to the right
            b[16:32] = p.bias.vector()[17:33]
        v = v + b
    if p.add is not None:
        v = v + p.add.view3.float()
    if c.epi == "dgelu":
        v = v * p.aux.view3.float()
    if mask is not None:
        v = v * mask
    if bug == "truncate":                                     # the bf16 store drops the low half instead of rounding to nearest even
        out = (v.view(torch.int32) & -65536).view(torch.float32).to(p.C.dtype)
    else:
        out = v.to(p.C.dtype)
    p.C.view3.copy_(out)
    first, ld = p.C.offset, p.C.ld
    if bug == "write_pad_col":
        p.C.flat[first + 3 * ld + N] = 1.0
    if bug == "write_row_after":
        p.C.flat[first + M * ld + 5] = 1.0
    if bug == "write_past_n":                                 # a 16-byte store of the last 4 columns of a row (N % 8 == 4, ldc % 8 == 0)
        assert N % 8 == 4 and ld % 8 == 0 and ld >= N + 4
        p.C.flat[first + 7 * ld + N: first + 7 * ld + N + 4] = 0.0
    if scratch is not None:                                   # split-K: every tile's counter goes up and is re-armed by the last arrival
        cnt = scratch[:E.SPLITK_COUNTER_BYTES].view(torch.int32)
        cnt[:4] += 3
        cnt[:4] -= 3
        if bug == "counter_left":
            cnt[2] = 1


def run(c, bug=None, seed=1, scratch=None):
    p = E.Problem(c, seed, DEV)
    mask = None
    if c.drop:
        mask = 2.0 * torch.randint(0, 2, (c.batch, c.M, c.N), generator=E.generator(seed + 1, DEV)).float()
    standin(p, mask, bug, scratch)
    ref, peak = p.expected(mask.reshape(p.C.view.shape) if mask is not None else None)
    E.assert_exact_range(peak, c.id)
    E.assert_bit_equal(p.C.view, ref, c.id)
    p.assert_surroundings(c.id)
    if scratch is not None:
        E.assert_counters_zero(scratch, c.id)
    return p


DEEP = E.case("dma64", 300, 264, 3072, bias="a", pad=(8, 8, 8))
CLEAN = [DEEP,
         E.case("dma64", 37, 132, 200, lay="nt", ldc_odd=True, bias="u", add=True, alpha=0.125, epi="dgelu", drop=True),
         E.case("dma64", 64, 72, 72, lay="nn", out="f32", add=True, alpha=2.0, pad=(8, 16, 24)),
         E.case("dma64", 72, 56, 136, lay="tn", batch=3, bias="a", add=True, epi="dgelu", pad=(8, 0, 8)),
         E.case("dma64", 40, 68, 64, lay="tt", batch=3, shared_b=True, drop=True),
         E.case("f32_64", 36, 132, 68, lay="nn", inp="f32", out="f32", bias="u", add=True, epi="dgelu")]


@pytest.mark.parametrize("c", CLEAN, ids=lambda c: c.id)
def test_correct_standin_passes_every_assertion(c):
    p = run(E.normalise(c), scratch=torch.zeros(E.SPLITK_COUNTER_BYTES + 64, dtype=torch.uint8))
    assert p.C.view.data_ptr() % 16 == 0 and p.A.view.data_ptr() % 16 == 0 and p.B.view.data_ptr() % 16 == 0
    if c.bias == "u":
        assert p.bias.vector().data_ptr() % 16 == 4


def test_deep_integer_product_is_exact_in_fp32_and_exercises_the_rounding():
    """K = 3072: the fp32 result, whole or in 64-deep chunks, IS the float64 one; a good share of the outputs is beyond 256,
    where bf16 no longer holds every integer, so the store's rounding is really exercised."""
    p = E.Problem(DEEP, 1, DEV)
    ref, peak = p.expected()
    whole = p.A.view.float() @ p.B.view.float().t() + p.bias.vector()
    assert torch.equal(whole.double(), ref)
    standin(p)
    assert torch.equal(p.C.view, E.rne(ref, torch.bfloat16))
    assert (ref.abs() > 256).double().mean().item() > 0.05
    assert (E.rne(ref, torch.bfloat16).double() != ref).double().mean().item() > 0.02


MUTATIONS = [
    # defect, case it is planted in, the assertion that must catch it
    ("drop_product", DEEP, "differ from the exact reference"),
    ("partial_twice", DEEP, "differ from the exact reference"),
    ("bias_shift", DEEP, "differ from the exact reference"),
    ("truncate", DEEP, "differ from the exact reference"),
    ("write_pad_col", DEEP, "C: 1 element.s. outside"),
    ("write_row_after", DEEP, "C: 1 element.s. outside"),
    ("write_past_n", E.case("dma64", 37, 132, 200, pad=(0, 0, 4), bias="a"), "C: 4 element.s. outside"),
    ("read_pad_a", DEEP, "differ from the exact reference"),
    ("counter_left", DEEP, "split-K counter"),
]


@pytest.mark.parametrize("bug,c,message", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_each_planted_defect_fails_its_assertion(bug, c, message):
    scratch = torch.zeros(E.SPLITK_COUNTER_BYTES + 64, dtype=torch.uint8)
    run(c, scratch=scratch)                                   # the same case is clean without the defect
    with pytest.raises(AssertionError, match=message):
        run(c, bug=bug, scratch=scratch)


def test_tolerance_metric_does_not_see_the_arithmetic_defects():
    """Why the exact layer exists: the existing metric (error relative to the tensor's maximum, 1.2e-2 in bf16) passes these
    arithmetic defects (and the shifted bias too whenever the bias is small against the output)."""
    for bug in ("drop_product", "partial_twice", "truncate"):
        p = E.Problem(DEEP, 1, DEV)
        standin(p, bug=bug)
        ref, _ = p.expected()
        E.assert_close_rel_to_max(p.C.view, ref, 1.2e-2, bug)


def test_a_case_that_leaves_the_exact_range_fails_loudly():
    p = E.Problem(E.case("dma64", 64, 64, 3072, alpha=2.0, add=True), 1, DEV)
    ref, peak = p.expected()
    E.assert_exact_range(peak, "in range")
    with pytest.raises(AssertionError, match="leaves the exact range"):
        E.assert_exact_range(peak * 2 ** 14, "scaled")
    for c in E.CASES:                                         # worst case of the table: K * 9 * |alpha| + 16, times aux 2, times dropout 2
        worst = (c.K * 9 * max(abs(c.alpha), 1.0) + 16) * (2 if c.epi == "dgelu" else 1) * (2 if c.drop else 1)
        E.assert_exact_range(worst, c.id)


def test_poisoned_and_canary_surroundings_are_detected_on_inputs_too():
    p = E.Problem(E.case("dma64", 24, 64, 72, bias="a", pad=(8, 8, 8)), 3, DEV)
    p.assert_surroundings("fresh")
    p.A.flat[p.A.offset + 72] = 0.0                           # a write into A's pad column
    with pytest.raises(AssertionError, match="A: 1 element"):
        p.assert_surroundings("dirty")


def test_case_table_is_well_formed():
    """Unique ids, shapes the ABI accepts, every condition of the issue present for every route that supports it."""
    ids = [c.id for c in E.CASES]
    assert len(ids) == len(set(ids))
    by_route = {}
    for c in E.CASES:
        ve = 4 if c.inp == "f32" else 8
        a_km, b_km = E.LAYOUTS[c.lay]
        assert c.N % 4 == 0 and c.K <= 3072 and (c.M % ve == 0 or not a_km) and (c.N % ve == 0 or not b_km), c.id
        assert (a_km and b_km) or c.K % ve == 0, c.id
        assert all(x % ve == 0 for x in c.pad[:2]) and c.pad[2] % 4 == 0, c.id
        # (the > 512-tile shapes are the expensive ones: their two tile widths share one set of conditions)
        by_route.setdefault("dma256" if c.route.startswith("dma256") else c.route, []).append(c)
    assert set(c.route for c in E.CASES) == set(E.ROUTES)
    for route, cs in by_route.items():
        f32 = route.startswith("f32")
        assert any(c.ldc_odd for c in cs) and any(c.bias == "u" for c in cs) and any(c.N % 8 == 4 for c in cs), route
        assert any(c.N % 8 == 4 and not c.ldc_odd and (c.N + c.pad[2]) % 8 == 0 for c in cs) or f32, route   # a 16-byte store could pass N
        assert any(all(c.pad) for c in cs) and any(c.add for c in cs) and any(c.alpha != 1.0 for c in cs), route
        assert any(c.out == "f32" for c in cs) and any(c.epi == "gelu" for c in cs), route
        if not route.startswith(("gemv", "splitk")):
            assert any(c.batch > 1 for c in cs), route
        if not route.startswith("gemv"):
            assert any(c.epi == "dgelu" for c in cs) and any(c.drop for c in cs), route
            assert any(c.epi == "dgelu" and c.drop and c.bias and c.add and c.alpha != 1.0 for c in cs), route
    print({r: len(cs) for r, cs in by_route.items()})


def test_every_gemm_kernel_of_the_library_is_named_by_a_case_or_exempt():
    """The static half of the route census (the GPU file checks that each case really launches the kernel it names)."""
    if not os.path.exists(E.lib_path()):
        import __graft_entry__ as ge
        ge.build()
    import test_gemm_exact_gpu as G
    G.check_census(E.library_gemm_kernels(E.lib_path()))
