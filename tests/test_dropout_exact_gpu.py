"""Exact layer of the dropout-stream tests on a real MI355X (tests/exact_dropout.py): the library's mask
probe (ops.dropout_mask over ops.Rng -- make_drop / drop_draw / drop_factor of csrc/common.h, the code every fused dropout site
runs) against the numpy restatement, factor for factor: the grid of seeds, offsets, sites and probabilities, Rng.advance() with
its carry, a 2^26-element site across the first 2^24-draw boundary, the independence statistics, and the keep bits at the
distances where the previous hash repeated whole blocks.  The checks are proved on the CPU by
tests/test_exact_dropout_harness_cpu.py."""
import pytest
import torch

import exact_dropout as X

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from gst_visdial_amd import ops as o
    return o


class Gpu(object):
    def __init__(self):
        self.device = torch.device(DEV, torch.cuda.current_device())
        self.last = None                                 # the 2^26-float site is made once per (p, site, seed, offset) in a row

    def rng(self, seed, offset):
        r = ops().Rng(self.device, seed=seed)
        r.state[1] = offset
        return r

    def mask(self, n, p, site, seed, offset):
        key = (n, p, site, seed, offset)
        if self.last is not None and self.last[0] == key:
            return self.last[1]
        self.last = None
        m = ops().dropout_mask(n, p, site, self.rng(seed, offset), self.device)
        if n >= X.LARGE_N:
            self.last = (key, m)
        return m

    def advance(self, seed, offset, times):
        r = self.rng(seed, offset)
        for _ in range(times):
            r.advance()
        return tuple(int(v) for v in r.state.cpu())


CHECKS = {"A_grid": X.check_grid, "B_advance": X.check_advance, "C_large_site": X.check_large_site,
          "D_independence": X.check_independence, "F_large_site_pairs": X.check_large_site_pairs}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_dropout_stream(name):
    CHECKS[name](Gpu())
