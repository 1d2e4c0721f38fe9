"""The stand-alone product D^T[n][m] = sum_k A[m][k] X[n][k] (`vmx_matvec_device`: the kernels the distortion, metal
and FFTLog steps use) on ragged shapes - matrix rows and walker counts that are not multiples of the 64 x 64 block tile,
K tails, every batch-size regime (streaming kernels for B <= 8, MFMA kernels above), every split-K factor the planner
chooses (1, 2, 4 and 8), the single-walker fallback above 5120 columns and the block-count edges of the single-walker
kernel.

Reference and tolerance: where the operands fit a longdouble product in about a second (M K B <~ 5e8) the result is held
elementwise to `(K + 2) u (|X| |A|^T)`, u = 2^-53 - the a-priori bound of an fp64 sum of K products in any order - against the
product in np.longdouble.  The larger shapes keep the comparison with a plain fp64 torch product of the same operands at
1e-13 of the result's scale (fp64 sums of ~1e3 terms in a different order)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# (M, K) and, per MFMA batch 9 / 37 / 64 / 130 / 256, the K split plan_gemm gives it (tiles = ceil(M / 64) ceil(B / 64);
# doubled up to 8 while tiles x split < 512, halved while a slab would be empty):
#   (70, 96)      2 / 2 / 2 / 2 / 2        (K = 96 is three K stages: no more than two non-empty slabs of 64)
#   (257, 300)    4 / 4 / 4 / 4 / 4        (K = 320 padded: four slabs of 96)
#   (1000, 1000)  8 / 8 / 8 / 8 / 8        (16 .. 64 tiles)
#   (2500, 2500)  8 / 8 / 8 / 8 / 4        (40 / 40 / 40 / 120 / 160 tiles)
#   (5000, 5000)  8 / 8 / 8 / 4 / 2        (79 / 79 / 79 / 237 / 316 tiles)
SHAPES = [(70, 96), (257, 300), (1000, 1000), (2500, 2500), (5000, 5000)]
BATCHES = [1, 3, 8, 9, 37, 64, 130, 256]
# (M, K, B): no split and a ragged walker tile (16 x 33 = 528 tiles); a leading dimension above 5120 (one walker leaves the
# LDS-resident k_gemv1 for k_gemv<1>); the block-count edges of gemv1_blocks (fewer rows than blocks; M > 512 x 24 rows
# doubles the blocks)
EXTRA = [(1000, 1000, 2053), (300, 5200, 1), (300, 5200, 3), (3, 64, 1), (12300, 64, 1)]
LD_LIMIT = 5e8
U = 2.0**-53
LD = np.longdouble


def planned_split(m, ld, batch):
    """plan_gemm's rule for a stand-alone product (vegamx.hip), restated: which K split an MFMA shape takes."""
    tiles = -(-m // 64) * -(-batch // 64)
    nsplit = 1
    while nsplit < 8 and tiles * nsplit < 512:
        nsplit *= 2
    klen = lambda ns: -(-(-(-ld // ns)) // 32) * 32
    while nsplit > 1 and klen(nsplit) * (nsplit - 1) >= ld:
        nsplit //= 2
    return nsplit


def _engine(max_batch=1):
    from vega_amd import VegaInterface
    return VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=max_batch)


def _pad(n):
    return (n + 31) // 32 * 32


def _operands(torch, m, k, batch, seed, signed=False):
    """A [m][ld], X [batch][ld] zero-padded to a multiple of 32 columns: centred noise, or - ``signed`` - rows of A of
    constant sign and X = 1, so that every partial sum grows and an error in a K range cannot cancel."""
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(seed)
    ld = _pad(k)
    a = torch.zeros(m, ld, dtype=torch.float64, device=dev)
    x = torch.zeros(batch, ld, dtype=torch.float64, device=dev)
    if signed:
        sign = torch.where(torch.arange(m, device=dev) % 3 == 0, -1.0, 1.0).to(torch.float64)
        a[:, :k] = (0.25 + torch.rand(m, k, dtype=torch.float64, device=dev, generator=gen)) * sign[:, None]
        x[:, :k] = 1.0
    else:
        a[:, :k] = torch.rand(m, k, dtype=torch.float64, device=dev, generator=gen) - 0.5
        x[:, :k] = torch.rand(batch, k, dtype=torch.float64, device=dev, generator=gen) - 0.5
    return a, x


def _product(eng, torch, a, x, m):
    batch = x.shape[0]
    y = torch.full((batch, _pad(m)), float('nan'), dtype=torch.float64, device=a.device)
    eng.matvec_device(a.data_ptr(), m, a.shape[1], x.data_ptr(), batch, y.data_ptr())
    eng.sync()
    return y


class _Reference:
    """The longdouble product of one pair of operands, made once for the leading `rows` vectors of X (the batches of a
    shape share their operands), and the bound (K + 2) u (|X| |A|^T).  The sum of absolute products is formed in fp64 and
    lowered by its own worst-case rounding, (1 - 2 K u): the bound used is never above the stated one."""

    def __init__(self, a, x, k, rows):
        ah = a[:, :k].cpu().numpy()
        xh = x[:rows, :k].cpu().numpy()
        self.ref = xh.astype(LD) @ ah.astype(LD).T
        self.bound = ((k + 2) * U * (1 - 2 * k * U)) * (np.abs(xh) @ np.abs(ah).T)


def _check(eng, torch, m, k, batch, a, x, reference, what):
    """A x[:batch]^T through the engine against ``reference`` (when it covers the batch) or the fp64 torch product."""
    y = _product(eng, torch, a, x[:batch].contiguous(), m)
    what = f'M={m} K={k} B={batch} {what}'
    if reference is not None:
        rows = slice(0, min(batch, reference.ref.shape[0]))        # (a single row when every vector is the same: broadcast)
        ref, bound = reference.ref[rows], reference.bound[rows]
        err = np.abs(y[:, :m].cpu().numpy().astype(LD) - ref)
        worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        assert np.all(err <= bound), (f'{what}: element {worst} off by {float(err[worst]):.3e}, bound '
                                      f'{float(np.broadcast_to(bound, err.shape)[worst]):.3e}')
        return float((err / bound).max())
    ref = x[:batch, :k] @ a[:, :k].T
    err = float((y[:, :m] - ref).abs().max() / ref.abs().max())
    assert err <= 1e-13, f'{what}: scaled error {err:.2e}'
    return None


def _check_shape(eng, torch, m, k, batches, seed, signed=False):
    """One pair of operands per shape, every batch a leading part of X; the longdouble reference covers the batches with
    M K B <= LD_LIMIT, the rest keep the fp64 torch product."""
    a, x = _operands(torch, m, k, max(batches), seed, signed)
    covered = [b for b in batches if m * k * b <= LD_LIMIT] if np.finfo(LD).nmant >= 63 else []
    reference = _Reference(a, x, k, 1 if signed else max(covered)) if covered else None
    return {b: _check(eng, torch, m, k, b, a, x, reference if b in covered else None, 'signed' if signed else '') for b in batches}


def test_ragged_products_every_batch_regime():
    import torch
    vega = _engine()
    for i, (m, k) in enumerate(SHAPES):
        _check_shape(vega.engine, torch, m, k, BATCHES, seed=17 * i)
    vega.close()


def test_every_split_factor_and_the_single_walker_edges():
    """The shapes of EXTRA, and that the shapes of this module reach every K split of plan_gemm."""
    import torch
    splits = {planned_split(m, _pad(k), b) for m, k in SHAPES for b in BATCHES if b > 8}
    splits |= {planned_split(m, _pad(k), b) for m, k, b in EXTRA if b > 8}
    assert splits == {1, 2, 4, 8}
    assert planned_split(1000, 1024, 2053) == 1 and 2053 % 64 != 0
    assert [planned_split(m, _pad(k), 256) for m, k in SHAPES] == [2, 4, 8, 4, 2]
    vega = _engine()
    worst = {}
    for i, (m, k, batch) in enumerate(EXTRA):
        worst[(m, k, batch)] = _check_shape(vega.engine, torch, m, k, [batch], seed=1000 + i)[batch]
    print('\nPRODUCT_RATIOS', worst)
    vega.close()


@pytest.mark.parametrize('batch', [1, 5, 9, 130])
def test_sums_that_only_grow(batch):
    """Rows of A of constant sign against X = 1: no cancellation hides a K range that is dropped, doubled or misplaced."""
    import torch
    vega = _engine()
    for m, k in ((257, 300), (1000, 1000)):
        _check_shape(vega.engine, torch, m, k, [batch], seed=5 + batch, signed=True)
    vega.close()


def test_operands_beyond_the_32_bit_offsets_are_refused():
    """k_gemm_nt44 addresses its operands with 32-bit byte offsets: an operand of 4 GiB or more is an error before anything is
    launched (the buffers here are small and real; nothing may read them at the stated sizes)."""
    import torch
    from vega_amd.engine import EngineError
    vega = _engine()
    dev = torch.device('cuda', 0)
    a = torch.zeros(64, 4096, dtype=torch.float64, device=dev)
    x = torch.zeros(9, 4096, dtype=torch.float64, device=dev)
    y = torch.zeros(9, 64, dtype=torch.float64, device=dev)
    rows = 2**32 // (4096 * 8)                                   # rows x 4096 doubles = 4 GiB exactly
    with pytest.raises(EngineError, match='4 GiB'):
        vega.engine.matvec_device(a.data_ptr(), rows, 4096, x.data_ptr(), 9, y.data_ptr())
    with pytest.raises(EngineError, match='4 GiB'):
        vega.engine.matvec_device(a.data_ptr(), 64, 4096, x.data_ptr(), rows, y.data_ptr())
    # ... and the engine still works
    vega.engine.matvec_device(a.data_ptr(), 64, 4096, x.data_ptr(), 9, y.data_ptr())
    vega.engine.sync()
    assert float(y.abs().max()) == 0.0
    vega.close()
