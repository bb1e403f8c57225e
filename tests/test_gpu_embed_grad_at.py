"""tt_embed_grad_rows_at through the C ABI (ops.embed_grad_rows_at): the segment sums of
tt_embed_grad_rows written at rows[dst[u]] of a larger buffer whose other rows the call zeroes.

Named rows must be the bits ops.embed_grad_rows gives on the same (dx, perm, seg_ptr); every
other row is +0 (the buffer is pre-filled with NaN, and the row after it must keep its NaN);
two calls give the same bits. Against a float64 sum the bound per element is that of
tests/test_gpu_embed_grad.py: L * 2^-24 * sum|terms| for a segment of L terms.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from two_towers_amd import _lib, ops  # noqa: E402

DEV = "cuda"


def pattern_a():
    """m = 3C + 5 sorted positions: a short segment, one id owning 2C + 9 positions (it crosses
    two chunk boundaries), singletons, a segment that ends exactly on the boundary 3C, and five
    singletons behind it."""
    C = ops.embed_grad_chunk()
    lens = [7, 2 * C + 9]
    lens += [1] * (3 * C - 4 - sum(lens)) + [4] + [1] * 5
    assert sum(lens) == 3 * C + 5 and sum(lens[:-5]) == 3 * C
    return torch.repeat_interleave(torch.arange(len(lens)) * 3 + 2, torch.tensor(lens)), lens


def pattern_b():
    """One segment only, longer than two chunks."""
    C = ops.embed_grad_chunk()
    return torch.full((2 * C + 3,), 5, dtype=torch.int64), [2 * C + 3]


@functools.lru_cache(maxsize=None)
def case(pattern, E):
    """(dx, perm, seg_ptr on the GPU, the plain kernel's rows, float64 sums, float64 sums of
    magnitudes, segment lengths), computed once per (pattern, E)."""
    g = torch.Generator().manual_seed(E + (1 if pattern == "a" else 2))
    ids, lens = pattern_a() if pattern == "a" else pattern_b()
    # pads in between and a random row order: perm is then a real permutation
    ids = torch.cat([ids, torch.full((ids.numel() // 10,), -1, dtype=torch.int64)])
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    n = ids.numel()
    ldx = E + 4 if pattern == "a" else E  # a strided dx: the rows of a wider buffer
    dx = torch.randn(n, ldx, generator=g)[:, :E]
    dxd = torch.zeros(n, ldx, device=DEV)[:, :E]
    dxd.copy_(dx)
    perm, seg_ptr, uniq = ops.embed_plan(ids.to(DEV))
    assert torch.diff(seg_ptr).cpu().tolist() == lens
    if pattern == "a":  # a few row numbers outside dx: they add nothing
        perm = perm.clone()
        perm[3], perm[40], perm[perm.numel() - 2] = n + 3, -2, 2 ** 31 - 1
    base = ops.embed_grad_rows(dxd, perm, seg_ptr, E)
    p, s = perm.cpu().long(), seg_ptr.cpu().tolist()
    ok = (p >= 0) & (p < n)
    terms = torch.where(ok[:, None], dx.double()[p.clamp(0, n - 1)], torch.zeros(1, dtype=torch.float64))
    seg = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    ref = torch.zeros(len(lens), E, dtype=torch.float64).index_add_(0, seg, terms)
    mag = torch.zeros(len(lens), E, dtype=torch.float64).index_add_(0, seg, terms.abs())
    assert s[-1] == p.numel()
    return dxd, perm, seg_ptr, base.cpu(), ref, mag, torch.tensor(lens, dtype=torch.float64)


def layout(name, U):
    """(dst, nrows) for U segments."""
    if name == "identity":
        return list(range(U)), U
    if name == "ends_unnamed":
        return [1 + 2 * u for u in range(U)], 2 * U + 1
    if name == "gaps":  # first and last row named, 0, 1 and 40 rows between neighbours
        dst = [0]
        for u in range(1, U):
            dst.append(dst[-1] + 1 + (0, 1, 40)[(u - 1) % 3])
        return dst, dst[-1] + 1
    if name == "dropped":  # the last entry lies outside the buffer
        return [1 + 2 * u for u in range(U - 1)] + [2 * U + 3], 2 * U + 1
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["identity", "ends_unnamed", "gaps", "dropped"])
@pytest.mark.parametrize("E", [300, 20, 7])
@pytest.mark.parametrize("pattern", ["a", "b"])
def test_rows_at_match_the_plain_kernel_and_zero_the_rest(pattern, E, name):
    dxd, perm, seg_ptr, base, ref, mag, lens = case(pattern, E)
    U, m = base.shape[0], perm.numel()
    C = ops.embed_grad_chunk()
    assert m > 2 * C and int(lens.max()) > 2 * C and (pattern == "b" or (m == 3 * C + 5 and 3 * C in seg_ptr.cpu().tolist()))
    dst, nrows = layout(name, U)
    assert all(b > a for a, b in zip(dst[:-1], dst[1:])) and nrows >= U
    dst_t = torch.tensor(dst, dtype=torch.int32, device=DEV)
    nb = _lib.load().tt_embed_grad_ws_size(m, E)
    outs = []
    for fill in (0xFF, 0x00):  # ws of NaN bytes, then of zeros: nothing may depend on it
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        rows = torch.full((nrows + 1, E), float("nan"), device=DEV)
        ops.embed_grad_rows_at(dxd, perm, seg_ptr, dst_t, nrows, E, rows=rows, ws=ws)
        assert bool(rows[nrows].isnan().all()), "the row after rows[nrows - 1] was written"
        outs.append(rows[:nrows].cpu())
    got = outs[0]
    assert not bool(got.isnan().any()), "a row was left unwritten"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two calls differ in their bits"
    kept = [u for u in range(U) if 0 <= dst[u] < nrows]
    assert len(kept) == (U - 1 if name == "dropped" else U)
    named = torch.tensor([dst[u] for u in kept], dtype=torch.int64)
    assert torch.equal(got[named].view(torch.int32), base[kept].view(torch.int32)), "not the plain kernel's bits"
    rest = torch.ones(nrows, dtype=torch.bool)
    rest[named] = False
    assert bool((got[rest] == 0).all()) and not bool(torch.signbit(got[rest]).any()), "an unnamed row is not +0"
    if not kept:  # one segment, dropped: nothing but zero rows
        return
    bound = lens[kept][:, None] * 2.0 ** -24 * mag[kept]
    err = (got[named].double() - ref[kept]).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"pattern {pattern} E={E} {name}: U={U} m={m} nrows={nrows}, worst error / bound {ratio:.3f}")
    assert bool((err <= bound).all()), ratio


@pytest.mark.parametrize("E", [300, 20, 7])
def test_no_segments_zeroes_every_row(E):
    """Pattern (c): nseg = m = 0 with nrows = 5 (a rank whose batch is all padding)."""
    perm = torch.zeros(0, dtype=torch.int32, device=DEV)
    seg_ptr = torch.zeros(1, dtype=torch.int32, device=DEV)
    dst = torch.zeros(0, dtype=torch.int32, device=DEV)
    dx = torch.randn(4, E, device=DEV)
    rows = torch.full((6, E), float("nan"), device=DEV)
    ops.embed_grad_rows_at(dx, perm, seg_ptr, dst, 5, E, rows=rows)
    assert bool((rows[:5] == 0).all()) and not bool(torch.signbit(rows[:5]).any()) and bool(rows[5].isnan().all())
