"""The trainable-embedding kernels through the C ABI (ops.embed_grad_rows ->
tt_embed_grad_rows, ops.sparse_adam_rows -> tt_sparse_adam_rows).

Segment sum: against a float64 index_add_ on the CPU. The bound per element is
L * 2^-24 * sum|terms| (L = the segment's length): the first-order bound of an fp32 sum of L
terms in any order, each term passing through at most L - 1 roundings of relative size
2^-24. Derived, not tuned; the worst ratio to it is printed (measured: at most 0.64,
the Zipf case at E 300; 0.49 for the chunk-boundary pattern).
Row update: against torch.optim.SparseAdam on the CPU in fp32 at the project's Adam bounds,
rtol 1e-5 / atol 1e-6 (tests/test_gpu_optim_clip.py).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from two_towers_amd import ops, towers  # noqa: E402

DEV = "cuda"
N, V = 3000, 500


def chunk():
    return ops.embed_grad_chunk()


def boundary_ids():
    """Sorted ids whose segments start or end exactly on, one before and one after a chunk
    boundary, with single-position segments at the boundaries, one segment covering two whole
    chunks and one covering a chunk exactly."""
    C = chunk()
    cuts = sorted({0, C - 1, C, C + 1, 2 * C - 1, 2 * C + 1, 3 * C, 4 * C, 6 * C + 1, 7 * C - 1, 7 * C, 8 * C - 2,
                   9 * C + 1, 10 * C, 10 * C + 1, 11 * C - 1, 12 * C})
    ids = torch.empty(cuts[-1], dtype=torch.int64)
    for u, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        ids[a:b] = 3 * u + 1
    return ids


def make_ids(pattern, g):
    if pattern == "one_id":
        return torch.full((N,), 7, dtype=torch.int64)
    if pattern == "distinct":
        return torch.randperm(N, generator=g)
    if pattern == "all_pad":
        return torch.full((N,), -1, dtype=torch.int64)
    if pattern == "single_row":
        return torch.tensor([V - 1])
    if pattern == "zipf":
        w = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
        ids = torch.multinomial(w, N, replacement=True, generator=g)
        ids[torch.rand(N, generator=g) < 0.1] = -1
        return ids
    if pattern == "boundaries":
        ids = boundary_ids()
        # pads in between and a random row order: perm is then a real permutation, while the
        # sorted list keeps its segment boundaries
        ids = torch.cat([ids, torch.full((ids.numel() // 10,), -1, dtype=torch.int64)])
        return ids[torch.randperm(ids.numel(), generator=g)]
    raise AssertionError(pattern)


@pytest.mark.parametrize("E", [300, 16, 6])
@pytest.mark.parametrize("pattern", ["one_id", "distinct", "all_pad", "single_row", "zipf", "boundaries"])
def test_segment_sum_matches_float64_index_add(pattern, E):
    g = torch.Generator().manual_seed(sum(map(ord, pattern)) + E)
    ids = make_ids(pattern, g)
    n = ids.numel()
    ldx = E + 4 if pattern == "zipf" else E  # a strided dx: the rows of a wider buffer
    dx = torch.randn(n, ldx, generator=g)[:, :E]
    nv = int(ids.max()) + 1 if n and int(ids.max()) >= 0 else 1
    ref = torch.zeros(nv, E, dtype=torch.float64).index_add_(0, ids[ids >= 0], dx[ids >= 0].double())
    mag = torch.zeros(nv, E, dtype=torch.float64).index_add_(0, ids[ids >= 0], dx[ids >= 0].double().abs())
    cnt = torch.bincount(ids[ids >= 0], minlength=nv).double()

    dxd = torch.zeros(n, ldx, device=DEV)[:, :E]
    dxd.copy_(dx)
    perm, seg_ptr, uniq = ops.embed_plan(ids.to(DEV))
    U, m = uniq.numel(), perm.numel()
    assert torch.equal(uniq.cpu(), torch.unique(ids[ids >= 0]))
    nb = towers._lib.load().tt_embed_grad_ws_size(m, E)
    outs = []
    for fill in (0xFF, 0x00):  # ws of NaN bytes, then of zeros: nothing may depend on it
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        rows = torch.full((U + 1, E), 12345.0, device=DEV)
        ops.embed_grad_rows(dxd, perm, seg_ptr, E, rows=rows, ws=ws)
        assert bool((rows[U] == 12345.0).all()), "the row after rows[U - 1] was written"
        outs.append(rows[:U].cpu())
    assert torch.equal(outs[0], outs[1]), "two calls differ in their bits"
    if pattern == "all_pad":
        assert U == 0 and m == 0
        return
    got = outs[0].double()
    u = uniq.cpu()
    bound = cnt[u, None] * 2.0 ** -24 * mag[u]
    err = (got - ref[u]).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{pattern} E={E}: U={U} m={m} longest segment {int(cnt.max())}, worst error / bound {ratio:.3f}")
    assert bool((err <= bound).all()), ratio
    if pattern == "one_id":
        assert U == 1 and int(cnt.max()) == N > 2 * chunk()
    if pattern == "boundaries":
        C = chunk()
        s = seg_ptr.cpu().tolist()
        assert {C - 1, C, C + 1, 2 * C - 1, 2 * C + 1, 3 * C, 4 * C} <= set(s) and m > 8 * C


def test_segment_sum_skips_rows_outside_dx():
    """A perm entry outside [0, n) adds nothing (and reads nothing out of bounds)."""
    E = 8
    dx = torch.arange(4 * E, dtype=torch.float32, device=DEV).view(4, E)
    perm = torch.tensor([0, 9, 2, -3, 3], dtype=torch.int32, device=DEV)
    seg_ptr = torch.tensor([0, 3, 5], dtype=torch.int32, device=DEV)
    rows = ops.embed_grad_rows(dx, perm, seg_ptr)
    assert torch.equal(rows[0], dx[0] + dx[2]) and torch.equal(rows[1], dx[3])


def sparse_grad(ids, vals, V, E):
    return torch.sparse_coo_tensor(torch.tensor(ids)[None], vals, (V, E)).coalesce()


STEP_IDS = [list(range(0, 10)), [5, 6, 8, 9, 10, 11, 12, 13, 14], [0, 1, 2, 3, 4, 7, 20], [10, 11, 20, 21]]


@pytest.mark.parametrize("E,dt", [(300, torch.bfloat16), (300, torch.float32), (6, torch.bfloat16), (6, torch.float32)])
def test_sparse_adam_rows_matches_torch_sparse_adam(E, dt):
    """4 steps whose id sets overlap partly; row 7 is touched in steps 1 and 3 but not 2 (the
    lazy rule: its moments do not decay in step 2). E 300: 16-byte accesses, bf16 copy of 320
    columns; E 6: the scalar path."""
    Vt = 40
    g = torch.Generator().manual_seed(E)
    w0 = torch.randn(Vt, E, generator=g)
    ref_p = torch.nn.Parameter(w0.clone())
    ref = torch.optim.SparseAdam([ref_p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    w, m, v = w0.clone().to(DEV), torch.zeros(Vt, E, device=DEV), torch.zeros(Vt, E, device=DEV)
    ep = ops.pad_cols(E, dt)
    copy = torch.zeros(Vt, ep, dtype=dt, device=DEV)
    copy[:, :E] = w.to(dt)
    copy0 = copy.clone()
    touched = set()
    for step, ids in enumerate(STEP_IDS, 1):
        vals = torch.randn(len(ids), E, generator=g)
        ref_p.grad = sparse_grad(ids, vals, Vt, E)
        ref.step()
        ops.sparse_adam_rows(w, m, v, torch.tensor(ids, dtype=torch.int32, device=DEV), vals.to(DEV), copy, lr=1e-2,
                             beta1=0.9, beta2=0.999, eps=1e-8, step=step)
        touched |= set(ids)
    assert 7 in STEP_IDS[0] and 7 in STEP_IDS[2] and 7 not in STEP_IDS[1]
    st = ref.state[ref_p]
    rtol, atol = 1e-5, 1e-6
    for name, a, b in (("weight", w, ref_p.detach()), ("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"])):
        gap = float(((a.cpu() - b).abs() / (atol + rtol * b.abs())).max())
        print(f"E={E} {dt} {name}: worst error / bound {gap:.3f}")
        assert torch.allclose(a.cpu(), b, rtol=rtol, atol=atol), (name, gap)
    t = sorted(touched)
    rest = [i for i in range(Vt) if i not in touched]
    assert rest
    assert torch.equal(w[rest].cpu(), w0[rest]) and not bool(m[rest].any()) and not bool(v[rest].any())
    assert torch.equal(copy[rest], copy0[rest])
    assert torch.equal(copy[t][:, :E], w[t].to(dt))  # bit for bit the cast of the fp32 master rows
    assert not bool(copy[:, E:].any())  # pad columns stay zero


def test_sparse_adam_honours_the_step_guard():
    """Guard word 1: no array changes and the step is taken off the counter at the next step();
    the step after it then equals torch's step 2, not 3."""
    Vt, E = 30, 12
    g = torch.Generator().manual_seed(2)
    table = tta.EmbeddingTable(torch.randn(Vt, E, generator=g)).to(DEV)
    copy = table.device_copy(torch.device(DEV, torch.cuda.current_device()), torch.bfloat16)
    opt = tta.SparseAdam(table.parameters(), lr=1e-2)
    ref_p = torch.nn.Parameter(table.weight.detach().cpu().clone())
    ref = torch.optim.SparseAdam([ref_p], lr=1e-2)
    p = table.weight
    dev = p.device
    grads = [sparse_grad(ids, torch.randn(len(ids), E, generator=g), Vt, E) for ids in ([1, 2, 3], [2, 3, 4], [3, 4, 5])]
    guard = towers.step_guard(dev)
    try:
        p.grad = grads[0].to(DEV)
        opt.step()
        ref_p.grad = grads[0]
        ref.step()
        before = [p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), copy.clone()]
        guard.fill_(1)
        p.grad = grads[1].to(DEV)
        opt.step()
        after = [p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], table.current_copy()]
        assert after[3] is copy
        for a, b in zip(after, before):
            assert torch.equal(a, b)
        assert int(opt.state[p]["step"]) == 2  # counted on the host until the read-back is settled
        guard.fill_(0)
        p.grad = grads[2].to(DEV)
        opt.step()
        assert int(opt.state[p]["step"]) == 2  # the skipped step was taken back, this one counted
        ref_p.grad = grads[2]
        ref.step()
        assert torch.allclose(p.detach().cpu(), ref_p.detach(), rtol=1e-5, atol=1e-6)
        assert torch.equal(table.current_copy()[:, :E], p.detach().to(torch.bfloat16))
    finally:
        guard.fill_(0)


def test_sparse_adam_rejects_dense_gradient():
    table = tta.EmbeddingTable(torch.randn(5, 4)).to(DEV)
    opt = tta.SparseAdam(table.parameters())
    table.weight.grad = torch.zeros(5, 4, device=DEV)
    with pytest.raises(tta._lib.TTError, match="sparse"):
        opt.step()
