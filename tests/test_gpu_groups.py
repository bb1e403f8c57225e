"""Group masks at the module level: the loss modules with `groups`, mining with row / column
ids, HardNegativeMarginLoss with groups, and the id all-gather under a process group.

Loss modules against float64 torch autograd of normalise -> masked scores -> cross_entropy
(B 200, fp32 h 64 and bf16 h 128, the 200 x 200 group pattern of tests/groups_cases.py). For
bf16 the reference rounds the normalised vectors to bf16 with a straight-through gradient, as
the module does: the kernels see bf16 operands and the normalisation's backward runs on the
unrounded fp32 vectors. Tolerances are those of the existing module-level tests:
  loss       bf16 |x - ref| <= 1e-5 |ref| + 2e-4, fp32 1e-4 |ref| + 1e-5 (tests/test_gpu_infonce_bwd.py,
             tests/test_gpu_infonce_sym.py); for the un-normalised in-batch MarginRankingLoss the
             absolute term is multiplied by max |S|, as oracle/loss_ref.py infonce_fwd_errs does;
  gradients  bf16 max-abs <= 1.5e-2 of the largest entry and cosine >= 0.9999; fp32 rtol 1e-4 /
             atol 1e-5.
Mining: the reference is mine_hard_negatives(k = nd, return_values=True) without groups on the
same inputs, filtered on the CPU by the group rule; its first k must equal the grouped call's
indices and values exactly (the prefix property stated in include/tt_hip.h).
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import groups_cases as G  # noqa: E402
from oracle import loss_ref as L  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
B = 200
DTYPES = [(F32, 64), (BF, 128)]


def _inputs(h, scale=1.0):
    gen = torch.Generator().manual_seed(11 + h)
    return scale * torch.randn(B, h, generator=gen), scale * torch.randn(B, h, generator=gen)


def _rounded(x, dt):
    """x as the kernels see it, with the straight-through gradient of the module."""
    if dt == F32:
        return x
    return x + (x.float().to(BF).double() - x).detach()


def _excl():
    grp, _ = G.groups_tiles_apart(B)
    return grp, G.excluded(B, B, 0, grp, grp)


def _reference(kind, q, d, dt):
    """(loss, dq, dd, max |S|) in float64 by torch autograd."""
    q64, d64 = q.double().requires_grad_(True), d.double().requires_grad_(True)
    _, ex = _excl()
    lab = torch.arange(B)
    if kind == "margin":  # un-normalised, / temperature 0.1, margin 0.2 off the diagonal
        s = _rounded(q64, dt) @ _rounded(d64, dt).t() / 0.1
        s = s - 0.2 * (1.0 - torch.eye(B, dtype=torch.float64))
    else:
        qn = _rounded(torch.nn.functional.normalize(q64, dim=1), dt)
        dn = _rounded(torch.nn.functional.normalize(d64, dim=1), dt)
        s = qn @ dn.t() / (0.07 if kind == "infonce" else 0.1)
    smax = float(s.detach().abs().max())
    s = s.masked_fill(ex, float("-inf"))
    loss = torch.nn.functional.cross_entropy(s, lab)
    if kind == "sym":
        loss = 0.5 * (loss + torch.nn.functional.cross_entropy(s.t(), lab))
    loss.backward()
    return float(loss), q64.grad, d64.grad, smax


def _module(kind, dt):
    import two_towers_amd as tta
    if kind == "infonce":
        return tta.InfoNCELoss(temperature=0.07, compute_dtype=dt)
    if kind == "sym":
        return tta.SymmetricInfoNCELoss(temperature=0.1, normalize=True, compute_dtype=dt)
    return tta.MarginRankingLoss(margin=0.2, temperature=0.1, compute_dtype=dt)


def _run(crit, q, d, **kw):
    ql, dl = q.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    loss = crit(ql, dl, **kw)
    loss.backward()
    return loss.detach().cpu(), ql.grad.cpu(), dl.grad.cpu()


@pytest.mark.parametrize("dt,h", DTYPES)
@pytest.mark.parametrize("kind", ["infonce", "sym", "margin"])
def test_loss_modules_with_groups_match_float64_autograd(kind, dt, h):
    q, d = _inputs(h, 0.25 if kind == "margin" else 1.0)
    grp, _ = _excl()
    rloss, rq, rd, smax = _reference(kind, q, d, dt)
    crit = _module(kind, dt)
    loss, dq, dd = _run(crit, q, d, groups=grp.to(DEV))
    scale = max(1.0, smax) if kind == "margin" else 1.0
    bound = 1e-5 * abs(rloss) + 2e-4 * scale if dt == BF else 1e-4 * abs(rloss) + 1e-5 * scale
    print(f"{kind} {dt}: loss {float(loss):.6f} ref {rloss:.6f} (bound {bound:.2e}), max |S| {smax:.1f}")
    assert abs(float(loss) - rloss) <= bound
    for name, got, ref in (("dq", dq, rq), ("dd", dd, rd)):
        assert bool(torch.isfinite(got).all()), name
        err, cos = L.whole_err(got, ref)
        print(f"{kind} {dt} {name}: max-abs {err:.3g} of the largest entry, 1 - cos {1 - cos:.3g}")
        if dt == BF:
            assert err <= 1.5e-2 and cos >= 0.9999, (name, err, cos)
        else:
            torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-5)
    # int64 ids on the host are converted; the ids never enter autograd
    loss2, dq2, dd2 = _run(crit, q, d, groups=grp.long())
    assert torch.equal(loss, loss2) and torch.equal(dq, dq2) and torch.equal(dd, dd2)


@pytest.mark.parametrize("dt,h", DTYPES)
@pytest.mark.parametrize("kind", ["infonce", "sym", "margin"])
def test_groups_none_is_the_ungrouped_module(kind, dt, h):
    """groups=None takes the ungrouped path: the same bits as the call without the argument;
    ids that are all negative go through the grouped kernels and give those bits too."""
    q, d = _inputs(h, 0.25 if kind == "margin" else 1.0)
    crit = _module(kind, dt)
    plain = _run(crit, q, d)
    for kw in (dict(groups=None), dict(groups=torch.full((B,), -1, dtype=torch.int32, device=DEV))):
        got = _run(crit, q, d, **kw)
        for a, b in zip(plain, got):
            assert L.bits_differ(a, b)[0] == 0, (kind, kw)


def test_groups_argument_errors():
    import two_towers_amd as tta
    from two_towers_amd._lib import TTError
    q, d = (t.to(DEV) for t in _inputs(64))
    with pytest.raises(TTError, match="groups"):
        tta.InfoNCELoss()(q, d, groups=torch.zeros(B - 1, dtype=torch.int32))
    with pytest.raises(TTError, match="groups"):
        tta.InfoNCELoss()(q, d, groups=torch.zeros(B))
    with pytest.raises(TTError, match="groups"):
        tta.MarginRankingLoss()(q, d, d, groups=torch.zeros(B, dtype=torch.int32))


# ------------------------------------------------------------------------------- mining
BQ, ND, LAB0 = 130, 300, 170


def _mining_inputs(h):
    """Rows < 120 in groups of four (i // 4) whose label columns 170 + i carry the ids: the four
    documents of a group are near copies of one another and of their queries, so a row's mates
    are its most similar documents: what ungrouped mining returns first."""
    gen = torch.Generator().manual_seed(5 + h)
    d = torch.randn(ND, h, generator=gen)
    q = torch.randn(BQ, h, generator=gen)
    rg = torch.full((BQ,), -1, dtype=torch.int32)
    rg[:120] = torch.arange(120, dtype=torch.int32) // 4
    cg = torch.full((ND,), -1, dtype=torch.int32)
    cg[LAB0:LAB0 + BQ] = rg
    for i in range(120):
        d[LAB0 + i] = d[LAB0 + 4 * (i // 4)] + 0.1 * torch.randn(h, generator=gen)
        q[i] = d[LAB0 + i] + 0.1 * torch.randn(h, generator=gen)
    return q.to(DEV), d.to(DEV), rg, cg


@pytest.mark.parametrize("dt,h", [(BF, 128), (F32, 36)])
def test_mining_with_groups_is_the_filtered_full_ranking(dt, h):
    from two_towers_amd._lib import TTError
    from two_towers_amd.losses import mine_hard_negatives
    q, d, rg, cg = _mining_inputs(h)
    full_i, full_v = (t.cpu() for t in mine_hard_negatives(q, d, LAB0, ND, dt, return_values=True))
    ex = G.excluded(BQ, ND, LAB0, rg, cg)
    plain5 = mine_hard_negatives(q, d, LAB0, 5, dt).cpu()
    assert bool(ex[torch.arange(BQ)[:, None], plain5.long()].any()), "the inputs do not make mates hard negatives"
    for k, path in ((5, "k + g = 8"), (14, "k + g = 17: the stored-score path")):
        idx, val = (t.cpu() for t in mine_hard_negatives(q, d, LAB0, k, dt, return_values=True, row_groups=rg,
                                                         col_groups=cg, max_group_size=4))
        for r in range(BQ):
            keep = ~ex[r, full_i[r].long()]
            assert torch.equal(idx[r], full_i[r][keep][:k]), (path, r)
            assert L.bits_differ(val[r], full_v[r][keep][:k])[0] == 0, (path, r)
        assert not bool(ex[torch.arange(BQ)[:, None], idx.long()].any()), "an excluded column was returned"
        auto = mine_hard_negatives(q, d, LAB0, k, dt, row_groups=rg.to(DEV), col_groups=cg.to(DEV)).cpu()
        assert torch.equal(auto, idx), "max_group_size=None"
    with pytest.raises(TTError, match="298"):  # k + g = 298 + 3 > nd = 300
        mine_hard_negatives(q, d, LAB0, 298, dt, row_groups=rg, col_groups=cg, max_group_size=4)
    with pytest.raises(TTError, match="go together"):
        mine_hard_negatives(q, d, LAB0, 5, dt, row_groups=rg)


def test_hard_negative_margin_loss_with_groups():
    import two_towers_amd as tta
    h = 36
    q, d, rg, cg = _mining_inputs(h)
    q, d = q[:, :].contiguous(), d[LAB0:LAB0 + BQ].contiguous()  # one id per pair: the square batch
    ex = G.excluded(BQ, BQ, 0, rg, rg)
    plain = tta.HardNegativeMarginLoss(k=5, margin=0.2)
    plain(q, d)
    assert bool(ex[torch.arange(BQ)[:, None], plain.last_indices.cpu().long()].any()), "no mate is mined without groups"
    for mgs in (4, None):
        crit = tta.HardNegativeMarginLoss(k=5, margin=0.2, max_group_size=mgs)
        ql, dl = q.clone().requires_grad_(True), d.clone().requires_grad_(True)
        loss = crit(ql, dl, groups=rg.to(DEV))
        loss.backward()
        idx = crit.last_indices.cpu()
        assert not bool(ex[torch.arange(BQ)[:, None], idx.long()].any()), "a mate was mined"
        qn = torch.nn.functional.normalize(q.double().cpu(), dim=1)
        dn = torch.nn.functional.normalize(d.double().cpu(), dim=1)
        ref = float(L.margin_ref(qn, dn, 0, idx, 0.2)[2].mean())
        assert abs(float(loss) - ref) <= 1e-5, (float(loss), ref)
        assert bool(torch.isfinite(ql.grad).all()) and bool(torch.isfinite(dl.grad).all())
        # the explicit-negative module on the mined rows is the same composition
        comp = tta.MarginRankingLoss(margin=0.2)(q, d, d[idx.to(DEV).long().reshape(-1)])
        assert abs(float(comp) - float(loss)) <= 1e-5


# ----------------------------------------------------- the id all-gather under a process group
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _forced_rank(port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TT_DIST_FORCE="1")
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        import two_towers_amd as tta
        from two_towers_amd import dist as tdp
        assert tdp.active(None)
        q, d = _inputs(64)
        grp, _ = G.groups_tiles_apart(B)
        res = []
        for crit in (tta.InfoNCELoss(temperature=0.07), tta.SymmetricInfoNCELoss(temperature=0.1, normalize=True)):
            loss, dq, dd = _run(crit, q, d, groups=grp.to(DEV))
            res.append((loss.numpy().copy(), dq.numpy().copy(), dd.numpy().copy()))
        out.put(res)
    finally:
        torch.distributed.destroy_process_group()


def test_forced_one_rank_process_group_gathers_the_ids():
    """TT_DIST_FORCE=1 in a one-rank RCCL group: the ids are all-gathered with the document rows
    and every collective is an identity, so InfoNCELoss with groups returns the bits of the
    process without a group. The symmetric loss then runs as two one-directional calls, both
    with the ids, and must agree with the fused grouped kernel within the fp32 tolerance."""
    import numpy as np
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    p = ctx.Process(target=_forced_rank, args=(_port(), out))
    p.start()
    res = out.get(timeout=180)
    p.join(timeout=60)
    assert p.exitcode == 0
    q, d = _inputs(64)
    grp, _ = G.groups_tiles_apart(B)
    here = _run(_module("infonce", F32), q, d, groups=grp.to(DEV))
    for a, b in zip(res[0], here):
        assert np.array_equal(a, b.numpy())
    sym = _run(_module("sym", F32), q, d, groups=grp.to(DEV))
    assert abs(float(res[1][0]) - float(sym[0])) <= 1e-4 * abs(float(sym[0])) + 1e-5
    for a, b in zip(res[1][1:], sym[1:]):
        torch.testing.assert_close(torch.from_numpy(a), b, rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------- training script
@pytest.mark.parametrize("loss", ["infonce", "hardneg"])
def test_train_mask_duplicates(tmp_path, loss):
    """pretok --groups -> train --mask_duplicates runs both losses over a store in which every
    third query repeats its predecessor; a store written without groups is a clear error."""
    import struct

    import numpy as np

    from two_towers_amd import pretok, train, w2v
    rng = np.random.default_rng(0)
    E, V, n = 16, 120, 96
    with open(tmp_path / "w2v.bin", "wb") as f:
        f.write(f"{V} {E}\n".encode())
        for i in range(V):
            f.write(f"t{i}".encode() + b" " + struct.pack(f"<{E}f", *rng.standard_normal(E)) + b"\n")
    w2v.save_store(w2v.read_word2vec_format(str(tmp_path / "w2v.bin")), str(tmp_path / "store"))
    docs = [" ".join(f"t{x}" for x in rng.integers(0, V, 12)) for _ in range(n)]
    queries = [" ".join(d.split()[:3]) for d in docs]
    for i in range(2, n, 3):
        queries[i] = queries[i - 1]  # one query, two selected passages
    with open(tmp_path / "pairs.tsv", "w") as f:
        for q, d in zip(queries, docs):
            f.write(f"{q}\t{d}\n")
    common = ["--vocab", str(tmp_path / "store"), "--pairs", str(tmp_path / "pairs.tsv"), "--max-length", "12",
              "--workers", "1"]
    pretok.main(common + ["--out", str(tmp_path / "ids"), "--groups"])
    store = pretok.PairIds(str(tmp_path / "ids"))
    assert store.max_group_size == 2 and int((np.bincount(store.groups) == 2).sum()) == n // 3
    args = ["--vocab", str(tmp_path / "store"), "--output_dir", str(tmp_path / "out"), "--num_epochs", "1",
            "--batch_size", "32", "--hidden_dim", "16", "--log_every", "1", "--loss", loss, "--mask_duplicates"]
    out = train.main(["--ids", str(tmp_path / "ids")] + args)
    log = open(f"{out}/training.log").read()
    losses = [float(x.split("Average Loss: ")[1].split()[0]) for x in log.splitlines() if "Average Loss" in x]
    assert len(losses) == 1 and np.isfinite(losses[0])
    pretok.main(common + ["--out", str(tmp_path / "ids_plain")])
    with pytest.raises(ValueError, match="groups"):
        train.main(["--ids", str(tmp_path / "ids_plain")] + args)
