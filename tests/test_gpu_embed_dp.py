"""A trainable EmbeddingTable under data parallelism (EmbeddingTable.set_process_group): the
ranks agree on the union of their distinct ids in the forward (dist.union_ids), each backward
writes its row sums at their positions in that union (tt_embed_grad_rows_at) and one all-reduce
of the [G, E] buffer leaves the same coalesced sparse gradient, the global batch's, on every
rank; the same SparseAdam step everywhere keeps the tables bit-identical.

Spawned tests share the box's GPU over gloo (world 2 and 3) as tests/test_gpu_dist.py does, and
run the same step in a one-rank RCCL group with TT_DIST_FORCE=1. The oracle is oracle/cpu_ref.py
on the whole batch with a sparse F.embedding, torch.optim.Adam and torch.optim.SparseAdam, as
in tests/test_gpu_embed_train.py, at that file's bounds: gradients rel (max-abs over max-abs)
< 2e-3, per-step loss rtol 2e-4, table weights rel < 1e-3. The in-process segment sums are held
to the bound of tests/test_gpu_embed_grad.py: L * 2^-24 * sum|terms| for an id seen L times.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from two_towers_amd import dist as tdp  # noqa: E402
from two_towers_amd import ops  # noqa: E402

DEV = "cuda"
V, E, H, T, GB, STEPS = 200, 16, 8, 7, 24, 3


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def make_ids(B, T, hi, g):
    """[B, T] ids with pads, tokens shared between the two towers and repeated inside a row."""
    q = torch.randint(0, hi, (B, T), generator=g)
    d = torch.randint(0, hi, (B, T), generator=g)
    q[:, -2:] = -1
    d[::2, -3:] = -1
    q[:, 1] = q[:, 0]  # repeated inside a row
    d[:, 0] = q[:, 0]  # shared between the towers
    q[0] = -1  # an all-pad row
    return q.to(torch.int32), d.to(torch.int32)


def lookup(table, ids):
    """table[ids] with zero rows for -1; the rows of ids >= 0 enter the graph as a sparse gradient."""
    ids = ids.long()
    out = torch.zeros(*ids.shape, table.shape[1], dtype=table.dtype)
    mask = ids >= 0
    return out.masked_scatter(mask[..., None].expand_as(out), F.embedding(ids[mask], table, sparse=True))


# ------------------------------------------------------------------ in process: the row plumbing
def test_three_parts_sum_to_the_whole_batch_rows():
    """A global batch split into three equal parts: the parts' buffers, added in rank order, hold
    the whole batch's row sums at exactly the whole batch's ids."""
    W, Ew = 3, 20
    g = torch.Generator().manual_seed(3)
    q, d = make_ids(GB, T, 60, g)
    n = GB // W
    parts = [torch.cat([q[r * n:(r + 1) * n].reshape(-1), d[r * n:(r + 1) * n].reshape(-1)]) for r in range(W)]
    plans = [ops.embed_plan(p.to(DEV)) for p in parts]
    guniq, dsts = tdp.union_of([pl[2] for pl in plans])
    whole = ops.embed_plan(torch.cat(parts).to(DEV))[2]
    assert torch.equal(guniq, whole) and guniq.dtype == torch.int64
    G = guniq.numel()
    assert any(pl[2].numel() < G for pl in plans)  # some rank has not seen every id
    dxs = [torch.randn(p.numel(), Ew, generator=g) for p in parts]
    total = torch.zeros(G, Ew, device=DEV)
    for pl, dst, dx in zip(plans, dsts, dxs):
        rows = torch.full((G, Ew), float("nan"), device=DEV)
        ops.embed_grad_rows_at(dx.to(DEV), pl[0], pl[1], dst, G, rows=rows)
        total += rows
    ids = torch.cat(parts).long()
    dx = torch.cat(dxs).double()
    ref = torch.zeros(V, Ew, dtype=torch.float64).index_add_(0, ids[ids >= 0], dx[ids >= 0])
    mag = torch.zeros(V, Ew, dtype=torch.float64).index_add_(0, ids[ids >= 0], dx[ids >= 0].abs())
    cnt = torch.bincount(ids[ids >= 0], minlength=V).double()
    u = guniq.cpu()
    bound = cnt[u, None] * 2.0 ** -24 * mag[u]
    err = (total.cpu().double() - ref[u]).abs()
    print(f"three parts: G={G}, worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ opt-in boundaries
def _one_backward(table):
    torch.manual_seed(11)
    m = tta.EnhancedTwoTowerModel(E, H).to(DEV).eval()
    m.set_embedding_table(table)
    g = torch.Generator().manual_seed(12)
    qi, di = make_ids(GB, T, 60, g)
    tta.InfoNCELoss()(*m(qi.to(DEV), di.to(DEV))).backward()
    return table.weight.grad


def test_table_that_has_not_opted_in_still_raises(monkeypatch):
    table = tta.EmbeddingTable(torch.randn(V, E)).to(DEV)
    monkeypatch.setattr(tta.dist, "rank_world", lambda group=None: (0, 2))
    with pytest.raises(tta._lib.TTError, match="data parallel") as ei:
        _one_backward(table)
    assert "set_process_group" in str(ei.value)


def test_opted_in_table_on_one_rank_gives_the_plain_gradient_bits():
    w0 = torch.randn(V, E, generator=torch.Generator().manual_seed(5))
    plain = _one_backward(tta.EmbeddingTable(w0).to(DEV))
    table = tta.EmbeddingTable(w0).to(DEV)
    assert table.set_process_group(None) is table
    opted = _one_backward(table)
    assert opted.is_sparse and opted.is_coalesced()
    assert torch.equal(opted._indices(), plain._indices())
    assert torch.equal(opted._values().view(torch.int32), plain._values().view(torch.int32))


# ------------------------------------------------------------------ the training driver
def test_train_driver_trains_and_saves_the_table(tmp_path):
    """python -m two_towers_amd.train --train_embeddings --max_steps 3 on one rank: the table
    moves, only in rows of ids the store holds, and is saved beside the model."""
    import struct

    import numpy as np

    from two_towers_amd import pretok, train, w2v
    rng = np.random.default_rng(0)
    Vt, n = 120, 96
    with open(tmp_path / "w2v.bin", "wb") as f:
        f.write(f"{Vt} {E}\n".encode())
        for i in range(Vt):
            f.write(f"t{i}".encode() + b" " + struct.pack(f"<{E}f", *rng.standard_normal(E)) + b"\n")
    vocab = w2v.read_word2vec_format(str(tmp_path / "w2v.bin"))
    w2v.save_store(vocab, str(tmp_path / "store"))
    docs = [" ".join(f"t{x}" for x in rng.integers(0, Vt // 2, 12)) for _ in range(n)]  # ids of the upper half unused
    with open(tmp_path / "pairs.tsv", "w") as f:
        for d in docs:
            f.write(" ".join(d.split()[:3]) + "\t" + d + "\n")
    pretok.main(["--vocab", str(tmp_path / "store"), "--pairs", str(tmp_path / "pairs.tsv"), "--out",
                 str(tmp_path / "ids"), "--max-length", "12", "--tokenizer", "enhanced", "--workers", "1"])
    out = train.main(["--ids", str(tmp_path / "ids"), "--vocab", str(tmp_path / "store"), "--output_dir",
                      str(tmp_path / "out"), "--num_epochs", "1", "--batch_size", "32", "--hidden_dim", "16",
                      "--train_embeddings", "--embed_lr", "0.01", "--max_steps", "3"])
    assert os.path.exists(f"{out}/best_model.pt")
    sd = torch.load(f"{out}/best_table.pt", map_location="cpu", weights_only=True)
    assert set(sd) == {"weight"} and tuple(sd["weight"].shape) == (Vt, E)
    moved = (sd["weight"] != torch.from_numpy(np.array(vocab.vectors, dtype=np.float32))).any(1)
    ids = np.concatenate([np.load(tmp_path / "ids" / f).reshape(-1) for f in ("q_ids.npy", "d_ids.npy")])
    used = torch.zeros(Vt, dtype=torch.bool)
    used[torch.from_numpy(np.unique(ids[ids >= 0])).long()] = True
    assert bool(moved.any()) and not bool((moved & ~used).any())


# ------------------------------------------------------------------ spawned: the training step
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup(world):
    """(model state, table, the global batches) from fixed seeds: the same on every rank and in
    the parent. Every batch has an id all ranks see (140) and one private to each rank
    (150 + rank); with world 2, rank 1's whole share of the second batch is padding."""
    torch.manual_seed(21)
    state = {k: v.detach().clone() for k, v in tta.EnhancedTwoTowerModel(E, H).state_dict().items()}
    g = torch.Generator().manual_seed(22)
    w0 = torch.randn(V, E, generator=g) * 0.5
    n = GB // world
    batches = []
    for step in range(STEPS):
        q, d = make_ids(GB, T, 120, g)
        for r in range(world):
            q[r * n + 1, 2] = 150 + r
            d[r * n + 1, 3] = 140
        if world == 2 and step == 1:
            q[n:] = -1
            d[n:] = -1
        batches.append((q, d))
    return state, w0, batches


def _train_rank(rank, world, port, backend, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if backend == "nccl":
        os.environ["TT_DIST_FORCE"] = "1"
        torch.cuda.set_device(0)
        torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        state, w0, batches = _setup(world)
        m = tta.EnhancedTwoTowerModel(E, H)
        m.load_state_dict(state)
        m = m.to(DEV).eval().set_process_group(None, overlap_grad_allreduce=world != 2)
        # rank 0's vectors are the ones every rank must end up training
        table = tta.EmbeddingTable(w0 if rank == 0 else torch.zeros(V, E)).to(DEV).set_process_group(None)
        assert torch.equal(table.weight.detach().cpu(), w0)
        m.set_embedding_table(table)
        crit = tta.InfoNCELoss(process_group=None)
        opt = tta.Adam(m.parameters(), lr=1e-3)
        opt_e = tta.SparseAdam(table.parameters(), lr=1e-2)
        params = list(m.parameters()) + list(table.parameters())
        n = GB // world
        res = {"rank": rank, "losses": []}
        for step, (q, d) in enumerate(batches):
            opt.zero_grad()
            opt_e.zero_grad()
            loss = crit(*m(q[rank * n:(rank + 1) * n].to(DEV), d[rank * n:(rank + 1) * n].to(DEV)))
            loss.backward()
            tdp.allreduce_grads(params)
            if step == 0:
                gr = table.weight.grad
                res["sparse"] = bool(gr.is_sparse and gr.is_coalesced())
                res["indices"] = gr._indices().cpu().numpy().copy()
                res["table_grad"] = gr.to_dense().cpu().numpy().copy()
                res["grads"] = {k: p.grad.cpu().numpy().copy() for k, p in m.named_parameters()}
            opt_e.step()
            opt.step()
            res["losses"].append(float(loss.detach()))
        st = opt_e.state[table.weight]
        res["weight"] = table.weight.detach().cpu().numpy().copy()
        res["exp_avg"] = st["exp_avg"].cpu().numpy().copy()
        res["exp_avg_sq"] = st["exp_avg_sq"].cpu().numpy().copy()
        copy = table.current_copy()
        res["copy_ok"] = copy is not None and torch.equal(copy[:, :E], table.weight.detach().to(copy.dtype))
        if backend == "nccl":
            res["families"] = _families_match_plain_table()
        out.put(res)
        torch.distributed.barrier()
    except BaseException as e:  # tell the parent now: it must not wait for its time limit
        out.put({"rank": rank, "error": repr(e)})
        raise
    finally:
        torch.distributed.destroy_process_group()


def _families_match_plain_table():
    """In a one-rank group every collective is an identity: for the margin and the simple family
    the opted-in table's gradient must be the plain table's, bit for bit."""
    from two_towers_amd import simple
    from two_towers_amd.margin import TwoTowerModel
    ok = {}
    g = torch.Generator().manual_seed(31)
    w0 = torch.randn(V, E, generator=g)
    qi, di = make_ids(GB, T, 60, g)
    for name in ("margin", "simple"):
        grads = []
        for opted in (False, True):
            torch.manual_seed(32)
            m = (TwoTowerModel(E, H) if name == "margin" else tta.SimpleTwoTower(E, H)).to(DEV).train()
            m.query_encoder.dropout = m.doc_encoder.dropout = 0.0  # train mode (it returns the vectors), no dropout
            for proj in ([m.projection] if name == "margin" else [m.query_proj, m.doc_proj]):
                proj[3].p = 0.0
            crit = tta.InfoNCELoss(temperature=0.1) if name == "margin" else simple.InfoNCELoss(temperature=0.1)
            table = tta.EmbeddingTable(w0).to(DEV)
            if opted:
                table.set_process_group(None)
            m.set_embedding_table(table)
            crit(*m(qi.to(DEV), di.to(DEV))).backward()
            grads.append(table.weight.grad)
        a, b = grads
        ok[name] = bool(b.is_coalesced() and torch.equal(a._indices(), b._indices())
                        and torch.equal(a._values().view(torch.int32), b._values().view(torch.int32)))
    return ok


_oracles = {}


def _oracle(world):
    """The single-process steps on the whole batches of this world size, computed once."""
    key = world
    if key in _oracles:
        return _oracles[key]
    state, w0, batches = _setup(world)
    pr = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    wr = w0.clone().requires_grad_(True)
    ropt = torch.optim.Adam(list(pr.values()), lr=1e-3)
    ropt_e = torch.optim.SparseAdam([wr], lr=1e-2)
    ref = {"losses": []}
    for step, (q, d) in enumerate(batches):
        ropt.zero_grad()
        ropt_e.zero_grad()
        rl = cpu_ref.infonce(*cpu_ref.forward(lookup(wr, q), lookup(wr, d), pr))
        rl.backward()
        if step == 0:
            ref["table_grad"] = wr.grad.to_dense().clone()
            ref["grads"] = {k: v.grad.clone() for k, v in pr.items()}
        ropt_e.step()
        ropt.step()
        ref["losses"].append(float(rl.detach()))
    ref["weight"] = wr.detach().clone()
    seen = [torch.unique(torch.cat([q.flatten(), d.flatten()]).long()) for q, d in batches]
    ref["seen0"] = seen[0][seen[0] >= 0]
    allseen = torch.unique(torch.cat(seen))
    ref["seen"] = allseen[allseen >= 0]
    ref["w0"] = w0
    _oracles[key] = ref
    return ref


def _check_step(res, ref):
    """Assertions 1-3 on one rank's results."""
    assert res["sparse"], "table gradient is not a coalesced sparse tensor"
    assert torch.equal(torch.from_numpy(res["indices"]), ref["seen0"][None]), "indices are not the global batch's ids"
    err = rel(res["table_grad"], ref["table_grad"])
    worst = max(rel(res["grads"][k], ref["grads"][k]) for k in ref["grads"])
    print(f"rank {res['rank']}: table gradient rel {err:.2e}, parameter gradients worst rel {worst:.2e}, "
          f"losses {res['losses']} reference {ref['losses']}")
    assert err < 2e-3 and worst < 2e-3, (err, worst)
    torch.testing.assert_close(torch.tensor(res["losses"]), torch.tensor(ref["losses"]), rtol=2e-4, atol=0.0)


@pytest.mark.parametrize("world", [2, 3])
def test_dp_table_training_matches_the_global_batch(world):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_train_rank, args=(r, world, port, "gloo", out)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = out.get(timeout=180)
        assert "error" not in r, r
        res[r["rank"]] = r
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = _oracle(world)
    expect = torch.zeros(V, dtype=torch.bool)
    expect[ref["seen"]] = True
    assert not bool(expect.all())
    for r in range(world):
        _check_step(res[r], ref)
        for k in ("weight", "exp_avg", "exp_avg_sq"):  # the same bits on every rank
            assert (res[r][k].view("int32") == res[0][k].view("int32")).all(), (r, k)
        moved = (torch.from_numpy(res[r]["weight"]) != ref["w0"]).any(1)
        assert torch.equal(moved, expect)
        assert rel(res[r]["weight"], ref["weight"]) < 1e-3
        assert res[r]["copy_ok"]


def test_rccl_one_rank_table_step_matches_reference():
    """The id all-gathers and the row all-reduce as RCCL calls: a one-rank group with
    TT_DIST_FORCE=1, as test_rccl_one_rank_train_step_matches_reference in tests/test_gpu_dist.py."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    p = ctx.Process(target=_train_rank, args=(0, 1, _port(), "nccl", out))
    p.start()
    res = out.get(timeout=180)
    assert "error" not in res, res
    p.join(timeout=60)
    assert p.exitcode == 0
    _check_step(res, _oracle(1))
    assert res["copy_ok"]
    assert res["families"] == {"margin": True, "simple": True}
