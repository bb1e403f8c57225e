"""Gradients out of the bottom of the towers, through the models: dL/dx for float inputs that
require grad, the sparse gradient of a trainable EmbeddingTable (all three model families),
SparseAdam steps, the coherence of the table's compute copy, and clip_grad_norm_ with a sparse
gradient in the list. The oracle is oracle/cpu_ref.py with requires_grad_ inputs on the CPU.

Bounds are those of the tests whose path is extended: fp32 gradients rel (max-abs over
max-abs) < 2e-3 and bf16 cos >= 0.998 / Frobenius <= 6 % (tests/test_gpu_model.py), per-step
loss rtol 2e-4 (the tiny_train trajectory, tests/test_gpu_golden.py), clipping rtol 1e-5
(tests/test_gpu_optim_clip.py).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from two_towers_amd import simple  # noqa: E402
from two_towers_amd.margin import TwoTowerModel  # noqa: E402

DEV = "cuda"


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def make_model(E, h, seed=0):
    torch.manual_seed(seed)
    m = tta.EnhancedTwoTowerModel(E, h)
    p = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m, p


# ------------------------------------------------------------------ float inputs
@pytest.mark.parametrize("E,h,B,T", [(16, 8, 16, 8), (40, 32, 100, 12), (300, 64, 64, 16)])
def test_input_gradients_fp32(E, h, B, T):
    """Measured rel errors of (q.grad, d.grad): (16, 8, 16, 8) 1.07e-06, 3.39e-07;
    (40, 32, 100, 12) 1.03e-06, 2.61e-06; (300, 64, 64, 16) 1.57e-06, 1.73e-06 (bound 2e-3)."""
    m, p = make_model(E, h)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, T, E, generator=g)
    d = torch.randn(B, T, E, generator=g)
    qd, dd = q.clone().to(DEV).requires_grad_(True), d.clone().to(DEV).requires_grad_(True)
    tta.InfoNCELoss()(*m(qd, dd)).backward()
    assert qd.grad is not None and dd.grad is not None
    assert qd.grad.shape == (B, T, E) and qd.grad.dtype == torch.float32
    qr, dr = q.clone().requires_grad_(True), d.clone().requires_grad_(True)
    cpu_ref.infonce(*cpu_ref.forward(qr, dr, p)).backward()
    eq, ed = rel(qd.grad, qr.grad), rel(dd.grad, dr.grad)
    print(f"input gradients fp32 {(E, h, B, T)}: rel q {eq:.2e} d {ed:.2e}")
    assert eq < 2e-3 and ed < 2e-3, (eq, ed)


def test_input_gradients_bf16():
    """bf16 storage / fp32 accumulation against the fp32 oracle on the same bf16-rounded inputs
    and weights. Measured: q cos 0.999658 frob 0.0262, d cos 0.999319 frob 0.0370 (bounds
    cos >= 0.998, Frobenius <= 6 %)."""
    E, h, B, T = 64, 32, 96, 10
    m, _ = make_model(E, h, 1)
    with torch.no_grad():
        for prm in m.parameters():
            prm.copy_(prm.to(torch.bfloat16).float())
    p = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).eval().set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(6)
    q = torch.randn(B, T, E, generator=g).to(torch.bfloat16).float()
    d = torch.randn(B, T, E, generator=g).to(torch.bfloat16).float()
    qd, dd = q.clone().to(DEV).requires_grad_(True), d.clone().to(DEV).requires_grad_(True)
    tta.InfoNCELoss(compute_dtype=torch.bfloat16)(*m(qd, dd)).backward()
    qr, dr = q.clone().requires_grad_(True), d.clone().requires_grad_(True)
    cpu_ref.infonce(*cpu_ref.forward(qr, dr, p)).backward()
    for name, a, b in (("q", qd.grad, qr.grad), ("d", dd.grad, dr.grad)):
        a, b = a.double().cpu(), b.double()
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        frob = float((a - b).norm() / b.norm())
        print(f"input gradients bf16 {name}: cos {cos:.6f} frob {frob:.4f}")
        assert cos >= 0.998 and frob <= 0.06, (name, cos, frob)


@pytest.mark.parametrize("train", [False, True])
def test_parameter_gradients_do_not_change_with_input_gradients(train):
    """Same seed, eval mode and train mode with dropout: asking for input gradients adds a
    GEMM after the layer-0 BPTT and changes no parameter gradient by a bit. One input alone
    requiring grad gives the same input gradient as both."""
    E, h, B, T = 24, 16, 40, 6
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B, T, E, generator=g).to(DEV)
    d = torch.randn(B, T, E, generator=g).to(DEV)
    outs = []
    for want in ((False, False), (True, True), (False, True)):
        m, _ = make_model(E, h, 2)
        m = m.to(DEV)
        m.train(train)
        qi, di = q.clone().requires_grad_(want[0]), d.clone().requires_grad_(want[1])
        torch.manual_seed(99)
        tta.InfoNCELoss()(*m(qi, di)).backward()
        outs.append(({k: v.grad.clone() for k, v in m.named_parameters()}, qi.grad, di.grad))
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]) and torch.equal(outs[0][0][k], outs[2][0][k]), k
    assert outs[0][1] is None and outs[0][2] is None and outs[2][1] is None
    assert torch.equal(outs[1][2], outs[2][2])


def test_frozen_parameters_still_give_input_gradients():
    """No parameter requires grad: the call must still take the training forward."""
    E, h, B, T = 16, 8, 12, 5
    m, p = make_model(E, h, 3)
    m = m.to(DEV).eval()
    for prm in m.parameters():
        prm.requires_grad_(False)
    g = torch.Generator().manual_seed(8)
    q, d = torch.randn(B, T, E, generator=g), torch.randn(B, T, E, generator=g)
    qd = q.clone().to(DEV).requires_grad_(True)
    tta.InfoNCELoss()(*m(qd, d.to(DEV))).backward()
    qr = q.clone().requires_grad_(True)
    cpu_ref.infonce(*cpu_ref.forward(qr, d, p)).backward()
    assert rel(qd.grad, qr.grad) < 2e-3


# ------------------------------------------------------------------ trainable table
V = 200


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
    """table[ids] with zero rows for -1; only the rows of ids >= 0 enter the graph, as a sparse
    gradient (nn.Embedding(sparse=True))."""
    ids = ids.long()
    out = torch.zeros(*ids.shape, table.shape[1], dtype=table.dtype)
    mask = ids >= 0
    return out.masked_scatter(mask[..., None].expand_as(out), F.embedding(ids[mask], table, sparse=True))


def simple_ref(q, d, p):
    """SimpleTwoTower.forward + the symmetric InfoNCE(0.1), dropout off."""
    def enc(x, e, pr):
        hn, _ = cpu_ref.gru_encoder(x, p, e)
        a = F.linear(torch.cat([hn[-2], hn[-1]], 1), p[pr + ".0.weight"], p[pr + ".0.bias"])
        a = torch.relu(F.layer_norm(a, (a.shape[1],), p[pr + ".1.weight"], p[pr + ".1.bias"], 1e-5))
        return F.normalize(F.linear(a, p[pr + ".4.weight"], p[pr + ".4.bias"]), dim=1)
    s = enc(q, "query_encoder", "query_proj") @ enc(d, "doc_encoder", "doc_proj").t() / 0.1
    lab = torch.arange(s.shape[0])
    return 0.5 * (F.cross_entropy(s, lab) + F.cross_entropy(s.t(), lab))


def family(name, E, h):
    """(model on the GPU with every dropout off, its loss, the CPU oracle's loss function)."""
    torch.manual_seed(11)
    if name == "enhanced":
        m = tta.EnhancedTwoTowerModel(E, h).eval()
        return m, tta.InfoNCELoss(), lambda q, d, p: cpu_ref.infonce(*cpu_ref.forward(q, d, p))
    m = TwoTowerModel(E, h) if name == "margin" else tta.SimpleTwoTower(E, h)
    m.train()
    m.query_encoder.dropout = 0.0
    m.doc_encoder.dropout = 0.0
    if name == "margin":
        m.projection[3].p = 0.0
        return m, tta.InfoNCELoss(temperature=0.1), lambda q, d, p: cpu_ref.infonce(
            *cpu_ref.margin_forward(q, d, p, True), temperature=0.1)
    m.query_proj[3].p = 0.0
    m.doc_proj[3].p = 0.0
    return m, simple.InfoNCELoss(temperature=0.1), simple_ref


@pytest.mark.parametrize("name", ["enhanced", "margin", "simple"])
def test_trainable_table_gradient(name):
    """weight.grad is a coalesced sparse [V, E] tensor over exactly the ids seen, equal to the
    oracle's table gradient, and the same bits in two backward passes. Measured rel error:
    enhanced 1.09e-06, margin 7.86e-07, simple 4.91e-07 (bound 2e-3)."""
    E, h, B, T = 20, 16, 24, 7
    m, crit, ref_loss = family(name, E, h)
    p = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV)
    g = torch.Generator().manual_seed(12)
    w0 = torch.randn(V, E, generator=g)
    qi, di = make_ids(B, T, 60, g)
    table = tta.EmbeddingTable(w0).to(DEV)
    m.set_embedding_table(table)
    grads = []
    for _ in range(2):
        table.weight.grad = None
        m.zero_grad()
        crit(*m(qi.to(DEV), di.to(DEV))).backward()
        grads.append(table.weight.grad)
    gr = grads[0]
    assert gr.is_sparse and gr.is_coalesced() and tuple(gr.shape) == (V, E) and gr.dtype == torch.float32
    seen = torch.unique(torch.cat([qi.flatten(), di.flatten()]).long())
    seen = seen[seen >= 0]
    assert torch.equal(gr._indices().cpu(), seen[None])
    assert torch.equal(grads[1]._indices(), gr._indices()) and torch.equal(grads[1]._values(), gr._values())
    wr = w0.clone().requires_grad_(True)
    ref_loss(lookup(wr, qi), lookup(wr, di), p).backward()
    ref = wr.grad.to_dense()
    err = rel(gr.to_dense(), ref)
    named = dict(m.named_parameters())
    worst = max(rel(named[k].grad, p[k].grad) for k in p)
    print(f"table gradient {name}: rel {err:.2e}; parameter gradients worst rel {worst:.2e}")
    assert err < 2e-3 and worst < 2e-3, (err, worst)
    unseen = torch.ones(V, dtype=torch.bool)
    unseen[seen] = False
    assert not bool(ref[unseen].any())


def test_frozen_table_takes_no_gradient():
    """trainable=False and a plain tensor: no table gradient, and the same outputs and
    parameter gradients, bit for bit, as the trainable table gives."""
    E, h, B, T = 20, 16, 24, 7
    g = torch.Generator().manual_seed(13)
    w0 = torch.randn(V, E, generator=g)
    qi, di = make_ids(B, T, 60, g)
    outs = []
    for kind in ("tensor", "frozen", "trainable"):
        m, crit, _ = family("enhanced", E, h)
        m = m.to(DEV)
        table = w0.to(DEV) if kind == "tensor" else tta.EmbeddingTable(w0, trainable=kind == "trainable").to(DEV)
        m.set_embedding_table(table)
        qv, dv = m(qi.to(DEV), di.to(DEV))
        crit(qv, dv).backward()
        if kind != "tensor":
            assert (table.weight.grad is not None) == (kind == "trainable")
        outs.append((qv.detach(), dv.detach(), {k: v.grad for k, v in m.named_parameters()}))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
        for k in o[2]:
            assert torch.equal(o[2][k], outs[0][2][k]), k


def test_ten_steps_adam_and_sparse_adam_match_torch():
    """tta.Adam on the model and tta.SparseAdam on the table against torch.optim.Adam +
    torch.optim.SparseAdam on the CPU oracle: per-step loss rtol 2e-4; the table rows that
    moved are exactly the ids seen, every other row keeps its bits."""
    E, h, B, T, steps = 16, 8, 16, 8, 10
    m, p0 = make_model(E, h, 21)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(22)
    w0 = torch.randn(V, E, generator=g) * 0.5
    batches = [make_ids(B, T, 120, g) for _ in range(steps)]
    table = tta.EmbeddingTable(w0).to(DEV)
    m.set_embedding_table(table)
    opt = tta.Adam(m.parameters(), lr=1e-3)
    opt_e = tta.SparseAdam(table.parameters(), lr=1e-2)
    crit = tta.InfoNCELoss()
    losses = []
    for qi, di in batches:
        opt.zero_grad()
        opt_e.zero_grad()
        loss = crit(*m(qi.to(DEV), di.to(DEV)))
        loss.backward()
        opt_e.step()
        opt.step()
        losses.append(float(loss.detach()))
    pr = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    wr = w0.clone().requires_grad_(True)
    ropt = torch.optim.Adam(list(pr.values()), lr=1e-3)
    ropt_e = torch.optim.SparseAdam([wr], lr=1e-2)
    ref_losses = []
    for qi, di in batches:
        ropt.zero_grad()
        ropt_e.zero_grad()
        rl = cpu_ref.infonce(*cpu_ref.forward(lookup(wr, qi), lookup(wr, di), pr))
        rl.backward()
        ropt_e.step()
        ropt.step()
        ref_losses.append(float(rl.detach()))
    print("losses", losses, "reference", ref_losses)
    torch.testing.assert_close(torch.tensor(losses), torch.tensor(ref_losses), rtol=2e-4, atol=0.0)
    seen = torch.unique(torch.cat([x.flatten() for b in batches for x in b]).long())
    seen = seen[seen >= 0]
    moved = (table.weight.detach().cpu() != w0).any(1)
    expect = torch.zeros(V, dtype=torch.bool)
    expect[seen] = True
    assert torch.equal(moved, expect) and not bool(expect.all())
    assert rel(table.weight, wr) < 1e-3


# ------------------------------------------------------------------ coherence, clipping, errors
def test_compute_copy_follows_every_writer():
    """After a tta.SparseAdam step (rows rewritten in place), a torch.optim.SparseAdam step and
    a weight.data.copy_ (both: full rebuild), encoding token ids equals encoding the float rows
    weight[ids] (fp32, atol 0, as test_token_ids_match_float_inputs)."""
    E, h, B, T = 32, 16, 20, 9
    m, _ = make_model(E, h, 3)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    table = tta.EmbeddingTable(torch.randn(V, E, generator=g)).to(DEV)
    m.set_embedding_table(table)
    qi, di = make_ids(B, T, V, g)
    qi, di = qi.to(DEV), di.to(DEV)

    def check(what):
        w = table.weight.detach()
        emb = torch.where((di >= 0)[..., None], w[di.clamp_min(0).long()], torch.zeros(E, device=DEV))
        with torch.no_grad():
            a = m.encode_doc(di)
            b = m.encode_doc(emb)
        assert torch.allclose(a, b, rtol=0, atol=0), what

    check("fresh table")
    copy = table.current_copy()
    assert copy is not None
    opt_e = tta.SparseAdam(table.parameters(), lr=1e-2)
    tta.InfoNCELoss()(*m(qi, di)).backward()
    before = table.weight.detach().clone()
    opt_e.step()
    assert not torch.equal(table.weight.detach(), before)
    assert table.current_copy() is copy  # kept in step row by row, not rebuilt
    check("after two_towers_amd.SparseAdam")
    topt = torch.optim.SparseAdam(table.parameters(), lr=1e-2)
    topt.step()
    assert table.current_copy() is None  # another writer: rebuilt at the next use
    check("after torch.optim.SparseAdam")
    table.weight.data.copy_(torch.randn(V, E, generator=g))
    check("after weight.data.copy_")
    with torch.no_grad():
        table.weight.copy_(torch.randn(V, E, generator=g))
    check("after copy_")
    table.load_state_dict({"weight": torch.randn(V, E, generator=g)})
    check("after load_state_dict")


def test_clip_grad_norm_with_sparse_gradient():
    E, h, B, T = 20, 16, 24, 7
    m, crit, _ = family("simple", E, h)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(41)
    table = tta.EmbeddingTable(torch.randn(V, E, generator=g)).to(DEV)
    m.set_embedding_table(table)
    qi, di = make_ids(B, T, 60, g)
    crit(*m(qi.to(DEV), di.to(DEV))).backward()
    params = list(m.parameters()) + [table.weight]
    refs = [torch.nn.Parameter(torch.zeros(p.shape)) for p in params]
    for r, p in zip(refs, params):
        r.grad = (p.grad.to_dense() if p.grad.is_sparse else p.grad).detach().cpu().clone()
    ref_norm = torch.nn.utils.clip_grad_norm_(refs, 0.25)
    assert float(ref_norm) > 0.25  # the clip is active
    idx = table.weight.grad._indices().clone()
    norm = tta.clip_grad_norm_(params, 0.25)
    torch.testing.assert_close(norm.cpu(), ref_norm, rtol=1e-5, atol=0.0)
    gs = table.weight.grad
    assert gs.is_sparse and gs.is_coalesced() and torch.equal(gs._indices(), idx)
    for r, p in zip(refs, params):
        got = p.grad.to_dense() if p.grad.is_sparse else p.grad
        torch.testing.assert_close(got.cpu(), r.grad, rtol=1e-5, atol=1e-12)


def test_trainable_table_under_data_parallel_raises(monkeypatch):
    E, h = 16, 8
    m, _ = make_model(E, h)
    m = m.to(DEV).eval()
    m.set_embedding_table(tta.EmbeddingTable(torch.randn(V, E)).to(DEV))
    ids = torch.randint(0, V, (4, 5), dtype=torch.int32, device=DEV)
    monkeypatch.setattr(tta.dist, "rank_world", lambda group=None: (0, 2))
    with pytest.raises(tta._lib.TTError, match="data parallel"):
        m(ids, ids)
    with torch.no_grad():  # nothing to train: allowed
        m(ids, ids)
    m.set_embedding_table(tta.EmbeddingTable(torch.randn(V, E), trainable=False).to(DEV))
    m(ids, ids)


def test_table_on_the_wrong_device_fails_loudly():
    m, _ = make_model(16, 8)
    m = m.to(DEV).eval()
    m.set_embedding_table(tta.EmbeddingTable(torch.randn(V, 16)))
    with pytest.raises(tta._lib.TTError, match="move the table"):
        m.encode_doc(torch.zeros(2, 3, dtype=torch.int32, device=DEV))
