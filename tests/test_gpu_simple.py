"""The Simple two-tower recipe (simple_two_tower.py) on the HIP path: SimpleTwoTower, the
symmetric InfoNCE, clip_grad_norm_ and AdamW, against fixtures made by running the
reference (tools/gen_simple_goldens.py: tests/golden/simple_tiny.npz, simple_tiny_b.npz).

Tolerances: run A (fp32) per-step losses and pre-clip norms rtol 1e-4, final weights
relative (max-abs over max) < 1e-3 per tensor, step-0 gradients 2e-3 relative
(test_gpu_margin.py's bounds); run B (bf16 towers on bf16-rounded weights and inputs) loss
2e-3 relative, per-tensor gradient cosine >= 0.998; SymmetricInfoNCELoss against float64
autograd at the fp32 kernel tolerance rtol 1e-4 / atol 1e-5; two gloo ranks against one
process at loss 1e-5 / gradients 1e-4 relative (test_gpu_dist.py's bounds)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from two_towers_amd import simple  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"


def rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def from_bits(a):
    return torch.from_numpy((a.astype(np.uint32) << 16).view(np.float32).copy())


def dropout_off(m):
    m.query_encoder.dropout = 0.0
    m.doc_encoder.dropout = 0.0
    m.query_proj[3].p = 0.0
    m.doc_proj[3].p = 0.0


def test_state_dict_keys_and_shapes_match_reference():
    z = np.load(os.path.join(GOLD, "simple_tiny.npz"))
    ref = {k[len("a.w0."):]: z[k].shape for k in z.files if k.startswith("a.w0.")}
    sd = tta.SimpleTwoTower(16, 16).state_dict()
    assert len(ref) == 44 and list(sd) == [k[len("a.w0."):] for k in z.files if k.startswith("a.w0.")]
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref


def test_simple_recipe_steps_match_reference():
    """simple_two_tower.py:233-240, 5 steps, dropout off: symmetric InfoNCE(0.1),
    clip_grad_norm_(1.0) (active at every step: the norms are 9.9-46), AdamW(1e-4, 0.01)."""
    z = np.load(os.path.join(GOLD, "simple_tiny.npz"))
    m = tta.SimpleTwoTower(16, 16)
    m.load_state_dict({k[len("a.w0."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("a.w0.")})
    m = m.to(DEV).train()
    dropout_off(m)
    bq, bd = torch.from_numpy(z["a.bq"]).to(DEV), torch.from_numpy(z["a.bd"]).to(DEV)
    opt = tta.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
    crit = simple.InfoNCELoss(temperature=0.1)
    losses, norms = [], []
    for s in range(5):
        opt.zero_grad()
        loss = crit(*m(bq[s % 2], bd[s % 2]))
        loss.backward()
        if s == 0:
            worst = {k: rel(p.grad, z["a.g0." + k]) for k, p in m.named_parameters()}
            print("step-0 gradient errors, worst", max(worst.values()))
            assert max(worst.values()) < 2e-3, worst
        norm = tta.clip_grad_norm_(m.parameters(), 1.0)
        assert norm.device.type == "cuda"
        opt.step()
        losses.append(float(loss.detach()))
        norms.append(float(norm))
    print("losses", losses, "reference", z["a.losses"].tolist())
    print("norms", norms, "reference", z["a.norms"].tolist())
    assert (z["a.norms"] > 1.0).all()
    np.testing.assert_allclose(losses, z["a.losses"], rtol=1e-4)
    np.testing.assert_allclose(norms, z["a.norms"], rtol=1e-4)
    sd = m.state_dict()
    worst = {k: rel(v, z["a.w5." + k]) for k, v in sd.items()}
    print("final weight errors, worst", max(worst.values()))
    assert max(worst.values()) < 1e-3, worst


def test_simple_bf16_towers_match_reference():
    z = np.load(os.path.join(GOLD, "simple_tiny_b.npz"))
    m = tta.SimpleTwoTower(32, 64)
    m.load_state_dict({k[len("b.w."):]: from_bits(z[k]) for k in z.files if k.startswith("b.w.")})
    m = m.to(DEV).train().set_compute_dtype(torch.bfloat16)
    dropout_off(m)
    qv, dv = m(from_bits(z["b.q"]).to(DEV), from_bits(z["b.d"]).to(DEV))
    assert qv.shape == (48, 32) and dv.shape == (48, 32)
    loss = simple.InfoNCELoss(temperature=0.1)(qv, dv)
    loss.backward()
    ref = float(z["b.loss"])
    print("loss", float(loss.detach()), "reference", ref)
    assert abs(float(loss.detach()) - ref) <= 2e-3 * abs(ref)
    cos = {}
    for k, p in m.named_parameters():
        g, r = p.grad.detach().cpu().double().reshape(-1), torch.from_numpy(z["b.g." + k].astype(np.float64)).reshape(-1)
        cos[k] = float((g * r).sum() / (g.norm() * r.norm()))
    print("gradient cosine, worst", min(cos.values()))
    assert min(cos.values()) >= 0.998, cos


def test_encode_matches_forward_and_eval_is_deterministic():
    torch.manual_seed(3)
    m = tta.SimpleTwoTower(16, 16).to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    q, d = torch.randn(9, 5, 16, generator=g).to(DEV), torch.randn(9, 5, 16, generator=g).to(DEV)
    with torch.no_grad():
        qv, dv = m(q, d)
        assert rel(m.encode_query(q), qv) < 1e-6 and rel(m.encode_doc(d), dv) < 1e-6
    torch.testing.assert_close(qv.norm(dim=1).cpu(), torch.ones(9), rtol=1e-5, atol=1e-5)


def _sym_ref(q, d, temperature, normalize):
    q = q.double().requires_grad_(True)
    d = d.double().requires_grad_(True)
    qn, dn = (torch.nn.functional.normalize(x, dim=1) for x in (q, d)) if normalize else (q, d)
    s = qn @ dn.t() / temperature
    i = torch.arange(s.shape[0], device=s.device)
    loss = 0.5 * ((torch.logsumexp(s, 1) - s[i, i]).mean() + (torch.logsumexp(s, 0) - s[i, i]).mean())
    loss.backward()
    return loss.detach(), q.grad, d.grad


@pytest.mark.parametrize("normalize", [False, True])
def test_symmetric_infonce_matches_float64_autograd(normalize):
    g = torch.Generator().manual_seed(9)
    q, d = torch.randn(150, 32, generator=g), torch.randn(150, 32, generator=g)
    if not normalize:  # the reference feeds normalised vectors
        q, d = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(d, dim=1)
    q1, d1 = q.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    loss = tta.SymmetricInfoNCELoss(temperature=0.1, normalize=normalize)(q1, d1)
    (3.0 * loss).backward()  # an upstream gradient other than 1
    rl, rq, rd = _sym_ref(q.to(DEV), d.to(DEV), 0.1, normalize)
    torch.testing.assert_close(loss.detach().double(), rl, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(q1.grad.double(), 3.0 * rq, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(d1.grad.double(), 3.0 * rd, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ two ranks over gloo
B, H = 64, 32  # rows per rank, vector width


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs():
    g = torch.Generator().manual_seed(8)
    return torch.randn(2 * B, H, generator=g), torch.randn(2 * B, H, generator=g)


def _rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q, d = _inputs()
        ql = q[rank * B:(rank + 1) * B].cuda().requires_grad_(True)
        dl = d[rank * B:(rank + 1) * B].cuda().requires_grad_(True)
        loss = tta.SymmetricInfoNCELoss(temperature=0.1, normalize=True)(ql, dl)
        loss.backward()
        out.put((rank, float(loss.detach()), ql.grad.cpu().numpy().copy(), dl.grad.cpu().numpy().copy()))
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks_match_single_process_fused():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = out.get(timeout=90)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    q, d = _inputs()
    q1, d1 = q.cuda().requires_grad_(True), d.cuda().requires_grad_(True)
    loss = tta.SymmetricInfoNCELoss(temperature=0.1, normalize=True)(q1, d1)
    loss.backward()
    ref_loss = float(loss.detach())
    for r in range(2):
        l, dq, dd = res[r]
        assert abs(l - ref_loss) <= 1e-5 * abs(ref_loss), (r, l, ref_loss)
        assert rel(dq, q1.grad[r * B:(r + 1) * B]) < 1e-4
        assert rel(dd, d1.grad[r * B:(r + 1) * B]) < 1e-4
