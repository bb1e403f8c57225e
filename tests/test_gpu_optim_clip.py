"""The optimiser side of the Simple recipe (simple_two_tower.py:193, :239): tt_grad_norm_multi /
tt_clip_scale_multi behind optim.clip_grad_norm_, and tt_adamw_multi behind optim.AdamW.

Tolerances. Sum of squares: relative 1e-5 against float64 (an fp32 tree sum over chunks of
at most 4096 elements is bounded near 2e-6). Clipped gradients: rtol 1e-5 against torch's
clip_grad_norm_ on CPU copies; below max_norm the coefficient is exactly 1 and the
gradients must not change by a bit. AdamW: test_adam_matches_torch's rtol 1e-5 / atol 1e-6
against torch.optim.AdamW(foreach=False); Adam with the same weight_decay (L2, coupled)
must land more than 100x that tolerance away, or the decay is not decoupled."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import call  # noqa: E402
from two_towers_amd.optim import Adam, AdamW, clip_grad_norm_  # noqa: E402

DEV = "cuda"
SIZES = [1, 3, 4095, 4096, 0, 4097, 100003]  # chunk edges, an empty tensor, many chunks


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in SIZES]


def _sumsq(ts, accumulate, sumsq):
    lib = _lib.load()
    n = len(ts)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    sizes = (ctypes.c_long * n)(*[t.numel() for t in ts])
    ws = torch.full((lib.tt_grad_norm_ws_size(sizes, n),), 0xFF, dtype=torch.uint8, device=DEV)
    call("tt_grad_norm_multi", ptrs, sizes, n, accumulate, sumsq.data_ptr(), ws.data_ptr(),
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def test_grad_norm_multi_matches_float64():
    a, b = _tensors(1), _tensors(2)
    ad, bd = [t.to(DEV) for t in a], [t.to(DEV) for t in b]
    ra = sum(float((t.double() ** 2).sum()) for t in a)
    rb = sum(float((t.double() ** 2).sum()) for t in b)
    s = torch.full((1,), float("nan"), device=DEV)
    _sumsq(ad, 0, s)
    one = float(s)
    print("one call rel err", abs(one - ra) / ra)
    assert abs(one - ra) <= 1e-5 * ra
    _sumsq(bd, 1, s)  # chained: the second call adds to the first
    two = float(s)
    print("chained rel err", abs(two - (ra + rb)) / (ra + rb))
    assert abs(two - (ra + rb)) <= 1e-5 * (ra + rb)
    s2 = torch.full((1,), float("nan"), device=DEV)
    _sumsq(ad, 0, s2)
    assert float(s2) == one  # deterministic
    _sumsq([], 0, s2)  # nothing to sum: zero, not the previous value
    assert float(s2) == 0.0


def _params(scale):
    g = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (300,), (4097,), (3, 3, 3), (0,), (130, 33)]
    grads = [torch.randn(s, generator=g) * scale for s in shapes]
    cpu, gpu = [], []
    for gr in grads:
        p = torch.zeros_like(gr).requires_grad_(True)
        p.grad = gr.clone()
        cpu.append(p)
        q = torch.zeros_like(gr, device=DEV).requires_grad_(True)
        q.grad = gr.clone().to(DEV)
        gpu.append(q)
    return cpu, gpu


def test_clip_grad_norm_above_max_norm_matches_torch():
    cpu, gpu = _params(1.0)
    ref = torch.nn.utils.clip_grad_norm_(cpu, 1.0)
    got = clip_grad_norm_(gpu, 1.0)
    assert isinstance(got, torch.Tensor) and got.device.type == "cuda" and got.dim() == 0
    assert float(ref) > 1.0
    torch.testing.assert_close(got.cpu(), ref, rtol=1e-5, atol=0.0)
    for a, b in zip(cpu, gpu):
        torch.testing.assert_close(b.grad.cpu(), a.grad, rtol=1e-5, atol=0.0)


def test_clip_grad_norm_below_max_norm_leaves_the_bits():
    cpu, gpu = _params(1e-3)
    before = [q.grad.clone() for q in gpu]
    ref = torch.nn.utils.clip_grad_norm_(cpu, 1.0)
    got = clip_grad_norm_(gpu, 1.0)
    assert float(ref) < 1.0 and got.device.type == "cuda"
    torch.testing.assert_close(got.cpu(), ref, rtol=1e-5, atol=0.0)
    for q, b in zip(gpu, before):
        assert torch.equal(q.grad, b)


def test_clip_grad_norm_rejects_other_gradients():
    p = torch.zeros(4, 6, device=DEV, requires_grad=True)
    p.grad = torch.ones(6, 4, device=DEV).t()  # not contiguous
    with pytest.raises(_lib.TTError):
        clip_grad_norm_([p], 1.0)
    p.grad = None
    h = torch.zeros(4, device=DEV, dtype=torch.float16, requires_grad=True)
    h.grad = torch.ones(4, device=DEV, dtype=torch.float16)
    with pytest.raises(_lib.TTError):
        clip_grad_norm_([h], 1.0)


def test_adamw_matches_torch_and_differs_from_adam():
    torch.manual_seed(0)
    ps = [torch.randn(s) for s in [(7, 5), (300,), (4097,), (3, 3, 3)]]
    gs = [[torch.randn_like(p) for p in ps] for _ in range(3)]
    ref = [p.clone().requires_grad_(True) for p in ps]
    mine = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    coupled = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    o1 = torch.optim.AdamW(ref, lr=1e-2, weight_decay=0.1, foreach=False)
    o2 = AdamW(mine, lr=1e-2, weight_decay=0.1)
    o3 = Adam(coupled, lr=1e-2, weight_decay=0.1)
    for step in range(3):
        for group in (ref, mine, coupled):
            for p, g in zip(group, gs[step]):
                p.grad = g.clone().to(p.device)
        o1.step()
        o2.step()
        o3.step()
    rtol, atol = 1e-5, 1e-6
    for a, b, c in zip(ref, mine, coupled):
        a, b, c = a.detach(), b.detach().cpu(), c.detach().cpu()
        assert torch.allclose(a, b, rtol=rtol, atol=atol), float((a - b).abs().max())
        gap = float(((c - a).abs() / (atol + rtol * a.abs())).max())
        print("Adam(L2) vs AdamW gap in tolerances:", gap)
        assert gap > 100.0
    d = AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)
