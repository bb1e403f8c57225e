"""The float64 GRU reference (oracle/gru_ref.py) and its per-row checker, on the CPU.

1. gru_fwd_ref with dt = None against torch.nn.GRU in double, bidirectional, with the input
   biases and the r|z hidden biases folded into G the way two_towers_amd/towers.py folds them
   (the n hidden bias stays with the recurrence as bhn).
2. gru_bwd_ref with dt = None against torch.autograd through gru_fwd_ref: dY only, dF only and
   both, both directions, T = 1 and T = 4.
3. The checker (row_err / dropout_err) catches the faults a kernel can hide inside a
   whole-model gradient: each planted fault must read at least 10x the bf16 tolerance of
   tests/test_gpu_gru_ref.py, while the honest cost of bf16 storage (the rounding-emulating
   reference against the exact one, on the same cases) stays within a quarter of it.
   Measured here: planted faults 0.22 .. 2.3 per row; bf16 emulation against exact at most
   3.6e-3 (B 64, T 6, H 64 read 5.2e-3 in dgh with dF alone, so that case runs T = 4).
"""
import numpy as np
import pytest
import torch

from oracle.cpu_ref import dropout_mask
from oracle.gru_ref import dropout_err, gru_bwd_ref, gru_fwd_ref, row_err, vec_err

TOL_BF16 = 2e-2  # the per-row bound of tests/test_gpu_gru_ref.py
BF = torch.bfloat16


def _case(B, T, H, seed, dt=None):
    """Inputs as tests/test_gpu_gru_ref.py draws them, rounded to dt."""
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(B * T, 3 * H, generator=g, dtype=torch.float64)
    whh = torch.randn(3 * H, H, generator=g, dtype=torch.float64) * H ** -0.5
    bhn = torch.randn(H, generator=g, dtype=torch.float64) * 0.5
    dY = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    dF = torch.randn(B, H, generator=g, dtype=torch.float64)
    if dt is not None:
        G, whh, dY = (x.to(dt).double() for x in (G, whh, dY))
        bhn, dF = bhn.float().double(), dF.float().double()
    return G, whh, bhn, dY, dF


def test_forward_matches_torch_gru():
    B, T, E, H = 5, 4, 7, 16
    torch.manual_seed(3)
    gru = torch.nn.GRU(E, H, num_layers=1, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, T, E, dtype=torch.float64)
    with torch.no_grad():
        want, hn = gru(x)
        for d, sfx in enumerate(("", "_reverse")):
            wih, whh = getattr(gru, f"weight_ih_l0{sfx}"), getattr(gru, f"weight_hh_l0{sfx}")
            bih, bhh = getattr(gru, f"bias_ih_l0{sfx}"), getattr(gru, f"bias_hh_l0{sfx}")
            fold = bih + torch.cat([bhh[:2 * H], torch.zeros(H, dtype=torch.float64)])
            G = (x @ wih.t() + fold).reshape(B * T, 3 * H)
            Y, S = gru_fwd_ref(G, whh, bhh[2 * H:], B, T, H, bool(d), None)
            assert float((Y - want[:, :, d * H:(d + 1) * H]).abs().max()) < 1e-13
            assert float((Y[:, 0 if d else T - 1] - hn[d]).abs().max()) < 1e-13
            assert S.shape == (B, T, 4 * H) and bool(torch.isfinite(S).all())


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("mode", ["dy", "dfinal", "both"])
def test_backward_matches_autograd(mode, reverse, T):
    B, H = 6, 16
    G, whh, bhn, dY, dF = _case(B, T, H, 11 + T + int(reverse))
    dY = dY if mode in ("dy", "both") else None
    dF = dF if mode in ("dfinal", "both") else None
    G, whh, bhn = (x.clone().requires_grad_(True) for x in (G, whh, bhn))
    Y, S = gru_fwd_ref(G, whh, bhn, B, T, H, reverse, None)
    # dL/dgh of autograd: a zero leaf added to gh_n inside S would need a hook; the sums
    # over (b, t) of dar | daz | dan are dL/dG's column sums and the sum of dhn is dL/dbhn
    loss = 0.0
    if dY is not None:
        loss = loss + (Y * dY).sum()
    if dF is not None:
        loss = loss + (Y[:, 0 if reverse else T - 1] * dF).sum()
    gG, gW, gb = torch.autograd.grad(loss, (G, whh, bhn))
    dgx, dgh, dbias = gru_bwd_ref(S.detach(), Y.detach(), dY, dF, whh.detach(), B, T, H, reverse, None)
    assert float((dgx - gG.reshape(B, T, 3 * H)).abs().max()) < 1e-13
    assert float((dbias[:3 * H] - gG.sum(0)).abs().max()) < 1e-12
    assert float((dbias[3 * H:] - gb).abs().max()) < 1e-12
    # dW_hh = sum_s [dar | daz | dhn]_s^T h_{s-1}: pins dgh element by element
    Yd = Y.detach()
    ts = [T - 1 - s for s in range(T)] if reverse else list(range(T))
    dW = torch.zeros_like(gW)
    for s in range(1, T):
        dghs = torch.cat([dgx[:, ts[s], :2 * H], dgh[:, ts[s]]], 1)
        dW += dghs.t() @ Yd[:, ts[s - 1]]
    assert float((dW - gW).abs().max()) < 1e-12


CASES = [(64, 4, 64, False), (64, 6, 512, True), (9, 1, 72, False)]


def _chain(B, T, H, reverse, dt, dY, dF, G, whh, bhn):
    """Forward, then the backward on the forward's outputs as the kernels store them."""
    Y, S = gru_fwd_ref(G, whh, bhn, B, T, H, reverse, dt)
    Ys, Ss = (Y, S) if dt is None else (Y.to(dt).double(), S.to(dt).double())
    dgx, dgh, dbias = gru_bwd_ref(Ss, Ys, dY, dF, whh, B, T, H, reverse, dt)
    return Y, S, dgx, dgh, dbias


@pytest.mark.parametrize("B,T,H,reverse", CASES)
def test_checker_catches_planted_faults(B, T, H, reverse):
    G, whh, bhn, dY, dF = _case(B, T, H, 5 * H + T, BF)
    Y, S, dgx, dgh, dbias = _chain(B, T, H, reverse, BF, dY, dF, G, whh, bhn)
    Ss, Ys = S.to(BF).double(), Y.to(BF).double()
    need = 10 * TOL_BF16
    b, t = B - 1, T - 1
    seen = []
    # one (b, t) row replaced by its neighbour (the previous batch row, same step)
    for name, ref in (("Y", Y), ("dan", dgx[:, :, 2 * H:]), ("dhn", dgh)):
        bad = ref.clone()
        bad[b, t] = ref[b - 1, t]
        e, idx = row_err(bad, ref)
        seen.append(e)
        assert e >= need and idx[:2] == (b, t), (name, e, idx)
    # one 8-column group of one row zeroed
    for name, ref in (("Y", Y), ("ar", S[:, :, :H]), ("dan", dgx[:, :, 2 * H:]), ("dar", dgx[:, :, :H])):
        bad = ref.clone()
        bad[b, t, 16:24] = 0
        e, idx = row_err(bad, ref)
        seen.append(e)
        assert e >= need and idx[:2] == (b, t) and 16 <= idx[2] < 24, (name, e, idx)
    # dF left out for the last batch row, dY present
    dF0 = dF.clone()
    dF0[b] = 0
    bgx, bgh, _ = gru_bwd_ref(Ss, Ys, dY, dF0, whh, B, T, H, reverse, BF)
    for name, bad, ref in (("dan", bgx[:, :, 2 * H:], dgx[:, :, 2 * H:]), ("dhn", bgh, dgh)):
        e, idx = row_err(bad, ref)
        seen.append(e)
        assert e >= need and idx[0] == b, (name, e, idx)
    # the dropout multiplier of one element flipped, a kept one and a dropped one
    p = 0.1
    mult = torch.from_numpy(dropout_mask(77, B * T, 2 * H, p, row0=3)[:, H:].astype(np.float64)).reshape(B, T, H)
    x1 = Y * mult
    assert dropout_err(x1, Y, mult)[0] == 0
    row = mult[b, t]
    for j in (int((row != 0).nonzero()[0]), int((row == 0).nonzero()[0])):
        bad_mult = mult.clone()
        bad_mult[b, t, j] = 0.0 if row[j] != 0 else 1.0 / (1.0 - p)
        wrong, _ = dropout_err(Y * bad_mult, Y, mult)
        assert wrong == 1, (j, wrong)  # the exact zero pattern catches it whatever its size
    j = int((Y[b, t].abs() * (row != 0)).argmax())  # a kept element that the row's scale shows
    bad_mult = mult.clone()
    bad_mult[b, t, j] = 0.0
    e, idx = dropout_err(Y * bad_mult, Y, mult)[1]
    seen.append(e)
    assert e >= need and idx == (b, t, j), (e, idx)
    print(f"planted faults B {B} T {T} H {H}: per-row error {min(seen):.3g} .. {max(seen):.3g}")


@pytest.mark.parametrize("B,T,H,reverse", CASES)
def test_bf16_emulation_stays_within_a_quarter_of_the_tolerance(B, T, H, reverse):
    """What bf16 storage of the recurrent operands costs: the rounding-emulating reference
    against the exact one on the same (bf16-rounded) inputs."""
    G, whh, bhn, dY, dF = _case(B, T, H, 5 * H + T, BF)
    Y, S, _, _, _ = _chain(B, T, H, reverse, BF, dY, dF, G, whh, bhn)
    Ye, Se, _, _, _ = _chain(B, T, H, reverse, None, dY, dF, G, whh, bhn)
    worst = {"Y": row_err(Y, Ye)[0]}
    for k, name in enumerate(("ar", "az", "an", "ghn")):
        worst[name] = row_err(S[:, :, k * H:(k + 1) * H], Se[:, :, k * H:(k + 1) * H])[0]
    # the backward on one and the same stored S, Y: the cost of rounding its own operands
    Ss, Ys = S.to(BF).double(), Y.to(BF).double()
    for mode, a, f in (("dy", dY, None), ("dfinal", None, dF), ("both", dY, dF)):
        dgx, dgh, db = gru_bwd_ref(Ss, Ys, a, f, whh, B, T, H, reverse, BF)
        egx, egh, eb = gru_bwd_ref(Ss, Ys, a, f, whh, B, T, H, reverse, None)
        worst[f"dgx/{mode}"] = row_err(dgx, egx)[0]
        worst[f"dgh/{mode}"] = row_err(dgh, egh)[0]
        worst[f"dbias/{mode}"] = vec_err(db, eb)[0]
    print(f"bf16 emulation against exact, B {B} T {T} H {H}: " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL_BF16 / 4, (k, v)
