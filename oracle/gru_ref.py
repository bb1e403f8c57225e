"""Float64 restatement of ONE GRU recurrence, forward and backward -- TEST INFRASTRUCTURE ONLY.

Written from the formulas in include/tt_hip.h (tt_gru_fwd / tt_gru_bwd), not from the
kernels: plain torch on the CPU, no GPU code, nothing read from outside the repository.
tests/test_gru_ref.py pins it against torch.nn.GRU and torch.autograd;
tests/test_gpu_gru_ref.py compares the HIP kernels with it value by value.

Rounding emulation. `dt` is the storage type of the kernels' tensors (torch.bfloat16 or
torch.float32) or None for exact arithmetic. The kernels keep the recurrent state and every
gate in fp32 and round only what they store, so the reference rounds exactly the two stored
operands that feed a later step's matrix product (q() below) and nothing else:
  forward   gh_s   = q(h_{s-1}) @ W_hh^T          (the product reads the stored layer output)
  backward  prod_s = q(dar|daz|dhn)_{s+1} @ W_hh  (the product reads the stored gradients)
Inputs are expected already rounded to dt; outputs are returned unrounded (float64).
"""
from __future__ import annotations

import torch


def _q(x: torch.Tensor, dt):
    """Round to the storage type dt and come back to float64 (dt None: exact)."""
    return x if dt is None else x.to(dt).double()


def _times(T: int, reverse: bool):
    """Time index t of processed step s, for s = 0..T-1."""
    return [T - 1 - s for s in range(T)] if reverse else list(range(T))


def gru_fwd_ref(G, whh, bhn, B, T, H, reverse, dt):
    """One recurrence of tt_gru_fwd. G [B*T, 3H] (or [B, T, 3H]) gate pre-activations r|z|n
    with every input bias and the r|z hidden biases folded in, whh [3H, H], bhn [H].
    Returns Y [B, T, H] (h_t) and S [B, T, 4H] = ar | az | an | ghn (the saved state)."""
    G = G.double().reshape(B, T, 3 * H)
    whh = whh.double()
    bhn = bhn.double()
    h = G.new_zeros(B, H)
    Y = G.new_empty(B, T, H)
    S = G.new_empty(B, T, 4 * H)
    for t in _times(T, reverse):
        gh = _q(h, dt) @ whh.t()
        ar = G[:, t, :H] + gh[:, :H]
        az = G[:, t, H:2 * H] + gh[:, H:2 * H]
        ghn = gh[:, 2 * H:] + bhn
        an = G[:, t, 2 * H:] + torch.sigmoid(ar) * ghn
        z = torch.sigmoid(az)
        h = (1 - z) * torch.tanh(an) + z * h  # the state itself is never rounded
        Y[:, t] = h
        S[:, t] = torch.cat([ar, az, an, ghn], 1)
    return Y, S


def gru_bwd_ref(S, Y, dY, dF, whh, B, T, H, reverse, dt):
    """BPTT of one recurrence (tt_gru_bwd). S [B, T, 4H] and Y [B, T, H] as gru_fwd_ref
    returns them (rounded to dt by the caller when the kernels' stored copies are meant),
    dY [B, T, H] or None, dF [B, H] (gradient of the state after the last processed step) or
    None, whh [3H, H]. Returns dgx [B, T, 3H] = dar | daz | dan, dgh [B, T, H] = dhn, and the
    bias column sums [4H] = sum over (b, t) of dar | daz | dan | dhn."""
    S = S.double().reshape(B, T, 4 * H)
    Y = Y.double().reshape(B, T, H)
    whh = whh.double()
    dY = None if dY is None else dY.double().reshape(B, T, H)
    dF = None if dF is None else dF.double().reshape(B, H)
    ts = _times(T, reverse)
    dgx = S.new_zeros(B, T, 3 * H)
    dgh = S.new_zeros(B, T, H)
    prod = S.new_zeros(B, H)
    carry = S.new_zeros(B, H)
    for s in range(T - 1, -1, -1):
        t = ts[s]
        dh = prod + carry
        if dY is not None:
            dh = dh + dY[:, t]
        if dF is not None and s == T - 1:
            dh = dh + dF
        ar, az, an, ghn = S[:, t].split(H, dim=1)
        r, z, n = torch.sigmoid(ar), torch.sigmoid(az), torch.tanh(an)
        hp = Y[:, ts[s - 1]] if s > 0 else torch.zeros_like(dh)
        dan = dh * (1 - z) * (1 - n * n)
        dar = dan * ghn * r * (1 - r)
        daz = dh * (hp - n) * z * (1 - z)
        dhn = dan * r
        carry = dh * z
        prod = torch.cat([_q(dar, dt), _q(daz, dt), _q(dhn, dt)], 1) @ whh
        dgx[:, t] = torch.cat([dar, daz, dan], 1)
        dgh[:, t] = dhn
    dbias = torch.cat([dgx.sum((0, 1)), dgh.sum((0, 1))])
    return dgx, dgh, dbias


def row_err(got, ref):
    """Worst per-row error of got against ref, both [..., C] with the same shape:
        err[row] = max_j |got - ref| / max(max_j |ref[row, :]|, 1e-3 * max |ref|)
    so that one wrong row, or one wrong column group of one row, is measured against that
    row's own scale and not diluted by the rest of the tensor; the floor keeps an (almost)
    all-zero reference row from dividing by nothing. A NaN / inf in got counts as infinite.
    Returns (worst, index): index is the position (row indices..., j) of the worst element."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    diff = torch.nan_to_num((got - ref).abs(), nan=float("inf"), posinf=float("inf"))
    amax = ref.abs().amax(-1, keepdim=True)
    scale = torch.clamp(amax, min=max(1e-3 * float(ref.abs().max()), 1e-300))
    err = diff / scale
    k = int(err.reshape(-1).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), err.shape))
    return float(err.reshape(-1)[k]), idx


def vec_err(got, ref):
    """Error of a vector of sums (bias gradients) relative to its largest reference entry.
    Returns (worst, index)."""
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    diff = torch.nan_to_num((got - ref).abs(), nan=float("inf"), posinf=float("inf"))
    err = diff / max(float(ref.abs().max()), 1e-300)
    k = int(err.argmax())
    return float(err[k]), (k,)


def dropout_err(x1, y, mult):
    """The dropout copy x1 against y * mult, where mult holds 0 or 1/(1-p) per element
    (oracle.cpu_ref.dropout_mask). Returns (number of elements whose zero pattern differs,
    row_err of x1 against y * mult). An element of y that is itself zero cannot show its
    mask and is left out of the pattern count."""
    x1 = x1.detach().double().cpu()
    y = y.detach().double().cpu()
    mult = torch.as_tensor(mult).double().reshape(y.shape)
    shown = y != 0
    wrong = int((((x1 != 0) != (mult != 0)) & shown).sum())
    return wrong, row_err(x1, y * mult)
