"""The no-grad encode path (towers.towers_infer: tt_gru_fwd_infer, no saved pre-activations,
no layer-1 output, no autograd state) against the training forward the same model runs with
grad enabled in eval mode (dropout 0): same kernels' arithmetic, so the outputs are
bit-identical, and the inference path must not hold the saved state in memory.

Reference behaviour: EnhancedTwoTowerModel.forward / encode (enhanced_two_tower.py:50-65)
and TwoTowerModel (margin_two_tower.py:59-61) under torch.no_grad().
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import two_towers_amd as tta  # noqa: E402
from two_towers_amd import margin, towers  # noqa: E402
from two_towers_amd._lib import option  # noqa: E402

DEV = "cuda"
E, HID, B, T, V = 300, 128, 256, 32, 500  # GRU hidden H = 2 * HID = 256


def _model(dt, seed=0):
    torch.manual_seed(seed)
    m = tta.EnhancedTwoTowerModel(E, HID).to(DEV).set_compute_dtype(dt)
    g = torch.Generator().manual_seed(seed + 1)
    m.set_embedding_table(torch.randn(V, E, generator=g).to(DEV))
    return m


def _ids(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, V, (B, T), generator=g).to(DEV), torch.randint(0, V, (B, T), generator=g).to(DEV))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_no_grad_encode_is_bit_identical_to_eval_forward(dt, monkeypatch):
    m = _model(dt).eval()
    q, d = _ids(3)
    used = []
    real = towers.towers_infer
    monkeypatch.setattr(towers, "towers_infer", lambda *a, **k: (used.append(1), real(*a, **k))[1])
    # grad enabled, eval mode: the training forward (TowersFn) with dropout 0
    rq, rd = m(q, d)
    eq, ed = m.encode_query(q), m.encode_doc(d)
    assert not used and rq.requires_grad and eq.requires_grad
    with torch.no_grad():
        iq, idd = m(q, d)
        jq, jd = m.encode_query(q), m.encode_doc(d)
    assert len(used) == 3 and not iq.requires_grad
    tta.check_gru_status()
    for name, a, b in (("q", iq, rq), ("d", idd, rd), ("encode_query", jq, eq), ("encode_doc", jd, ed)):
        ne = int((a.view(torch.int32) != b.detach().view(torch.int32)).sum().item())
        print(f"{dt} {name}: {ne} of {a.numel()} values differ")
        assert ne == 0, name
    assert torch.isfinite(iq).all() and float(iq.abs().max()) > 0


def test_margin_model_no_grad_is_bit_identical():
    """margin.TwoTowerModel (head "none": the towers return cat(h_fwd, h_rev)), H 64, B 48, T 6."""
    torch.manual_seed(2)
    m = margin.TwoTowerModel(40, 64).to(DEV).set_compute_dtype(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(4)
    q = torch.randn(48, 6, 40, generator=g).to(DEV)
    d = torch.randn(48, 6, 40, generator=g).to(DEV)
    ref = m(q, d)
    rq = m.encode_query(q)
    with torch.no_grad():
        out = m(q, d)
        oq = m.encode_query(q)
    assert not out.requires_grad
    assert torch.equal(out, ref.detach()) and torch.equal(oq, rq.detach())


def test_train_step_after_no_grad_encode_is_unchanged():
    """The packed-weight cache and the step guard of the inference path do not leak into
    training: a train-mode step (dropout drawn from the same seed) after a no-grad eval
    encode gives the gradients of the same step without that encode, bit for bit (the
    training step is deterministic, tests/test_gpu_model.py). Option gru_fwd_xc = 2 puts
    both paths on the column-split kernels, so each watches a workspace status word."""
    q, d = _ids(7)
    grads = []
    dev = torch.device("cuda", torch.cuda.current_device())
    for encode_first in (False, True):
        m = _model(torch.bfloat16, seed=11)
        with option("gru_fwd_xc", 2):
            if encode_first:
                m.eval()
                with torch.no_grad():
                    m(q, d)
                    m.encode_query(q)
            m.train()
            torch.manual_seed(6)
            qv, dv = m(q, d)
            tta.InfoNCELoss(compute_dtype=torch.bfloat16)(qv, dv).backward()
        tta.check_gru_status()
        assert int(towers.step_guard(dev).item()) == 0
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
    assert len(grads[0]) == 44
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
        assert float(grads[0][k].abs().max()) > 0, k


def test_no_grad_encode_allocates_no_saved_state():
    """Peak memory above the resident set of one call, after a warm-up call of each kind. The
    eval forward with grad enabled keeps S ([B*T, 4H] per direction, layer and tower) for a
    backward; the no-grad encode must stay below it by at least one layer's S of one tower,
    both directions: 2 * B*T * 4H * 2 bytes (bf16). Only a path that never allocates S can."""
    H = 2 * HID
    floor = 2 * B * T * 4 * H * 2
    m = _model(torch.bfloat16).eval()
    q, d = _ids(5)

    def peak(no_grad):
        with torch.set_grad_enabled(not no_grad):
            out = m(q, d)  # warm-up: packed weights, table, workspace sizes
            del out
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = m(q, d)
            torch.cuda.synchronize()
            top = torch.cuda.max_memory_allocated()
            del out
        return top - base

    train_fwd = peak(False)
    infer = peak(True)
    print(f"peak above resident: eval forward with grad {train_fwd} B, no-grad encode {infer} B, "
          f"gap {train_fwd - infer} B, floor {floor} B")
    assert train_fwd - infer >= floor
