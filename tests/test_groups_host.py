"""Group masks, host side: pretok.pair_groups, the pair store's groups round trip, and the
yardstick of the GPU tests shown to bite.

The GPU tests (test_gpu_groups_ref.py) compare the grouped kernels with the masked float64
reference of tests/groups_cases.py through oracle/loss_ref.py's comparison functions. Here the
UNMASKED float64 reference, which is what a kernel that ignored the ids would compute, is put
through the same comparisons against the masked one, on the same cases, and must fail each of
them: otherwise those tests would pass without the feature.
"""
import json
import os

import numpy as np
import pytest
import torch

import groups_cases as G
from oracle import loss_ref as L
from oracle.loss_ref import BF16, F32, INV_TAU
from two_towers_amd.data import Vocab
from two_towers_amd.pretok import PairIds, pair_groups, pretokenize


def _fails(what, errs):
    with pytest.raises(AssertionError):
        L.check(what, errs)


# --------------------------------------------------------------------------- pair_groups
def test_pair_groups_hand_built():
    """pairs 0, 1: a duplicate query; 2, 3: a duplicate document; 4, 5, 6: the chain q1-d1,
    q1-d2, q3-d2; 7, 8: singletons. Ids are dense and numbered by first appearance."""
    q = np.array([[1, 2], [1, 2], [3, 0], [4, 0], [5, 5], [5, 5], [6, 6], [7, 0], [8, 0]], dtype=np.int32)
    d = np.array([[10, 0], [11, 0], [12, 1], [12, 1], [13, 0], [14, 0], [14, 0], [15, 0], [16, 0]], dtype=np.int32)
    g, m = pair_groups(q, d)
    assert g.dtype == np.int32 and g.tolist() == [0, 0, 1, 1, 2, 2, 2, 3, 4]
    assert m == 3


def test_pair_groups_edges():
    g, m = pair_groups(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
    assert g.shape == (0,) and m == 0
    g, m = pair_groups(np.array([[1], [2], [3]]), np.array([[4], [5], [6]]))
    assert g.tolist() == [0, 1, 2] and m == 1
    # a chain that closes late: 0-2 by query, 1-3 by query, 2-3 by document -> one group of 4
    g, m = pair_groups(np.array([[1], [2], [1], [2]]), np.array([[7], [8], [9], [9]]))
    assert g.tolist() == [0, 0, 0, 0] and m == 4
    with pytest.raises(ValueError):
        pair_groups(np.zeros((2, 1)), np.zeros((3, 1)))


# ---------------------------------------------------------------------------- pair store
def _vocab():
    words = ["alpha", "beta", "gamma", "delta", "epsilon"]
    return Vocab(words, np.zeros((len(words), 4), np.float32))


def test_pretokenize_groups_round_trip(tmp_path):
    qs = ["alpha beta", "alpha beta", "gamma", "delta", "epsilon alpha"]
    ds = ["beta", "gamma delta", "epsilon", "epsilon", "alpha"]
    v = _vocab()
    out = str(tmp_path / "ids")
    meta = pretokenize(qs, ds, v, out, max_length=4, workers=1, groups=True)
    assert meta["max_group_size"] == 2
    with open(os.path.join(out, "meta.json")) as f:
        assert json.load(f)["max_group_size"] == 2
    store = PairIds(out, v, mmap=False)
    assert store.max_group_size == 2 and store.groups.tolist() == [0, 0, 1, 1, 2]
    got = list(store.batches(2, device="cpu", shuffle=False, drop_last=False, with_groups=True))
    assert [len(b) for b in got] == [3, 3, 3]
    assert torch.cat([b[2] for b in got]).tolist() == [0, 0, 1, 1, 2] and got[0][2].dtype == torch.int32
    for (q, d, g), (q2, d2) in zip(got, store.batches(2, device="cpu", shuffle=False, drop_last=False)):
        assert torch.equal(q, q2) and torch.equal(d, d2)
    # shuffled: the ids travel with their pairs
    for q, d, g in store.batches(2, device="cpu", shuffle=True, seed=3, with_groups=True):
        for r in range(q.shape[0]):
            i = next(i for i in range(5) if np.array_equal(store.q[i], q[r].numpy()) and np.array_equal(store.d[i], d[r].numpy()))
            assert int(g[r]) == int(store.groups[i])


def test_store_without_groups_still_loads(tmp_path):
    v = _vocab()
    out = str(tmp_path / "ids")
    meta = pretokenize(["alpha", "beta"], ["gamma", "delta"], v, out, max_length=3, workers=1)
    assert "max_group_size" not in meta and not os.path.exists(os.path.join(out, "groups.npy"))
    store = PairIds(out, v)
    assert store.groups is None and store.max_group_size is None
    assert all(len(b) == 2 for b in store.batches(2, device="cpu", shuffle=False))
    with pytest.raises(ValueError, match="groups"):
        next(store.batches(2, device="cpu", with_groups=True))


# ------------------------------------------------------------------ the yardstick bites
@pytest.mark.parametrize("name,dt", [(n, dt) for n, c in G.FWD_CASES.items() for dt in c[2]])
def test_unmasked_reference_fails_forward_comparison(name, dt):
    q, d, rg, cg, per_tau = G.fwd_case(name, dt)
    assert bool(G.excluded(q.shape[0], d.shape[0], G.FWD_CASES[name][3], rg, cg).any())
    for inv_tau, (lse, row, ulse, urow, smax) in per_tau.items():
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(row).all())
        errs = L.infonce_fwd_errs(ulse.float(), urow.float(), lse, row, dt, smax)
        print(f"{name} {dt} inv_tau {inv_tau:.3g}: ignoring the ids moves lse by {errs[0][1]:.3g} x its bound")
        _fails(f"{name} unmasked", errs)
        # and the masked reference passes against itself rounded to fp32
        L.check(f"{name} masked", L.infonce_fwd_errs(lse.float(), row.float(), lse, row, dt, smax))


def test_all_but_label_excluded_reference_is_the_label_score():
    for dt in (F32, BF16):
        q, d, rg, cg, per_tau = G.fwd_case("all_but_label_excluded", dt)
        for inv_tau, (lse, row, _, _, _) in per_tau.items():
            s = L.infonce_scores(q, d, inv_tau, 0.0, 128)
            assert float((lse - s[0, 128]).abs()) == 0.0 and float(row.abs()) == 0.0


@pytest.mark.parametrize("dt,bq,nd,h,lab0,offdiag,pattern", [(*c[:6], c[7]) for c in G.BWD_CASES])
def test_unmasked_reference_fails_backward_comparison(dt, bq, nd, h, lab0, offdiag, pattern):
    q, d, rg, cg, g, lse, rq, rd, bounds, uq, ud = G.bwd_case(dt, bq, nd, h, lab0, offdiag, pattern)
    errs = L.infonce_bwd_errs(uq.float(), ud.float(), rq, rd, dt, bounds)
    print(f"{dt} {bq} x {nd} x {h}: " + ", ".join(f"{n} {e:.3g} (bound {b:.3g})" for n, e, _, b in errs))
    _fails("unmasked backward", errs)
    L.check("masked backward", L.infonce_bwd_errs(rq.float(), rd.float(), rq, rd, dt, bounds))


@pytest.mark.parametrize("dt,n,h", [c[:3] for c in G.SYM_CASES])
def test_unmasked_reference_fails_symmetric_comparison(dt, n, h):
    q, d, grp, g, (lr, lc, row, rq, rd), bounds, (ulr, ulc, urow, uq, ud) = G.sym_case(dt, n, h)
    _fails("unmasked lse_row", L.infonce_fwd_errs(ulr.float(), urow.float(), lr, row, dt))
    _fails("unmasked lse_col", L.infonce_fwd_errs(ulc.float(), urow.float(), lc, row, dt))
    _fails("unmasked sym backward", L.infonce_bwd_errs(uq.float(), ud.float(), rq, rd, dt, bounds))
    L.check("masked sym", L.infonce_fwd_errs(lr.float(), row.float(), lr, row, dt)
            + L.infonce_fwd_errs(lc.float(), row.float(), lc, row, dt)
            + L.infonce_bwd_errs(rq.float(), rd.float(), rq, rd, dt, bounds))
