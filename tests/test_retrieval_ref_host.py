"""oracle/retrieval_ref.py on the CPU: each float64 reference pinned against a plain Python
loop at tiny sizes; each comparison shown to reject one planted defect applied to the
reference's own output on the exact input family; and tt_scan_geometry (host code, nothing is
launched) against the geometry every case of tests/test_gpu_scan_ref.py was written for.

Defects at (bq 40, nd 300, h 32, tps 2, label offset 248, k 5), elements that differ from the
reference out of the compared ones (test_comparisons_accept_the_reference_and_reject_planted_
defects prints them with -s):
  chunk maxima without each split's last tile   120 of 200 maxima, and 165 of 200 top-k columns
  a tie given to the higher column              160 of 200 top-k columns (h 32: many natural ties)
  label unmasked where its block spans 2 tiles  14 of 200 top-k columns, 3 of 200 chunk maxima
  padded zero columns counted (theta < 0)       13 of 40 counts, each by the 20 padded columns
  s >= theta above the threshold column         38 of 40 counts
The weakest is the unmasked label seen through the chunk maxima: 3 entries. Only the four
positives of the spanning block that are copies of their query can be a chunk's maximum (one of
them shares its chunk with another copy of the same query, which ties with it); the other
positives are random documents and almost never are. That is why the family plants such
positives, and why the GPU suite compares the top-k as well as every chunk maximum."""
import ctypes

import pytest
import torch

from oracle import retrieval_ref as R
from two_towers_amd import _lib


# ---------------------------------------------------------------- references against plain loops
def _tiny(seed=0, bq=5, nd=150, h=16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (bq, h), generator=g).float(), torch.randint(-2, 3, (nd, h), generator=g).float()


def _loop_scores(q, d, lab):
    s = [[sum(float(a) * float(b) for a, b in zip(qr, dr)) for dr in d.tolist()] for qr in q.tolist()]
    if lab >= 0:
        for i in range(len(s)):
            s[i][lab + i] = -1.0
    return s


@pytest.mark.parametrize("lab", [-1, 0, 60, 145])
def test_scores_order_and_chunk_maxima_against_loops(lab):
    q, d = _tiny(lab + 2)
    s = _loop_scores(q, d, lab)
    ref = R.scores64(q, d, lab)
    assert ref.dtype == torch.float64 and ref.tolist() == s
    idx, val = R.order_ref(ref, 7, block=2)
    for i, row in enumerate(s):
        order = sorted(range(len(row)), key=lambda j: (-row[j], j))[:7]
        assert idx[i].tolist() == order and val[i].tolist() == [row[j] for j in order]
    assert any(val[i, a] == val[i, a + 1] for i in range(5) for a in range(6))  # ties are exercised
    cm = R.chunk_max_ref(ref)
    assert cm.shape == (5, 3)
    for i, row in enumerate(s):
        assert cm[i].tolist() == [max(row[c:c + 64]) for c in (0, 64, 128)]  # 128..149: the tail excluded


def test_rank_rule_against_loops():
    q, d = _tiny(9, bq=6)
    d[100] = d[7]
    d[149] = d[7]
    s = _loop_scores(q, d, -1)
    relevant = [{7, 100, 149}, set(), {100, 3}, {149}, {0}, {20, 21, 22, 148}]
    ptr, idx = R.csr(relevant)
    assert ptr.tolist() == [0, 3, 3, 5, 6, 7, 11] and idx.tolist() == [7, 100, 149, 3, 100, 149, 0, 20, 21, 22, 148]
    ref = R.scores64(q, d)
    theta, tcol = R.best_relevant_ref(ref, ptr, idx)
    for i, rel in enumerate(relevant):
        if not rel:
            assert (float(theta[i]), int(tcol[i])) == (0.0, -1)
            continue
        best = max(s[i][j] for j in rel)
        col = min(j for j in rel if s[i][j] == best)
        assert (float(theta[i]), int(tcol[i])) == (best, col)
    assert int(tcol[0]) == 7 and int(tcol[3]) == 149
    for off, lo, hi in ((0, 0, 150), (0, 0, 70), (70, 70, 150)):
        cnt = R.count_ref(ref[:, lo:hi], theta, tcol, off)
        for i in range(6):
            t, c = float(theta[i]), int(tcol[i])
            want = 0 if c < 0 else sum(1 for j in range(lo, hi) if s[i][j] > t or (s[i][j] == t and j < c))
            assert int(cnt[i]) == want
    whole = R.count_ref(ref, theta, tcol)
    assert torch.equal(whole, R.count_ref(ref[:, :70], theta, tcol) + R.count_ref(ref[:, 70:], theta, tcol, 70))
    assert int(whole[3]) >= 2  # columns 7 and 100 tie with 149 from below


def test_eps_is_the_fp32_accumulation_bound():
    assert R.gamma(256) == 256 * 2.0 ** -24 / (1 - 256 * 2.0 ** -24)
    q, d = _tiny(1)
    e = R.eps_elem(q, d)
    a = sum(abs(float(x) * float(y)) for x, y in zip(q[2].tolist(), d[17].tolist()))
    assert float(e[2, 17]) == pytest.approx(R.gamma(16) * a, rel=1e-15)
    # an fp32 sum of the products in any order stays inside it
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 256, generator=g).bfloat16().float()
    y = torch.randn(64, 256, generator=g).bfloat16().float()
    ref = (x.double() * y.double()).sum(1)
    for perm in (torch.arange(256), torch.arange(255, -1, -1), torch.randperm(256, generator=g)):
        acc = torch.zeros(64)
        for k in perm.tolist():
            acc = acc + x[:, k] * y[:, k]
        assert bool(((acc.double() - ref).abs() <= R.gamma(256) * (x.double() * y.double()).abs().sum(1)).all())


# ---------------------------------------------------------------- the exact family and the defects
BQ, ND, H, TPS, LAB, K = 40, 300, 32, 2, 248, 5


def test_exact_family_is_exact_and_holds_what_it_promises():
    inp = R.exact_inputs(BQ, ND, H, TPS, LAB)
    for t in (inp.q, inp.d):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3
        assert torch.equal(t, t.bfloat16().float())
    assert bool((inp.q[:, :R.POS8] == 3).all())
    s = R.scores64(inp.q, inp.d)
    for kind, cols in inp.typed.items():
        assert len(cols) >= 3 and bool((s[:, cols] == R.TYPE_SCORE[kind]).all())
    # thresholds: every in-tile position, the three signs, duplicates on both sides, empty rows
    live = [(r, c) for r, c in enumerate(inp.tcol) if c >= 0]
    assert {c % 64 for _, c in live} == set(R.TCOL_POS)
    assert {inp.planted[c] for _, c in live} == {"neg", "zero", "pos"}
    assert any(c >= (ND // 64) * 64 for _, c in live)                      # one in the partial tile
    for r, c in live:
        same = inp.typed[inp.planted[c]]
        assert c < max(same) and (min(same) < c or c == 0)
    assert inp.tcol.count(-1) == 2 and all(not inp.relevant[r] for r in (15, 31))
    ptr, idx = R.csr(inp.relevant)
    theta, tcol = R.best_relevant_ref(s, ptr, idx)
    assert tcol.tolist() == inp.tcol
    assert {float(t) for t, c in zip(theta, inp.tcol) if c >= 0} == {-72.0, 0.0, 72.0}
    # featured rows: their copies lead the row's order, lowest column first
    ms = R.scores64(inp.q, inp.d, LAB)
    order, _ = R.order_ref(ms, 16)
    assert len(inp.featured) >= 16
    for r, cols in inp.featured.items():
        cols = [c for c in cols if c != LAB + r]  # its own positive reads -1
        assert len(cols) >= 1 and order[r, :len(cols)].tolist() == cols
    # a quarter of the positives would be the row's best score if left unmasked
    for r in range(1, BQ, 4):
        assert float(s[r, LAB + r]) == float(s[r].max()) and float(ms[r, LAB + r]) == -1.0
    # deterministic
    again = R.exact_inputs(BQ, ND, H, TPS, LAB)
    assert torch.equal(again.d, inp.d) and again.tcol == inp.tcol


def test_comparisons_accept_the_reference_and_reject_planted_defects():
    inp = R.exact_inputs(BQ, ND, H, TPS, LAB)
    s = R.scores64(inp.q, inp.d, LAB)
    idx, val = R.order_ref(s, K)
    cm = R.chunk_max_ref(s)
    assert R.rejected(R.topk_exact_errs(idx.int(), val.float(), idx, val)) == 0
    assert R.rejected(R.cm_exact_errs(cm.float(), cm)) == 0
    R.check("reference", R.topk_exact_errs(idx.int(), val.float(), idx, val) + R.cm_exact_errs(cm.float(), cm), quiet=True)

    # 1. chunk maxima that leave out the last tile of every split, and the top-k that follows
    bad_cm = R.defect_cm_skips_last_tile(s, TPS)
    n_cm = R.rejected(R.cm_exact_errs(bad_cm, cm))
    bi, bv = R.defect_topk_from_cm(s, bad_cm, K)
    n_top = R.rejected(R.topk_exact_errs(bi, bv, idx, val)[:1])
    print(f"last tile skipped: {int(n_cm)} of {cm.numel()} maxima, {int(n_top)} of {idx.numel()} columns")
    assert n_cm == 120 and n_top >= 1
    # 2. a tie given to the higher column
    bi, bv = R.defect_tie_to_higher_column(s, K)
    assert torch.equal(bv, val)  # the values alone do not show it
    n_tie = R.rejected(R.topk_exact_errs(bi, bv, idx, val))
    print(f"tie to the higher column: {int(n_tie)} of {idx.numel()} columns")
    assert n_tie >= len(inp.featured)
    # 3. a label left unmasked where its block's labels lie in two tiles
    bs = R.defect_unmasked_spanning_labels(inp.q, inp.d, LAB)
    assert (LAB // 64) != ((LAB + 15) // 64)
    bi, bv = R.order_ref(bs, K)
    n_lab = R.rejected(R.topk_exact_errs(bi, bv, idx, val)[:1])
    n_lab_cm = R.rejected(R.cm_exact_errs(R.chunk_max_ref(bs), cm))
    print(f"label unmasked: {int(n_lab)} of {idx.numel()} columns, {int(n_lab_cm)} of {cm.numel()} maxima")
    assert n_lab >= 4 and n_lab_cm >= 1
    with pytest.raises(AssertionError, match="chunk maxima"):
        R.check("defect", R.cm_exact_errs(R.chunk_max_ref(bs), cm), quiet=True)

    # ranks
    raw = R.scores64(inp.q, inp.d)
    ptr, ridx = R.csr(inp.relevant)
    theta, tcol = R.best_relevant_ref(raw, ptr, ridx)
    count = R.count_ref(raw, theta, tcol)
    assert R.rejected(R.rank_exact_errs(theta.float(), tcol.int(), count.int(), theta, tcol, count)) == 0
    # 4. the padded zero columns of the partial tile counted against a negative theta
    bad = R.defect_count_padded_columns(raw, theta, tcol)
    diff = bad - count
    neg = (theta < 0) & (tcol >= 0)
    assert int(neg.sum()) >= 5 and bool((diff[neg] == 320 - ND).all()) and bool((diff[~neg] == 0).all())
    print(f"padded columns counted: {int((diff != 0).sum())} of {BQ} counts, each by {320 - ND}")
    assert R.rejected(R.equal_errs("count", bad, count)) == int(neg.sum())
    # 5. s >= theta applied above the threshold column
    bad = R.defect_count_ge_above(raw, theta, tcol)
    n_ge = R.rejected(R.equal_errs("count", bad, count))
    print(f"s >= theta above tcol: {int(n_ge)} of {BQ} counts")
    assert n_ge >= int((tcol >= 0).sum()) - 2 and bool((bad >= count).all())


def test_interval_comparisons_on_the_mantissa_family():
    """An fp32 summation of the family passes every interval condition; a result off by three
    eps, a swapped pair, a repeated column, a returned positive, a missed column and a count
    outside the interval are each rejected."""
    bq, nd, h, k, lab = 24, 700, 128, 5, 100
    q, d, relevant = R.mantissa_inputs(bq, nd, h)
    assert torch.equal(q, q.bfloat16().float())
    s = R.scores64(q, d, lab)
    eps = R.eps_elem(q, d)
    s32 = (q @ d.t())
    s32[torch.arange(bq), lab + torch.arange(bq)] = -1.0
    idx, val = R.order_ref(s32.double(), k)
    val = val.float()
    assert R.check("fp32", R.topk_interval_errs(idx, val, s, eps, lab), quiet=True) < 1
    names = lambda errs: {n for n, e, _, b in errs if e > b}
    v2 = val.clone(); v2[3, 1] += 3 * float(eps[3, idx[3, 1]])
    assert "value / eps" in names(R.topk_interval_errs(idx, v2, s, eps, lab))
    i2 = idx.clone(); i2[4, [0, 1]] = idx[4, [1, 0]]; v2 = val.clone(); v2[4, [0, 1]] = val[4, [1, 0]]
    assert names(R.topk_interval_errs(i2, v2, s, eps, lab)) == {"unsorted pairs"}
    i2 = idx.clone(); i2[5, 2] = idx[5, 1]
    assert "repeated columns" in names(R.topk_interval_errs(i2, val, s, eps, lab))
    i2 = idx.clone(); i2[6, 4] = lab + 6
    assert "positive returned" in names(R.topk_interval_errs(i2, val, s, eps, lab))
    i2, v2 = idx.clone(), val.clone()
    nxt = R.order_ref(s32.double(), k + 1)
    i2[7, 0], v2[7, :] = nxt[0][7, k], torch.cat([val[7, 1:], nxt[1][7, k:].float()])
    i2[7, :k - 1], i2[7, k - 1] = idx[7, 1:].clone(), nxt[0][7, k]
    assert "columns above the k-th value + 2 eps" in names(R.topk_interval_errs(i2, v2, s, eps, lab))

    raw = R.scores64(q, d)
    ptr, ridx = R.csr(relevant)
    theta, tcol = R.best_relevant_ref((q @ d.t()).double(), ptr, ridx)
    count = R.count_ref((q @ d.t()).double(), theta, tcol)
    assert R.check("fp32", R.rank_interval_errs(theta.float(), tcol, count, raw, eps, ptr, ridx), quiet=True) < 1
    c2 = count.clone(); c2[1] += 40
    assert names(R.rank_interval_errs(theta.float(), tcol, c2, raw, eps, ptr, ridx)) == {
        "count outside [#(s > theta + 2 eps), #(s >= theta - 2 eps)]"}
    c2 = count.clone(); c2[0] = 1
    assert int(tcol[4]) < 0 or True
    none = [i for i, r in enumerate(relevant) if not r]
    c2 = count.clone(); c2[none[0]] = 3
    assert "count of a row without a relevant column" in names(
        R.rank_interval_errs(theta.float(), tcol, c2, raw, eps, ptr, ridx))
    t2 = tcol.clone(); t2[1] = (int(tcol[1]) + 1) % nd
    assert names(R.rank_interval_errs(theta.float(), t2, count, raw, eps, ptr, ridx)) & {"tcol not relevant", "theta / eps"}


# ---------------------------------------------------------------- tt_scan_geometry
def geometry(what, bq, nd, h, k=5, dtype=_lib.DT_BF16):
    g = _lib.ScanGeom()
    assert _lib.load().tt_scan_geometry(what, dtype, bq, nd, h, k, ctypes.byref(g)) == 0
    return g


class options:
    """Host-side option values for the duration of a block (nothing is launched here)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        lib = _lib.load()
        self.old = {k: _lib.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            assert lib.tt_set_option(k.encode(), v) == 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _lib.load().tt_set_option(k.encode(), v)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case_table_geometry(case):
    """Every case of the GPU suite plans the tiles per split it was written for, under each
    variant and block map, for the top-k scan and for the counting scan."""
    c = case
    for v in c.variants():
        for hn_map in (0, 1, 2):
            with options(hn_scan_v=v, hn_map=hn_map, hn_scan_gemm=0, hn_gemm=0, rank_gemm=0):
                for k in (1, 5, 16):
                    g = geometry(0, c.bq, c.nd, c.h, k)
                    assert (g.scan, g.variant, g.rows, g.nch) == (1, v, c.rows(v), c.nch), (c.name, v)
                    assert (g.rt, g.s, g.tps, g.last) == c.geom(v), (c.name, v, (g.rt, g.s, g.tps, g.last))
                    assert g.map == c.map_applied(v, hn_map), (c.name, v, hn_map, g.map)
                g = geometry(1, c.bq, c.nd, c.h)
                assert (g.scan, g.variant, g.rows, g.nch) == (1, 0, c.rows(0), c.nch)
                assert (g.rt, g.s, g.tps, g.last) == c.geom(0), (c.name, "count", (g.rt, g.s, g.tps, g.last))
                assert g.map == c.map_applied(0, hn_map)


def test_case_table_reaches_what_the_suite_claims():
    h256 = [c for c in R.CASES if c.h == 256]
    for v in (0, 5):
        nts = {n for c in h256 for n in (c.geom(v)[2], c.geom(v)[3])}
        assert nts >= {1, 2, 3, 4, 5, 6, 7, 8}
    assert {n for c in h256 for n in (c.geom(4)[2], c.geom(4)[3])} >= {1, 2, 3, 5, 6, 7, 8}
    for h, vs in ((128, (0,)), (256, (0, 4, 5)), (512, (0,))):
        for v in vs:
            assert any(c.geom(v)[3] < c.geom(v)[2] for c in R.CASES if c.h == h), (h, v)   # a short last split
            assert any(c.geom(v)[2] >= 2 for c in R.CASES if c.h == h)                    # the woven epilogue
    assert any(c.map2 and c.geom(0)[2] % 2 == 1 and c.geom(0)[2] > 1 for c in h256)    # map 2 at an odd nt
    assert len(R.MANTISSA_CASES) == 9 and {c.h for c in R.MANTISSA_CASES} == {128, 256, 512}
    for c in R.CASES:
        offs = R.label_offsets(c.bq, c.nd, c.geom(5 if c.h == 256 else 0)[2])
        assert offs[:2] == [-1, 0] and offs[-1] == c.nd - c.bq and all(o + c.bq <= c.nd for o in offs)
        assert any(o > 0 and o % 64 for o in offs), c.name


def test_scan_geometry_follows_the_fallbacks_and_the_options():
    lib = _lib.load()
    assert "tt_scan_geometry" in _lib.EXPORTED
    with options(hn_scan_v=5, hn_map=2, hn_scan_gemm=0, hn_gemm=0, rank_gemm=0):
        g = geometry(0, 8192, 8192, 256)
        assert (g.scan, g.variant, g.rows, g.map, g.nch, g.rt, g.s, g.tps, g.last) == (1, 5, 256, 2, 128, 32, 8, 16, 16)
        g = geometry(0, 8192, 65536, 256)   # v 5 has no staging cap
        assert (g.variant, g.rt, g.s, g.tps, g.last) == (5, 32, 8, 128, 128)
        # the variant is h 256's; the CM offsets of v 5 must fit 32 bits
        assert geometry(0, 8192, 8192, 128).variant == 0 and geometry(0, 8192, 8192, 512).variant == 0
        assert geometry(0, 65536, 1 << 19, 256).variant == 0 and geometry(0, 65536, (1 << 19) - 64, 256).variant == 5
        # not the streamed path: every field 0
        for args in ((0, 100, 1000, 64, 5), (0, 100, 1000, 256, 17), (1, 100, 1000, 96, 5), (0, 0, 1000, 256, 5),
                     (1, 100, 0, 256, 5)):
            g = geometry(*args)
            assert (g.scan, g.rows, g.nch, g.s, g.tps, g.last) == (0, 0, 0, 0, 0, 0), args
        assert geometry(0, 100, 1000, 256, dtype=_lib.DT_F32).scan == 0
        assert geometry(1, 100, 1000, 256, 99).scan == 1   # k is the top-k's
        with options(hn_gemm=1):
            assert geometry(0, 100, 1000, 256).scan == 0 and geometry(1, 100, 1000, 256).scan == 1
        with options(rank_gemm=1):
            assert geometry(1, 100, 1000, 256).scan == 0 and geometry(0, 100, 1000, 256).scan == 1
        with options(hn_scan_gemm=1):
            assert geometry(0, 100, 1000, 256).scan == 2 and geometry(1, 100, 1000, 256).scan == 1
    with options(hn_scan_v=0, hn_map=2):
        g = geometry(0, 8192, 65536, 256)   # the 32-tile staging cap
        assert (g.variant, g.s, g.tps, g.last) == (0, 32, 32, 32)
        g = geometry(1, 8192, 65536, 256)   # a count stages nothing
        assert (g.s, g.tps) == (8, 128)
    with options(hn_scan_v=3):
        assert geometry(0, 300, 1000, 256).variant == 0
    # s, tps and last always tile nch exactly
    for bq, nd in ((1, 1), (1, 64), (1, 65), (257, 6400), (70000, 640), (5000, 70000)):
        for what in (0, 1):
            g = geometry(what, bq, nd, 256)
            assert g.nch == (nd + 63) // 64 and (g.s - 1) * g.tps + g.last == g.nch and 1 <= g.last <= g.tps
            assert g.rt == (bq + g.rows - 1) // g.rows
    assert lib.tt_scan_geometry(0, _lib.DT_BF16, 16, 64, 256, 5, None) == _lib.TT_EINVAL
    g = _lib.ScanGeom()
    assert lib.tt_scan_geometry(2, _lib.DT_BF16, 16, 64, 256, 5, ctypes.byref(g)) == _lib.TT_EINVAL
