"""The streamed score scan (tt_score.hip hn_scan_kernel) at asserted multi-tile geometries,
through the C ABI (tt_hardneg_topk with k <= 16; tt_rank_best_relevant + tt_rank_count), against
the float64 restatement in oracle/retrieval_ref.py. The case table, the input families and the
comparison functions are retrieval_ref's; tests/test_retrieval_ref_host.py pins the references
against plain loops, shows that each comparison rejects a planted defect, and asserts the case
table's geometry on the CPU.

Every case asserts, before anything is launched, that tt_scan_geometry plans what the case was
written for under the options in force: the variant after the fallbacks, rows per workgroup,
(RT, S, tps, tiles of the last split) and the block map after the map 2 fallback. Between them
the cases run 1 to 8 tiles per workgroup, a last split shorter than the others for hn_scan_v 0,
4 and 5 and for h 128 and h 512, map 2 applied at 3 tiles per split, and the counting epilogue
woven into the next tile's k-steps at all three widths (retrieval_ref.CASES says which shape
reaches what).

Every call is guarded: val is prefilled with NaN, idx / tcol / count with a sentinel, each has
guard bands that must survive, the workspace is exactly tt_hardneg_ws_size /
tt_rank_count_ws_size bytes between guard bands that must survive, and each call runs twice
from two different poison fills of outputs and workspace, for identical bits.

Exact family (integer rows, every score exact in fp32): torch.equal with the float64 reference
  hard negatives  k in {1, 5, 16} x label_offset in {-1, 0, one that is no multiple of 64 and
                  splits a 16-query block's labels over two tiles of two splits, for 16 queries
                  one inside a split's middle tile, nd - bq (the partial tile)}:
                  idx, val, and EVERY chunk maximum at the start of the workspace (the -1 of a
                  chunk that holds only the positive included); hn_scan_v 0 / 4 / 5 (h 256),
                  hn_map 0 / 1 / 2, and hn_scan_gemm 1 -- each against float64 directly.
  ranks           theta, tcol and count in one call, in two document blocks (col_offset and
                  accumulate, the boundary 24 columns into a tile near the middle, so the second
                  call's threshold columns lie below its first column for about half the rows),
                  hn_map 0 / 1 / 2, and bit equality with rank_gemm 1.
Full-mantissa family (normalised bf16 rows, no near-tie excluded), three shapes per width: the
interval conditions of retrieval_ref.topk_interval_errs / rank_interval_errs with
eps = gamma_h sum_k |q_k d_k|.

Largest errors measured on an MI355X (test_zz_report prints them with -s):
  exact family   0 differing elements in every case, variant, block map, k and label offset
                 (idx, val, chunk maxima, theta, tcol, count).
  full mantissa  largest |got - float64| as a fraction of eps, h 128 / 256 / 512:
                 top-k value (k 16)  0.0166 (2048x6100) / 0.0083 (2304x6100) / 0.0041 (1024x6100)
                 theta               0.0070 (2048x6100) / 0.0039 (2100x4100) / 0.0020 (1024x6100)
                 identical across hn_scan_v 0 / 4 / 5 (one MFMA sequence per score). eps is a
                 worst case over signs; random signs leave about sqrt(h) of it and most partial
                 sums of 16-bit products are exact in fp32.
No kernel missed a check.
"""
import ctypes
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import retrieval_ref as R  # noqa: E402
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import call, option  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
GUARD = 512                 # elements (bytes for the workspace) before and after every buffer
WS_GUARD_BYTE = 0x3C
FILLS = (0x7F, 0xA5)        # workspace poison: 0x7F7F7F7F is 3.4e38 as a float, above any score
IDX_FILLS = (-7, 0x5A5A5A5A)
WORST = {}                  # (what, h) -> (largest error / eps, case)


def geometry(what, c, k=5):
    g = _lib.ScanGeom()
    call("tt_scan_geometry", what, _lib.DT_BF16, c.bq, c.nd, c.h, k, ctypes.byref(g))
    return g


def assert_geometry(what, c, v, hn_map, k=5, scan=1):
    g = geometry(what, c, k)
    tag = (c.name, "count" if what else "top-k", v, hn_map)
    assert (g.scan, g.variant, g.rows, g.nch) == (scan, v, c.rows(v), c.nch), tag
    assert (g.rt, g.s, g.tps, g.last) == c.geom(v), (tag, (g.rt, g.s, g.tps, g.last))
    assert g.map == c.map_applied(v, hn_map), (tag, g.map)


class Guarded:
    """A buffer of n elements between two guard bands."""

    def __init__(self, n, dtype, fill, guard_fill=None):
        self.n, self.fill = n, fill if guard_fill is None else guard_fill
        self.full = torch.full((2 * GUARD + n,), self.fill, dtype=dtype, device=DEV)
        self.view = self.full[GUARD:GUARD + n]
        if guard_fill is not None:
            self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def assert_guards(self, what):
        for band in (self.full[:GUARD], self.full[GUARD + self.n:]):
            ok = torch.isnan(band).all() if self.fill != self.fill else (band == self.fill).all()
            assert bool(ok), f"{what}: written outside the buffer"


def run_hardneg(qd, dd, lab, k, rep):
    """One guarded tt_hardneg_topk call: (idx [bq, k] int32, val [bq, k], CM [bq, nch]) on the device."""
    lib = _lib.load()
    (bq, h), nd = qd.shape, dd.shape[0]
    nch = (nd + 63) // 64
    nws = lib.tt_hardneg_ws_size(_lib.DT_BF16, bq, nd, h, k)
    assert nws >= bq * nch * 4
    idx = Guarded(bq * k, torch.int32, IDX_FILLS[rep])
    val = Guarded(bq * k, torch.float32, float("nan"))
    ws = Guarded(nws, torch.uint8, FILLS[rep], WS_GUARD_BYTE)
    call("tt_hardneg_topk", _lib.DT_BF16, qd.data_ptr(), bq, dd.data_ptr(), nd, h, lab, k, idx.ptr(), val.ptr(),
         ws.ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = f"tt_hardneg_topk {bq}x{nd}x{h} label {lab} k {k}"
    for b, n in ((idx, "idx"), (val, "val"), (ws, "workspace")):
        b.assert_guards(f"{what}: {n}")
    assert not bool(torch.isnan(val.view).any()), f"{what}: val left unwritten"
    assert bool(((idx.view >= 0) & (idx.view < nd)).all()), f"{what}: idx left unwritten or out of range"
    cm = ws.view[:bq * nch * 4].view(torch.float32).view(bq, nch)
    return idx.view.view(bq, k).clone(), val.view.view(bq, k).clone(), cm.clone()


def hardneg_twice(qd, dd, lab, k, what):
    a, b = run_hardneg(qd, dd, lab, k, 0), run_hardneg(qd, dd, lab, k, 1)
    for x, y, n in zip(a, b, ("idx", "val", "chunk maxima")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {n} differ between two runs"
    return a


def run_rank(qd, dd, ptr, ridx, rep, blocks=None):
    """tt_rank_best_relevant, then tt_rank_count over consecutive document blocks; guarded.
    Returns (theta, tcol, count) on the device."""
    lib = _lib.load()
    (Q, h), N = qd.shape, dd.shape[0]
    theta = Guarded(Q, torch.float32, float("nan"))
    tcol = Guarded(Q, torch.int32, IDX_FILLS[rep])
    count = Guarded(Q, torch.int32, 0x7F7F7F7F if rep == 0 else -3)
    st = torch.cuda.current_stream().cuda_stream
    what = f"rank {Q}x{N}x{h}"
    call("tt_rank_best_relevant", _lib.DT_BF16, qd.data_ptr(), Q, dd.data_ptr(), N, h, ptr.data_ptr(), ridx.data_ptr(),
         theta.ptr(), tcol.ptr(), None, st)
    b0 = 0
    for n in blocks or [N]:
        ws = Guarded(lib.tt_rank_count_ws_size(_lib.DT_BF16, Q, n, h), torch.uint8, FILLS[rep], WS_GUARD_BYTE)
        call("tt_rank_count", _lib.DT_BF16, qd.data_ptr(), Q, dd[b0:].data_ptr(), n, h, b0, theta.ptr(), tcol.ptr(),
             count.ptr(), 1 if b0 else 0, ws.ptr(), st)
        torch.cuda.synchronize()
        ws.assert_guards(f"{what}: workspace")
        b0 += n
    assert b0 == N
    for b, n in ((theta, "theta"), (tcol, "tcol"), (count, "count")):
        b.assert_guards(f"{what}: {n}")
    assert not bool(torch.isnan(theta.view).any()), f"{what}: theta left unwritten"
    assert bool(((tcol.view >= -1) & (tcol.view < N)).all()), f"{what}: tcol left unwritten"
    assert bool(((count.view >= 0) & (count.view <= N)).all()), f"{what}: count left unwritten"
    return theta.view.clone(), tcol.view.clone(), count.view.clone()


def rank_twice(qd, dd, ptr, ridx, what, blocks=None):
    a, b = run_rank(qd, dd, ptr, ridx, 0, blocks), run_rank(qd, dd, ptr, ridx, 1, blocks)
    for x, y, n in zip(a, b, ("theta", "tcol", "count")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {n} differ between two runs"
    return a


def variant(c, v):
    return option("hn_scan_v", v if c.h == 256 else _lib.get_option("hn_scan_v"))


IDS = [c.name for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_hardneg_exact_against_float64(case):
    """Exact family: idx, val and every chunk maximum equal the float64 reference, for every
    variant, block map, k and label offset; 0 elements differed on an MI355X."""
    c = case
    tps = c.geom(c.variants()[0])[2]
    for lab in R.label_offsets(c.bq, c.nd, tps):
        inp = R.exact_inputs(c.bq, c.nd, c.h, tps, lab)
        qd, dd = inp.q.to(DEV, BF16), inp.d.to(DEV, BF16)
        s = R.scores64(qd, dd, lab)
        ref_idx, ref_val = R.order_ref(s, min(16, c.nd))
        ref_cm = R.chunk_max_ref(s)

        def compare(got, k, what):
            idx, val, cm = got
            R.check(what, R.topk_exact_errs(idx, val, ref_idx[:, :k], ref_val[:, :k]) + R.cm_exact_errs(cm, ref_cm),
                    quiet=True)

        with option("hn_scan_gemm", 0), option("hn_gemm", 0):
            for v in c.variants():
                with variant(c, v):
                    for k in (1, 5, 16):
                        what = f"{c.name} label {lab} v {v} k {k}"
                        assert_geometry(0, c, v, _lib.get_option("hn_map"), k)
                        compare(hardneg_twice(qd, dd, lab, k, what), k, what)
                    for m in (0, 1, 2):
                        with option("hn_map", m):
                            assert_geometry(0, c, v, m)
                            compare(run_hardneg(qd, dd, lab, 5, m % 2), 5, f"{c.name} label {lab} v {v} map {m}")
            with option("hn_scan_gemm", 1):
                assert geometry(0, c).scan == 2
                compare(hardneg_twice(qd, dd, lab, 5, f"{c.name} scan gemm"), 5, f"{c.name} label {lab} scan gemm")
        print(f"{c.name} label {lab}: 0 elements differ ({c.reaches})")


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_rank_exact_against_float64(case):
    """Exact family: theta, tcol and count equal the float64 reference in one call, in two
    document blocks, under every block map, and bit for bit on the stored path; 0 elements
    differed on an MI355X."""
    c = case
    inp = R.exact_inputs(c.bq, c.nd, c.h, c.geom(0)[2], -1, seed=1)
    qd, dd = inp.q.to(DEV, BF16), inp.d.to(DEV, BF16)
    s = R.scores64(qd, dd)
    ptr, ridx = R.csr(inp.relevant, DEV)
    ref_theta, ref_tcol = R.best_relevant_ref(s, ptr, ridx)
    assert ref_tcol.tolist() == inp.tcol
    assert {float(t) for t in ref_theta[ref_tcol >= 0]} == {-72.0, 0.0, 72.0}
    ref_count = R.count_ref(s, ref_theta, ref_tcol)
    assert int(ref_count.max()) > 0

    def compare(got, what):
        R.check(what, R.rank_exact_errs(*got, ref_theta, ref_tcol, ref_count), quiet=True)

    n1 = (c.nd // 2 // 64) * 64 + 24
    assert 0 < n1 < c.nd and 0 < int((ref_tcol >= n1).sum()) and 0 < int(((ref_tcol >= 0) & (ref_tcol < n1)).sum())
    with option("rank_gemm", 0):
        for m in (0, 1, 2):
            with option("hn_map", m):
                assert_geometry(1, c, 0, m)
                scan = rank_twice(qd, dd, ptr, ridx, f"{c.name} map {m}")
                compare(scan, f"{c.name} count, map {m}")
        assert geometry(1, dataclasses.replace(c, nd=n1)).scan == 1
        compare(rank_twice(qd, dd, ptr, ridx, f"{c.name} blocks", [n1, c.nd - n1]), f"{c.name} count in two blocks")
    with option("rank_gemm", 1):
        assert geometry(1, c).scan == 0
        stored = run_rank(qd, dd, ptr, ridx, 0)
        compare(stored, f"{c.name} stored path")
    for x, y in zip(scan, stored):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    print(f"{c.name}: 0 elements differ, counts up to {int(ref_count.max())}")


MIDS = [c.name for c in R.MANTISSA_CASES]


@pytest.mark.parametrize("case", R.MANTISSA_CASES, ids=MIDS)
def test_hardneg_mantissa_against_float64(case):
    """Full-mantissa family, k 16, labels at 0 and at the odd offset, every variant: each value
    within eps of the float64 score of its column, sorted, columns distinct, no positive, no
    outside column above the k-th value + 2 eps. Largest |value - float64| / eps measured:
    see the module docstring."""
    c = case
    q, d, _ = R.mantissa_inputs(c.bq, c.nd, c.h)
    qd, dd = q.to(DEV, BF16), d.to(DEV, BF16)
    eps = R.eps_elem(qd, dd)
    k = 16
    for lab in R.label_offsets(c.bq, c.nd, c.geom(0)[2])[1:3]:
        s = R.scores64(qd, dd, lab)
        for v in c.variants():
            with variant(c, v), option("hn_scan_gemm", 0), option("hn_gemm", 0):
                what = f"{c.name} label {lab} v {v}"
                assert_geometry(0, c, v, _lib.get_option("hn_map"), k)
                idx, val, _ = hardneg_twice(qd, dd, lab, k, what)
                worst = R.check(what, R.topk_interval_errs(idx, val, s, eps, lab), quiet=True)
                print(f"{what}: value error {worst:.3g} of eps")
                if worst >= WORST.get(("top-k value", c.h), (-1.0, ""))[0]:
                    WORST[("top-k value", c.h)] = (worst, what)


@pytest.mark.parametrize("case", R.MANTISSA_CASES, ids=MIDS)
def test_rank_mantissa_against_float64(case):
    """Full-mantissa family: tcol is relevant, theta within eps of its float64 score, no relevant
    column above theta + 2 eps, count within [#(s > theta + 2 eps), #(s >= theta - 2 eps)], in
    one call and in two blocks (identical counts). Largest |theta - float64| / eps measured: see
    the module docstring."""
    c = case
    q, d, relevant = R.mantissa_inputs(c.bq, c.nd, c.h)
    qd, dd = q.to(DEV, BF16), d.to(DEV, BF16)
    eps = R.eps_elem(qd, dd)
    s = R.scores64(qd, dd)
    ptr, ridx = R.csr(relevant, DEV)
    with option("rank_gemm", 0):
        assert_geometry(1, c, 0, _lib.get_option("hn_map"))
        theta, tcol, count = rank_twice(qd, dd, ptr, ridx, c.name)
        worst = R.check(c.name, R.rank_interval_errs(theta, tcol, count, s, eps, ptr, ridx), quiet=True)
        n1 = (c.nd // 2 // 64) * 64 + 24
        _, _, parts = rank_twice(qd, dd, ptr, ridx, c.name, [n1, c.nd - n1])
        assert torch.equal(parts, count)
    print(f"{c.name}: theta error {worst:.3g} of eps")
    if worst >= WORST.get(("theta", c.h), (-1.0, ""))[0]:
        WORST[("theta", c.h)] = (worst, c.name)


def test_zz_report():
    """Prints the largest error per quantity and width (run with -s after the cases above)."""
    for (what, h), (worst, name) in sorted(WORST.items()):
        print(f"{what}, h {h}: {worst:.3g} of eps ({name})")
