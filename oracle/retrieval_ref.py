"""Float64 restatement of tt_hardneg_topk (k <= 16) and of the full-rank pair
tt_rank_best_relevant / tt_rank_count, the input families, the comparison functions and the
case tables that tests/test_retrieval_ref_host.py and tests/test_gpu_scan_ref.py share -- TEST
INFRASTRUCTURE ONLY.

Written from the contract in include/tt_hip.h, not from the kernels: plain torch in float64 on
the operands' device, nothing read from outside the repository. Operands are taken as the kernel
sees them (bf16-rounded, then widened).

References
  scores64        S = Q D^T, column label_offset + row set to -1 (label_offset < 0: none)
  order_ref       per row the first k columns by (value descending, column ascending), and
                  their values (a stable sort, in row blocks)
  chunk_max_ref   [bq, nch]: the maximum of S over each 64-column chunk, the columns past nd
                  excluded (every chunk holds at least one column)
  best_relevant_ref / count_ref
                  theta = the largest score over a row's relevant columns, tcol = the lowest
                  column that reaches it (0 and -1 for a row without one); count = the columns
                  col_offset + j of a block with s > theta, or s == theta and col_offset + j < tcol

Two input families
  exact          integer rows in [-3, 3] (exact_inputs): every score is an integer below 2^13,
                 exact in fp32 in any order, so everything is compared with torch.equal. The
                 first 8 components of every query are 3, so the three kinds of planted
                 documents (+3, 0, -3 there and zero elsewhere) score +72, 0 and -72 against
                 EVERY query: thresholds of either sign and of exactly zero, each with exact
                 duplicates on both sides of the threshold column and with the natural ties of
                 integer scores. Copies of featured query rows are planted as documents (a
                 row's own copies score |q|^2, far above anything random), so the row's top-k
                 is a run of exact ties whose columns sit where the tile loop can go wrong; and
                 a quarter of the positives are copies of their query, so a positive left
                 unmasked is the row's best score.
  full mantissa  normalised random rows rounded to bf16 (mantissa_inputs). No near-tie is
                 excluded; the conditions (topk_interval_errs, rank_interval_errs) hold for every
                 row with eps_ij = gamma_h sum_k |q_ik d_jk|, gamma_h = h u / (1 - h u),
                 u = 2^-24: the bound on a length-h fp32 sum of exact products in any order
                 (bf16 x bf16 products are exact in fp32).

Comparison functions return lists of (name, error, index, bound); check() prints the worst and
asserts error <= bound for each.
"""
from __future__ import annotations

import dataclasses

import torch

TILE = 64
U = 2.0 ** -24
POS8 = 8            # leading query components held at 3
TYPE_SCORE = {"pos": 9.0 * POS8, "zero": 0.0, "neg": -9.0 * POS8}
# in-tile positions of the threshold column: the span edges of the counting epilogue's
# single-compare form (elements [0, 19] and [32, 51] of a lane's 64) and the tile's ends
TCOL_POS = (0, 19, 20, 31, 32, 51, 63)


def gamma(h: int) -> float:
    return h * U / (1.0 - h * U)


# ---------------------------------------------------------------- references
def scores64(q, d, label_offset=-1):
    s = q.double() @ d.double().t()
    if label_offset >= 0:
        r = torch.arange(q.shape[0], device=s.device)
        s[r, label_offset + r] = -1.0
    return s


def order_ref(s, k, block=1024):
    out = []
    for r0 in range(0, s.shape[0], block):
        out.append(torch.sort(-s[r0:r0 + block], dim=1, stable=True).indices[:, :k])
    idx = torch.cat(out) if out else torch.zeros(0, k, dtype=torch.long, device=s.device)
    return idx, torch.gather(s, 1, idx)


def chunk_max_ref(s):
    bq, nd = s.shape
    nch = (nd + TILE - 1) // TILE
    p = torch.full((bq, nch * TILE), float("-inf"), dtype=s.dtype, device=s.device)
    p[:, :nd] = s
    return p.view(bq, nch, TILE).amax(dim=2)


def csr(relevant, dev="cpu"):
    """(rel_ptr [Q + 1], rel_idx) int32 from a list of column collections."""
    ptr, idx = [0], []
    for rel in relevant:
        idx += sorted(rel)
        ptr.append(len(idx))
    return (torch.tensor(ptr, dtype=torch.int32, device=dev), torch.tensor(idx, dtype=torch.int32, device=dev))


def best_relevant_ref(s, rel_ptr, rel_idx):
    """(theta float64 [Q], tcol int64 [Q])."""
    Q, N = s.shape
    dev = s.device
    ptr, idx = rel_ptr.long().to(dev), rel_idx.long().to(dev)
    rows = torch.repeat_interleave(torch.arange(Q, device=dev), ptr[1:] - ptr[:-1])
    vals = s[rows, idx]
    theta = torch.full((Q,), float("-inf"), dtype=s.dtype, device=dev).scatter_reduce(0, rows, vals, "amax")
    cand = torch.where(vals == theta[rows], idx, torch.full_like(idx, N))
    tcol = torch.full((Q,), N, dtype=torch.long, device=dev).scatter_reduce(0, rows, cand, "amin")
    none = tcol == N
    return torch.where(none, torch.zeros_like(theta), theta), torch.where(none, -torch.ones_like(tcol), tcol)


def count_ref(s, theta, tcol, col_offset=0):
    """Columns of the block s (global columns col_offset ...) that beat (theta, tcol); int64 [Q]."""
    cols = col_offset + torch.arange(s.shape[1], device=s.device)
    th = theta.double()[:, None]
    beats = (s > th) | ((s == th) & (cols[None, :] < tcol[:, None]))
    return torch.where(tcol >= 0, beats.sum(dim=1), torch.zeros_like(tcol))


def eps_elem(q, d):
    """The derived fp32 accumulation bound per score: gamma_h sum_k |q_k d_k|."""
    return gamma(q.shape[1]) * (q.double().abs() @ d.double().abs().t())


# ---------------------------------------------------------------- geometry tables
@dataclasses.dataclass(frozen=True)
class ScanCase:
    bq: int
    nd: int
    h: int
    plan: tuple            # (RT, S, tps, last) at 256 rows per workgroup (h 512: 128 rows)
    plan4: tuple = None    # the same at 512 rows per workgroup (hn_scan_v 4); None: as plan
    map2: bool = False     # hn_map 2 applies (RT even, S % 4 == 0)
    map2_4: bool = None    # ... under hn_scan_v 4; None: as map2
    reaches: str = ""

    @property
    def name(self):
        return f"{self.bq}x{self.nd}x{self.h}"

    @property
    def nch(self):
        return (self.nd + TILE - 1) // TILE

    def variants(self):
        return (5, 0, 4) if self.h == 256 else (0,)

    def rows(self, v):
        return 128 if self.h == 512 else 512 if v == 4 else 256

    def geom(self, v):
        return self.plan4 if v == 4 and self.plan4 is not None else self.plan

    def map_applied(self, v, hn_map):
        m2 = self.map2_4 if v == 4 and self.map2_4 is not None else self.map2
        return 0 if hn_map == 2 and not m2 else hn_map


CASES = [
    ScanCase(16, 16576, 256, (1, 130, 2, 1), reaches="nt 2 and nt 1, rows past bq"),
    ScanCase(16, 33000, 256, (1, 172, 3, 3), reaches="nt 3, partial tile"),
    ScanCase(2304, 6100, 256, (9, 24, 4, 4), (5, 48, 2, 2), reaches="nt 4: the 5-slot ring one short of t == 4"),
    ScanCase(4096, 4100, 256, (16, 13, 5, 5), (8, 22, 3, 2), reaches="nt 5: VM_T4; partial tile in a full split"),
    ScanCase(16, 81950, 256, (1, 214, 6, 3), reaches="nt 6 > ring depth, short last split"),
    ScanCase(16, 98400, 256, (1, 220, 7, 5), reaches="nt 7"),
    ScanCase(16, 131000, 256, (1, 256, 8, 7), reaches="v 4 staging cap 8, short last split"),
    ScanCase(2100, 4100, 256, (9, 22, 3, 2), (5, 33, 2, 1), reaches="partial row tile, short last split"),
    ScanCase(2048, 6100, 256, (8, 32, 3, 3), (4, 48, 2, 2), map2=True, reaches="map 2 applied at an odd nt"),
    ScanCase(600, 12300, 256, (3, 65, 3, 1), (2, 97, 2, 1), reaches="odd RT, last split of one tile"),
    ScanCase(300, 1000, 256, (2, 16, 1, 1), (1, 16, 1, 1), map2=True, map2_4=False, reaches="one tile per split"),
    ScanCase(40, 70, 256, (1, 2, 1, 1), reaches="two chunks, one tile per split"),
    ScanCase(16, 16576, 128, (1, 130, 2, 1), reaches="h 128: nt 2 and nt 1"),
    ScanCase(2048, 6100, 128, (8, 32, 3, 3), map2=True, reaches="h 128: odd nt under map 2"),
    ScanCase(600, 12300, 128, (3, 65, 3, 1), reaches="h 128: last split of one tile"),
    ScanCase(40, 70, 128, (1, 2, 1, 1), reaches="h 128: one tile per split"),
    ScanCase(16, 49152, 512, (1, 256, 3, 3), reaches="h 512: the 2-slot ring with 3 tiles"),
    ScanCase(1100, 4100, 512, (9, 22, 3, 2), reaches="h 512: partial row tile, short last split"),
    ScanCase(1024, 6100, 512, (8, 32, 3, 3), map2=True, reaches="h 512: odd nt under map 2"),
    ScanCase(300, 1000, 512, (3, 16, 1, 1), reaches="h 512: one tile per split"),
]

# full-mantissa family: three shapes per width
MANTISSA_CASES = [c for c in CASES if (c.bq, c.nd, c.h) in {
    (16, 81950, 256), (2304, 6100, 256), (2100, 4100, 256),
    (16, 16576, 128), (2048, 6100, 128), (600, 12300, 128),
    (16, 49152, 512), (1100, 4100, 512), (1024, 6100, 512)}]


def label_offsets(bq, nd, tps):
    """-1, 0, one that is no multiple of 64 and puts a 16-query block's labels on both sides
    of the boundary between two splits (where it fits), for a few queries and three or more
    tiles per split one inside a split's middle tile, and the last bq columns (the partial
    tile)."""
    odd = 2 * tps * TILE - 8
    if odd + bq > nd:
        odd = min(TILE - 8, nd - bq - 1)
    out = [-1, 0]
    if odd > 0:
        out.append(odd)
    mid = (tps + tps // 2) * TILE + 24
    if tps >= 3 and bq <= 32 and mid + bq <= nd:
        out.append(mid)
    if nd - bq not in out:
        out.append(nd - bq)
    return out


# ---------------------------------------------------------------- exact family
@dataclasses.dataclass
class ExactInputs:
    q: torch.Tensor          # [bq, h] float32, integer-valued
    d: torch.Tensor          # [nd, h]
    planted: dict            # column -> what holds it
    featured: dict           # query row -> the columns holding copies of it
    typed: dict              # "pos" / "zero" / "neg" -> columns
    relevant: list           # per query, the relevant columns (rank tests)
    tcol: list               # per query, the intended threshold column (-1: none)


def _type_doc(kind, h):
    v = torch.zeros(h)
    v[:POS8] = {"pos": 3.0, "zero": 0.0, "neg": -3.0}[kind]
    return v


def exact_inputs(bq, nd, h, tps, label_offset=-1, seed=0):
    """See the module docstring. tps: tiles per split of the plan the case is written for; it
    decides where the planted columns go. Deterministic in its arguments."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * bq + 31 * nd + h)
    q = torch.randint(-3, 4, (bq, h), generator=g).float()
    d = torch.randint(-3, 4, (nd, h), generator=g).float()
    q[:, :POS8] = 3.0
    nch = (nd + TILE - 1) // TILE
    last0 = (nch - 1) * TILE                      # first column of the last (partial) tile
    planted, featured, typed = {}, {}, {"pos": [], "zero": [], "neg": []}

    def put(col, what, vec):
        if 0 <= col < nd and col not in planted:
            planted[col] = what
            d[col] = vec
            return True
        return False

    # threshold documents: one group per (in-tile position, kind), each in a tile of its own
    # kind of place: a split's first, middle and last tile, the partial tile and its neighbour
    tiles = [0, tps - 1, tps, tps + tps // 2, 2 * tps - 1, nch - 1, nch - 2, (nch // 2) | 1]
    tiles = [t for i, t in enumerate(tiles) if 0 <= t < nch and t not in tiles[:i]]
    groups = []
    kinds = ("neg", "zero", "pos")  # rotated per position: a corpus of a few tiles still gets every kind
    for gi, (kind, pos) in enumerate((kinds[(i + n) % 3], p) for i, p in enumerate(TCOL_POS) for n in range(3)):
        for j in range(len(tiles)):
            col = tiles[(gi + j) % len(tiles)] * TILE + pos
            if put(col, kind, _type_doc(kind, h)):
                typed[kind].append(col)
                groups.append((kind, col))
                break
    for kind in typed:  # the corpus's last columns (the partial tile) and its first hold one of each kind
        for col in (nd - 1 - ("neg", "zero", "pos").index(kind), ("neg", "zero", "pos").index(kind) + 1):
            if put(col, kind, _type_doc(kind, h)):
                typed[kind].append(col)
    # copies of featured query rows: the row's top-k is then a run of exact ties
    rows = sorted({r for r in list(range(min(bq, 16))) + list(range(max(bq - 16, 0), bq))
                   + [x for m in (256, 512, 1024) for x in (m - 1, m, m + 1) if x < bq]})
    for f, r in enumerate(rows):
        s0 = (1 + f) * tps * TILE % max(last0, 1) // TILE * TILE   # a split's first tile
        kinds = [
            (s0 + 3 + f % 8, s0 + 50 - f % 8),                                  # within a tile
            (s0 + 60 - f % 4, s0 + TILE + 5 + f % 4),                           # the two tiles of a pair
            (s0 + tps * TILE - 2 - f % 4, s0 + tps * TILE + 1 + f % 4),         # a split's last tile and the next's first
            (last0 + f % 8, nd - 4 - f % 8, TILE + 9 + f),                      # the partial tile, and far below it
            (s0 + (tps // 2) * TILE + 20 + f % 8, last0 - tps * TILE + 30 + f % 8),  # a middle tile, the last split
        ]
        cols = [c for c in kinds[f % len(kinds)] + kinds[(f + 2) % len(kinds)] if put(c, f"copy of query {r}", q[r])]
        if len(cols) >= 2:
            featured[r] = sorted(cols)
    # exact duplicates of every threshold document below and above it: the same tile, the
    # neighbouring tiles and another split
    for kind, col in list(groups):
        for off in (-1, 1, -5, 7, -TILE, TILE, -tps * TILE - 3, tps * TILE + 3, 2 * tps * TILE):
            if put(col + off, kind, _type_doc(kind, h)):
                typed[kind].append(col + off)

    # a quarter of the positives are their query itself
    if label_offset >= 0:
        for r in range(1, bq, 4):
            planted.pop(label_offset + r, None)
            for cols in featured.values():
                if label_offset + r in cols:
                    cols.remove(label_offset + r)
            for cols in typed.values():
                if label_offset + r in cols:
                    cols.remove(label_offset + r)
            put(label_offset + r, f"positive copy of query {r}", q[r])
    groups = [(kind, col) for kind, col in groups if planted.get(col) == kind]

    # relevance: query r takes group r * stride + seed (cyclically); one row in 16 has none;
    # every third row also lists the nearest duplicate above its threshold column (a tie between
    # two relevant columns, which goes to the lower)
    relevant, tcol = [], []
    stride = next(x for x in (4, 5, 7, 1) if len(groups) % x)  # 16 rows still meet every position
    for r in range(bq):
        if r % 16 == 15 or not groups:
            relevant.append(set())
            tcol.append(-1)
            continue
        kind, col = groups[(r * stride + seed) % len(groups)]
        rel = {col}
        if r % 3 == 1:
            rel |= set(sorted(c for c in typed[kind] if c > col and planted.get(c) == kind)[:1])
        tcol.append(col)
        relevant.append(rel)
    return ExactInputs(q, d, planted, featured, typed, relevant, tcol)


def mantissa_inputs(bq, nd, h, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * bq + 31 * nd + h + 1)
    q = torch.nn.functional.normalize(torch.randn(bq, h, generator=g), dim=1).bfloat16().float()
    d = torch.nn.functional.normalize(torch.randn(nd, h, generator=g), dim=1).bfloat16().float()
    d[nd - 7] = d[11]  # one exact duplicate far apart
    relevant = [set(torch.randint(0, nd, (i % 4,), generator=g).tolist()) | ({11, nd - 7} if i % 5 == 0 else set())
                for i in range(bq)]
    return q, d, relevant


# ---------------------------------------------------------------- comparisons
def _first(mask):
    i = torch.nonzero(mask.flatten())
    return int(i[0]) if len(i) else -1


def equal_errs(name, got, ref):
    """Elements that differ (bound 0). got and ref are compared in float64 / int64."""
    g = got.double() if got.is_floating_point() else got.long()
    r = ref.double() if ref.is_floating_point() else ref.long()
    if g.shape != r.shape:
        return [(name + " shape", 1.0, -1, 0.0)]
    bad = g.to(r.device) != r
    return [(name, float(bad.sum()), _first(bad), 0.0)]


def topk_exact_errs(idx, val, ref_idx, ref_val):
    return equal_errs("top-k columns", idx, ref_idx) + equal_errs("top-k values", val, ref_val)


def cm_exact_errs(cm, ref_cm):
    return equal_errs("chunk maxima", cm, ref_cm)


def rank_exact_errs(theta, tcol, count, ref_theta, ref_tcol, ref_count):
    return (equal_errs("theta", theta, ref_theta) + equal_errs("tcol", tcol, ref_tcol)
            + equal_errs("count", count, ref_count))


def topk_interval_errs(idx, val, s, eps, label_offset):
    """idx, val: the call's result; s the (masked) float64 scores, eps = eps_elem."""
    dev = s.device
    idx, v = idx.long().to(dev), val.double().to(dev)
    rows = torch.arange(s.shape[0], device=dev)
    frac = (v - torch.gather(s, 1, idx)).abs() / torch.gather(eps, 1, idx)
    errs = [("value / eps", float(frac.max()), int(frac.argmax()), 1.0)]
    unsorted = (v[:, :-1] < v[:, 1:]) | ((v[:, :-1] == v[:, 1:]) & (idx[:, :-1] > idx[:, 1:]))
    errs.append(("unsorted pairs", float(unsorted.sum()), _first(unsorted), 0.0))
    srt = idx.sort(dim=1).values
    dup = srt[:, :-1] == srt[:, 1:]
    errs.append(("repeated columns", float(dup.sum()), _first(dup), 0.0))
    if label_offset >= 0:
        hit = idx == (label_offset + rows)[:, None]
        errs.append(("positive returned", float(hit.sum()), _first(hit), 0.0))
    rest = s.scatter(1, idx, float("-inf"))
    over = rest > v[:, -1:] + 2.0 * eps
    errs.append(("columns above the k-th value + 2 eps", float(over.sum()), _first(over), 0.0))
    return errs


def rank_interval_errs(theta, tcol, count, s, eps, rel_ptr, rel_idx, col_offset=0):
    """theta, tcol: tt_rank_best_relevant's; count: tt_rank_count's over the block s (global
    columns col_offset ...; theta / tcol checks need col_offset = 0 and the whole matrix)."""
    dev = s.device
    Q, N = s.shape
    th, tc, cnt = theta.double().to(dev), tcol.long().to(dev), count.long().to(dev)
    ptr, ridx = rel_ptr.long().to(dev), rel_idx.long().to(dev)
    rows = torch.repeat_interleave(torch.arange(Q, device=dev), ptr[1:] - ptr[:-1])
    has = ptr[1:] > ptr[:-1]
    errs = [("tcol < 0 iff no relevant column", float(((tc >= 0) != has).sum()), _first((tc >= 0) != has), 0.0)]
    live = tc >= 0
    if col_offset == 0:
        rel = torch.zeros(Q, N, dtype=torch.bool, device=dev)
        rel[rows, ridx] = True
        t = tc.clamp(min=0)
        r = torch.arange(Q, device=dev)
        notrel = live & ~rel[r, t]
        errs.append(("tcol not relevant", float(notrel.sum()), _first(notrel), 0.0))
        frac = torch.where(live, (th - s[r, t]).abs() / eps[r, t], torch.zeros_like(th))
        errs.append(("theta / eps", float(frac.max()), int(frac.argmax()), 1.0))
        better = (rel & (s - 2.0 * eps > th[:, None])).any(dim=1) & live
        errs.append(("a relevant column above theta + 2 eps", float(better.sum()), _first(better), 0.0))
    lo = (s > th[:, None] + 2.0 * eps).sum(dim=1)
    hi = (s >= th[:, None] - 2.0 * eps).sum(dim=1)
    bad = live & ((cnt < lo) | (cnt > hi))
    errs.append(("count outside [#(s > theta + 2 eps), #(s >= theta - 2 eps)]", float(bad.sum()), _first(bad), 0.0))
    dead = ~live & (cnt != 0)
    errs.append(("count of a row without a relevant column", float(dead.sum()), _first(dead), 0.0))
    return errs


def check(what, errs, quiet=False):
    worst = 0.0
    for name, err, index, bound in errs:
        if not quiet:
            print(f"{what}: {name}: {err:.4g} (bound {bound:.4g}, at {index})")
        assert err <= bound, f"{what}: {name}: {err:.6g} > {bound:.6g} at flat index {index}"
        if bound > 0:
            worst = max(worst, err / bound)
    return worst


def rejected(errs):
    """The largest error / bound excess of a comparison (> 0: it rejects); for bound 0 the error."""
    return max((e / b - 1.0) if b > 0 else e for _, e, _, b in errs)


# ---------------------------------------------------------------- planted defects
def defect_cm_skips_last_tile(s, tps):
    """Chunk maxima whose last tile of every split never saw its scores (-inf there)."""
    cm = chunk_max_ref(s).clone()
    nch = cm.shape[1]
    last = [t for t in range(nch) if t % tps == tps - 1 or t == nch - 1]
    cm[:, last] = float("-inf")
    return cm


def defect_topk_from_cm(s, cm, k):
    """The top-k that follows from chunk maxima cm: columns of chunks at -inf are never seen."""
    bq, nd = s.shape
    dead = torch.repeat_interleave(cm == float("-inf"), TILE, dim=1)[:, :nd]
    return order_ref(torch.where(dead, torch.full_like(s, float("-inf")), s), k)


def defect_tie_to_higher_column(s, k):
    idx = torch.sort(s.flip(1), dim=1, descending=True, stable=True).indices[:, :k]
    idx = s.shape[1] - 1 - idx
    return idx, torch.gather(s, 1, idx)


def defect_unmasked_spanning_labels(q, d, label_offset):
    """Scores whose positive is left unmasked in every 16-query block whose labels lie in two
    tiles."""
    s = scores64(q, d, label_offset)
    raw = scores64(q, d, -1)
    for r0 in range(0, q.shape[0], 16):
        r1 = min(r0 + 16, q.shape[0])
        if (label_offset + r0) // TILE != (label_offset + r1 - 1) // TILE:
            r = torch.arange(r0, r1)
            s[r, label_offset + r] = raw[r, label_offset + r]
    return s


def defect_count_padded_columns(s, theta, tcol):
    """Counts that take the zero scores padding the partial tile for documents."""
    bq, nd = s.shape
    nch = (nd + TILE - 1) // TILE
    p = torch.zeros(bq, nch * TILE, dtype=s.dtype, device=s.device)
    p[:, :nd] = s
    return count_ref(p, theta, tcol)


def defect_count_ge_above(s, theta, tcol):
    """Counts with s >= theta on both sides of the threshold column."""
    cols = torch.arange(s.shape[1], device=s.device)
    th = theta.double()[:, None]
    beats = (s >= th) & (cols[None, :] != tcol[:, None])
    return torch.where(tcol >= 0, beats.sum(dim=1), torch.zeros_like(tcol))
