"""Generate tests/golden/fullrank_tiny.npz by running the REFERENCE's validate_margin.compute_mrr.

TEST INFRASTRUCTURE ONLY. Run where the reference checkout exists (TT_REFERENCE names it, as
for oracle/gen_goldens.py), on the CPU:
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_fullrank_golden.py [seed]
validate_margin.py imports tqdm and utils (which imports gensim.downloader and datasets) at
module level but only dereferences them inside main(); stub modules satisfy the imports. The
fixture is data (inputs + expected outputs); no reference source is restated: the model, the
featurisation, the scoring, the sort and the 1/rank rule are the reference's own.

Setup: a seeded margin_two_tower.TwoTowerModel(16, 8) in eval mode, a made-up vocabulary of
64 alphabetic words with 16-d vectors, 40 distinct documents and 12 queries of a few words
each, relevant sets of 0, 1 and 3 documents. compute_mrr scores one query against all 40
documents, sorts them (stable, descending) and returns 1/rank of the first relevant one
and the first three (document, score) pairs. A query without relevant documents returns 0.

The reference ranks fp32 scores, so two documents closer than rounding could legitimately
order differently on another machine. The generator therefore measures, per query, the
smallest gap between the best relevant score and every other document's score, and the
smallest gap between neighbours among the first four scores (what the top 3 depend on), and
refuses to write a fixture in which either is below GAP_MIN = 100 x the 1e-4 bound
(relative to the largest |score|) that tests/test_gpu_margin.py holds the similarity matrix
to. Another seed is the remedy, never a smaller bound.

Forty random documents of an untrained 8-wide tower score within a narrow band of each
other, closer than that bound almost everywhere. So the generator draws a larger pool of
made-up texts (POOL_D documents, POOL_Q queries), scores it once with the reference model,
and picks from it, by a seeded random search, 40 documents and 12 queries whose first four
scores are GAP_MIN apart; each query's relevant set is then drawn among the documents that
stand GAP_MIN clear of every other score of that query (the best relevant one) and, for the
three-member sets, documents scoring below it. The numbers in the fixture are still nothing
but compute_mrr's output on the chosen texts.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from oracle import gen_goldens  # noqa: E402

GAP_MIN = 100 * 1e-4
E, H, NDOC, NQ, NWORD = 16, 8, 40, 12, 64
POOL_D, POOL_Q, TRIES = 400, 120, 4000
SEED = 3


def import_validate_reference():
    gen_goldens.import_reference()  # gensim stubs + the reference on sys.path
    for name, attrs in (("datasets", ("load_dataset",)), ("tqdm", ("tqdm",)),
                        ("utils", ("load_or_cache_word2vec", "load_or_cache_msmarco"))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    gd = sys.modules["gensim.downloader"]
    if not hasattr(gd, "load"):
        gd.load = None
    import margin_two_tower as mt  # noqa: E402
    import validate_margin as vm  # noqa: E402
    return mt, vm


def make_words(rng):
    """Alphabetic made-up words that none of the reference's marker rewrites touches."""
    cons, vow = "bdfgklmnprstvz", "aeiou"
    words = set()
    while len(words) < NWORD:
        n = int(rng.integers(2, 4))
        words.add("".join(cons[int(rng.integers(len(cons)))] + vow[int(rng.integers(len(vow)))] for _ in range(n)))
    banned = {"is", "are", "has", "have", "part", "of", "to", "a", "an", "the"}
    return sorted(words - banned)


def make_texts(rng, words, n, lo, hi):
    out = []
    while len(out) < n:
        t = " ".join(words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(lo, hi))))
        if t not in out:
            out.append(t)
    return out


def clear_of_others(s, t):
    """Smallest distance from score s[t] to any other score of the row."""
    others = torch.cat([s[:t], s[t + 1:]])
    return float((others - s[t]).abs().min())


def first4_gap(s):
    first4 = torch.sort(s, descending=True).values[:4]
    return float((first4[:-1] - first4[1:]).min())


def pick(rng, sim, scale):
    """(document subset, query subset, relevant sets as positions in the subset) or None."""
    need = GAP_MIN * scale * 1.05  # a margin over the bound, for the re-check on the chosen texts
    for _ in range(TRIES):
        dsel = np.sort(rng.choice(sim.shape[1], NDOC, replace=False))
        sub = sim[:, dsel]
        qok = [i for i in range(sim.shape[0]) if first4_gap(sub[i]) >= need]
        if len(qok) < NQ:
            continue
        qsel, relevant = [], []
        for i in (int(x) for x in rng.permutation(qok)):
            k = len(qsel)
            n = (1, 3, 0)[k % 3]
            if n == 0:
                qsel.append(i)
                relevant.append([])
            else:
                clear = [t for t in range(NDOC) if clear_of_others(sub[i], t) >= need]
                lower = {t: [u for u in range(NDOC) if sub[i][u] < sub[i][t]] for t in clear}
                clear = [t for t in clear if len(lower[t]) >= n - 1]
                if not clear:
                    continue
                t = clear[int(rng.integers(len(clear)))]
                rest = [int(u) for u in rng.choice(lower[t], size=n - 1, replace=False)]
                qsel.append(i)
                relevant.append(sorted([t] + rest))
            if len(qsel) == NQ:
                return dsel, qsel, relevant
    return None


def gen(seed):
    mt, vm = import_validate_reference()
    rng = np.random.default_rng(seed)
    words = make_words(rng)
    vecs = (1.5 * rng.standard_normal((len(words), E))).astype(np.float32)
    w2v = gen_goldens.FakeW2V(words, vecs)
    pool_d = make_texts(rng, words, POOL_D, 4, 12)
    pool_q = make_texts(rng, words, POOL_Q, 2, 6)
    torch.manual_seed(seed)
    model = mt.TwoTowerModel(E, H).eval()

    def scores(qs, ds):  # the reference model's own cosine scores, as compute_mrr forms them
        with torch.no_grad():
            qe = torch.stack([mt.SimpleDataset.text_to_embedding(q, w2v) for q in qs])
            de = torch.stack([mt.SimpleDataset.text_to_embedding(d, w2v) for d in ds])
            return torch.nn.functional.cosine_similarity(model.encode_query(qe).unsqueeze(1),
                                                         model.encode_doc(de).unsqueeze(0), dim=2).double()

    pool_sim = scores(pool_q, pool_d)
    chosen = pick(rng, pool_sim, float(pool_sim.abs().max()))
    if chosen is None:
        print(f"seed {seed}: no subset of the pool meets the gaps")
        return False
    dsel, qsel, relevant = chosen
    docs = [pool_d[j] for j in dsel]
    queries = [pool_q[i] for i in qsel]
    pos = {d: j for j, d in enumerate(docs)}
    rr, top3, top3s, gap_rel, gap_top = [], [], [], [], []
    for q, rel in zip(queries, relevant):
        m, top = vm.compute_mrr(model, q, {docs[j] for j in rel}, docs, w2v, torch.device("cpu"))
        rr.append(m)
        top3.append([pos[d] for d, _ in top])
        top3s.append([s for _, s in top])
    sim = scores(queries, docs)
    scale = float(sim.abs().max())
    for i, rel in enumerate(relevant):
        gap_top.append(first4_gap(sim[i]) / scale)
        if rel:
            t = max(rel, key=lambda j: float(sim[i][j]))
            gap_rel.append(clear_of_others(sim[i], t) / scale)
    g_rel, g_top = min(gap_rel), min(gap_top)
    print(f"seed {seed}: min gap best-relevant {g_rel:.4g}, first-four {g_top:.4g} (need {GAP_MIN:g}); rr {rr}")
    if g_rel < GAP_MIN or g_top < GAP_MIN:
        return False
    ranks = [0 if m == 0.0 else int(round(1.0 / m)) for m in rr]
    assert sorted({len(r) for r in relevant}) == [0, 1, 3] and len(set(ranks)) >= 4, (relevant, ranks)
    ptr = np.cumsum([0] + [len(r) for r in relevant]).astype(np.int32)
    out = gen_goldens.sd_arrays("w.", model.state_dict())
    out.update(words=np.array(words), vecs=vecs, docs=np.array(docs), queries=np.array(queries), rel_ptr=ptr,
               rel_idx=np.array([j for r in relevant for j in r], dtype=np.int32),
               rr=np.array(rr, dtype=np.float64), rank=np.array(ranks, dtype=np.int32),
               top3=np.array(top3, dtype=np.int32), top3_scores=np.array(top3s, dtype=np.float32),
               gap_rel=np.float64(g_rel), gap_top=np.float64(g_top), seed=np.int32(seed))
    path = os.path.join(OUT, "fullrank_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    return True


if __name__ == "__main__":
    torch.set_num_threads(4)
    if not gen(int(sys.argv[1]) if len(sys.argv) > 1 else SEED):
        sys.exit("gaps below the bound: pick another seed")
