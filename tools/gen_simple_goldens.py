"""Generate tests/golden/simple_tiny.npz (run A) and simple_tiny_b.npz (run B) by running the REFERENCE's simple_two_tower.py.

TEST INFRASTRUCTURE ONLY. Run in the build container (where the reference checkout exists;
TT_REFERENCE names it, as for oracle/gen_goldens.py):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_simple_goldens.py
simple_two_tower.py imports gensim.downloader, datasets and tqdm at module level but only
dereferences them inside main(); stub modules satisfy the imports (the gensim stubs are
oracle.gen_goldens.import_reference's). The fixture is data (inputs + expected outputs); no
reference source is restated: the model, the loss, AdamW and clip_grad_norm_ are the
reference's / torch's own.

Run A  SimpleTwoTower(16, 16), B 24, T 7, two alternating batches, model seed 6, every
       dropout off, 5 steps of simple_two_tower.py:233-240 (symmetric InfoNCE(0.1),
       clip_grad_norm_(1.0), AdamW(lr 1e-4, weight_decay 0.01)): initial weights, batches,
       per-step losses and pre-clip norms, step-0 gradients, final weights.
Run B  (E 32, H 64, B 48, T 10), weights and inputs rounded to bf16, one forward and
       backward: inputs, weights, loss, gradients. To keep the file small the bf16-valued
       weights and inputs are stored as their 16 bits (uint16: exact) and each gradient
       as float16 of g / max|g| with the scale beside it (relative rounding 5e-4, far
       inside the cosine bound the test checks). Run B has its own file because the
       two runs together do not fit the 1 MiB limit on a committed file.
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


def import_simple_reference():
    gen_goldens.import_reference()  # gensim stubs + the reference on sys.path
    for name, attrs in (("datasets", ("load_dataset",)), ("tqdm", ("tqdm",))):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, None)
            sys.modules[name] = mod
    gd = sys.modules["gensim.downloader"]
    if not hasattr(gd, "load"):
        gd.load = None
    import simple_two_tower as st  # noqa: E402
    return st


def bf16_bits(t):
    """A bf16-valued fp32 tensor as its upper 16 bits (exact)."""
    a = t.detach().contiguous().numpy().view(np.uint32)
    assert not (a & 0xFFFF).any()
    return (a >> 16).astype(np.uint16)


def dropout_off(model):
    model.query_encoder.dropout = 0.0  # nn.GRU reads the attribute at call time
    model.doc_encoder.dropout = 0.0
    model.query_proj[3].p = 0.0
    model.doc_proj[3].p = 0.0


def run_a(st, dtype=torch.float32):
    torch.manual_seed(6)
    model = st.SimpleTwoTower(16, 16).to(dtype)  # train mode, as simple_two_tower.main leaves it
    dropout_off(model)
    init = gen_goldens.sd_arrays("a.w0.", model.state_dict())
    g = torch.Generator().manual_seed(21)
    batches = [(torch.randn(24, 7, 16, generator=g), torch.randn(24, 7, 16, generator=g)) for _ in range(2)]
    criterion = st.InfoNCELoss(temperature=0.1)
    optimizer = torch.optim.AdamW(model.parameters(), lr=0.0001, weight_decay=0.01)
    losses, norms, one_dir, grads0 = [], [], [], {}
    for s in range(5):  # simple_two_tower.py:233-240
        q, d = batches[s % 2]
        optimizer.zero_grad()
        query_vec, doc_vec = model(q.to(dtype), d.to(dtype))
        loss = criterion(query_vec, doc_vec)
        loss.backward()
        if s == 0:
            grads0 = {f"a.g0.{k}": p.grad.detach().float().numpy().copy() for k, p in model.named_parameters()}
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        optimizer.step()
        losses.append(loss.item())
        norms.append(float(norm))
        with torch.no_grad():  # the one-directional loss, to show the test can tell them apart
            sim = query_vec @ doc_vec.t() / 0.1
            one_dir.append(torch.nn.functional.cross_entropy(sim, torch.arange(len(sim))).item())
    final = gen_goldens.sd_arrays("a.w5.", model.state_dict())
    return init, batches, np.array(losses), np.array(norms), np.array(one_dir), grads0, final


def gen(st):
    init, batches, losses, norms, one_dir, grads0, final = run_a(st)
    assert (norms > 1.0).all(), norms  # the clip is active at every step
    # the one-directional loss is far outside the tests' 1e-4: they can tell the two apart
    assert (np.abs(one_dir - losses) > 0.03 * np.abs(losses)).all(), (one_dir, losses)
    _, _, l64, n64, _, _, f64 = run_a(st, torch.float64)
    print("run A norms", norms)
    print("run A fp32 vs float64: losses", float(np.abs(losses - l64).max() / np.abs(l64).max()), "weights",
          max(float(np.abs(final[k] - f64[k]).max() / (np.abs(f64[k]).max() + 1e-12)) for k in final))
    out = dict(init)
    out.update(final)
    out.update(grads0)
    out["a.losses"] = losses.astype(np.float32)
    out["a.norms"] = norms.astype(np.float32)
    out["a.bq"] = np.stack([b[0].numpy() for b in batches])
    out["a.bd"] = np.stack([b[1].numpy() for b in batches])
    path = os.path.join(OUT, "simple_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    out = {}

    E, H, B, T = 32, 64, 48, 10
    torch.manual_seed(7)
    model = st.SimpleTwoTower(E, H)
    dropout_off(model)
    with torch.no_grad():
        for prm in model.parameters():
            prm.copy_(prm.to(torch.bfloat16).float())
    g = torch.Generator().manual_seed(22)
    q = torch.randn(B, T, E, generator=g).to(torch.bfloat16).float()
    d = torch.randn(B, T, E, generator=g).to(torch.bfloat16).float()
    out.update({f"b.w.{k}": bf16_bits(v) for k, v in model.state_dict().items()})
    loss = st.InfoNCELoss(temperature=0.1)(*model(q, d))
    loss.backward()
    out["b.q"], out["b.d"] = bf16_bits(q), bf16_bits(d)
    out["b.loss"] = np.float32(loss.item())
    for k, p in model.named_parameters():
        scale = float(p.grad.abs().max())
        out[f"b.gs.{k}"] = np.float32(scale)
        out[f"b.g.{k}"] = (p.grad / scale).numpy().astype(np.float16)
    path = os.path.join(OUT, "simple_tiny_b.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen(import_simple_reference())
