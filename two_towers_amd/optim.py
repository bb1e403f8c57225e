"""Adam for the inner loop of train_enhanced.py:43,63 as one multi-tensor HIP launch.

Same hyper-parameters and update formula as torch.optim.Adam (non-amsgrad,
non-maximize); state lives in fp32 tensors per parameter ('exp_avg', 'exp_avg_sq',
'step' like torch, so optimizer.state_dict() keeps torch's structure).

AdamW (simple_two_tower.py:193) is the same step with decoupled weight decay
(tt_adamw_multi); clip_grad_norm_ (simple_two_tower.py:239) is torch's rule in three
launches for up to 48 gradients, the norm staying on the device.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ops, towers
from ._lib import call, stream_ptr
from .embedding import table_of

_MAXT = 48


class Adam(torch.optim.Optimizer):
    _KERNEL = "tt_adam_multi"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._guard_reads = []  # (event, pinned int32[1] copy of the guard, params) per earlier launch

    def settle_skipped_steps(self):
        """Take every earlier step that the device skipped (its step guard was set) off the
        step counters of the parameters it covered, so Adam's bias correction counts applied
        updates only. Called by step(); waits for the earlier steps' launches (the host is
        normally a whole forward and backward ahead of them, so this rarely blocks)."""
        reads, self._guard_reads = self._guard_reads, []
        for ev, word, plist in reads:
            ev.synchronize()
            if int(word.item()) != 0:
                for p in plist:
                    self.state[p]["step"] -= 1

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.settle_skipped_steps()
        stepped = {}  # device -> parameters launched this step
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            _lib.require_gpu(*ps)
            b1, b2 = group["betas"]
            # torch keeps one step counter per parameter; parameters stepped together share it
            buckets = {}
            for p in ps:
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise _lib.TTError("two_towers_amd Adam expects contiguous fp32 parameters and gradients")
                st["step"] += 1
                buckets.setdefault(int(st["step"].item()), []).append(p)
            # the device's step guard: non-zero when a column-split GRU forward since the
            # last step timed out (towers.watch_gru_status); the kernel then changes nothing
            dev = ps[0].device
            guard = towers.step_guard(dev)
            for step, plist in buckets.items():
                for i in range(0, len(plist), _MAXT):
                    chunk = plist[i:i + _MAXT]
                    n = len(chunk)
                    arr = lambda xs: (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
                    sizes = (ctypes.c_long * n)(*[p.numel() for p in chunk])
                    call(self._KERNEL, arr(chunk), arr([p.grad for p in chunk]),
                         arr([self.state[p]["exp_avg"] for p in chunk]),
                         arr([self.state[p]["exp_avg_sq"] for p in chunk]), sizes, n, group["lr"], b1, b2,
                         group["eps"], group["weight_decay"], step, guard.data_ptr(), stream_ptr(dev))
            # the kernel writes through raw pointers: record the in-place update for autograd
            # and for the packed-weight cache of the towers (towers._packed)
            torch.autograd.graph.increment_version(ps)
            stepped.setdefault(dev, []).extend(ps)
        for dev, plist in stepped.items():
            g = towers.step_guard(dev)
            with torch.cuda.device(dev):
                word = torch.zeros(1, dtype=torch.int32, pin_memory=True)
                word.copy_(g, non_blocking=True)  # did the device skip this step? (settle_skipped_steps)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                g.zero_()  # stream-ordered after every launch above
            self._guard_reads.append((ev, word, plist))
        return loss


class AdamW(Adam):
    """torch.optim.AdamW's defaults and update (decoupled weight decay: p *= 1 - lr * wd
    before the Adam update, the gradient untouched); everything else is Adam's step."""
    _KERNEL = "tt_adamw_multi"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class SparseAdam(torch.optim.Optimizer):
    """torch.optim.SparseAdam on the rows of an EmbeddingTable that the step's batch touched
    (tt_sparse_adam_rows): the same update formula and state keys ('step', 'exp_avg',
    'exp_avg_sq'), moments of untouched rows left alone. The gradient must be sparse (what
    the towers' backward leaves in table.weight.grad). The table's compute-dtype copy is
    rewritten row by row in the same launch, so no full rebuild follows the step.

    The device step guard (towers.step_guard) is honoured as by Adam: a step fed by a
    timed-out forward changes nothing and is taken off the step counter at the next step().
    Unlike Adam, this optimiser leaves the guard set: in an iteration that also steps the
    model's Adam, step this one first, and Adam's launch then reads the same word before
    Adam clears it (alone, the guard is cleared by the forward after the host has been told
    of the timeout, towers.reset_guard_if_reported)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("invalid SparseAdam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._guard_reads = []

    settle_skipped_steps = Adam.settle_skipped_steps

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.settle_skipped_steps()
        stepped = {}
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not g.is_sparse:
                    raise _lib.TTError("two_towers_amd SparseAdam expects a sparse gradient (an EmbeddingTable "
                                       "weight after backward); use two_towers_amd.Adam for dense gradients")
                _lib.require_gpu(p, g)
                if p.dtype != torch.float32 or p.dim() != 2 or not p.is_contiguous():
                    raise _lib.TTError("two_towers_amd SparseAdam expects a contiguous fp32 [V, E] parameter")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                g = g if g.is_coalesced() else g.coalesce()  # the update is non-linear: ids must be distinct
                ids = g._indices()[0].to(torch.int32).contiguous()
                vals = g._values().to(torch.float32).contiguous()
                table = table_of(p)
                copy = table.current_copy() if table is not None else None
                dev = p.device
                with torch.cuda.device(dev):
                    ops.sparse_adam_rows(p, st["exp_avg"], st["exp_avg_sq"], ids, vals, copy, lr=group["lr"], beta1=b1,
                                         beta2=b2, eps=group["eps"], step=int(st["step"].item()),
                                         guard=towers.step_guard(dev))
                # the kernel writes through raw pointers: record the in-place update, then mark
                # the compute copy as standing for the new version (its rows were rewritten)
                torch.autograd.graph.increment_version(p)
                if copy is not None:
                    table.copy_updated()
                stepped.setdefault(dev, []).append(p)
        for dev, plist in stepped.items():
            gd = towers.step_guard(dev)
            with torch.cuda.device(dev):
                word = torch.zeros(1, dtype=torch.int32, pin_memory=True)
                word.copy_(gd, non_blocking=True)  # did the device skip this step? (settle_skipped_steps)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
            self._guard_reads.append((ev, word, plist))
        return loss


def _dense_views(grads):
    """Sparse gradients stand in the norm and the scaling through their values tensor: the
    sum of squares of a coalesced gradient's values is that of the dense gradient."""
    out = []
    for g in grads:
        if g.is_sparse:
            if not g.is_coalesced():
                raise _lib.TTError("two_towers_amd clip_grad_norm_ expects coalesced sparse gradients")
            g = g._values()
        out.append(g)
    return out


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (2-norm, error_if_nonfinite
    False) on the device: the squared norm of every gradient (tt_grad_norm_multi), then
    g *= min(1, max_norm / (norm + 1e-6)) (tt_clip_scale_multi). Returns the total norm as
    a device tensor; nothing waits on the host. Gradients must be contiguous fp32; a
    coalesced sparse gradient (EmbeddingTable) counts, and is scaled, through its values."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = _dense_views([p.grad for p in parameters if p.grad is not None])
    if not grads:
        return torch.zeros(())
    _lib.require_gpu(*grads)
    dev = grads[0].device
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev:
            raise _lib.TTError("two_towers_amd clip_grad_norm_ expects contiguous fp32 gradients on one device")
    lib = _lib.load()
    st = stream_ptr(dev)
    sumsq = torch.empty(1, dtype=torch.float32, device=dev)
    total = torch.empty((), dtype=torch.float32, device=dev)
    chunks = [grads[i:i + _MAXT] for i in range(0, len(grads), _MAXT)]
    args = []
    for chunk in chunks:
        n = len(chunk)
        args.append(((ctypes.c_void_p * n)(*[g.data_ptr() for g in chunk]),
                     (ctypes.c_long * n)(*[g.numel() for g in chunk]), n))
    for i, (ptrs, sizes, n) in enumerate(args):
        ws = torch.empty(lib.tt_grad_norm_ws_size(sizes, n), dtype=torch.uint8, device=dev)
        call("tt_grad_norm_multi", ptrs, sizes, n, int(i > 0), sumsq.data_ptr(), ws.data_ptr(), st)
    for ptrs, sizes, n in args:
        call("tt_clip_scale_multi", ptrs, sizes, n, sumsq.data_ptr(), float(max_norm), total.data_ptr(), st)
    torch.autograd.graph.increment_version(grads)
    return total
