"""Bucketed gradient all-reduce for the data-parallel learner (one process per GPU, RCCL over xGMI).

The reference (``dist_helper.py:421-431``) all-reduces each of its 394-474 parameter tensors one by one
after backward.  Here every parameter's ``.grad`` is a *view* into a small number of flat buckets.

Backward has ONE launch structure at every world size (the single-rank one): ``torch.autograd.grad``
over all parameters, then one native multi-tensor copy writes every gradient into its bucket slot - no
per-parameter ``AccumulateGrad`` add into zeroed buckets and no per-parameter Python hook.  ``synchronize``
then issues one async RCCL all-reduce per bucket (AVG inside RCCL) back to back and waits for them.

Why not overlap the collectives with backward through per-parameter hooks (round 2's design)?  On this
learner the step is host-issue bound (``profiles/r2dz_*``: ~1,250 launches, host time ~ wall time): ~460
Python hook calls per step are a few ms of host time on EVERY rank, while the whole exposed collective is
small - 132 MB of fp32 gradients on an 8-GPU ring moves 2 x 7/8 x 132 MB per link, about 0.8-1.5 ms at
the 150-300 GB/s an xGMI ring sustains, against a 30-90 ms step.  Buckets default to 32 MB so the copy of
one bucket and the reduction of the previous one pipeline inside RCCL; the whole reduction is two to five
calls.

Two-phase backward (``backward_phased``, multi-rank by default): the step's autograd graph is cut at the encoders'
outputs - downstream modules read detached leaf copies of them (``Model._encode``, ``encoder_boundary`` holds the
(output, leaf) pairs).  Phase 1 differentiates the loss w.r.t. everything downstream of the cut (core LSTM, heads,
critics: ~12 M of the ~31 M parameters) AND the leaves; those parameters' gradients are then final, so their
buckets are copied and their all-reduce is issued right away, and runs on RCCL's stream while phase 2 (the
encoders' backward from every (output, leaf gradient) pair, one autograd call) computes.  No per-parameter hooks: two
``autograd.grad`` calls and one multi-tensor copy per phase.  The buckets are built per phase (phase-1 parameters
first), so no bucket mixes the two.  ``comm_dtype=torch.bfloat16`` sends bf16 on the wire (half the bytes;
averaged by RCCL, converted back into the fp32 buckets).
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch
import torch.distributed as dist

from . import dist as pdist


def copy_into(dst: List[torch.Tensor], src: List[torch.Tensor]):
    """dst[i].copy_(src[i]) for all i: one native multi-tensor launch on the GPU (dtype-converting).  Pairs whose
    strides differ (a channels_last conv-weight gradient into its contiguous bucket view) go through one strided
    multi-tensor launch instead of a ``copy_`` each (25 launches per fp32 step)."""
    if not dst:
        return
    if dst[0].is_cuda:
        from ..ops import native
        C = native.ensure_loaded()
        same, sd, ss, spec = ([], []), [], [], []
        for d, s in zip(dst, src):
            if d.stride() != s.stride() and d.is_contiguous() and 0 < s.dim() <= 4 and s.numel() > 0 and \
                    d.dtype in (torch.float32, torch.bfloat16) and s.dtype in (torch.float32, torch.bfloat16) and \
                    min(s.stride()) >= 0:
                sd.append(d)
                ss.append(s)
                spec += native._view_spec(s, s)
            else:
                same[0].append(d)
                same[1].append(s)
        if same[0]:
            C.multi_copy(*same)
        if sd:
            C.multi_strided_copy(sd, ss, spec)
    else:
        torch._foreach_copy_(dst, src)


def accumulate_into(dst: List[torch.Tensor], src: List[Optional[torch.Tensor]], scale: float = 1.0):
    """dst[i] = (dst[i] + src[i]) * scale for all i, in fp32 (gradient accumulation over micro-batches): the add and
    the multiply are two roundings, a bf16 source is widened exactly.  A source of None adds nothing: its slot only
    takes the scale.  ``dst`` must be fp32 - a partial sum is never kept in bf16.  One native multi-tensor launch on
    the GPU (a second, strided one for the pairs ``copy_into`` sends there); ``torch._foreach_add_`` +
    ``_foreach_mul_`` on the CPU."""
    scale = float(scale)
    if scale == 1.0:      # nothing to do for the slots without a source
        keep = [i for i, s in enumerate(src) if s is not None]
        dst, src = [dst[i] for i in keep], [src[i] for i in keep]
    if not dst:
        return
    for d in dst:
        if d.dtype != torch.float32:
            raise TypeError(f'accumulate_into: fp32 accumulators only, got {d.dtype}')
    if dst[0].is_cuda:
        from ..ops import native
        C = native.ensure_loaded()
        same, sd, ss, spec = ([], []), [], [], []
        for d, s in zip(dst, src):
            if s is not None and d.stride() != s.stride() and d.is_contiguous() and 0 < s.dim() <= 4 and \
                    s.numel() > 0 and s.dtype in (torch.float32, torch.bfloat16) and min(s.stride()) >= 0:
                sd.append(d)
                ss.append(s)
                spec += native._view_spec(s, s)
            else:
                same[0].append(d)
                same[1].append(s)
        if same[0]:
            C.multi_accumulate(same[0], same[1], scale)
        if sd:
            C.multi_strided_accumulate(sd, ss, spec, scale)
    else:
        pairs = [(d, s) for d, s in zip(dst, src) if s is not None]
        if pairs:
            torch._foreach_add_([d for d, _ in pairs], [s if s.dtype == torch.float32 else s.float() for _, s in pairs])
        if scale != 1.0:
            torch._foreach_mul_(dst, scale)


class _Bucket:
    __slots__ = ('params', 'flat', 'ready', 'handle', 'comm')

    def __init__(self, params: List[torch.nn.Parameter], dtype, device):
        self.params = params
        n = sum(p.numel() for p in params)
        self.flat = torch.zeros(n, dtype=dtype, device=device)
        self.ready = 0
        self.handle = None
        self.comm = None


class GradientReducer:
    def __init__(self, params: Iterable[torch.nn.Parameter], bucket_mb: float = 32.0,
                 comm_dtype: Optional[torch.dtype] = None, group=None, overlap: bool = True,
                 phase_of=None):
        self.group = group
        self.world = pdist.get_world_size()
        self.overlap = overlap
        self.comm_dtype = comm_dtype
        self.keep_comm = False  # master-weight mode reads the fp32 reduction directly (reduced())
        params = [p for p in params if p.requires_grad]
        self.params = params
        self.buckets: List[_Bucket] = []
        self._owner = {}
        # phase_of(p) -> 0 (downstream of the encoders: final after backward phase 1) or 1 (the encoders); every
        # parameter in phase 0 without one
        ph = [int(phase_of(p)) if phase_of is not None else 0 for p in params]
        self.phase_params = [[p for p, k in zip(params, ph) if k == i] for i in (0, 1)]
        self.phase_buckets: List[List[_Bucket]] = [[], []]
        # backward visits layers roughly in reverse registration order; parameters of different dtypes
        # (bf16 GEMM weights + fp32 norm affines under master weights) go to separate bucket chains so
        # the interleaving does not fragment the buckets
        limit = int(bucket_mb * 1024 * 1024)
        for phase in (0, 1):
            keys = []
            members = [p for p, k in zip(params, ph) if k == phase]
            for p in reversed(members):
                if (p.dtype, p.device) not in keys:
                    keys.append((p.dtype, p.device))
            for key in keys:
                cur, cur_bytes = [], 0
                for p in reversed(members):
                    if (p.dtype, p.device) != key:
                        continue
                    if cur and cur_bytes + p.numel() * p.element_size() > limit:
                        self.phase_buckets[phase].append(self._add_bucket(cur))
                        cur, cur_bytes = [], 0
                    cur.append(p)
                    cur_bytes += p.numel() * p.element_size()
                if cur:
                    self.phase_buckets[phase].append(self._add_bucket(cur))
        self._hooks = []
        # called with (params, autograd's gradients) before they are copied into the buckets (the deferred weight
        # gradients' check, ops/native.py defer_verify)
        self.grad_hook = None
        self.use_avg = self.world > 1 and dist.get_backend(group) == 'nccl'

    def _add_bucket(self, params):
        b = _Bucket(params, params[0].dtype, params[0].device)
        off = 0
        for p in params:
            n = p.numel()
            # same strides as the parameter (channels_last conv weights) so fused optimizers that walk
            # param and grad storage in lockstep see matching elements
            p.grad = b.flat[off:off + n].as_strided(p.shape, p.stride())
            self._owner[p] = b
            off += n
        self.buckets.append(b)
        return b

    @property
    def num_buckets(self) -> int:
        return len(self.buckets)

    def _launch(self, b: _Bucket):
        if b.handle is not None or self.world == 1:
            return
        buf = b.flat
        comm_dtype = self.comm_dtype
        if comm_dtype is None and buf.dtype == torch.bfloat16 and self.keep_comm:
            comm_dtype = torch.float32  # bf16 gradients are summed across ranks in fp32
        if comm_dtype is not None and comm_dtype != buf.dtype:
            b.comm = buf.to(comm_dtype)
            buf = b.comm
        op = dist.ReduceOp.AVG if self.use_avg else dist.ReduceOp.SUM
        b.handle = dist.all_reduce(buf, op=op, group=self.group, async_op=True)

    def backward(self, loss: torch.Tensor, before_copy=None, accumulate: bool = False, scale: float = 1.0,
                 no_collective: bool = False):
        """Gradients of ``loss`` into the bucket views: ``autograd.grad`` + one multi-tensor copy (native on
        the GPU), at every world size; buckets holding a parameter without a gradient are zeroed first.
        ``before_copy``: called between autograd and the copy (the deferred weight gradients join there).
        ``accumulate``: micro-batch 2..k of an accumulation window - the copy becomes ``(bucket + g) * scale``
        (:func:`accumulate_into`; ``scale`` is 1 until the window's last micro-batch, then 1/k) and nothing is
        zeroed.  ``no_collective`` (every micro-batch but the last) only matters to ``backward_phased``."""
        grads = torch.autograd.grad(loss, self.params, allow_unused=True)
        if before_copy is not None:
            before_copy()
        self._store(self.params, grads, self.buckets, accumulate, scale)

    def _store(self, params, grads, buckets, accumulate: bool = False, scale: float = 1.0):
        if self.grad_hook is not None:
            self.grad_hook(params, grads)
        if accumulate:
            # a parameter without a gradient in this micro-batch adds nothing (its slot keeps the earlier sum, nothing
            # is zeroed); the window's closing scale still reaches every slot, in the same launch
            accumulate_into([p.grad for p in params], list(grads), scale)
            return
        dst, src = [], []
        stale = set()
        for p, g in zip(params, grads):
            if g is not None:
                dst.append(p.grad)
                src.append(g)
            else:
                stale.add(id(self._owner[p]))
        for b in buckets:
            if id(b) in stale:
                b.flat.zero_()
        copy_into(dst, src)

    def backward_phased(self, loss: torch.Tensor, boundary, before_copy=None, accumulate: bool = False,
                        scale: float = 1.0, no_collective: bool = False):
        """Two-phase backward (module docstring): phase 1 = the loss w.r.t. the phase-0 parameters and the
        boundary leaves; their buckets are filled and (multi-rank) their all-reduce issued; phase 2 = the encoder
        outputs, with the leaves' gradients, w.r.t. the phase-1 parameters.  ``boundary``: the (encoder output,
        leaf) pairs of ``Model.encoder_boundary``.  ``before_copy`` runs before the first copy.  ``accumulate`` /
        ``scale``: as in :meth:`backward`; ``no_collective``: the early all-reduce is not issued (the buckets
        hold a partial sum until the window's last micro-batch)."""
        p0, p1 = self.phase_params
        outs, leaves = [o for o, _ in boundary], [lf for _, lf in boundary]
        g = torch.autograd.grad(loss, p0 + leaves, allow_unused=True)
        if before_copy is not None:
            before_copy()
        self._store(p0, g[:len(p0)], self.phase_buckets[0], accumulate, scale)
        if not no_collective:
            for b in self.phase_buckets[0]:
                self._launch(b)               # RCCL's stream, beside the encoders' backward below
        roots = [(t, gt) for t, gt in zip(outs, g[len(p0):]) if gt is not None]
        if roots and p1:
            g2 = torch.autograd.grad([t for t, _ in roots], p1, grad_outputs=[gt for _, gt in roots],
                                     allow_unused=True)
        else:
            g2 = [None] * len(p1)
        self._store(p1, g2, self.phase_buckets[1], accumulate, scale)

    def zero_grad(self, buffers: bool = True):
        """Reset the per-step state; ``buffers=False`` leaves the bucket memory alone (``backward`` overwrites
        every slot, zeroing the buckets of unused parameters itself)."""
        for b in self.buckets:
            if buffers:
                b.flat.zero_()
            b.ready = 0
            b.handle = None
            b.comm = None
        for p in self.params:  # re-attach in case someone set grads to None
            if p.grad is None or p.grad.data_ptr() == 0:
                raise RuntimeError('gradient view detached from its bucket; use GradientReducer.zero_grad()')

    def synchronize(self):
        if self.world == 1:
            return
        for b in self.buckets:
            self._launch(b)  # buckets with unused params (or overlap disabled) go now
        for b in self.buckets:
            b.handle.wait()
            if b.comm is not None:
                if not self.use_avg:
                    b.comm.div_(self.world)
                if not self.keep_comm:
                    b.flat.copy_(b.comm)
            elif not self.use_avg:
                b.flat.div_(self.world)
            b.handle = None

    def reduced(self, b: _Bucket) -> torch.Tensor:
        """The bucket's averaged gradient (the fp32 communication copy when one was used)."""
        return b.comm if b.comm is not None else b.flat

    def remove(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []
