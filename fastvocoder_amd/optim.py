"""``Adam``: torch.optim.Adam with gradient clipping folded in, as three HIP launches for the whole parameter set
(csrc/optim.hip; the reference's loop runs ``clip_grad_norm_`` and ``Adam.step()``, bin/train.py:126-136, and names the
fused form itself, apex.optimizers.FusedAdam, train.py:338).

The constructor, the param groups and the per-parameter state (``step`` a CPU fp32 scalar tensor, ``exp_avg``,
``exp_avg_sq``) are torch.optim.Adam's, so ``state_dict()`` / ``load_state_dict()`` interchange with it in both
directions and a reference checkpoint's ``'optimizer'`` entry loads.  What the kernels do not do is refused when the
optimizer is built: ``amsgrad``, ``weight_decay != 0``, ``maximize``, ``capturable``, ``differentiable``, ``fused``,
and parameters that are not contiguous fp32 tensors.

``step(max_norm=None)``: with ``max_norm`` the gradients of ALL groups are clipped to that total 2-norm first
(``clip_grad_norm_``'s semantics: scaled by ``min(1, max_norm / (norm + 1e-6))``, and ``.grad`` holds the scaled
values afterwards) and the norm comes back as a 0-d device tensor; the factor stays on the device, so nothing is read
on the host.  Parameters whose ``.grad`` is None are skipped: their state and their step count do not move.

The table the kernels walk (pointers, element counts, ``lr / bias_correction1`` and ``1 / sqrt(bias_correction2)`` per
tensor, and the chunks) is rebuilt on the host every step -- ``zero_grad(set_to_none=True)`` moves the ``.grad``
pointers -- and uploaded with one asynchronous copy from pinned memory; a pinned buffer is reused only once the copy
that read it has completed (an event per buffer, queried, never waited for).

Data-parallel training: ``step(max_norm=None, process_group=<a torch.distributed group>)`` averages the gradients over
the group's ranks first, with ONE collective.  Every parameter that ``requires_grad``, of every group, in optimizer
order, owns a span of one flat fp32 bucket (``bucket_layout``: 16-byte-aligned offsets, spans padded to 4 floats; the
layout is static and the bucket is allocated once per optimizer).  One launch (``fv_grad_bucket_pack``) writes
``grad / world`` into every span -- and zeros into the padding and into the span of a parameter without a local
gradient --, ``parallel.all_reduce_sum`` adds the buckets of the ranks in place, and the norm and Adam launches above
run over rows whose gradient pointer is the span; the source pointers ride in the same pinned upload as the table.
Afterwards ``p.grad`` IS the parameter's view into the bucket: it holds the averaged (and, with ``max_norm``, clipped)
gradient, and the next step overwrites it -- clone it to keep it.  Unlike the single-process rule, a parameter that
requires grad but has no local ``.grad`` is NOT skipped: it contributes zeros, its step count advances and it is
updated like the rest, so that every rank sends the same number of words and applies the same update whatever its
shard of the batch touched, and no rank waits for another.  A group of one rank takes the same path.  Learning rates
are not rescaled by the world size.  Nothing is read on the host (under ``nccl``; a ``gloo`` group stages the bucket
through pinned host memory, parallel.all_reduce_sum).
"""
import math

import numpy as np
import torch

import torch.distributed

from . import _native, parallel

ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"),
                ("inv_sqrt_bc2", "<f4")])
CHUNK = np.dtype([("tensor", "<i4"), ("index", "<i4")])
BUCKET_ALIGN = 4        # floats: every span of the gradient bucket starts on a 16-byte boundary
assert ROW.itemsize == _native.ADAM_ROW_BYTES and CHUNK.itemsize == _native.ADAM_CHUNK_BYTES


def bias_factors(lr, beta1, beta2, step):
    """(step_size, inv_sqrt_bc2) of a tensor at ``step`` (>= 1): lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step)."""
    return lr / (1.0 - beta1 ** step), 1.0 / math.sqrt(1.0 - beta2 ** step)


def bucket_layout(params):
    """Where the gradients of ``params`` (in this order; those with ``requires_grad=False`` are left out) live in the
    flat bucket -> (offset of each in floats, total floats).  Every offset is a multiple of 4 floats (16 bytes) and a
    span is the element count rounded up to 4 floats, so spans never overlap.  Pure host arithmetic."""
    offsets, total = [], 0
    for p in params:
        if not p.requires_grad:
            continue
        offsets.append(total)
        total += (p.numel() + BUCKET_ALIGN - 1) // BUCKET_ALIGN * BUCKET_ALIGN
    return offsets, total


def adam_table(rows, src=None):
    """rows: [(p_ptr, g_ptr, m_ptr, v_ptr, n, step_size, inv_sqrt_bc2)] -> (bytes of the table as a uint8 ndarray,
    first chunk of every row + the total).  Layout: the fv_adam_tensor rows, then row 0's chunks, row 1's, ...; with
    ``src`` (one pointer per row: fv_grad_bucket_pack's sources, 0 for none) those follow as uint64."""
    table = np.zeros(len(rows), dtype=ROW)
    for k, name in enumerate(ROW.names):
        table[name] = [r[k] for r in rows]
    counts = (table["n"] + _native.ADAM_CHUNK - 1) // _native.ADAM_CHUNK
    first = np.concatenate(([0], np.cumsum(counts)))
    chunks = np.zeros(int(first[-1]), dtype=CHUNK)
    chunks["tensor"] = np.repeat(np.arange(len(rows), dtype=np.int32), counts)
    chunks["index"] = np.arange(int(first[-1]), dtype=np.int64) - np.repeat(first[:-1], counts)
    parts = (table.view(np.uint8), chunks.view(np.uint8))
    if src is not None:
        if len(src) != len(rows):
            raise ValueError(f"{len(src)} source pointers for {len(rows)} rows")
        parts += (np.asarray(src, dtype="<u8").view(np.uint8),)
    return np.concatenate(parts), first


def _check_group(group):
    for key, why in (("amsgrad", "the max of the second moments is not kept"),
                     ("maximize", "the kernels descend"),
                     ("capturable", "the step count lives on the host"),
                     ("differentiable", "the update is not on the autograd graph"),
                     ("fused", "this optimizer is its own fused form")):
        if group.get(key):
            raise ValueError(f"fastvocoder_amd.optim.Adam does not support {key}=True ({why}); use torch.optim.Adam")
    if group.get("weight_decay", 0) != 0:
        raise ValueError(f"fastvocoder_amd.optim.Adam does not support weight_decay={group['weight_decay']} (the "
                         "reference trains with 0); use torch.optim.Adam")
    if torch.is_tensor(group["lr"]):
        raise ValueError("fastvocoder_amd.optim.Adam takes lr as a float (a tensor lr would be read on the host "
                         "every step)")
    for p in group["params"]:
        if p.dtype != torch.float32:
            raise ValueError(f"fastvocoder_amd.optim.Adam updates fp32 parameters, got {p.dtype} "
                             f"(shape {tuple(p.shape)})")
        if not p.is_contiguous():
            raise ValueError(f"fastvocoder_amd.optim.Adam updates contiguous parameters, got strides {p.stride()} for "
                             f"shape {tuple(p.shape)}")


class Adam(torch.optim.Adam):
    def __init__(self, params, *args, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._pinned = []           # [(pinned uint8 tensor, event of the copy that last read it)]
        self._workspace = None      # fp32 device words: the per-chunk partial sums of the norm
        self._bucket = None         # (key, flat fp32 device tensor, {parameter: its view}) of the data-parallel step

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        _check_group(self.param_groups[-1])

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_pinned", [])
        self.__dict__.setdefault("_workspace", None)
        self.__dict__.setdefault("_bucket", None)
        for group in self.param_groups:
            _check_group(group)
        for state in self.state.values():       # a checkpoint loaded with map_location=<device> carries the counts there
            step = state.get("step")
            if torch.is_tensor(step) and (step.device.type != "cpu" or step.dtype != torch.float32):
                state["step"] = step.detach().to("cpu", torch.float32)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            _check_group(group)

    def _state_of(self, p):
        state = self.state[p]
        if len(state) == 0:         # torch.optim.Adam._init_group
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    def _rows(self):
        """The table rows of the parameters that have a gradient (their step counts advanced), the chunk range of
        every group, and the tensors whose contents the launches change."""
        rows, touched, spans, device = [], [], [], None
        at = 0
        for group in self.param_groups:
            _check_group(group)
            beta1, beta2 = group["betas"]
            lr = float(group["lr"])
            begin = at
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("fastvocoder_amd.optim.Adam does not support sparse gradients")
                if not p.is_cuda:
                    raise _native.NativeError(f"a parameter lives on {p.device}; the HIP kernels need a ROCm device "
                                              "tensor (there is no CPU path in fastvocoder_amd)")
                device = p.device if device is None else device
                state = self._state_of(p)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for t, name in ((g, "gradient"), (m, "exp_avg"), (v, "exp_avg_sq")):
                    if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape or t.device != device:
                        raise _native.NativeError(
                            f"the {name} of a parameter of shape {tuple(p.shape)} on {device} must be a contiguous "
                            f"fp32 tensor of that shape there, got {t.dtype} {tuple(t.shape)} on {t.device} "
                            f"contiguous={t.is_contiguous()}")
                if p.numel() == 0:
                    continue
                rows.append((p, g, m, v, state, lr, beta1, beta2))
                at += 1
            spans.append((begin, at, beta1, beta2, group["eps"]))
        for k, (p, g, m, v, state, lr, beta1, beta2) in enumerate(rows):     # every check has passed: advance
            state["step"] += 1
            step = float(state["step"])             # a CPU tensor: no device read
            rows[k] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) \
                + bias_factors(lr, beta1, beta2, step)
            touched += [p, g, m, v]
        return rows, touched, spans, device

    def _bucket_views(self):
        """(the flat bucket, the view of every parameter that requires grad); allocated once, again only when the
        parameter set or its device changes."""
        params = [p for group in self.param_groups for p in group["params"] if p.requires_grad]
        for p in params:
            if not p.is_cuda:
                raise _native.NativeError(f"a parameter lives on {p.device}; the HIP kernels need a ROCm device "
                                          "tensor (there is no CPU path in fastvocoder_amd)")
        if not params:
            return None, {}
        device = params[0].device
        key = (device, tuple((id(p), p.numel()) for p in params))
        if self._bucket is None or self._bucket[0] != key:
            offsets, total = bucket_layout(params)
            flat = torch.zeros(max(total, BUCKET_ALIGN), dtype=torch.float32, device=device)
            views = {p: flat[off:off + p.numel()].view(p.shape) for p, off in zip(params, offsets)}
            self._bucket = (key, flat, views)
        return self._bucket[1], self._bucket[2]

    def _rows_bucket(self):
        """``_rows`` for the data-parallel step: a row for EVERY parameter that requires grad, its gradient pointer
        the parameter's span of the bucket; also the source pointers (0: no local gradient) and the views."""
        flat, views = self._bucket_views()
        rows, touched, spans, src = [], [], [], []
        device = None if flat is None else flat.device
        at = 0
        for group in self.param_groups:
            _check_group(group)
            beta1, beta2 = group["betas"]
            lr = float(group["lr"])
            begin = at
            for p in group["params"]:
                if not p.requires_grad:
                    continue
                g = p.grad
                if g is not None and g.is_sparse:
                    raise RuntimeError("fastvocoder_amd.optim.Adam does not support sparse gradients")
                state = self._state_of(p)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for t, name in ((g, "gradient"), (m, "exp_avg"), (v, "exp_avg_sq")):
                    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape
                                          or t.device != device):
                        raise _native.NativeError(
                            f"the {name} of a parameter of shape {tuple(p.shape)} on {device} must be a contiguous "
                            f"fp32 tensor of that shape there, got {t.dtype} {tuple(t.shape)} on {t.device} "
                            f"contiguous={t.is_contiguous()}")
                if p.numel() == 0:
                    continue
                rows.append((p, views[p], m, v, state, lr, beta1, beta2))
                src.append(0 if g is None else g.data_ptr())
                at += 1
            spans.append((begin, at, beta1, beta2, group["eps"]))
        for k, (p, g, m, v, state, lr, beta1, beta2) in enumerate(rows):     # every check has passed: advance
            state["step"] += 1
            step = float(state["step"])
            rows[k] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) \
                + bias_factors(lr, beta1, beta2, step)
            touched += [p, g, m, v]
        return rows, touched, spans, device, src, flat, views

    def _upload(self, host, device):
        """The table on ``device``: one asynchronous copy from a pinned buffer no earlier copy may still be reading."""
        slot = None
        for k, (buf, event) in enumerate(self._pinned):
            if buf.numel() >= host.size and event.query():
                slot = k
                break
        if slot is None:
            cap = max(4096, 1 << int(host.size - 1).bit_length())
            self._pinned.append((torch.empty(cap, dtype=torch.uint8).pin_memory(), None))
            slot = len(self._pinned) - 1
        buf = self._pinned[slot][0]
        buf[:host.size].numpy()[:] = host
        table = torch.empty(host.size, dtype=torch.uint8, device=device)
        table.copy_(buf[:host.size], non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(device))
        self._pinned[slot] = (buf, event)
        return table

    @torch.no_grad()
    def step(self, closure=None, *, max_norm=None, process_group=None):
        """One update of every parameter that has a gradient -> the total gradient norm before clipping as a 0-d device
        tensor, or None without ``max_norm``.  ``closure`` is not supported (the reference's loop has none).

        ``process_group`` (a torch.distributed group, ``torch.distributed.group.WORLD`` for the default one; None:
        this process alone, the path above): the gradients are averaged over the group's ranks first -- pack with
        scale 1 / world into the flat bucket, one all-reduce, then the same launches over the bucket.  Every parameter
        that requires grad is updated, one without a local gradient with the other ranks' mean (it contributes
        zeros); afterwards ``p.grad`` is the parameter's view into the bucket, holding the averaged, clipped gradient
        until the next step overwrites it.  The norm returned is that of the averaged gradient."""
        if closure is not None:
            raise ValueError("fastvocoder_amd.optim.Adam.step takes no closure")
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError(f"max_norm must be a non-negative number, got {max_norm}")
        src = flat = views = None
        if process_group is None:
            rows, touched, spans, device = self._rows()
        else:
            rows, touched, spans, device, src, flat, views = self._rows_bucket()
        if not rows:
            return None
        host, first = adam_table(rows, src)
        n_tensors, n_chunks = len(rows), int(first[-1])
        with torch.cuda.device(device):
            table = self._upload(host, device)
            if process_group is not None:
                world = torch.distributed.get_world_size(process_group)
                _native.grad_bucket_pack(table, n_tensors, n_chunks, float(np.float32(1.0) / np.float32(world)))
                parallel.all_reduce_sum(flat, process_group)
                for p, view in views.items():
                    p.grad = view
            coef = norm = None
            if max_norm is not None:
                need = _native.grad_sq_norm_workspace_floats(n_chunks)
                if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
                    self._workspace = torch.empty(need, dtype=torch.float32, device=device)
                out = torch.empty(2, dtype=torch.float32, device=device)
                _native.grad_sq_norm(table, n_tensors, n_chunks, float(max_norm), self._workspace, out)
                norm, coef = out[0], out[1:]
            for begin, end, beta1, beta2, eps in spans:
                if end > begin:
                    lo, hi = int(first[begin]), int(first[end])
                    _native.adam_step(table, n_tensors, n_chunks, coef, beta1, beta2, eps, lo, hi - lo)
        # the kernels wrote through raw pointers: move the version counters, so that whatever is cached against the
        # parameters (the generators' packed weights, the plans) is rebuilt
        torch.autograd.graph.increment_version(touched)
        return norm
