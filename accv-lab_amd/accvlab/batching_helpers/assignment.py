"""(extension) Batched linear sum assignment — the Hungarian matching of DETR-style heads on ragged cost matrices, without
the round trip of the reference's matcher (packages/batching_helpers/example/matcher.py:52-74: ``cost.to_device(cpu)``,
``split``, ``scipy.optimize.linear_sum_assignment`` per frame, ``combine_data``, copy back).

GPU tensors run one HIP launch (``accv_linear_assignment``, one workgroup per frame); CPU tensors run the host
implementation of the same algorithm (``accv_linear_assignment_host``), which gives the same bits.  There is no CPU
fallback for GPU tensors.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from .data_format import RaggedBatch

__all__ = ["batched_linear_sum_assignment"]

_DTYPES = _nat.FLOAT_DTYPE_CODES
MAX_LARGE = 4096   # max(R, C) of the padded shape
MAX_SMALL = 1024   # min(R, C) of the padded shape
_MSG = {1: "cost matrix is infeasible", 2: "matrix contains invalid numeric entries"}   # scipy's texts
_THREADS = {None: 0, 256: 0, 64: _nat.LSA_THREADS_64, 1024: _nat.LSA_THREADS_1024}


def _counts(sizes: torch.Tensor, device) -> torch.Tensor:
    return sizes.to(device=device, dtype=torch.int64).contiguous()


def batched_linear_sum_assignment(cost, *, maximize: bool = False, check: bool = True, _threads: Optional[int] = None):
    """Per-frame ``scipy.optimize.linear_sum_assignment`` of a batch of (ragged) cost matrices.

    Args:
        cost: one of
            - a ``RaggedBatch`` ``[B, R, C_max]`` with ``non_uniform_dim=2`` (frame b is ``cost[b, :, :C_b]``, the padded
              columns are never read) — what the matcher builds;
            - a ``RaggedBatch`` ``[B, R_max, C]`` with ``non_uniform_dim=1`` (padded rows);
            - a dense ``[B, R, C]`` tensor (every frame full);
            - a ``[R, C]`` tensor: one frame, returned as plain tensors like scipy.
            float32 / float64 / float16 / bfloat16 (the latter two are widened); any strides.  Read only; no gradient.
        maximize: maximum-cost matching instead of minimum-cost.
        check: ``True`` reads the per-frame status back (one small synchronisation) and raises ``ValueError`` with scipy's
            message for an infeasible frame or one with invalid entries.  ``False`` never synchronises (the call can be
            captured in a graph) and also returns the status.
        _threads: lanes per frame of the GPU launch, 64, 256 (default) or 1024 — a tuning hint for benchmarks; the
            results do not depend on it.

    Semantics per frame (scipy's): a complete matching of the smaller side of least (greatest) total cost; ``+inf``
    (``-inf`` under ``maximize``) forbids a pair; NaN and ``-inf`` (``+inf`` under ``maximize``) are invalid.  Exact:
    costs are widened to float64 and the solver keeps its duals in float64.  Equal-cost alternatives are broken by a
    fixed rule, so results are bitwise reproducible, and the GPU and CPU solvers agree bit for bit.

    Limits: ``max(R, C) <= 4096`` and ``min(R, C) <= 1024`` of the padded shape; larger inputs raise ``ValueError``.

    Returns:
        ``(row_ind, col_ind)`` (``check=True``) or ``(row_ind, col_ind, status)`` (``check=False``).  For batched input
        ``row_ind`` / ``col_ind`` are int64 RaggedBatches ``[B, min(R, C_max)]`` sharing their sample sizes
        (``min(R_b, C_b)``, computed on the device, 0 for a failed frame) and mask; ``row_ind`` ascends and
        ``cost[b, row_ind, col_ind]`` are the chosen pairs; padded entries are 0.  ``status`` is int32 ``[B]`` on the
        device: 0 ok, 1 infeasible, 2 invalid entry.  For a 2-D ``cost``: int64 tensors of length ``min(R, C)`` (and a
        0-d status; with ``check=False`` the indices of a failed frame are zeros).
    """
    row_counts = col_counts = None
    single = False
    if isinstance(cost, RaggedBatch):
        if cost.num_batch_dims != 1 or cost.tensor.dim() != 3 or cost.non_uniform_dim not in (1, 2):
            raise ValueError("batched_linear_sum_assignment: a RaggedBatch cost must be [B, R, C] with one batch "
                             f"dimension and non_uniform_dim 1 or 2, got shape {tuple(cost.tensor.shape)}, "
                             f"non_uniform_dim {cost.non_uniform_dim}")
        x = cost.tensor
        if cost.non_uniform_dim == 2:
            col_counts = _counts(cost.sample_sizes, x.device)
        else:
            row_counts = _counts(cost.sample_sizes, x.device)
    elif isinstance(cost, torch.Tensor):
        if cost.dim() == 2:
            x, single = cost.unsqueeze(0), True
        elif cost.dim() == 3:
            x = cost
        else:
            raise ValueError(f"batched_linear_sum_assignment: expected a [R, C] or [B, R, C] cost, got {cost.dim()} "
                             "dimensions")
    else:
        raise TypeError(f"batched_linear_sum_assignment: cost must be a tensor or a RaggedBatch, got {type(cost).__name__}")
    if x.dtype not in _DTYPES:
        raise TypeError(f"batched_linear_sum_assignment: cost must be float32, float64, float16 or bfloat16, got {x.dtype}")
    if _threads not in _THREADS:
        raise ValueError(f"batched_linear_sum_assignment: _threads must be 64, 256 or 1024, got {_threads!r}")
    x = x.detach()
    B, R, C = (int(s) for s in x.shape)
    if max(R, C) > MAX_LARGE or min(R, C) > MAX_SMALL:
        raise ValueError(f"batched_linear_sum_assignment: {R} x {C} cost matrices exceed the limit "
                         f"(max(R, C) <= {MAX_LARGE} and min(R, C) <= {MAX_SMALL})")

    dev = x.device
    W = min(R, C)
    row = torch.empty((B, W), dtype=torch.int64, device=dev)
    col = torch.empty((B, W), dtype=torch.int64, device=dev)
    sizes = torch.empty((B,), dtype=torch.int64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    flags = (_nat.LSA_MAXIMIZE if maximize else 0) | _THREADS[_threads]
    if B == 0 or W == 0:
        row.zero_(), col.zero_(), sizes.zero_(), status.zero_()
    else:
        args = (x.data_ptr(), _DTYPES[x.dtype], B, R, C, x.stride(0), x.stride(1), x.stride(2),
                row_counts.data_ptr() if row_counts is not None else 0,
                col_counts.data_ptr() if col_counts is not None else 0, flags,
                row.data_ptr(), col.data_ptr(), sizes.data_ptr(), status.data_ptr())
        if x.is_cuda:   # the device entry takes a workspace behind the host entry's arguments
            ws = _nat.workspace(_nat.lib().accv_linear_assignment_workspace_bytes(B, R, C, _DTYPES[x.dtype]), dev)
            args += (ws.data_ptr(), ws.numel())
        elif dev.type != "cpu":
            raise RuntimeError(f"batched_linear_sum_assignment: unsupported device {dev}")
        _ops.run("accv_linear_assignment", args, dev, "batched_linear_sum_assignment")

    if check:
        st = status.cpu()
        for code in (2, 1):   # scipy validates the entries before it solves
            bad = (st == code).nonzero()
            if bad.numel():
                raise ValueError(_MSG[code] if single else f"{_MSG[code]} (frame {int(bad[0])})")
    if single:
        out = (row[0], col[0])
        return out if check else out + (status[0],)
    row_rb = RaggedBatch(row, sample_sizes=sizes)
    col_rb = row_rb.create_with_sample_sizes_like_self(col)
    return (row_rb, col_rb) if check else (row_rb, col_rb, status)
