"""The specification of row-wise Adagrad, written from its formulas and from nothing else: the oracle has no
Adagrad, so this function is what tests/test_update_adagrad_cpu.py pins on hand-worked rows and what the GPU tests
(tests/test_gpu_update_adagrad.py, tests/test_gpu_adagrad_module.py) hold the kernels to.

For a touched row ``w`` of stored width d with summed gradient ``acc`` and state ``s``::

    g = acc                                   (normalized = 0)
    g = (acc - uh * (acc . uh)) * inv         (normalized = 1: inv = 1 / max(|w|, 1e-12), uh = w * inv)
    g = g + wd * w                            (skipped when wd == 0)
    q = (1 / d) * sum_c g_c^2
    s = s + q
    w = w - lr * g / (sqrt(s) + eps)

The three sums over a row (|w|^2, acc . uh, sum g^2) are taken in the order the contract names ("the group
butterfly"): the four consecutive channels 4c .. 4c+3 left to right, then an xor butterfly over the d/4 partial sums, widest
stride first (``group_sum``).  In fp64 the order is immaterial; in fp32 it makes E -- the specification's own rounding
error, which the 4 E rule of the GPU tests is built on -- the error of the contract's arithmetic rather than of whatever
order ``torch.sum`` happens to take.  That matters where a tensor has ONE touched row and E is a sample of one: ``sum`` is a
reduction of d squares (d + d roundings), and against ``torch.sum`` a single row came out at E = 0.1 ulp by luck while the
contract's order sits 1.1 ulp from fp64 (bucket-9000-one-run-d32, plain, wd = 0, step 1: measured on the MI355X).

Every function works on COMPACT rows (row k of each tensor belongs to unique id k) in the dtype asked for; the
hyper-parameters enter at their fp32 values, as the kernel receives them.
"""
from __future__ import annotations

import numpy as np
import torch


def f32(x: float) -> float:
    return float(np.float32(x))


def group_sum(x: torch.Tensor) -> torch.Tensor:
    """``[rows, d] -> [rows, 1]``: channels 4c .. 4c+3 left to right, then the xor butterfly over the d/4 partial sums."""
    rows, d = x.shape
    p = x.reshape(rows, d // 4, 4)
    lanes = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    idx = torch.arange(d // 4)
    m = d // 8
    while m >= 1:
        lanes = lanes + lanes[:, idx ^ m]
        m //= 2
    return lanes[:, :1]


def adagrad_rows(w: torch.Tensor, s: torch.Tensor, acc: torch.Tensor, *, normalized: bool, lr: float, eps: float, wd: float,
                 dtype: torch.dtype = torch.float64) -> tuple[torch.Tensor, torch.Tensor]:
    """One step on compact rows: ``(w', s')`` in `dtype`."""
    w, s, g = w.to(dtype), s.to(dtype), acc.to(dtype)
    lr, eps, wd = f32(lr), f32(eps), f32(wd)
    d = w.shape[1]
    if normalized:
        inv = 1.0 / torch.sqrt(group_sum(w * w)).clamp_min(f32(1e-12))
        uh = w * inv
        g = (g - uh * group_sum(g * uh)) * inv
    if wd != 0.0:
        g = g + wd * w
    q = (1.0 / d) * group_sum(g * g)[:, 0]
    s = s + q
    w = w - lr * g / (torch.sqrt(s) + eps)[:, None]
    return w, s


def coalesce(ids: torch.Tensor, grad: torch.Tensor, n_rows: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(unique valid ids ascending, float64 sums of their gradient rows); ids outside [0, n_rows) are skipped."""
    ids, grad = ids.cpu(), grad.cpu().double()
    keep = (ids >= 0) & (ids < n_rows)
    uniq, inv = torch.unique(ids[keep], return_inverse=True)
    sums = torch.zeros(len(uniq), grad.shape[1], dtype=torch.float64)
    sums.index_add_(0, inv, grad[keep])
    return uniq, sums


def adagrad_update(table: torch.Tensor, state_sum: torch.Tensor, ids: torch.Tensor, grad: torch.Tensor, *, normalized: bool, lr: float,
                   eps: float, wd: float) -> None:
    """A whole sparse update in place, in the tensors' dtype (the CPU stand-in of ``mf_update_adagrad``)."""
    uniq, sums = coalesce(ids, grad, table.shape[0])
    if len(uniq) == 0:
        return
    w, s = adagrad_rows(table[uniq], state_sum[uniq], sums, normalized=normalized, lr=lr, eps=eps, wd=wd, dtype=table.dtype)
    table[uniq] = w
    state_sum[uniq] = s


def check_4e(before_w, before_s, acc, got_w, got_s, *, normalized, lr, eps, wd, margin: int = 4) -> list[tuple]:
    """The project's rule for row arithmetic (tests/test_gpu_update.py): with E the largest elementwise difference between
    the spec in fp32 and in fp64, the kernel may differ from fp64 by margin * E, floored at one fp32 ulp of the tensor's
    largest value; per tensor.  Returns [(name, E, kernel deviation, bound)]; the caller prints and asserts."""
    w64, s64 = adagrad_rows(before_w, before_s, acc, normalized=normalized, lr=lr, eps=eps, wd=wd, dtype=torch.float64)
    w32, s32 = adagrad_rows(before_w, before_s, acc, normalized=normalized, lr=lr, eps=eps, wd=wd, dtype=torch.float32)
    out = []
    for name, k64, k32, got in (("table", w64, w32, got_w), ("sum", s64, s32, got_s)):
        e = float((k32.double() - k64).abs().max())
        dev = float((got.double() - k64).abs().max())
        ulp = float(np.spacing(np.float32(float(k64.abs().max()))))
        out.append((name, e, dev, max(margin * e, ulp)))
    return out
