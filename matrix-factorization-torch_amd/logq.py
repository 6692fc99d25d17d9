"""Producers of the table the logQ correction reads (``losses``: ``logq=`` / ``logq_table=``; absent upstream).

:func:`logq_from_counts` is the static table: the log of each item's share of the interactions.

:class:`StreamingLogQ` estimates, on the device and from the batches themselves, the log of the rate at which an id
enters a batch (Yi et al. 2019, "Sampling-bias-corrected neural modeling", Algorithms 2 and 3): per bucket the step of
the last sighting and a moving average ``gap`` of the steps between sightings, ``logq = -log(gap)``.  That is the quantity
the correction wants when the columns of a batch are positives AND uniform negatives -- an item enters with probability
``1 - (1 - p_j)^B (1 - 1/M)^B``, far from its share ``p_j`` in the tail of a catalog.  It needs no pass over the data,
and in its hashed form (``num_hashes`` >= 1: the largest gap among the id's buckets) its state does not grow with the
catalog.  The rule, bit for bit: include/mf_hip.h (``mf_logq_update``), DESIGN.md 4.

    est = StreamingLogQ(num_items, alpha=0.01, device="cuda")     # direct: one bucket per item row
    logq = est.update(item_idx)                                   # step += 1; the rows' values after the update
    loss = fn(u, v, target, item_idx=item_idx, logq_table=est.table)

The state is all in buffers (``state_dict``, ``.to()`` and checkpoints carry it) and the step counter lives on the device,
so ``update`` is the same one or two launches in and out of a captured graph.  No CPU path: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _lib


def logq_from_counts(counts: torch.Tensor) -> torch.Tensor:
    """The static table: log of each item's share of the interactions (counts clamped at 1, shares in float64), fp32."""
    p = torch.as_tensor(counts).to(torch.float64).clamp_min(1.0)
    return (p / p.sum()).log().to(torch.float32)


class StreamingLogQ(torch.nn.Module):
    MAX_HASHES = 4

    def __init__(self, num_buckets: int, *, alpha: float = 0.01, num_hashes: int = 0, seed: int = 0, device=None) -> None:
        super().__init__()
        if int(num_buckets) < 1 or int(num_buckets) >= 2**31:
            msg = f"num_buckets must be in 1 .. 2^31 - 1: {num_buckets}"
            raise ValueError(msg)
        if not 0.0 < float(alpha) <= 1.0:            # (nan fails both comparisons)
            msg = f"alpha must be in (0, 1]: {alpha}"
            raise ValueError(msg)
        if not 0 <= int(num_hashes) <= self.MAX_HASHES:
            msg = f"num_hashes must be 0 (direct) or 1..{self.MAX_HASHES} (hashed): {num_hashes}"
            raise ValueError(msg)
        self.num_buckets, self.alpha, self.num_hashes, self.seed = int(num_buckets), float(alpha), int(num_hashes), int(seed)
        shape = (self.num_buckets,) if self.num_hashes == 0 else (self.num_hashes, self.num_buckets)
        self.register_buffer("last_seen", torch.zeros(shape, dtype=torch.int32, device=device))
        self.register_buffer("gap", torch.zeros(shape, dtype=torch.float32, device=device))
        self.register_buffer("step", torch.zeros(1, dtype=torch.int64, device=device))
        if self.num_hashes == 0:     # [num_buckets] logQ of every row (0.0 where never seen), kept current by update()
            self.register_buffer("table", torch.zeros(shape, dtype=torch.float32, device=device))

    def __getattr__(self, name: str):
        if name == "table" and "table" not in self.__dict__.get("_buffers", ()):      # no such buffer: hashed mode
            msg = "a hashed StreamingLogQ has no table over ids: read rows with lookup(ids)"
            raise AttributeError(msg)
        return super().__getattr__(name)

    def _ids(self, ids: torch.Tensor) -> torch.Tensor:
        ids = _lib.dev_i64(ids, "ids").reshape(-1)
        if ids.device != self.gap.device:
            raise _lib.MfHipError(f"ids are on {ids.device}, the estimator on {self.gap.device}")
        return ids

    def _on_gpu(self) -> None:
        if not self.gap.is_cuda:
            raise _lib.MfHipError(f"the estimator must live on the GPU (got {self.gap.device}); this package has no CPU path")

    @torch.no_grad()
    def update(self, ids: torch.Tensor, *, rows: bool = True) -> torch.Tensor | None:
        """One step: the counter advances, every distinct bucket of ``ids`` is updated once; returns logQ of ``ids`` [n]
        after the update (``rows=False``: nothing is read back -- one launch -- and None is returned)."""
        ids = self._ids(ids)
        self._on_gpu()
        out = torch.empty(ids.numel(), dtype=torch.float32, device=ids.device) if rows else None
        self.step.add_(1)
        _lib.check(_lib.lib().mf_logq_update(
            self.last_seen.data_ptr(), self.gap.data_ptr(), self.num_buckets, self.num_hashes, self.seed, ids.data_ptr(), ids.numel(),
            0, self.step.data_ptr(), self.alpha, self.table.data_ptr() if self.num_hashes == 0 else None, _lib.ptr(out),
            _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def lookup(self, ids: torch.Tensor) -> torch.Tensor:
        """logQ of ``ids`` [n] as the state stands; changes nothing."""
        ids = self._ids(ids)
        self._on_gpu()
        out = torch.empty(ids.numel(), dtype=torch.float32, device=ids.device)
        _lib.check(_lib.lib().mf_logq_lookup(self.gap.data_ptr(), self.num_buckets, self.num_hashes, self.seed, ids.data_ptr(),
                                             ids.numel(), out.data_ptr(), _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def reset(self) -> None:
        """Back to the initial state: nothing seen, step 0."""
        for buf in self.buffers():
            buf.zero_()

    def extra_repr(self) -> str:
        return f"num_buckets={self.num_buckets}, alpha={self.alpha}, num_hashes={self.num_hashes}, seed={self.seed}"
