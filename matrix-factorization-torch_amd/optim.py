"""Sparse row optimisers for :class:`models.EmbeddingTower` tables.

``configure_optimizers`` of the reference returns dense ``torch.optim.AdamW``
(xfmr_rec/lightning.py:238-239).  With embedding tables only the gathered rows
receive gradient, so the update is a scatter over the touched rows
(``mf_update_sgd`` / ``mf_update_adam`` / ``mf_update_adagrad``): duplicate ids are
summed first, every touched row is read and written once.  Spec: ``oracle/embed.py``
(no reference implementation); row-wise Adagrad's: DESIGN.md 2.  The
classes are ``torch.optim.Optimizer`` subclasses, so Lightning's automatic
optimisation can drive them.

The optimiser kind is named in ``KINDS`` ("sgd" / "adagrad" / "adam" -> class); :func:`row_update` (one table) and
:func:`row_update_pair` (two tables, one launch) are the only callers of the update exports, for the optimisers' one
``step()``, the sharded trainer (``distributed.HipOps.update``) and tools/lab/update_probe.py alike.
"""
from __future__ import annotations

import functools
import os

import torch

from . import _lib, models


def _pending_pooled(p: torch.Tensor, items: list):
    """A step in which a pooled tower (:class:`models.HistoryPoolingTower`, :class:`models.FeatureBagTower`) parked its
    deferred gradient on ``p`` (a :class:`models.PooledGrad`): ONE coalesce over all
    sources -- the rows the other towers parked (``(ids, grad, normalized)``), then each pooled entry -- gives the table
    one list of at most min(rows, entries) unique ids (padded with -1), whatever order autograd ran the backwards in."""
    rows = [x for x in items if not isinstance(x, models.PooledGrad)]
    pooled = [x for x in items if isinstance(x, models.PooledGrad)]
    norms = {n for _, _, n in rows} | {x.normalize for x in pooled}
    if len(norms) != 1:
        raise _lib.MfHipError("a table was gathered both with and without normalisation in one step")
    ids = g = None
    if rows:
        ids = torch.cat([i for i, _, _ in rows]) if len(rows) > 1 else rows[0][0]
        g = torch.cat([x for _, x, _ in rows]) if len(rows) > 1 else rows[0][1]
    for x in pooled:
        ids, g = x.coalesce(p, ids, g)
    if ids.numel() == 0:
        items.clear()
        return None
    return ids, g, norms.pop()


def _pending(p: torch.Tensor):
    items = getattr(p, "_mf_pending", None)
    if not items:
        return None
    if any(isinstance(x, models.PooledGrad) for x in items):
        return _pending_pooled(p, items)
    if len(items) == 1:
        ids, g, norm = items[0]
    else:
        if len({n for _, _, n in items}) != 1:
            raise _lib.MfHipError("a table was gathered both with and without normalisation in one step")
        ids = torch.cat([i for i, _, _ in items])
        g = torch.cat([x for _, x, _ in items])
        norm = items[0][2]
    return ids, g, norm


_side_streams: dict = {}


def run_table_jobs(jobs) -> None:
    """Run independent per-table update jobs (callables issuing work on the *current* stream).  Default: one
    after the other on the caller's stream.  With ``MF_TABLE_STREAMS=1`` the first runs on the caller's stream
    and the others on cached side streams, forked from and joined back with events: the chains do overlap
    (~35 us of small kernels), but on this part a cross-stream join costs a 20-30 us bubble in the stream it
    rejoins -- measured at B = 8192: 1.1767 ms / step with two streams against 1.1644 on one."""
    if not jobs:
        return
    if len(jobs) == 1 or os.environ.get("MF_TABLE_STREAMS") != "1":
        for job in jobs:
            job()
        return
    cur = torch.cuda.current_stream()
    fork = torch.cuda.Event()
    fork.record(cur)
    joins = []
    for k, job in enumerate(jobs[1:]):
        key = (cur.device, k)
        side = _side_streams.get(key)
        if side is None:
            side = _side_streams[key] = torch.cuda.Stream(device=cur.device)
        side.wait_event(fork)
        with torch.cuda.stream(side):
            job()
            done = torch.cuda.Event()
            done.record(side)
        joins.append(done)
    jobs[0]()
    for done in joins:
        cur.wait_event(done)


def _hyper_args(kind: str, hyper: dict, step: int, step_dev, pair: bool = False) -> tuple:
    """The hyper-parameter arguments of ``kind``'s export, in its order.  (``mf_update_pair`` serves SGD too, with Adam's list:
    step, betas and eps unused.)"""
    if kind == "adagrad":
        return hyper["lr"], hyper["eps"], hyper["weight_decay"]
    if kind == "adam":
        return step, step_dev, hyper["lr"], *hyper["betas"], hyper["eps"], hyper["weight_decay"]
    return (1, None, hyper["lr"], 0.0, 0.0, 0.0, hyper["weight_decay"]) if pair else (hyper["lr"], hyper["weight_decay"])


def _table_args(lib, job: tuple, state_slots: int) -> tuple:
    """One job -- (table, state, ids, grad, normalized) -- as the exports take it, in three parts: (table, its state tensors
    [NULL up to ``state_slots``], rows), (ids, their number, gradient rows, normalised or not), (workspace, its bytes)."""
    table, state, ids, grad, normalized = job
    n = ids.numel()
    ws = _lib.workspace(lib.mf_update_ws_bytes(n, table.shape[1]), table.device)
    ptrs = [s.data_ptr() for s in state] + [None] * (state_slots - len(state))
    return (table.data_ptr(), *ptrs, table.shape[0]), (ids.data_ptr(), n, grad.data_ptr(), int(normalized)), (ws.data_ptr(), ws.numel())


def row_update(kind: str, table, state: tuple, ids, grad, normalized, hyper: dict, step: int = 1, step_dev=None, *, lib=None) -> None:
    """ONE table through its export (``mf_update_sgd`` / ``mf_update_adagrad`` / ``mf_update_adam``) on the current stream.
    ``state``: the kind's state tensors in the export's order -- ``()``, ``(sum,)``, ``(exp_avg, exp_avg_sq)``; ``hyper``: a
    parameter group (or ``distributed.optimizer_hyper``); ``step`` / ``step_dev``: Adam's global step, by value or (non-None)
    the address of a device counter.  ``lib``: another build of the library (tools/lab/update_probe.py)."""
    lib = lib or _lib.lib()
    rows, lst, ws = _table_args(lib, (table, state, ids, grad, normalized), len(state))
    _lib.check(getattr(lib, "mf_update_" + kind)(*rows, table.shape[1], *lst, *_hyper_args(kind, hyper, step, step_dev), *ws,
                                                 _lib.stream_ptr()))


def row_update_pair(kind: str, job_a: tuple, job_b: tuple, hyper: dict, step: int = 1, step_dev=None, *, lib=None) -> bool:
    """Two tables in ONE launch (``mf_update_pair`` / ``mf_update_pair_adagrad``) -- the usual step: user rows and item rows.
    A job: (table, state, ids, grad, normalized), as :func:`row_update` takes them.  False, and nothing launched: the tables'
    widths differ, a list is empty or beyond the one-launch range, or ``MF_UPDATE_PAIR`` is not "1" -- the caller updates the
    tables one by one."""
    if os.environ.get("MF_UPDATE_PAIR", "1") != "1":
        return False
    d = job_a[0].shape[1]
    if job_b[0].shape[1] != d or not (0 < job_a[2].numel() <= 65536 and 0 < job_b[2].numel() <= 65536):
        return False
    lib = lib or _lib.lib()
    fn, head, slots = (lib.mf_update_pair_adagrad, (d,), 1) if kind == "adagrad" else (lib.mf_update_pair, (int(kind == "adam"), d), 2)
    tables = [x for job in (job_a, job_b) for part in _table_args(lib, job, slots) for x in part]
    _lib.check(fn(*head, *tables, *_hyper_args(kind, hyper, step, step_dev, pair=True), _lib.stream_ptr()))
    return True


class _SparseRowOptimizer(torch.optim.Optimizer):
    """What the sparse row optimisers share: THE ``step``.  A subclass names its ``kind`` (the exports :func:`row_update` and
    :func:`row_update_pair` reach) and says what state a table has (``_state_of``); where it needs to, it checks a parameter
    group before anything is launched (``_check_group``) and opens a table's step (``_begin``)."""

    kind: str

    def zero_grad(self, set_to_none: bool = True) -> None:
        super().zero_grad(set_to_none=set_to_none)
        for group in self.param_groups:
            for p in group["params"]:
                if getattr(p, "_mf_pending", None):
                    p._mf_pending.clear()

    @staticmethod
    def _check(p: torch.Tensor) -> None:
        if p.grad is not None:
            raise _lib.MfHipError("dense gradient on an embedding table: gather rows through EmbeddingTower")
        if p.dim() != 2 or not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise _lib.MfHipError("embedding table must be a contiguous 2-D fp32 tensor on the GPU")

    def _check_group(self, group: dict) -> None:
        pass

    def _state_of(self, p: torch.Tensor, group: dict) -> tuple:
        """The state tensors of table ``p`` in the export's order, allocated on first use."""
        return ()

    def _begin(self, p: torch.Tensor) -> tuple:
        """Opens the step of a table with pending rows: (step, step_dev) for its update call."""
        return 1, None

    def init_state(self) -> None:
        """Allocate every table's state now instead of inside the first ``step`` (Adam: two table-sized allocations and
        memsets per table -- a multi-millisecond stall in the middle of an otherwise steady first step)."""
        for group in self.param_groups:
            for p in group["params"]:
                self._state_of(p, group)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        jobs = []       # (table, state, ids, grad, normalized, group, step, step_dev) of every table with pending rows
        for group in self.param_groups:
            self._check_group(group)
            for p in group["params"]:
                self._check(p)
                pend = _pending(p)
                if pend is not None:
                    jobs.append((p, self._state_of(p, group), *pend, group, *self._begin(p)))
        # the usual step -- user rows and item rows, one parameter group, the same global step -- is ONE launch
        a, b = jobs if len(jobs) == 2 else (None, None)
        if not (a and a[5] is b[5] and a[6] == b[6] and (a[7] is None) == (b[7] is None)
                and row_update_pair(self.kind, a[:5], b[:5], *a[5:])):
            run_table_jobs([functools.partial(row_update, self.kind, *job) for job in jobs])
        for job in jobs:
            job[0]._mf_pending.clear()
        return loss


class SparseSGD(_SparseRowOptimizer):
    """row -= lr * (sum of the row's gradients + weight_decay * row), touched rows only."""

    kind = "sgd"

    def __init__(self, params, lr: float = 1e-2, weight_decay: float = 0.0) -> None:
        super().__init__(params, {"lr": lr, "weight_decay": weight_decay})


class RowAdam(_SparseRowOptimizer):
    """Lazy row-wise AdamW: moments of touched rows only, global step for the bias
    correction, decoupled weight decay (torch.optim.AdamW's defaults otherwise)."""

    kind = "adam"

    def __init__(self, params, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01) -> None:
        super().__init__(params, {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay})
        # capturable: the global step lives in device memory and is bumped by a kernel of the step itself, so that a
        # step captured in a hipGraph (``graph.CapturedStep``) keeps counting when it is replayed -- a by-value
        # argument would be frozen at capture.  Same bits either way: the bias correction is evaluated on the device.
        self.capturable = False

    def on_replay(self) -> None:
        """Called once per graph replay of a captured step: keeps the host-side step counts in line."""
        for group in self.param_groups:
            for p in group["params"]:
                if self.state[p] and "step_t" in self.state[p]:
                    self.state[p]["step"] += 1

    def _state_of(self, p: torch.Tensor, group: dict) -> tuple:
        state = self.state[p]
        if not state:
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p)
            state["exp_avg_sq"] = torch.zeros_like(p)
        return state["exp_avg"], state["exp_avg_sq"]

    def _begin(self, p: torch.Tensor) -> tuple:
        state = self.state[p]
        step_dev = None
        if self.capturable:
            if "step_t" not in state:
                state["step_t"] = torch.full((1,), state["step"], dtype=torch.int64, device=p.device)
            state["step_t"] += 1                   # a kernel: replayed with the graph
            step_dev = state["step_t"].data_ptr()
        if not (self.capturable and torch.cuda.is_current_stream_capturing()):
            state["step"] += 1                     # (a capture runs no kernel: the replays count, via on_replay)
        return state["step"], step_dev


class RowAdagrad(_SparseRowOptimizer):
    """Row-wise Adagrad (the "exact row-wise Adagrad" of FBGEMM / torchrec): ONE fp32 of state per table row, ``sum``, where
    :class:`RowAdam` keeps two tables of moments.  For a touched row ``w`` with summed gradient ``g`` (plus the coupled L2 term
    ``weight_decay * w``, like :class:`SparseSGD` and ``torch.optim.Adagrad``)::

        sum[row] += mean(g ** 2);  w -= lr * g / (sqrt(sum[row]) + eps)

    The defaults are ``torch.optim.Adagrad``'s; there is no ``lr_decay`` and no step counter, so a step captured in a hipGraph
    (``graph.CapturedStep``) replays as it is.  The mean runs over the table's STORED width: a model width padded to the next of
    32, 64, 128, 256 has zero channels with zero gradient, which dilute it (a stored width of 2 x the model's halves ``sum``)."""

    kind = "adagrad"

    def __init__(self, params, lr: float = 1e-2, eps: float = 1e-10, weight_decay: float = 0.0,
                 initial_accumulator_value: float = 0.0) -> None:
        if not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not eps > 0.0:
            raise ValueError(f"Invalid epsilon value (must be > 0): {eps}")
        if not weight_decay >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not initial_accumulator_value >= 0.0:
            raise ValueError(f"Invalid initial_accumulator_value value: {initial_accumulator_value}")
        super().__init__(params, {"lr": lr, "eps": eps, "weight_decay": weight_decay,
                                  "initial_accumulator_value": initial_accumulator_value})

    def _check_group(self, group: dict) -> None:
        if not (group["lr"] >= 0.0 and group["eps"] > 0.0 and group["weight_decay"] >= 0.0):
            raise ValueError(f"RowAdagrad needs lr >= 0, eps > 0 and weight_decay >= 0: {group['lr'] = }, {group['eps'] = }, "
                             f"{group['weight_decay'] = }")

    def _state_of(self, p: torch.Tensor, group: dict) -> tuple:
        state = self.state[p]
        if not state:
            state["sum"] = torch.full((p.shape[0],), float(group["initial_accumulator_value"]), dtype=torch.float32, device=p.device)
        return (state["sum"],)


KINDS = {"sgd": SparseSGD, "adagrad": RowAdagrad, "adam": RowAdam}


class TowerOptimizer(torch.optim.Optimizer):
    """ONE optimiser for towers that own both embedding tables and dense parameters (:class:`models.HistoryTransformerTower`):
    ``sparse`` (one of ``KINDS``) steps the tables from the rows their backwards parked, ``dense``
    (``torch.optim.AdamW``, the reference's own optimiser, xfmr_rec/lightning.py:238-239) steps the parameters that received
    ordinary ``.grad`` tensors.  ``step`` / ``zero_grad`` / ``state_dict`` / ``load_state_dict`` drive both; ``param_groups`` are
    the two optimisers' own group dicts, so a scheduler that edits them reaches both."""

    def __init__(self, sparse: _SparseRowOptimizer, dense: torch.optim.Optimizer) -> None:
        self.sparse, self.dense = sparse, dense
        super().__init__(sparse.param_groups + dense.param_groups, {})
        self.param_groups = sparse.param_groups + dense.param_groups      # (the same dicts, not copies)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.sparse.step()
        self.dense.step()
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.sparse.zero_grad(set_to_none=set_to_none)
        self.dense.zero_grad(set_to_none=set_to_none)

    def state_dict(self) -> dict:
        return {"sparse": self.sparse.state_dict(), "dense": self.dense.state_dict()}

    def load_state_dict(self, state_dict: dict) -> None:
        self.sparse.load_state_dict(state_dict["sparse"])
        self.dense.load_state_dict(state_dict["dense"])


def tower_optimizer(towers: torch.nn.ModuleDict, kind: str, lr: float) -> torch.optim.Optimizer:
    """The optimiser of a tower dict: ``KINDS[kind]`` over the tables; when a tower owns dense parameters
    (``encoder_parameters``), a :class:`TowerOptimizer` that also steps those with AdamW."""
    if kind not in KINDS:
        msg = f"the towers' optimiser must be 'adam', 'sgd' or 'adagrad': {kind = }"
        raise ValueError(msg)
    dense = [p for t in towers.values() if hasattr(t, "encoder_parameters") for p in t.encoder_parameters()]
    tables = [p for p in towers.parameters() if not any(p is q for q in dense)]
    sparse = KINDS[kind](tables, lr=lr)
    return TowerOptimizer(sparse, torch.optim.AdamW(dense, lr=lr)) if dense else sparse
