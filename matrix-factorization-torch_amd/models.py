"""Towers: embedding tables instead of the reference's text encoder.

``xfmr_rec/models.py`` builds ONE randomly initialised BERT wrapped as
Transformer -> mean-Pooling -> Normalize (models.py:27-63) and the Lightning module
encodes user / item JSON text with it (xfmr_rec/lightning.py:60-74).  The north-star
of this repository replaces that tower by user / item **embedding tables**
(``ModelConfig`` keeps the reference's field names where they still mean something):
the forward is a coalesced row gather on the GPU (``mf_gather_rows``), ending in the
same L2-normalisation, and the backward does not build a dense table gradient: it
parks ``(row ids, row gradients)`` on the parameter for the sparse optimisers of
``optim.py``.  No reference implementation exists for this part; the
spec is ``oracle/embed.py``.
"""
from __future__ import annotations

import math
from typing import Literal

import pydantic
import torch

from . import _lib


class ModelConfig(pydantic.BaseModel):
    """Fields of ``xfmr_rec.models.ModelConfig`` (models.py:14-24) that survive the
    tower swap, plus the table sizes.  ``hidden_size`` is the embedding width d."""

    num_users: int = 6041          # ML-1M: 6,040 users + padding row 0
    num_items: int = 3884          # ML-1M: 3,883 items + padding row 0 (idx are 1-based, prepare.py:85)
    hidden_size: int = 64
    normalize: bool = True         # models.Normalize() at the end of the tower (models.py:59)
    init_std: float | None = None  # default 1/sqrt(hidden_size)
    num_hashes: int = 0            # > 0: hash / bloom towers (config 5): num_users / num_items are BUCKET counts
    hash_seed: int = 0
    # "history": the user vector is the pooled item rows of the user's history (HistoryPoolingTower), not a table row
    # "transformer": a BERT encoder over those rows, then the pool (HistoryTransformerTower)
    user_tower: Literal["table", "history", "features", "transformer"] = "table"
    pooling_mode: str = "mean"     # models.py:24 ("cls" needs user_tower="transformer"; "pooler" is refused everywhere)
    max_history: int | None = None
    # the encoder of user_tower="transformer" (the reference's field names, models.py:14-24; BertConfig's meanings)
    num_hidden_layers: int = 1
    num_attention_heads: int = 4
    intermediate_size: int | None = None       # None: hidden_size, as the reference's module config
    hidden_act: str = "gelu"
    max_position_embeddings: int = 64
    # training dropout of that encoder (BertConfig's names; the reference trains with BertConfig's defaults, 0.1 / 0.1).
    # 0.0 here: the tower then computes the eval-mode function in training too, as it always did
    hidden_dropout_prob: float = 0.0
    attention_probs_dropout_prob: float = 0.0
    dropout_seed: int = 0
    # arithmetic of that encoder's dense layers: "bf16-mixed" rounds both operands of their GEMMs to bf16 and accumulates in
    # fp32 (the reference trains under precision "bf16-mixed", xfmr_rec/lightning.py trainer_defaults); see check_precision
    precision: Literal["fp32", "bf16-mixed"] = "fp32"
    # "features": the vector is the pooled hashed-attribute tokens of the entity (FeatureBagTower); when both towers are
    # feature towers they share ONE bucket table, as the reference's towers share one encoder (lightning.py:60-74)
    item_tower: Literal["table", "features"] = "table"
    feature_buckets: int = 65535   # bucket rows of the feature table (keys 0..65535 sort in two 8-bit radix passes)
    feature_combiner: Literal["sum", "mean", "sqrtn"] = "mean"    # mean: the reference mean-pools (models.py:24)
    feature_seed: int = 0
    feature_text_fields: tuple[str, ...] = ("title",)             # fields split into words (data.FeatureHasher)

    @pydantic.model_validator(mode="after")
    def _check_pooling_mode(self):
        # (a model validator: which modes exist depends on user_tower)
        if self.user_tower == "transformer":
            check_transformer_shape(self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.intermediate_size,
                                    self.hidden_act, self.max_position_embeddings, self.max_history, self.pooling_mode)
            if self.num_hashes > 0 or self.item_tower != "table":
                msg = ("user_tower='transformer' encodes the rows of a plain item table: hashed towers (num_hashes > 0) and "
                       "item_tower='features' are not supported")
                raise ValueError(msg)
        else:
            check_pooling_mode(self.pooling_mode)
        return self

    @pydantic.model_validator(mode="after")
    def _check_dropout(self):
        for name in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
            p = check_dropout_prob(getattr(self, name), name)
            if p > 0.0 and self.user_tower != "transformer":
                msg = f"{name} is the dropout of user_tower='transformer' (no other tower has dropout): {name} = {p}, {self.user_tower = }"
                raise ValueError(msg)
        check_dropout_seed(self.dropout_seed)
        return self

    @pydantic.model_validator(mode="after")
    def _check_precision(self):
        if check_precision(self.precision) != "fp32" and self.user_tower != "transformer":
            msg = (f"precision is the arithmetic of user_tower='transformer' (no other tower has a precision mode): "
                   f"{self.precision = }, {self.user_tower = }")
            raise ValueError(msg)
        return self

    @pydantic.field_validator("max_history")
    @classmethod
    def _check_max_history(cls, v: int | None) -> int | None:
        if v is not None and v < 1:
            msg = f"max_history must be None or >= 1: {v = }"
            raise ValueError(msg)
        return v

    @pydantic.field_validator("feature_buckets")
    @classmethod
    def _check_feature_buckets(cls, v: int) -> int:
        if not 2 <= v <= FEATURE_MAX_BUCKETS:
            msg = f"feature_buckets must be in [2, 2^20] (the backward's radix sort covers 2^20 rows): {v = }"
            raise ValueError(msg)
        return v

    @pydantic.model_validator(mode="after")
    def _check_feature_towers(self):
        if "features" in (self.user_tower, self.item_tower):
            if self.num_hashes > 0:
                msg = "feature towers hash attributes, not ids: num_hashes > 0 is not supported with a 'features' tower"
                raise ValueError(msg)
            if self.user_tower == "history":
                msg = "user_tower='history' pools item-table rows and needs item_tower='table' (a feature item tower has no row per item)"
                raise ValueError(msg)
        return self


POOLING_MODES = ("mean", "max")
FEATURE_COMBINERS = ("sum", "mean", "sqrtn")
FEATURE_MAX_BUCKETS = 1 << 20


def check_pooling_mode(mode: str) -> str:
    """The reference's ``pooling_mode`` (models.py:24) minus the two modes that read transformer outputs."""
    if mode in ("cls", "pooler"):
        msg = (f"pooling_mode {mode!r} pools a transformer's [CLS] / pooler output and there is no transformer here: "
               f"the history tower pools item-table rows, use one of {POOLING_MODES}")
        raise ValueError(msg)
    if mode not in POOLING_MODES:
        msg = f"pooling_mode must be one of {POOLING_MODES}: {mode = }"
        raise ValueError(msg)
    return mode


TRANSFORMER_POOLING_MODES = ("mean", "max", "cls")
HIDDEN_ACTS = ("gelu", "relu", "silu", "gelu_new")      # the kernels' activation codes, in this order
XFMR_MAX_POSITIONS = 64
# ``HistoryTransformerTower.encode(path="auto")`` takes the one-launch kernel (``mf_xfmr_encode``) up to this many users and
# the training forward above it; None: at every batch size.  The two are bit-identical, so this is a speed decision only.
# Measured on an MI355X (``tools/xfmr_encode_probe.py``, ``profiles/xfmr_encode_probe.json``; the table is in DESIGN.md section
# 4, *Serving encode*): fused is 1.02-3.4 x faster at B = 1, 8 and 64 at all three probe shapes, slower at B = 512 at (128, 64,
# 512) and at B >= 4096 everywhere (a workgroup per user re-reads the weights; the forward's GEMMs share them).
XFMR_ENCODE_FUSED_MAX_USERS: int | None = 64
ENCODE_PATHS = ("auto", "fused", "forward")


def check_transformer_shape(hidden_size: int, num_hidden_layers: int, num_attention_heads: int, intermediate_size: int | None,
                            hidden_act: str, max_position_embeddings: int, max_history: int | None, pooling_mode: str) -> None:
    """The limits of ``csrc/mf_xfmr.hip``, as explicit errors."""
    if pooling_mode == "pooler":
        msg = ("pooling_mode 'pooler' is not supported: what sentence-transformers' Pooling does with it could not be checked; "
               f"use one of {TRANSFORMER_POOLING_MODES}")
        raise ValueError(msg)
    if pooling_mode not in TRANSFORMER_POOLING_MODES:
        msg = f"pooling_mode must be one of {TRANSFORMER_POOLING_MODES}: {pooling_mode = }"
        raise ValueError(msg)
    if hidden_size not in (32, 64, 128):
        msg = f"the transformer tower supports hidden_size in (32, 64, 128): {hidden_size = }"
        raise ValueError(msg)
    if not 1 <= num_hidden_layers <= 4:  # noqa: PLR2004
        msg = f"num_hidden_layers must be in 1..4: {num_hidden_layers = }"
        raise ValueError(msg)
    if num_attention_heads < 1 or hidden_size % num_attention_heads or hidden_size // num_attention_heads not in (8, 16, 32, 64):
        msg = (f"hidden_size / num_attention_heads must be a whole head width in (8, 16, 32, 64): {hidden_size = }, "
               f"{num_attention_heads = }")
        raise ValueError(msg)
    inter = hidden_size if intermediate_size is None else intermediate_size
    if inter < 32 or inter % 32 or inter > 4 * hidden_size:  # noqa: PLR2004
        msg = f"intermediate_size must be a multiple of 32 in [32, 4 * hidden_size]: {intermediate_size = }"
        raise ValueError(msg)
    if hidden_act not in HIDDEN_ACTS:
        msg = f"hidden_act must be one of {HIDDEN_ACTS}: {hidden_act = }"
        raise ValueError(msg)
    if not 1 <= max_position_embeddings <= XFMR_MAX_POSITIONS:
        msg = f"max_position_embeddings must be in 1..{XFMR_MAX_POSITIONS}: {max_position_embeddings = }"
        raise ValueError(msg)
    if max_history is not None and not 1 <= max_history <= max_position_embeddings:
        msg = f"max_history must be None or in 1..max_position_embeddings = {max_position_embeddings}: {max_history = }"
        raise ValueError(msg)


def check_dropout_prob(p: float, name: str = "p") -> float:
    """A dropout probability is in [0, 1) (torch.nn.Dropout's p = 1 would need a scale of 1 / 0)."""
    p = float(p)
    if not 0.0 <= p < 1.0:          # (nan fails both)
        msg = f"{name} must be in [0, 1): {p}"
        raise ValueError(msg)
    return p


PRECISIONS = ("fp32", "bf16-mixed")                      # the kernels' precision codes, in this order (include/mf_hip.h)


def check_precision(precision: str) -> str:
    """``"fp32"``, or ``"bf16-mixed"``: both operands of every GEMM of the encoder's six dense layers per layer (forward and
    both backward forms) rounded to bf16, fp32 accumulation, everything else fp32 (*Mixed precision*)."""
    if precision not in PRECISIONS:
        msg = f"precision must be one of {PRECISIONS}: {precision = }"
        raise ValueError(msg)
    return precision


def check_dropout_seed(seed: int) -> int:
    if not 0 <= int(seed) < 1 << 64:
        msg = f"dropout_seed must fit an unsigned 64-bit word: {seed = }"
        raise ValueError(msg)
    return int(seed)


def dropout_threshold(p: float) -> int:
    """``thr = round(p * 65536)`` (halves up, at most 65535) of ``include/mf_numerics.h``: an element is kept iff its
    16-bit field is >= thr, so the probability that counts is ``thr / 65536`` and the scale ``1 / (1 - thr / 65536)``;
    thr = 0 means the site is off."""
    return min(int(math.floor(check_dropout_prob(p) * 65536.0 + 0.5)), 65535)


def _park(table: torch.Tensor, item) -> None:
    """Park one gradient source on the table for the sparse optimisers of ``optim.py``, which read and clear the list."""
    pending = getattr(table, "_mf_pending", None)
    if pending is None:
        pending = []
        table._mf_pending = pending
    pending.append(item)


def _check_table(table: torch.Tensor, what: str) -> None:
    if not table.is_cuda or table.dtype != torch.float32 or not table.is_contiguous():
        raise _lib.MfHipError(f"{what} table must be a contiguous fp32 tensor on the GPU")


def _normalize_backward(u: torch.Tensor, inv: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """The gradient w.r.t. p of u = p * inv, inv = 1 / max(|p|, 1e-12), from the gradient ``g`` w.r.t. u (rows of ``[n, d]``)."""
    n, d = u.shape
    gp = torch.empty_like(g)
    _lib.check(_lib.lib().mf_normalize_backward(u.data_ptr(), inv.data_ptr(), g.data_ptr(), n, d, gp.data_ptr(), _lib.stream_ptr()))
    return gp


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: torch.Tensor, idx: torch.Tensor, normalize: bool):
        _check_table(table, "embedding")
        ids = _lib.dev_i64(idx, "idx").reshape(-1)
        n, d = ids.numel(), table.shape[1]
        out = torch.empty(n, d, dtype=torch.float32, device=table.device)
        _lib.check(_lib.lib().mf_gather_rows(table.data_ptr(), table.shape[0], d, ids.data_ptr(), n, int(normalize),
                                             out.data_ptr(), None, _lib.stream_ptr()))
        ctx.table = table
        ctx.ids = ids
        ctx.normalize = bool(normalize)
        return out.reshape(*idx.shape, d)

    @staticmethod
    def backward(ctx, grad_out):
        table = ctx.table
        g = grad_out.reshape(-1, table.shape[1]).to(torch.float32).contiguous()
        _park(table, (ctx.ids, g, ctx.normalize))
        return None, None, None


class EmbeddingTower(torch.nn.Module):
    """``tower(idx) -> [*, d]`` unit-norm rows; drop-in for ``module(text)``."""

    def __init__(self, num_embeddings: int, embedding_dim: int, *, normalize: bool = True,
                 init_std: float | None = None, device=None) -> None:
        super().__init__()
        if embedding_dim not in _lib.SUPPORTED_WIDTHS:
            msg = f"embedding_dim must be one of {_lib.SUPPORTED_WIDTHS}: {embedding_dim = }"
            raise ValueError(msg)
        std = init_std if init_std is not None else 1.0 / math.sqrt(embedding_dim)
        w = torch.randn(num_embeddings, embedding_dim, device=device) * std
        self.weight = torch.nn.Parameter(w)
        self.normalize = normalize

    @property
    def num_embeddings(self) -> int:
        return self.weight.shape[0]

    @property
    def embedding_dim(self) -> int:
        return self.weight.shape[1]

    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        return _GatherRows.apply(self.weight, idx, self.normalize)

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.embedding_dim}, normalize={self.normalize}"


class _GatherHashed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: torch.Tensor, idx: torch.Tensor, num_hashes: int, seed: int, normalize: bool):
        _check_table(table, "embedding")
        ids = _lib.dev_i64(idx, "idx").reshape(-1)
        n, d = ids.numel(), table.shape[1]
        out = torch.empty(n, d, dtype=torch.float32, device=table.device)
        inv = torch.empty(n, dtype=torch.float32, device=table.device)
        _lib.check(_lib.lib().mf_gather_hashed(table.data_ptr(), table.shape[0], d, ids.data_ptr(), n, num_hashes, seed,
                                               int(normalize), out.data_ptr(), inv.data_ptr(), _lib.stream_ptr()))
        ctx.table, ctx.ids, ctx.cfg = table, ids, (num_hashes, seed, bool(normalize))
        ctx.save_for_backward(out, inv)
        return out.reshape(*idx.shape, d)

    @staticmethod
    def backward(ctx, grad_out):
        table, ids = ctx.table, ctx.ids
        num_hashes, seed, normalize = ctx.cfg
        out, inv = ctx.saved_tensors
        n, d = ids.numel(), table.shape[1]
        lib = _lib.lib()
        g = grad_out.reshape(-1, d).to(torch.float32).contiguous()
        if normalize:      # gradient w.r.t. the summed rows: the same for each of the id's bucket rows
            g = _normalize_backward(out, inv, g)
        buckets = torch.empty(n * num_hashes, dtype=torch.int64, device=table.device)
        _lib.check(lib.mf_hash_buckets(ids.data_ptr(), n, num_hashes, seed, table.shape[0], buckets.data_ptr(),
                                       _lib.stream_ptr()))
        _park(table, (buckets, g.repeat_interleave(num_hashes, dim=0), False))
        return None, None, None, None, None


class HashEmbeddingTower(torch.nn.Module):
    """Hash / bloom embedding tower (BASELINE config 5: 100 M items x 10 M users do not get a row
    each): ``tower(idx)`` = L2-normalised sum of the ``num_hashes`` bucket rows of every id
    (``include/mf_numerics.h`` ``mf_hash_bucket``; spec ``oracle/embed.py``, no reference
    counterpart).  Works with the same sparse optimisers: the backward parks the bucket rows."""

    def __init__(self, num_buckets: int, embedding_dim: int, *, num_hashes: int = 2, seed: int = 0,
                 normalize: bool = True, init_std: float | None = None, device=None) -> None:
        super().__init__()
        if embedding_dim not in _lib.SUPPORTED_WIDTHS:
            msg = f"embedding_dim must be one of {_lib.SUPPORTED_WIDTHS}: {embedding_dim = }"
            raise ValueError(msg)
        if not 1 <= num_hashes <= 4:  # noqa: PLR2004
            msg = f"num_hashes must be in 1..4: {num_hashes = }"
            raise ValueError(msg)
        std = init_std if init_std is not None else 1.0 / math.sqrt(embedding_dim * num_hashes)
        self.weight = torch.nn.Parameter(torch.randn(num_buckets, embedding_dim, device=device) * std)
        self.num_hashes, self.seed, self.normalize = num_hashes, int(seed), normalize

    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        return _GatherHashed.apply(self.weight, idx, self.num_hashes, self.seed, self.normalize)

    def buckets(self, idx: torch.Tensor) -> torch.Tensor:
        """``[*, num_hashes]`` table rows of every id."""
        ids = _lib.dev_i64(idx, "idx").reshape(-1)
        out = torch.empty(ids.numel() * self.num_hashes, dtype=torch.int64, device=ids.device)
        _lib.check(_lib.lib().mf_hash_buckets(ids.data_ptr(), ids.numel(), self.num_hashes, self.seed, self.weight.shape[0],
                                              out.data_ptr(), _lib.stream_ptr()))
        return out.reshape(*idx.shape, self.num_hashes)

    def extra_repr(self) -> str:
        return f"{self.weight.shape[0]} buckets, {self.weight.shape[1]}, num_hashes={self.num_hashes}, normalize={self.normalize}"


class PooledGrad:
    """A pooled tower's deferred contribution to a table's gradient (parked on the table by its backward, resolved by the
    optimiser, ``optim._pending``): ``coalesce`` merges it, in one pass, with the rows other sources parked on the same
    table in the same step.  ``normalize``: whether the table's rows were normalised when read."""

    normalize: bool
    n_bound: int           # host bound of this source's entries

    def coalesce(self, table: torch.Tensor, ids: torch.Tensor | None, grad: torch.Tensor | None):
        """``(unique ids [capacity] (then -1), summed rows [capacity, d])`` of this source plus ``(ids, grad)``; capacity =
        min(rows, entries)."""
        n_extra = 0 if ids is None else ids.numel()
        cap = min(table.shape[0], n_extra + self.n_bound)
        out_ids = torch.empty(cap, dtype=torch.int64, device=table.device)
        out_grad = torch.empty(cap, table.shape[1], dtype=torch.float32, device=table.device)
        if cap:
            _lib.check(self._launch(_lib.lib(), table, ids, grad, n_extra, cap, out_ids, out_grad))
        return out_ids, out_grad

    def _launch(self, lib, table, ids, grad, n_extra: int, cap: int, out_ids, out_grad) -> int:
        """Ask for the workspace and make the tower's C call; returns its code."""
        raise NotImplementedError


class PooledHistoryGrad(PooledGrad):
    """The history tower's contribution to its item table's gradient, parked on the table by the backward and resolved by
    the optimiser (``optim._pending``): there it is coalesced, in one pass, with the rows other towers parked on the same
    table in the same step, so that the table receives ONE list of at most min(rows, entries) unique ids."""

    def __init__(self, ctx, grad_p: torch.Tensor) -> None:
        self.mode, self.normalize = ctx.mode, ctx.norm_item
        self.items, self.lo, self.off, self.count = ctx.items, ctx.lo, ctx.off, ctx.count
        self.arg, self.n_bound, self.grad_p = ctx.arg, ctx.n_entries, grad_p

    def _launch(self, lib, table, ids, grad, n_extra, cap, out_ids, out_grad):
        rows, d = table.shape
        ws = _lib.workspace(lib.mf_pool_backward_ws_bytes(n_extra, self.n_bound, d), table.device)
        return lib.mf_pool_backward(rows, d, self.mode, self.items.data_ptr(), self.lo.numel(), self.lo.data_ptr(), self.off.data_ptr(),
                                    self.count.data_ptr(), _lib.ptr(self.arg), self.grad_p.data_ptr(), self.n_bound,
                                    _lib.ptr(ids), _lib.ptr(grad), n_extra, cap, out_ids.data_ptr(), out_grad.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _lib.stream_ptr())


def _history_segments(dev, history, count: bool = True):
    """``(start, end, items, n_entries)`` of either input form (one host read of the entry count for segments; ``count=False``
    leaves it out: ``n_entries`` is then None)."""
    if isinstance(history, (tuple, list)):
        start, end, items = (_lib.dev_i64(t, name) for t, name in zip(history, ("start", "end", "items")))
        start, end = start.reshape(-1), end.reshape(-1)
        if start.numel() != end.numel():
            msg = f"start and end must have the same length: {start.numel()} != {end.numel()}"
            raise ValueError(msg)
        items = items.reshape(-1)
        n_entries = (int((end - start).clamp_min(0).sum()) if start.numel() else 0) if count else None
    else:
        pad = _lib.dev_i64(history, "history")
        if pad.dim() != 2:  # noqa: PLR2004
            msg = f"a padded history must be [B, L]: {tuple(pad.shape) = }"
            raise ValueError(msg)
        b, length = pad.shape
        start = torch.arange(b, device=dev, dtype=torch.int64) * length
        end = start + length
        items = pad.reshape(-1)
        n_entries = b * length
    if items.numel() == 0:
        items = torch.zeros(1, dtype=torch.int64, device=dev)
    return start, end, items, n_entries


class _PoolRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: torch.Tensor, start: torch.Tensor, end: torch.Tensor, items: torch.Tensor, n_entries: int,
                mode: int, max_history: int, norm_item: bool, norm_user: bool):
        _check_table(table, "embedding")
        lib = _lib.lib()
        rows, d = table.shape
        b = start.numel()
        dev = table.device
        u = torch.empty(b, d, dtype=torch.float32, device=dev)
        inv = torch.empty(b, dtype=torch.float32, device=dev)
        count = torch.empty(b, dtype=torch.int32, device=dev)
        lo = torch.empty(b, dtype=torch.int64, device=dev)
        off = torch.empty(b + 1, dtype=torch.int64, device=dev)
        arg = torch.empty(b, d, dtype=torch.int32, device=dev) if mode == 1 else None
        ws = _lib.workspace(lib.mf_pool_ws_bytes(b, n_entries, d, mode), dev)
        _lib.check(lib.mf_pool_forward(table.data_ptr(), rows, d, start.data_ptr(), end.data_ptr(), items.data_ptr(), items.numel(),
                                       b, n_entries, max_history, mode, int(norm_item), int(norm_user), u.data_ptr(), inv.data_ptr(),
                                       count.data_ptr(), lo.data_ptr(), off.data_ptr(), _lib.ptr(arg), ws.data_ptr(), ws.numel(),
                                       _lib.stream_ptr()))
        ctx.table, ctx.items, ctx.lo, ctx.off, ctx.count, ctx.arg = table, items, lo, off, count, arg
        ctx.mode, ctx.n_entries, ctx.norm_item, ctx.norm_user = mode, n_entries, bool(norm_item), bool(norm_user)
        ctx.save_for_backward(u, inv)
        return u

    @staticmethod
    def backward(ctx, grad_u):
        table = ctx.table
        u, inv = ctx.saved_tensors
        g = grad_u.to(torch.float32).contiguous()
        if ctx.norm_user:
            g = _normalize_backward(u, inv, g)
        _park(table, PooledHistoryGrad(ctx, g))
        return (None,) * 9


class HistoryPoolingTower(torch.nn.Module):
    """``tower(history) -> [B, d]``: the L2-normalised mean (or channel-wise max) of the item-table rows of every user's
    history -- the id-only counterpart of ``PoolingTransformer`` (xfmr_rec/models.py:66-84: pool the non-zero rows by
    ``pooling_mode``, then Normalize).  It owns no parameter: it reads the item tower's table, and its backward lands on that
    table's sparse update (coalesced with the item tower's own rows of the step, ``optim._pending``).  A user who is not
    in any table, or whose history changed after training, is served by pooling the current history.

    ``history``: ``(start [B], end [B], items)`` -- user b's list is ``items[start[b]:end[b]]`` (a CSR ``(off[:-1], off[1:],
    items)``, or ``InteractionTable``'s rolling windows into ``sorted_item``) -- or a padded ``[B, L]`` int64 matrix (0 =
    padding, the reference's ``pad_tensors`` layout).  Ids outside ``[1, num_items)`` are padding; ``max_history = L`` pools
    the last L valid entries of each list.  HIP kernels ``mf_pool_forward`` / ``mf_pool_backward``."""

    def __init__(self, item_tower: torch.nn.Module, *, pooling_mode: str = "mean", max_history: int | None = None,
                 normalize: bool = True) -> None:
        super().__init__()
        if not isinstance(item_tower, EmbeddingTower):
            msg = (f"HistoryPoolingTower pools the rows of a plain EmbeddingTower (one row per item); got {type(item_tower).__name__}"
                   " (a hashed tower's rows are shared by many items)")
            raise ValueError(msg)
        if max_history is not None and max_history < 1:
            msg = f"max_history must be None or >= 1: {max_history = }"
            raise ValueError(msg)
        object.__setattr__(self, "item_tower", item_tower)     # shared, not registered: the table is saved / optimised once
        self.pooling_mode = check_pooling_mode(pooling_mode)
        self.max_history = max_history
        self.normalize = normalize

    @property
    def weight(self) -> torch.nn.Parameter:
        return self.item_tower.weight

    def segments(self, history):
        """``(start, end, items, n_entries)`` of either input form (one host read of the entry count for segments)."""
        return _history_segments(self.weight.device, history)

    def forward(self, history) -> torch.Tensor:
        start, end, items, n_entries = self.segments(history)
        if start.numel() == 0:
            return torch.zeros(0, self.weight.shape[1], device=self.weight.device)
        return _PoolRows.apply(self.weight, start, end, items, n_entries, POOLING_MODES.index(self.pooling_mode),
                               self.max_history or 0, self.item_tower.normalize, self.normalize)

    def extra_repr(self) -> str:
        return f"pooling_mode={self.pooling_mode}, max_history={self.max_history}, normalize={self.normalize}"


class TransformerHistoryGrad(PooledGrad):
    """The transformer tower's contribution to its item table's gradient: one entry per packed token, key = the token's
    item id, row = dL/dx_t (``mf_xfmr_backward``'s ``grad_x``), coalesced with the rows other towers parked on the table."""

    def __init__(self, ctx, grad_x: torch.Tensor) -> None:
        self.normalize, self.stash, self.grad_x = ctx.norm_item, ctx.stash, grad_x
        self.b, self.n_bound, self.layers, self.inter = ctx.b, ctx.t_cap, ctx.shape[0], ctx.shape[2]

    def _launch(self, lib, table, ids, grad, n_extra, cap, out_ids, out_grad):
        rows, d = table.shape
        ws = _lib.workspace(lib.mf_xfmr_coalesce_ws_bytes(n_extra, self.n_bound, d), table.device)
        return lib.mf_xfmr_coalesce(rows, d, self.b, self.n_bound, self.layers, self.inter, self.stash.data_ptr(),
                                    self.grad_x.data_ptr(), _lib.ptr(ids), _lib.ptr(grad), n_extra, cap, out_ids.data_ptr(),
                                    out_grad.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())


def _pointer_array(tensors):
    import ctypes

    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _EncodeHistory(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: torch.Tensor, start: torch.Tensor, end: torch.Tensor, items: torch.Tensor, n_entries: int, cfg: tuple,
                *params: torch.Tensor):
        layers, heads, inter, act, mode, max_history, norm_item, norm_user = cfg[:8]
        drop = cfg[8] if len(cfg) > 8 else None      # (p_hidden, p_attn, seed, call): the *_dropout exports; None: the plain ones
        prec = cfg[9] if len(cfg) > 9 else _lib.XFMR_FP32    # not fp32: the *_mixed exports (dropout or not)
        _check_table(table, "embedding")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MfHipError("the transformer tower does not support hipGraph capture")
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.MfHipError("encoder parameters must be contiguous fp32 tensors on the GPU")
        lib = _lib.lib()
        rows, d = table.shape
        b = start.numel()
        dev = table.device
        t_cap = min(n_entries, b * max_history)
        u = torch.empty(b, d, dtype=torch.float32, device=dev)
        inv = torch.empty(b, dtype=torch.float32, device=dev)
        arg = torch.empty(b, d, dtype=torch.int32, device=dev) if mode == 1 else None
        stash = _lib.workspace(lib.mf_xfmr_ws_bytes(b, t_cap, d, layers, inter), dev)
        params = tuple(p.detach() for p in params)
        args = (table.data_ptr(), rows, d, start.data_ptr(), end.data_ptr(), items.data_ptr(), items.numel(), b, t_cap, max_history,
                layers, heads, inter, act, mode, int(norm_item), int(norm_user), _pointer_array(params), u.data_ptr(), inv.data_ptr(),
                _lib.ptr(arg), stash.data_ptr(), stash.numel())
        if prec != _lib.XFMR_FP32:
            _lib.check(lib.mf_xfmr_forward_mixed(*args, *(drop or (0.0, 0.0, 0, 0)), prec, _lib.stream_ptr()))
        elif drop is None:
            _lib.check(lib.mf_xfmr_forward(*args, _lib.stream_ptr()))
        else:
            _lib.check(lib.mf_xfmr_forward_dropout(*args, *drop, _lib.stream_ptr()))
        ctx.table, ctx.stash, ctx.arg, ctx.params, ctx.drop, ctx.prec = table, stash, arg, params, drop, prec
        ctx.b, ctx.t_cap, ctx.shape, ctx.mode = b, t_cap, (layers, heads, inter, act), mode
        ctx.max_history, ctx.norm_item, ctx.norm_user = max_history, bool(norm_item), bool(norm_user)
        ctx.save_for_backward(u, inv)
        return u

    @staticmethod
    def backward(ctx, grad_u):
        table, params = ctx.table, ctx.params
        u, inv = ctx.saved_tensors
        d = u.shape[1]
        layers, heads, inter, act = ctx.shape
        grads = [torch.empty_like(p) for p in params]
        if ctx.t_cap == 0:                           # no valid token in the batch: no gradient anywhere
            return (None,) * 6 + tuple(g.zero_() for g in grads)
        lib = _lib.lib()
        g = grad_u.to(torch.float32).contiguous()
        grad_x = torch.empty(ctx.t_cap, d, dtype=torch.float32, device=u.device)
        drop, prec = ctx.drop, ctx.prec
        plain = drop is None and prec == _lib.XFMR_FP32
        ws_bytes = lib.mf_xfmr_backward_ws_bytes if plain else lib.mf_xfmr_backward_dropout_ws_bytes
        ws = _lib.workspace(ws_bytes(ctx.t_cap, d, inter), u.device)
        args = (d, ctx.b, ctx.t_cap, ctx.max_history, params[0].shape[0], layers, heads, inter, act, ctx.mode, int(ctx.norm_user),
                _pointer_array(params), _pointer_array(grads), ctx.stash.data_ptr(), g.data_ptr(), u.data_ptr(), inv.data_ptr(),
                _lib.ptr(ctx.arg), grad_x.data_ptr(), ws.data_ptr(), ws.numel())
        if prec != _lib.XFMR_FP32:                   # the forward's precision
            _lib.check(lib.mf_xfmr_backward_mixed(*args, *(drop or (0.0, 0.0, 0, 0)), prec, _lib.stream_ptr()))
        elif drop is None:
            _lib.check(lib.mf_xfmr_backward(*args, _lib.stream_ptr()))
        else:                                        # the same (seed, call): the kernels regenerate the forward's masks
            _lib.check(lib.mf_xfmr_backward_dropout(*args, *drop, _lib.stream_ptr()))
        _park(table, TransformerHistoryGrad(ctx, grad_x))
        return (None,) * 6 + tuple(grads)


class _Names(torch.nn.Module):
    """A parameter container: only there so that ``state_dict`` carries BertModel's names."""


class HistoryTransformerTower(torch.nn.Module):
    """``tower(history) -> [B, d]``: ``Normalize(Pool(BertEncoder(rows of the user's last L history items)))`` -- the
    sequence form of the reference's tower, ``PoolingTransformer.forward(inputs_embeds)`` (xfmr_rec/models.py:66-84), so the
    user vector depends on the ORDER of the history.  ``history`` as for :class:`HistoryPoolingTower`; the last
    ``max_history`` (default ``max_position_embeddings``, at most 64) valid entries are kept, the oldest at position 0.
    ``pooling_mode``: "mean" / "max" over the valid positions, or "cls" = position 0.  The tower shares the item tower's
    table (its backward lands on that table's sparse update) and owns the encoder's dense parameters, named as
    ``transformers.BertModel``'s ``state_dict`` names them (no word-embedding table, no pooler dense); those receive ordinary
    ``.grad`` tensors.  fp32 throughout, LayerNorm eps 1e-12.  HIP kernels ``mf_xfmr_forward`` / ``mf_xfmr_backward`` /
    ``mf_xfmr_coalesce``; :meth:`encode` is the serving path (``mf_xfmr_encode``: one launch, no stash).  The tower may be
    applied more than once before a step (each call parks its own table gradient;
    the optimiser chains the coalesces, the dense gradients accumulate).  No hipGraph capture: ``forward`` raises
    ``MfHipError`` when the stream is capturing.

    **Dropout** (BertConfig's names): ``hidden_dropout_prob`` on the embeddings, the attention output and the FFN output,
    ``attention_probs_dropout_prob`` on the softmax, where ``BertModel`` has them.  Both default to 0.0, not BertConfig's
    0.1: the reference builds its BERT with BertConfig's defaults and trains it in train mode, so **0.1 / 0.1 is what the
    reference trains with**; pass them to train that model.  Dropout applies iff ``tower.training`` and a probability is
    non-zero (torch's rule); ``eval()`` computes the function without it.  The masks are counter-based
    (``include/mf_numerics.h``: a function of ``dropout_seed``, the number of the training forward, the site and the
    element's (user, position, column)), generated inside the kernels ``mf_xfmr_forward_dropout`` /
    ``mf_xfmr_backward_dropout`` -- no mask tensor exists and the backward regenerates the same bits, so a step is
    bit-reproducible.  Each training forward uses the next ``call`` number (``self.dropout_call``, a Python int);
    :meth:`manual_seed` sets the seed and resets the counter.  Seed and counter are NOT part of ``state_dict`` (its names
    keep mirroring ``BertModel``): a resumed run that wants the same masks calls ``manual_seed`` itself.

    **Precision**: ``precision="bf16-mixed"`` (default ``"fp32"``) rounds both operands of every GEMM of the six dense layers
    of each encoder layer to bf16 (round-to-nearest-even), forward and backward, and accumulates in fp32
    (``mf_xfmr_forward_mixed`` / ``mf_xfmr_backward_mixed``); outputs, parameters, gradients and everything else stay fp32,
    and a step stays bit-reproducible.  This is autocast's treatment of ``nn.Linear`` without the bf16 outputs; the attention
    matmuls stay fp32.  The mode is the tower's in training, evaluation and serving alike."""

    def __init__(self, item_tower: torch.nn.Module, *, num_hidden_layers: int = 1, num_attention_heads: int = 4,
                 intermediate_size: int | None = None, hidden_act: str = "gelu", max_position_embeddings: int = 64,
                 pooling_mode: str = "mean", max_history: int | None = None, normalize: bool = True,
                 initializer_range: float = 0.02, device=None, hidden_dropout_prob: float = 0.0,
                 attention_probs_dropout_prob: float = 0.0, dropout_seed: int = 0, precision: str = "fp32") -> None:
        super().__init__()
        self.precision = check_precision(precision)
        self.hidden_dropout_prob = check_dropout_prob(hidden_dropout_prob, "hidden_dropout_prob")
        self.attention_probs_dropout_prob = check_dropout_prob(attention_probs_dropout_prob, "attention_probs_dropout_prob")
        self.manual_seed(dropout_seed)
        if not isinstance(item_tower, EmbeddingTower):
            msg = (f"HistoryTransformerTower encodes the rows of a plain EmbeddingTower (one row per item); got "
                   f"{type(item_tower).__name__} (a hashed tower's rows are shared by many items)")
            raise ValueError(msg)
        h = item_tower.embedding_dim
        check_transformer_shape(h, num_hidden_layers, num_attention_heads, intermediate_size, hidden_act, max_position_embeddings,
                                max_history, pooling_mode)
        if item_tower.num_embeddings > FEATURE_MAX_BUCKETS:
            msg = f"the item table must have at most 2^20 rows (the backward's radix sort): {item_tower.num_embeddings = }"
            raise ValueError(msg)
        object.__setattr__(self, "item_tower", item_tower)     # shared, not registered: the table is saved / optimised once
        inter = h if intermediate_size is None else intermediate_size
        self.num_hidden_layers, self.num_attention_heads, self.intermediate_size = num_hidden_layers, num_attention_heads, inter
        self.hidden_act, self.max_position_embeddings = hidden_act, max_position_embeddings
        self.pooling_mode, self.normalize = pooling_mode, normalize
        self.max_history = max_position_embeddings if max_history is None else max_history
        dev = device if device is not None else item_tower.weight.device

        def linear(n_out, n_in):
            m = torch.nn.Linear(n_in, n_out, device=dev)
            torch.nn.init.normal_(m.weight, std=initializer_range)       # BertPreTrainedModel._init_weights
            torch.nn.init.zeros_(m.bias)
            return m

        def names(**children):
            m = _Names()
            for k, v in children.items():
                m.add_module(k, v)
            return m

        def norm():
            return torch.nn.LayerNorm(h, eps=1e-12, device=dev)

        emb = names(position_embeddings=torch.nn.Embedding(max_position_embeddings, h, device=dev),
                    token_type_embeddings=torch.nn.Embedding(2, h, device=dev), LayerNorm=norm())
        torch.nn.init.normal_(emb.position_embeddings.weight, std=initializer_range)
        torch.nn.init.normal_(emb.token_type_embeddings.weight, std=initializer_range)
        self.embeddings = emb
        layers = [names(attention=names(self=names(query=linear(h, h), key=linear(h, h), value=linear(h, h)),
                                        output=names(dense=linear(h, h), LayerNorm=norm())),
                        intermediate=names(dense=linear(inter, h)),
                        output=names(dense=linear(h, inter), LayerNorm=norm()))
                  for _ in range(num_hidden_layers)]
        self.encoder = names(layer=torch.nn.ModuleList(layers))

    @property
    def weight(self) -> torch.nn.Parameter:
        return self.item_tower.weight

    def encoder_parameters(self) -> list[torch.nn.Parameter]:
        """The dense parameters in the kernels' order (``include/mf_hip.h``): 4 + 16 per layer."""
        e = self.embeddings
        out = [e.position_embeddings.weight, e.token_type_embeddings.weight, e.LayerNorm.weight, e.LayerNorm.bias]
        for layer in self.encoder.layer:
            a = layer.attention
            for m in (a.self.query, a.self.key, a.self.value, a.output.dense, a.output.LayerNorm, layer.intermediate.dense,
                      layer.output.dense, layer.output.LayerNorm):
                out += [m.weight, m.bias]
        return out

    def manual_seed(self, seed: int) -> "HistoryTransformerTower":
        """Set the dropout seed and restart the count of training forwards: the masks of the forwards that follow are those
        of a fresh tower built with ``dropout_seed=seed``."""
        self.dropout_seed, self.dropout_call = check_dropout_seed(seed), 0
        return self

    def segments(self, history):
        """As :meth:`HistoryPoolingTower.segments`."""
        return _history_segments(self.weight.device, history)

    def _config(self) -> tuple:
        """The kernels' view of the tower, without dropout or precision: the eval-mode fp32 function."""
        return (self.num_hidden_layers, self.num_attention_heads, self.intermediate_size, HIDDEN_ACTS.index(self.hidden_act),
                TRANSFORMER_POOLING_MODES.index(self.pooling_mode), self.max_history, self.item_tower.normalize, self.normalize)

    def _forward(self, history, dropout: bool) -> torch.Tensor:
        if self.weight.is_cuda and torch.cuda.is_current_stream_capturing():    # (before ``segments``: its host read would fail first)
            raise _lib.MfHipError("the transformer tower does not support hipGraph capture")
        start, end, items, n_entries = self.segments(history)
        if start.numel() == 0:
            return torch.zeros(0, self.weight.shape[1], device=self.weight.device)
        cfg = self._config()
        if dropout and (self.hidden_dropout_prob > 0.0 or self.attention_probs_dropout_prob > 0.0):
            cfg += ((self.hidden_dropout_prob, self.attention_probs_dropout_prob, self.dropout_seed, self.dropout_call),)
            self.dropout_call += 1
        if self.precision != "fp32":
            cfg = cfg[:8] + (cfg[8] if len(cfg) > 8 else None, PRECISIONS.index(self.precision))  # noqa: PLR2004
        return _EncodeHistory.apply(self.weight, start, end, items, n_entries, cfg, *self.encoder_parameters())

    def forward(self, history) -> torch.Tensor:
        return self._forward(history, self.training)

    def encode(self, history, *, path: str = "auto") -> torch.Tensor:
        """``[B, d]`` query vectors for serving and metrics: the eval-mode function of :meth:`forward` (no dropout even when
        ``tower.training``; ``dropout_call`` does not advance), detached -- no graph, no stash kept, nothing parked on the
        table, no ``torch.no_grad()`` needed around it.  ``history`` as for :meth:`forward`.

        ``path="fused"``: ``mf_xfmr_encode`` -- one launch, one workgroup per user, every activation in LDS, no per-token memory
        and no host read; fp32 only (``ValueError`` on a ``bf16-mixed`` tower).  ``path="forward"``: the training forward's
        kernels in eval mode at the tower's precision.  At fp32 the two are bit-identical.  ``path="auto"``: ``"forward"`` when
        the tower is not fp32 (the precision stays the tower's own in serving) or there are more than
        ``XFMR_ENCODE_FUSED_MAX_USERS`` users, ``"fused"`` otherwise."""
        if path not in ENCODE_PATHS:
            msg = f"path must be one of {ENCODE_PATHS}: {path = }"
            raise ValueError(msg)
        if path == "fused" and self.precision != "fp32":
            msg = f"the fused encode kernel is fp32: a {self.precision!r} tower encodes through path='forward' (or 'auto')"
            raise ValueError(msg)
        start, end, items, _ = _history_segments(self.weight.device, history, count=False)      # (no host read)
        if path == "auto":
            limit = XFMR_ENCODE_FUSED_MAX_USERS
            fused = self.precision == "fp32" and (limit is None or start.numel() <= limit)
            path = "fused" if fused else "forward"
        if path == "forward":
            with torch.no_grad():
                return self._forward(history, dropout=False)
        table = self.weight.detach()
        _check_table(table, "embedding")
        params = tuple(p.detach() for p in self.encoder_parameters())
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.MfHipError("encoder parameters must be contiguous fp32 tensors on the GPU")
        rows, d = table.shape
        b = start.numel()
        u = torch.empty(b, d, dtype=torch.float32, device=table.device)
        if b == 0:
            return u
        layers, heads, inter, act, mode, max_history, norm_item, norm_user = self._config()
        lib = _lib.lib()
        _lib.check(lib.mf_xfmr_encode(table.data_ptr(), rows, d, start.data_ptr(), end.data_ptr(), items.data_ptr(), items.numel(), b,
                                      max_history, layers, heads, inter, act, mode, int(norm_item), int(norm_user),
                                      _pointer_array(params), u.data_ptr(), _lib.stream_ptr()))
        return u

    def extra_repr(self) -> str:
        return (f"layers={self.num_hidden_layers}, heads={self.num_attention_heads}, intermediate={self.intermediate_size}, "
                f"act={self.hidden_act}, pooling_mode={self.pooling_mode}, max_history={self.max_history}, normalize={self.normalize}, "
                f"hidden_dropout_prob={self.hidden_dropout_prob}, attention_probs_dropout_prob={self.attention_probs_dropout_prob}"
                + (f", precision={self.precision}" if self.precision != "fp32" else ""))


class FeatureBagGrad(PooledGrad):
    """A feature tower's contribution to its bucket table's gradient: entry e of bag b carries w_e * c_b * g_p[b]
    (``mf_bag_backward``), coalesced with the rows other sources parked on the table -- with both feature towers on one
    table, the second tower's coalesce takes the first one's list as its extra rows."""

    normalize = False

    def __init__(self, ctx, grad_p: torch.Tensor) -> None:
        self.idx, self.seg, self.max_len, self.scale, self.grad_p = ctx.idx, ctx.seg, ctx.max_len, ctx.scale, grad_p
        self.n_bound = self.scale.numel() * self.max_len

    def _launch(self, lib, table, ids, grad, n_extra, cap, out_ids, out_grad):
        rows, d = table.shape
        b = self.scale.numel()
        start, end, tokens, weights = self.seg
        ws = _lib.workspace(lib.mf_bag_backward_ws_bytes(n_extra, b, self.max_len, d), table.device)
        return lib.mf_bag_backward(rows, d, _lib.ptr(self.idx), b, start.data_ptr(), end.data_ptr(), start.numel(),
                                   tokens.data_ptr(), tokens.numel(), _lib.ptr(weights), self.max_len, self.scale.data_ptr(),
                                   self.grad_p.data_ptr(), _lib.ptr(ids), _lib.ptr(grad), n_extra, cap, out_ids.data_ptr(),
                                   out_grad.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())


class _BagRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: torch.Tensor, idx: torch.Tensor | None, b: int, seg: tuple, max_len: int, combiner: int,
                normalize: bool):
        _check_table(table, "feature")
        lib = _lib.lib()
        rows, d = table.shape
        dev = table.device
        start, end, tokens, weights = seg
        u = torch.empty(b, d, dtype=torch.float32, device=dev)
        inv = torch.empty(b, dtype=torch.float32, device=dev)
        scale = torch.empty(b, dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.mf_bag_ws_bytes(b, max_len, d), dev)
        _lib.check(lib.mf_bag_forward(table.data_ptr(), rows, d, _lib.ptr(idx), b, start.data_ptr(), end.data_ptr(), start.numel(),
                                      tokens.data_ptr(), tokens.numel(), _lib.ptr(weights), max_len, combiner, int(normalize),
                                      u.data_ptr(), inv.data_ptr(), scale.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        ctx.table, ctx.idx, ctx.seg, ctx.max_len, ctx.scale, ctx.normalize = table, idx, seg, max_len, scale, bool(normalize)
        ctx.save_for_backward(u, inv)
        return u

    @staticmethod
    def backward(ctx, grad_u):
        table = ctx.table
        u, inv = ctx.saved_tensors
        g = grad_u.to(torch.float32).contiguous()
        if ctx.normalize:
            g = _normalize_backward(u, inv, g)
        _park(table, FeatureBagGrad(ctx, g))
        return (None,) * 7


class FeatureBagTower(torch.nn.Module):
    """``tower(idx) -> [*, d]``: the pooled hashed-attribute tokens of entity ``idx`` -- an EmbeddingBag over one bucket
    table, the id-only counterpart of the reference's text encoder over an entity's JSON attributes
    (xfmr_rec/lightning.py:60-74, prepare.py:69-127).  ``set_bags`` registers every entity's bag (``data.FeatureBags``, from
    ``data.FeatureHasher``) on the device; ``forward(idx)`` then reads entity ``idx[b]``'s bag (ids outside the registered
    range give an empty bag, u = 0), so the loss path and the samplers are unchanged; ``embed(bags)`` embeds entities that
    were never registered (cold start).  p = sum / mean / sqrtn of w_e F[t_e]; u = p / max(|p|, 1e-12) when ``normalize``.
    ``num_embeddings`` is the number of registered entities; ``weight`` is the bucket table.  ``share_with``: use that
    tower's table (not registered here: it is optimised and saved once).  HIP kernels ``mf_bag_forward`` /
    ``mf_bag_backward``: no host read per call, so a step through this tower can be captured."""

    def __init__(self, num_buckets: int, embedding_dim: int, *, combiner: str = "mean", normalize: bool = True,
                 init_std: float | None = None, device=None, share_with: "FeatureBagTower | None" = None) -> None:
        super().__init__()
        if combiner not in FEATURE_COMBINERS:
            msg = f"combiner must be one of {FEATURE_COMBINERS}: {combiner = }"
            raise ValueError(msg)
        if share_with is not None:
            object.__setattr__(self, "weight", share_with.weight)       # shared, not registered
        else:
            if embedding_dim not in _lib.SUPPORTED_WIDTHS:
                msg = f"embedding_dim must be one of {_lib.SUPPORTED_WIDTHS}: {embedding_dim = }"
                raise ValueError(msg)
            if not 2 <= num_buckets <= FEATURE_MAX_BUCKETS:  # noqa: PLR2004
                msg = f"num_buckets must be in [2, 2^20]: {num_buckets = }"
                raise ValueError(msg)
            std = init_std if init_std is not None else 1.0 / math.sqrt(embedding_dim)
            self.weight = torch.nn.Parameter(torch.randn(num_buckets, embedding_dim, device=device) * std)
        self.combiner, self.normalize = combiner, normalize
        self.bags = None

    @staticmethod
    def _segments(bags, device):
        bags = bags.to(device)
        tokens = bags.tokens if bags.tokens.numel() else torch.zeros(1, dtype=torch.int64, device=device)
        return bags, (bags.off[:-1].contiguous(), bags.off[1:].contiguous(), tokens, bags.weights)

    def set_bags(self, bags) -> None:
        """Register every entity's bag (``data.FeatureBags``; entity e = row e, row 0 is usually the empty padding bag)."""
        self.bags, self._seg = self._segments(bags, self.weight.device)

    @property
    def num_embeddings(self) -> int:
        if self.bags is None:
            msg = "no bags registered: call set_bags first"
            raise ValueError(msg)
        return len(self.bags)

    @property
    def embedding_dim(self) -> int:
        return self.weight.shape[1]

    def _apply_bags(self, idx, b: int, seg, max_len: int) -> torch.Tensor:
        if b == 0:
            return torch.zeros(0, self.weight.shape[1], device=self.weight.device)
        return _BagRows.apply(self.weight, idx, b, seg, max_len, FEATURE_COMBINERS.index(self.combiner), self.normalize)

    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        if self.bags is None:
            msg = "FeatureBagTower.forward(idx) reads registered bags: call set_bags first (or embed(bags))"
            raise ValueError(msg)
        ids = _lib.dev_i64(idx, "idx").reshape(-1)
        out = self._apply_bags(ids, ids.numel(), self._seg, self.bags.max_len)
        return out.reshape(*idx.shape, self.weight.shape[1])

    def embed(self, bags) -> torch.Tensor:
        """``[len(bags), d]`` vectors of entities given by their bags (not registered)."""
        bags, seg = self._segments(bags, self.weight.device)
        return self._apply_bags(None, len(bags), seg, bags.max_len)

    def extra_repr(self) -> str:
        return f"{self.weight.shape[0]} buckets, {self.weight.shape[1]}, combiner={self.combiner}, normalize={self.normalize}"


def init_towers(config: ModelConfig, device=None) -> torch.nn.ModuleDict:
    """Counterpart of ``init_bert`` + ``to_sentence_transformer`` (models.py:27-63).  ``user_tower="history"``: the user
    tower is a :class:`HistoryPoolingTower` over the item table (plain tables only); ``"transformer"``: a
    :class:`HistoryTransformerTower` over it.  ``"features"``: a
    :class:`FeatureBagTower`; with both towers so, one shared bucket table."""
    def table(name):
        return EmbeddingTower(getattr(config, f"num_{name}s"), config.hidden_size, normalize=config.normalize,
                              init_std=config.init_std, device=device)

    if "features" in (config.user_tower, config.item_tower):
        kw = {"combiner": config.feature_combiner, "normalize": config.normalize}
        item = (FeatureBagTower(config.feature_buckets, config.hidden_size, init_std=config.init_std, device=device, **kw)
                if config.item_tower == "features" else table("item"))
        if config.user_tower != "features":
            user = table("user")
        elif isinstance(item, FeatureBagTower):
            user = FeatureBagTower(config.feature_buckets, config.hidden_size, share_with=item, **kw)
        else:
            user = FeatureBagTower(config.feature_buckets, config.hidden_size, init_std=config.init_std, device=device, **kw)
        return torch.nn.ModuleDict({"user": user, "item": item})
    if config.user_tower == "transformer":
        item = table("item")
        user = HistoryTransformerTower(item, num_hidden_layers=config.num_hidden_layers,
                                       num_attention_heads=config.num_attention_heads, intermediate_size=config.intermediate_size,
                                       hidden_act=config.hidden_act, max_position_embeddings=config.max_position_embeddings,
                                       pooling_mode=config.pooling_mode, max_history=config.max_history,
                                       normalize=config.normalize, device=device, hidden_dropout_prob=config.hidden_dropout_prob,
                                       attention_probs_dropout_prob=config.attention_probs_dropout_prob,
                                       dropout_seed=config.dropout_seed, precision=config.precision)
        return torch.nn.ModuleDict({"user": user, "item": item})
    if config.user_tower == "history":
        if config.num_hashes > 0:
            msg = "user_tower='history' pools plain item-table rows; hashed towers (num_hashes > 0) are not supported"
            raise ValueError(msg)
        item = table("item")
        user = HistoryPoolingTower(item, pooling_mode=config.pooling_mode, max_history=config.max_history,
                                   normalize=config.normalize)
        return torch.nn.ModuleDict({"user": user, "item": item})
    if config.num_hashes > 0:
        return torch.nn.ModuleDict(
            {
                name: HashEmbeddingTower(rows, config.hidden_size, num_hashes=config.num_hashes,
                                         seed=config.hash_seed + salt, normalize=config.normalize,
                                         init_std=config.init_std, device=device)
                for salt, (name, rows) in enumerate((("user", config.num_users), ("item", config.num_items)))
            }
        )
    return torch.nn.ModuleDict({"user": table("user"), "item": table("item")})
