"""Exact brute-force retrieval over the item table (replaces the LanceDB ANN index), and the reference's probing of a
partitioned index on top of it.

Reference: ``ItemProcessor.get_index`` embeds every item and builds an
``IVF_HNSW_PQ`` cosine index (xfmr_rec/data/lightning.py:182-235);
``ItemProcessor.search`` runs one query with a ``movie_id NOT IN (...)`` prefilter
and returns the ``top_k`` rows with ``score = 1 - cosine distance``, best first
(:237-259).  Here the "index" is the unit-norm item matrix itself, resident in HBM,
and ``search`` is an exact scan (``mf_topk``): same scores for unit-norm rows, exact
instead of approximate, batched over queries, ties broken by lowest item row.
``PartitionedIndex`` adds the inverted-file half of that index (``num_partitions`` cells, ``num_probes`` of them visited
per query): which rows a query looks at becomes approximate, how they are scored and ordered stays exact.
``QuantizedIndex`` adds the other half, the product quantiser with its exact refine (``num_sub_vectors``, ``refine_factor``).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from collections import OrderedDict
from typing import Sequence

import numpy as np
import torch

from . import _lib
from .params import ITEM_ID_COL, ITEM_IDX_COL, TOP_K


def _csr(exclude: Sequence[Sequence[int]] | None, q: int, device):
    """Per-query exclusion lists -> (offsets[Q+1], sorted row indices) on the GPU."""
    if exclude is None:
        return None, None
    if len(exclude) != q:
        msg = f"one exclusion list per query expected: {len(exclude) = }, {q = }"
        raise ValueError(msg)
    lens = np.fromiter((len(e) for e in exclude), dtype=np.int64, count=q)
    off = np.zeros(q + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    flat = np.concatenate([np.sort(np.asarray(e, dtype=np.int64)) for e in exclude]) if off[-1] else np.zeros(1, np.int64)
    return torch.from_numpy(off).to(device), torch.from_numpy(flat).to(device)


_U64 = 1 << 64


@dataclasses.dataclass(frozen=True)
class TagFilter:
    """A predicate over the items' tag words (``ItemIndex.set_tags``: 64 boolean attributes per row), three 64-bit masks: a row
    with tag word t is admissible iff ``(t & all_of) == all_of and (any_of == 0 or t & any_of) and not t & none_of`` -- the
    ``where`` of the reference's ``search(...).where(filter, prefilter=True)`` (data/lightning.py:247-259) for attribute
    predicates.  Hashable: the key of an index's cached views."""

    any_of: int = 0
    all_of: int = 0
    none_of: int = 0

    def __post_init__(self) -> None:
        for name in ("any_of", "all_of", "none_of"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < _U64:
                msg = f"{name} must be an int in [0, 2**64): {v!r}"
                raise ValueError(msg)
            object.__setattr__(self, name, int(v))
        if self.all_of & self.none_of:
            msg = f"all_of and none_of share bits, so no row is admissible: {self.all_of & self.none_of:#x}"
            raise ValueError(msg)


def _is_filter_sequence(where) -> bool:
    return isinstance(where, (list, tuple))


class ItemIndex:
    """Item embeddings ``[N, d]`` (row r = global item row ``idx_base + r``) on one GPU.  A snapshot, like the table the
    reference's ``get_index`` writes: the derived copies (``blocked()``, ``bf16_index()``) are built on first use from the
    rows as they are then -- ``refresh()`` after changing the rows in place."""

    def __init__(self, embeddings: torch.Tensor, *, idx_base: int = 0) -> None:
        emb = _lib.dev_f32(embeddings.detach(), "embeddings")
        self.dim = emb.shape[1]
        dp = _lib.padded_width(self.dim)
        if dp != self.dim:
            emb = torch.nn.functional.pad(emb, (0, dp - self.dim))
        self.embeddings = emb.contiguous()
        self.idx_base = int(idx_base)
        self._blocked: torch.Tensor | None = None      # second copy for the small-batch scan, built on first use
        self._bf16: torch.Tensor | None = None         # bf16 copy + largest row norm for the prefilter path, built on first use
        self._ws: dict = {}                              # search workspaces, kept between calls
        self.tags: torch.Tensor | None = None            # int64 [N]: 64 boolean attributes per row (set_tags)
        self._views: OrderedDict = OrderedDict()         # TagFilter -> FilteredView, least recently used first

    MAX_VIEWS = 8      # cached views per index: each is a second copy of its rows

    SMALL_Q = 32       # at most this many queries can take the bandwidth-bound matrix-vector path (mf_topk_small)
    # "auto" (measured at N = 62,423, d = 128, us of device time per call): scan 15 at Q = 1 (FMA chains, HBM-bound), and for
    # 2 .. 32 queries -- one MFMA tile side: the fp32 matrix core computes all of them in the time of one -- see
    # profiles/r03_topk_small_probe.log; bf16 prefilter 42 / 44 / 51 / 70 at Q = 32 / 256 / 512 / 1024 (five launches: ~35 us floor);
    # fp32 tiles 95 / 86 / 98 / 133 / 219
    AUTO_SMALL_Q = 32  # scan up to here, then the bf16 prefilter (d >= 64), else the fp32 tile engine
    SCAN_MAX_EXCL = 8192     # exclusion entries (all queries of a call) the scan stages in LDS: EX_CAP of mf_topk_small.hip

    PATHS = ("auto", "scan", "tiles", "bf16", "deep")
    TILE_MAX_K = 64    # "scan", "tiles" and "bf16" hold a row's result in one wavefront; "auto" sends deeper lists to "deep"
    DEEP_MAX_K = _lib.MF_TOPK_DEEP_MAX_K

    def blocked(self) -> torch.Tensor:
        """The catalog in the blocked layout of ``mf_topk_small`` (``[64-row block][chunk][row]``), built once."""
        if self._blocked is None:
            lib = _lib.lib()
            n, d = self.embeddings.shape
            out = torch.empty(lib.mf_topk_blocked_bytes(n, d) // 4, dtype=torch.float32, device=self.embeddings.device)
            _lib.check(lib.mf_topk_blocked_build(self.embeddings.data_ptr(), n, d, out.data_ptr(), _lib.stream_ptr()))
            self._blocked = out
        return self._blocked

    BF16_MIN_Q = 5     # "auto" takes the bf16-prefilter path from here (and d >= 64, N >= BF16_MIN_N)
    BF16_MIN_N = 2048

    def bf16_index(self) -> torch.Tensor:
        """bf16 rows + the largest row norm, the prefilter index of ``mf_topk_bf3``; built once."""
        if self._bf16 is None:
            lib = _lib.lib()
            n, d = self.embeddings.shape
            out = torch.empty(lib.mf_topk_bf3_index_bytes(n, d), dtype=torch.uint8, device=self.embeddings.device)
            _lib.check(lib.mf_topk_bf3_build(self.embeddings.data_ptr(), n, d, out.data_ptr(), out.numel(), _lib.stream_ptr()))
            self._bf16 = out
        return self._bf16

    def refresh(self) -> None:
        """Forget the derived copies: they are rebuilt from the current rows at the next search.  The cached views of
        ``filtered`` are copies of rows too, and go with them."""
        self._blocked = self._bf16 = None
        self._views.clear()

    def set_tags(self, tags: torch.Tensor) -> None:
        """The rows' tag words, ``int64 [num_items]`` (bit i of row r: the row has attribute i), moved to the index's device:
        what a ``TagFilter`` is evaluated on.  Drops the cached views."""
        if not isinstance(tags, torch.Tensor) or tags.dtype != torch.int64 or tags.shape != (self.num_items,):
            msg = f"tags should be an int64 tensor of shape ({self.num_items},): {getattr(tags, 'dtype', type(tags))}, {tuple(getattr(tags, 'shape', ()))}"
            raise ValueError(msg)
        self.tags = tags.detach().to(self.embeddings.device).contiguous()
        self._views.clear()

    def filtered(self, where, *, cache: bool = True) -> "FilteredView":
        """The view of the rows ``where`` admits: a ``TagFilter`` over ``tags``, or a ``bool [num_items]`` allow-mask (the same
        kernel with the mask as the tag word and ``all_of = 1``; never cached).  Built once per filter -- the predicate over
        the catalog, the admissible rows compacted in ascending order, gathered into a dense sub-catalog -- with the one host
        read of the view's size; a search of the view reads nothing back.  The last ``MAX_VIEWS`` filters' views are kept
        (``cache=False``: neither looked up nor kept) until ``refresh()``, ``rebuild()`` or ``set_tags()``."""
        if isinstance(where, TagFilter):
            if self.tags is None:
                msg = "a TagFilter needs the rows' tags: call set_tags first"
                raise ValueError(msg)
            if cache and where in self._views:
                self._views.move_to_end(where)
                return self._views[where]
            view = FilteredView(self, self.tags, where)
            if cache:
                self._views[where] = view
                while len(self._views) > self.MAX_VIEWS:
                    self._views.popitem(last=False)
            return view
        if isinstance(where, torch.Tensor) and where.dtype == torch.bool and where.shape == (self.num_items,):
            return FilteredView(self, where.to(self.embeddings.device).to(torch.int64), TagFilter(all_of=1))
        msg = f"where should be a TagFilter or a bool tensor of shape ({self.num_items},): {where!r}"
        raise ValueError(msg)

    def _sub_index(self, embeddings: torch.Tensor, rows: torch.Tensor) -> "ItemIndex":  # noqa: ARG002
        """An index of this class over gathered rows, local rows from 0: what a view searches.  Its width is the STORED one
        (the view hands it queries padded like the rows)."""
        return ItemIndex(embeddings)

    def _where_groups(self, where, nq: int):
        """A sequence of per-query filters -> ``[(filter, query numbers int64 on the host)]``, one entry per distinct filter in
        the order of first appearance."""
        if len(where) != nq:
            msg = f"one filter per query expected: {len(where) = }, {nq = }"
            raise ValueError(msg)
        groups: dict = {}
        for i, f in enumerate(where):
            if not isinstance(f, TagFilter):
                msg = f"a sequence of filters holds TagFilters: {f!r}"
                raise ValueError(msg)
            groups.setdefault(f, []).append(i)
        return [(f, torch.tensor(qs, dtype=torch.int64)) for f, qs in groups.items()]

    @staticmethod
    def _sub_csr(csr, exclude, qs: torch.Tensor, device):
        """The lists of the queries ``qs`` (host int64), from a device CSR (sizing the result is a host read) or host lists: a
        device CSR ``(offsets, entries -- exactly as many as the lists hold)`` or None."""
        if csr is not None:
            off, ids = csr
            sel = qs.to(device)
            lens = off[sel + 1] - off[sel]
            sub_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), torch.cumsum(lens, 0)])
            owner = torch.repeat_interleave(torch.arange(sel.numel(), device=device), lens)
            at = off[sel][owner] + torch.arange(owner.numel(), device=device) - sub_off[owner]
            return sub_off, ids[at]
        if exclude is not None:
            return _csr([exclude[i] for i in qs.tolist()], qs.numel(), device)
        return None

    def _search_groups(self, q: torch.Tensor, top_k: int, where, exclude, exclude_csr, kw) -> tuple[torch.Tensor, torch.Tensor]:
        nq = q.shape[0]
        if exclude is not None and len(exclude) != nq:
            msg = f"one exclusion list per query expected: {len(exclude) = }, {nq = }"
            raise ValueError(msg)
        scores = torch.empty(nq, top_k, dtype=torch.float32, device=q.device)
        rows = torch.empty(nq, top_k, dtype=torch.int64, device=q.device)
        for f, qs in self._where_groups(where, nq):
            sel = qs.to(q.device)
            sub = self._sub_csr(exclude_csr, exclude, qs, q.device)
            s, r = self.filtered(f).search(q[sel], top_k, exclude_csr=sub, **kw)
            scores[sel], rows[sel] = s, r
        return scores, rows

    def _workspace(self, key, nbytes: int) -> torch.Tensor:
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[key] = _lib.workspace(nbytes, self.embeddings.device)
        return ws

    @property
    def num_items(self) -> int:
        return self.embeddings.shape[0]

    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        """The queries as the engines take them: fp32 on the device, ``[Q, dim]``, padded to the catalog's width."""
        q = _lib.dev_f32(queries, "queries")
        if q.dim() != 2 or q.shape[1] != self.dim:
            msg = f"queries should be (num_queries, {self.dim}): {tuple(q.shape) = }"
            raise ValueError(msg)
        if self.embeddings.shape[1] != self.dim:
            q = torch.nn.functional.pad(q, (0, self.embeddings.shape[1] - self.dim))
        return q

    def positions(self, queries: torch.Tensor, targets_csr: tuple[torch.Tensor, torch.Tensor], *,
                  exclude: Sequence[Sequence[int]] | None = None,
                  exclude_csr: tuple[torch.Tensor, torch.Tensor] | None = None,
                  where=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(pos int64 [T], score fp32 [T], ncand int64 [Q])``: for every entry of ``targets_csr = (offsets [Q + 1], GLOBAL
        item rows [T])`` its exact place among the query's admissible rows -- the rows ``search`` selects from, in its order
        (0 = best) -- and its score; -1 / -inf for a row that is excluded or outside the catalog.  ``ncand`` is the number of
        admissible rows per query.  A position below ``k`` is the column ``search(..., k, path="deep")`` returns the row at
        (``mf_target_positions``: no list is built, so there is no deepest k).  ``where`` (a ``TagFilter``, an allow-mask or one
        ``TagFilter`` per query): the rows it does not admit count as excluded (``filtered``)."""
        if where is not None:
            return self._positions_where(queries, targets_csr, where, exclude, exclude_csr)
        q = self._queries(queries)
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        t_off, t_ids = (_lib.dev_i64(t, name) for t, name in zip(targets_csr, ("target offsets", "target rows")))
        if t_off.numel() != nq + 1:
            msg = f"one target list per query expected: {t_off.numel() = }, {nq = }"
            raise ValueError(msg)
        off, ids = exclude_csr if exclude_csr is not None else _csr(exclude, nq, q.device)
        nt = t_ids.numel()
        pos = torch.empty(nt, dtype=torch.int64, device=q.device)
        score = torch.empty(nt, dtype=torch.float32, device=q.device)
        ncand = torch.empty(nq, dtype=torch.int64, device=q.device)
        if nt == 0:       # keep the pointers valid
            t_ids, pos_arg, score_arg = (torch.zeros(1, dtype=dt, device=q.device) for dt in (torch.int64, torch.int64, torch.float32))
        else:
            pos_arg, score_arg = pos, score
        lib = _lib.lib()
        ws = self._workspace(("positions", nq), lib.mf_target_positions_ws_bytes(nq, n, d))
        _lib.check(lib.mf_target_positions(q.data_ptr(), nq, self.embeddings.data_ptr(), n, d, t_off.data_ptr(), t_ids.data_ptr(), nt,
                                           _lib.ptr(off), _lib.ptr(ids), self.idx_base, ws.data_ptr(), ws.numel(), pos_arg.data_ptr(),
                                           score_arg.data_ptr(), ncand.data_ptr(), _lib.stream_ptr()))
        return pos, score, ncand

    def _positions_where(self, queries, targets_csr, where, exclude, exclude_csr):
        if not _is_filter_sequence(where):
            return self.filtered(where).positions(queries, targets_csr, exclude=exclude, exclude_csr=exclude_csr)
        q = self._queries(queries)
        nq = q.shape[0]
        t_off, t_ids, nt = self._targets(nq, targets_csr, q.device)
        if exclude is not None and len(exclude) != nq:
            msg = f"one exclusion list per query expected: {len(exclude) = }, {nq = }"
            raise ValueError(msg)
        pos = torch.empty(nt, dtype=torch.int64, device=q.device)
        score = torch.empty(nt, dtype=torch.float32, device=q.device)
        ncand = torch.empty(nq, dtype=torch.int64, device=q.device)
        entry = torch.arange(nt, dtype=torch.int64, device=q.device)
        for f, qs in self._where_groups(where, nq):
            sel = qs.to(q.device)
            sub_off, sub_at = self._sub_csr((t_off, entry), None, qs, q.device)      # (the entries' numbers: where the answers go)
            p, s, c = self.filtered(f).positions(q[sel], (sub_off, t_ids[sub_at]), exclude_csr=self._sub_csr(exclude_csr, exclude, qs, q.device))
            pos[sub_at], score[sub_at], ncand[sel] = p, s, c
        return pos, score, ncand

    def _targets(self, nq: int, targets_csr, device) -> tuple[torch.Tensor, torch.Tensor, int]:
        """A target CSR as the shard exports take it: ``(offsets, rows -- one valid word when the lists are empty, entries)``."""
        t_off, t_ids = (_lib.dev_i64(t, name) for t, name in zip(targets_csr, ("target offsets", "target rows")))
        if t_off.numel() != nq + 1:
            msg = f"one target list per query expected: {t_off.numel() = }, {nq = }"
            raise ValueError(msg)
        nt = t_ids.numel()
        return t_off, (t_ids if nt else torch.zeros(1, dtype=torch.int64, device=device)), nt

    @staticmethod
    def _shard_map(stride: int, offset: int) -> tuple[int, int]:
        stride, offset = int(stride), int(offset)
        if stride < 1 or offset < 0:
            msg = f"global row = local row * stride + offset needs stride >= 1 and offset >= 0: {stride = }, {offset = }"
            raise ValueError(msg)
        return stride, offset

    def target_words(self, queries: torch.Tensor, targets_csr: tuple[torch.Tensor, torch.Tensor], *, stride: int = 1,
                     offset: int = 0) -> torch.Tensor:
        """``int64 [T]``: for every entry of ``targets_csr = (offsets [Q + 1], GLOBAL item rows [T])`` whose row this index
        holds -- local row l is global row ``l * stride + offset`` -- the 32-bit order word of its score (``mf_orderable`` of
        the chain score: the word the searches rank by), 0 for a row it does not hold.  Exclusion lists play no part.  The
        first half of positions over a row-sharded catalog (``mf_target_words``): the maximum over the shards is the word
        ``key_positions`` takes."""
        q = self._queries(queries)
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        stride, offset = self._shard_map(stride, offset)
        t_off, t_ids, nt = self._targets(nq, targets_csr, q.device)
        words = torch.empty(nt, dtype=torch.int64, device=q.device)
        out = words if nt else torch.zeros(1, dtype=torch.int64, device=q.device)       # keep the pointer valid
        _lib.check(_lib.lib().mf_target_words(q.data_ptr(), nq, self.embeddings.data_ptr(), n, d, t_off.data_ptr(), t_ids.data_ptr(), nt,
                                              stride, offset, out.data_ptr(), _lib.stream_ptr()))
        return words

    def key_positions(self, queries: torch.Tensor, targets_csr: tuple[torch.Tensor, torch.Tensor], words: torch.Tensor, *,
                      stride: int = 1, offset: int = 0,
                      exclude_local_csr: tuple[torch.Tensor, torch.Tensor] | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(above int64 [T], score fp32 [T], ncand int64 [Q])``: this shard's share of every target's position.  ``words``
        are the targets' order words after the maximum over all shards (``target_words``); ``above[e]`` counts this shard's
        admissible rows that stand before target e in the GLOBAL order (word descending, then global row ascending), or is
        -1 when the word is 0 or this shard holds the row and finds it excluded; ``ncand`` counts the shard's admissible
        rows.  Summed over the shards they are ``positions`` on the whole catalog.  ``exclude_local_csr``: per-query lists of
        LOCAL rows (entries outside the shard are ignored).  ``mf_key_positions``."""
        q = self._queries(queries)
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        stride, offset = self._shard_map(stride, offset)
        t_off, t_ids, nt = self._targets(nq, targets_csr, q.device)
        w = _lib.dev_i64(words, "words")
        if w.numel() != nt:
            msg = f"one word per target entry expected: {w.numel() = }, {nt = }"
            raise ValueError(msg)
        off, ids = exclude_local_csr if exclude_local_csr is not None else (None, None)
        above = torch.empty(nt, dtype=torch.int64, device=q.device)
        score = torch.empty(nt, dtype=torch.float32, device=q.device)
        ncand = torch.empty(nq, dtype=torch.int64, device=q.device)
        if nt == 0:       # keep the pointers valid
            w, above_arg, score_arg = (torch.zeros(1, dtype=dt, device=q.device) for dt in (torch.int64, torch.int64, torch.float32))
        else:
            above_arg, score_arg = above, score
        lib = _lib.lib()
        ws = self._workspace(("positions", nq), lib.mf_key_positions_ws_bytes(nq, n, d))
        _lib.check(lib.mf_key_positions(q.data_ptr(), nq, self.embeddings.data_ptr(), n, d, t_off.data_ptr(), t_ids.data_ptr(), w.data_ptr(),
                                        nt, stride, offset, _lib.ptr(off), _lib.ptr(ids), ws.data_ptr(), ws.numel(), above_arg.data_ptr(),
                                        score_arg.data_ptr(), ncand.data_ptr(), _lib.stream_ptr()))
        return above, score, ncand

    def search(self, queries: torch.Tensor, top_k: int = TOP_K, *, exclude: Sequence[Sequence[int]] | None = None,
               exclude_csr: tuple[torch.Tensor, torch.Tensor] | None = None,
               path: str = "auto", where=None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(scores [Q, k] fp32, rows [Q, k] int64)``, best first; ``exclude`` holds GLOBAL
        item rows per query (or pass a prebuilt device CSR with sorted ids).  ``path``: "scan" = the
        matrix-vector kernel (at most ``SMALL_Q`` queries), "tiles" = the fp32 MFMA tile engine, "bf16" = two bf16
        MFMA scans that pick the few dozen rows per query worth an exact fp32 score (d >= 64), "deep" = score once, then
        a radix select per query (``mf_topk_deep``: any ``top_k`` up to ``DEEP_MAX_K``; the other three stop at
        ``TILE_MAX_K``); "auto" takes "deep" exactly when ``top_k > TILE_MAX_K`` and otherwise picks by the number of
        queries; all four give the same bits.  ``where`` (a ``TagFilter``, a ``bool [num_items]`` allow-mask, or a sequence of
        one ``TagFilter`` per query): only the rows it admits are candidates -- the same search through ``filtered(where)``, bit
        for bit what this search returns with every other row on every query's exclusion list."""
        if where is not None:
            if _is_filter_sequence(where):
                return self._search_groups(self._queries(queries), int(top_k), where, exclude, exclude_csr, {"path": path})
            return self.filtered(where).search(queries, top_k, exclude=exclude, exclude_csr=exclude_csr, path=path)
        q = self._queries(queries)
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        off, ids = exclude_csr if exclude_csr is not None else _csr(exclude, nq, q.device)
        if path not in self.PATHS:
            msg = f"path must be 'auto', 'scan', 'tiles', 'bf16' or 'deep': {path = }"
            raise ValueError(msg)
        if path == "bf16" and d < 64:
            msg = f"the bf16 path needs an embedding width of at least 64: {d = }"
            raise ValueError(msg)
        if path == "scan" and nq > self.SMALL_Q:
            msg = f"the scan path takes at most {self.SMALL_Q} queries: {nq = }"
            raise ValueError(msg)
        if path == "deep" or (path == "auto" and top_k > self.TILE_MAX_K):
            return self._run("deep", q, top_k, off, ids)
        # the few-query scan matches exclusion entries against every 64-row block: staged in LDS up to SCAN_MAX_EXCL entries
        # (all queries together), a walk over each query's list per block beyond -- measured at N = 62,423: Q = 8 x 2,000 ids
        # 89 us, Q = 32 x 30,000 ids 4 ms, against 46 / 85 us through the prefilter (which builds bit rows once).  So "auto"
        # sends long lists -- a heavy user's history -- to the other engines
        entries = 0 if ids is None else int(ids.numel())
        bf16_ok = n >= self.BF16_MIN_N and d >= 64
        scan_ok = nq <= self.AUTO_SMALL_Q and (entries <= self.SCAN_MAX_EXCL or not bf16_ok and entries <= 16 * self.SCAN_MAX_EXCL)
        if path == "scan" or (path == "auto" and scan_ok):
            # the reference's own shape: one query (or a handful) per call -- bandwidth-bound scan, two launches
            return self._run("scan", q, top_k, off, ids)
        if path == "bf16" or (path == "auto" and (nq >= self.BF16_MIN_Q or not scan_ok) and bf16_ok):
            # a shape outside the prefilter's descriptor limits (MF_ENOTSUP, decided on the host before any launch) goes
            # to the fp32 tile engine when the caller left the choice to us; an explicit path="bf16" raises
            out = self._run("bf16", q, top_k, off, ids, refusal_ok=path == "auto")
            if out is not None:
                return out
        return self._run("tiles", q, top_k, off, ids)

    def default_path(self, top_k: int) -> str:  # noqa: ARG002
        """The ``path`` a caller that only knows ``top_k`` should pass to ``search`` (``ItemProcessor``, the module's metrics and
        predictions): ``"auto"`` here, the cell scan that serves the depth on a ``PartitionedIndex``, ``"pq"`` on a quantised one."""
        return "auto"

    def serving_path(self, top_k: int) -> str:
        """The ``path`` that serves ``top_k`` rows at every depth the index has a search for -- what ``ItemProcessor.search``, the
        module's metrics and its predictions pass.  ``default_path`` here and on a ``PartitionedIndex``; a ``QuantizedIndex`` sends
        lists beyond ``TILE_MAX_K`` rows to its deep search."""
        return self.default_path(top_k)

    # engine ->(workspace-size export, search export, workspace key, the source tensors behind the queries)
    _ENGINES = {
        "deep": ("mf_topk_deep_ws_bytes", "mf_topk_deep", "deep", lambda self: (self.embeddings,)),
        "scan": ("mf_topk_small_ws_bytes", "mf_topk_small", "small", lambda self: (self.blocked(),)),
        "bf16": ("mf_topk_bf3_ws_bytes", "mf_topk_bf3", "bf16", lambda self: (self.embeddings, self.bf16_index())),
        "tiles": ("mf_topk_ws_bytes", "mf_topk", "tile", lambda self: (self.embeddings,)),
    }

    def _run(self, engine: str, q: torch.Tensor, top_k: int, off, ids, refusal_ok: bool = False):
        """One engine's search export on its kept workspace: ``(scores, rows)``, or None for MF_ENOTSUP with ``refusal_ok``."""
        ws_bytes, export, key, sources = self._ENGINES[engine]
        lib = _lib.lib()
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        scores = torch.empty(nq, top_k, dtype=torch.float32, device=q.device)
        rows = torch.empty(nq, top_k, dtype=torch.int64, device=q.device)
        ws = self._workspace((key, nq, top_k), getattr(lib, ws_bytes)(nq, n, d, top_k))
        rc = getattr(lib, export)(q.data_ptr(), nq, *(t.data_ptr() for t in sources(self)), n, d, top_k, _lib.ptr(off), _lib.ptr(ids),
                                  self.idx_base, ws.data_ptr(), ws.numel(), scores.data_ptr(), rows.data_ptr(), _lib.stream_ptr())
        if rc == _lib.MF_ENOTSUP and refusal_ok:
            return None
        _lib.check(rc)
        return scores, rows


def default_num_partitions(num_items: int) -> int:
    """The reference's default (``num_partitions = 2 ** int(log2(num_items) / 2)``, data/lightning.py:203), within 1..N."""
    n = int(num_items)
    return max(1, min(n, 2 ** int(math.log2(max(n, 1)) / 2)))


def partition_layout(assign: torch.Tensor, num_partitions: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Where the rows of a catalog go when it is stored cell by cell: ``(perm [N], cell_blk [C + 1], row_of [Npad])``, all
    int64 on ``assign``'s device.  ``assign[r]`` in ``[0, C)`` is row r's cell.  ``perm`` lists the rows by cell, inside a cell
    in ascending row (a stable sort); every cell is padded to a multiple of 64 rows; ``cell_blk[c]`` is the first 64-row block
    of cell c (``cell_blk[c] == cell_blk[c + 1]``: an empty cell, ``Npad = 64 * cell_blk[C]``); ``row_of[p]`` is the row at
    padded position p, -1 for padding.  Torch ops only."""
    c = int(num_partitions)
    if assign.dim() != 1 or assign.dtype != torch.int64 or assign.numel() == 0 or c < 1:
        msg = f"assign should be a non-empty int64 vector and num_partitions >= 1: {tuple(assign.shape) = }, {assign.dtype = }, {c = }"
        raise ValueError(msg)
    if int(assign.min()) < 0 or int(assign.max()) >= c:
        msg = f"cells must lie in [0, {c}): {int(assign.min()) = }, {int(assign.max()) = }"
        raise ValueError(msg)
    dev = assign.device
    sorted_cell, perm = torch.sort(assign, stable=True)
    bounds = torch.searchsorted(sorted_cell, torch.arange(c + 1, dtype=torch.int64, device=dev))      # first sorted place of every cell
    blocks = (bounds[1:] - bounds[:-1] + 63) // 64
    cell_blk = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(blocks, 0)])
    at = cell_blk[sorted_cell] * 64 + (torch.arange(assign.numel(), dtype=torch.int64, device=dev) - bounds[sorted_cell])
    row_of = torch.full((int(cell_blk[-1]) * 64,), -1, dtype=torch.int64, device=dev)
    row_of[at] = perm
    return perm, cell_blk, row_of


class CellMask:
    """Allow bitmaps over a partitioned index's cell order (``PartitionedIndex.cell_mask``): ``words``, ``int64 [F, Npad // 64]`` on
    the device -- the bit patterns of ``F`` masks' 64-bit words, bit ``lane`` of word ``blk`` set iff the row at cell-ordered
    position ``blk * 64 + lane`` is admissible (``mf_filter_cell_bits``) -- and ``row_of``, the layout they were built for: a
    search takes a mask only on the index whose ``row_of`` is that very tensor, so a mask from before ``rebuild()`` is refused.
    ``Npad / 8`` bytes per mask, where a view (``filtered``) copies its rows."""

    def __init__(self, words: torch.Tensor, row_of: torch.Tensor) -> None:
        self.words, self.row_of = words, row_of

    @property
    def num_masks(self) -> int:
        return self.words.shape[0]


class PartitionedIndex(ItemIndex):
    """An ``ItemIndex`` that can also search like the reference's inverted-file index (``get_index`` builds ``num_partitions``
    cells, ``search`` visits ``num_probes = 8`` of them: data/lightning.py:203, 222-229, 250-259): the catalog is kept a second
    time ordered by cell, and ``search`` scans the ``nprobe`` cells whose centroids score best against the query.  Which rows are
    looked at is the only approximation: every row looked at is scored and ordered exactly, so the result is bit for bit the
    exact engines' answer over the union of the probed cells, and ``nprobe = num_partitions`` gives ``ItemIndex.search``'s.
    The original matrix stays: ``positions``, ``target_words`` and ``search(path="exact")`` are the parent's, on all rows.
    The reference's ``refine_factor`` and ``num_sub_vectors`` belong to its product quantiser: ``QuantizedIndex`` below adds
    it to these cells; here every probed row is scored exactly, so there is nothing to refine."""

    MAX_PROBES = 64     # cells one query may visit (mf_ivf_scan)
    ASSIGN_BATCH = 16384       # rows per nearest-centroid search of the build

    def __init__(self, embeddings: torch.Tensor, centroids: torch.Tensor, assign: torch.Tensor, *, idx_base: int = 0,
                 num_probes: int = 8) -> None:
        super().__init__(embeddings, idx_base=idx_base)
        self.num_probes = int(num_probes)
        self._build_args: dict | None = None             # how ``build`` made this index: ``rebuild`` runs it again
        self._install(centroids, assign)

    @classmethod
    def from_assignment(cls, embeddings: torch.Tensor, centroids: torch.Tensor, assign: torch.Tensor, *, idx_base: int = 0,
                        num_probes: int = 8) -> "PartitionedIndex":
        """The index over given cells: ``centroids [C, dim]``, ``assign [N]`` int64 in ``[0, C)`` (cells may be empty)."""
        return cls(embeddings, centroids, assign, idx_base=idx_base, num_probes=num_probes)

    @classmethod
    def build(cls, embeddings: torch.Tensor, num_partitions: int | None = None, *, iters: int = 10, seed: int = 0,
              num_probes: int = 8, idx_base: int = 0) -> "PartitionedIndex":
        """Cells by spherical k-means, the same for the same rows and seed: the first centroids are the rows at the first C
        places of a permutation drawn on the host; an iteration puts every row in the cell of its best centroid (the exact
        engines' top-1: chain score, lowest cell on ties) and replaces every centroid by the unit-length mean of its rows,
        added in row order (``mf_ivf_cell_mean``); an empty cell keeps its centroid.  A last assignment follows the last
        update, so every row lies in the cell of its best final centroid.  ``num_partitions=None``: the reference's default."""
        index = cls.__new__(cls)
        ItemIndex.__init__(index, embeddings, idx_base=idx_base)
        index.num_probes = int(num_probes)
        n = index.num_items
        c = default_num_partitions(n) if num_partitions is None else int(num_partitions)
        if not 1 <= c <= n or iters < 0:
            msg = f"num_partitions must be in 1..{n} and iters >= 0: {c = }, {iters = }"
            raise ValueError(msg)
        index._build_args = {"num_partitions": c, "iters": int(iters), "seed": int(seed)}
        index._install(*index._kmeans(c, int(iters), int(seed)))
        return index

    def _assign(self, centroids: torch.Tensor) -> torch.Tensor:
        coarse = ItemIndex(centroids)
        rows = self.embeddings
        out = [coarse.search(rows[a : a + self.ASSIGN_BATCH], 1)[1][:, 0] for a in range(0, rows.shape[0], self.ASSIGN_BATCH)]
        return torch.cat(out)

    def _kmeans(self, c: int, iters: int, seed: int) -> tuple[torch.Tensor, torch.Tensor]:
        emb = self.embeddings
        n, d = emb.shape
        first = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:c]
        centroids = emb[first.to(emb.device)].clone()
        lib = _lib.lib()
        edges = torch.arange(c + 1, dtype=torch.int64, device=emb.device)
        for _ in range(iters):
            cells, order = torch.sort(self._assign(centroids), stable=True)
            cell_off = torch.searchsorted(cells, edges)
            _lib.check(lib.mf_ivf_cell_mean(emb.data_ptr(), n, d, order.data_ptr(), cell_off.data_ptr(), c, 1, centroids.data_ptr(),
                                            _lib.stream_ptr()))
        return centroids, self._assign(centroids)

    def _install(self, centroids: torch.Tensor, assign: torch.Tensor) -> None:
        cen = _lib.dev_f32(centroids.detach(), "centroids")
        if cen.dim() != 2 or cen.shape[0] < 1 or cen.shape[1] not in (self.dim, self.embeddings.shape[1]):
            msg = f"centroids should be (num_partitions, {self.dim}): {tuple(cen.shape) = }"
            raise ValueError(msg)
        if cen.shape[1] != self.embeddings.shape[1]:
            cen = torch.nn.functional.pad(cen, (0, self.embeddings.shape[1] - cen.shape[1]))
        a = _lib.dev_i64(assign, "assign").reshape(-1)
        if a.numel() != self.num_items:
            msg = f"one cell per row expected: {a.numel() = }, {self.num_items = }"
            raise ValueError(msg)
        self.centroids = cen.contiguous()
        self.assign = a
        self.num_partitions = cen.shape[0]
        self.perm, self.cell_blk, self.row_of = partition_layout(a, self.num_partitions)
        self.max_cell_blocks = int((self.cell_blk[1:] - self.cell_blk[:-1]).max())
        self.coarse = ItemIndex(self.centroids)
        self._cells = None
        self._views.clear()                              # (a view keeps the cells of its build)
        self._masks: dict = {}                           # TagFilter -> CellMask of these cells (cell_mask)

    def _sub_index(self, embeddings: torch.Tensor, rows: torch.Tensor) -> "PartitionedIndex":
        """The view's index keeps the cells: the same centroids, every gathered row in the cell it had -- so the same probes."""
        return PartitionedIndex.from_assignment(embeddings, self.centroids, self.assign[rows], num_probes=self.num_probes)

    def set_tags(self, tags: torch.Tensor) -> None:
        """The parent's; the cached masks of ``cell_mask`` were evaluated on the old tags and go with the views."""
        super().set_tags(tags)
        self._masks.clear()

    def cell_mask(self, where, *, cache: bool = True) -> CellMask:
        """The allow bitmap(s) of ``where`` over this index's cells, for ``search(allow=...)``: a ``TagFilter`` over ``tags``, a
        ``bool [num_items]`` tensor (the same kernel with the mask as the tag word and ``all_of = 1``), or a sequence of these
        (``F`` masks in one tensor, one ``mf_filter_cell_bits`` launch each; a search names each query's mask by ``allow_of``).
        No host read and no copy of rows: ``Npad / 8`` bytes per mask.  The mask of a single ``TagFilter`` is kept per index
        (``cache=False``: neither looked up nor kept) until ``set_tags()``, ``rebuild()`` or a new assignment -- and, unlike a
        view, through ``refresh()``: a mask depends on the tags and the cells, not on the rows' values."""
        if isinstance(where, CellMask):
            return where
        single = not _is_filter_sequence(where)
        filters = [where] if single else list(where)
        if not filters:
            msg = "a sequence of filters must not be empty"
            raise ValueError(msg)
        n, dev = self.num_items, self.embeddings.device
        for f in filters:
            if isinstance(f, TagFilter):
                if self.tags is None:
                    msg = "a TagFilter needs the rows' tags: call set_tags first"
                    raise ValueError(msg)
            elif not (isinstance(f, torch.Tensor) and f.dtype == torch.bool and f.shape == (n,)):
                msg = f"a filter should be a TagFilter or a bool tensor of shape ({n},): {f!r}"
                raise ValueError(msg)
        keyed = single and cache and isinstance(where, TagFilter)
        if keyed and where in self._masks:
            return self._masks[where]
        lib = _lib.lib()
        npad = self.row_of.numel()
        words = torch.empty(len(filters), npad // 64, dtype=torch.int64, device=dev)
        for i, f in enumerate(filters):
            tag_words, f = (self.tags, f) if isinstance(f, TagFilter) else (f.to(dev).to(torch.int64), TagFilter(all_of=1))
            _lib.check(lib.mf_filter_cell_bits(tag_words.data_ptr(), n, f.any_of, f.all_of, f.none_of, self.row_of.data_ptr(), npad,
                                               words[i].data_ptr(), _lib.stream_ptr()))
        mask = CellMask(words, self.row_of)
        if keyed:
            self._masks[where] = mask
        return mask

    def _allow_route(self, allow, allow_of, where, path: str, paths: tuple) -> None:
        """What ``search`` can refuse about ``allow`` / ``allow_of`` before it has looked at the queries: nothing is launched."""
        if allow is None:
            if allow_of is not None:
                msg = "allow_of names the masks of allow=: it needs one"
                raise ValueError(msg)
            return
        if where is not None:
            msg = "allow= and where= are two routes for one filter: give one of them"
            raise ValueError(msg)
        if path not in paths:
            msg = f"allow= filters the cell scans in place (path in {paths}); the exact engines have no bitmap route: {path = }"
            raise ValueError(msg)
        if isinstance(allow, CellMask) and allow.row_of is not self.row_of:
            msg = "this CellMask was built for another cell layout (before rebuild(), or on another index): build it again"
            raise ValueError(msg)

    def _allow_masks(self, allow, allow_of, nq: int):
        """``allow`` / ``allow_of`` (``_allow_route`` has passed them) for ``nq`` checked queries -> ``(CellMask, allow_of int64 [Q]
        on the device or None)``, ``(None, None)`` without ``allow``.  A mask given as a filter is built here, after every
        refusal."""
        if allow is None:
            return None, None
        if type(allow) is CellMask and allow_of is None and allow.words.shape[0] == 1:      # (the common call, kept short: it is timed
            return allow, None                                                               #  beside the unfiltered search)
        num_masks = allow.num_masks if isinstance(allow, CellMask) else len(allow) if _is_filter_sequence(allow) else 1
        if allow_of is None:
            if num_masks != 1:
                msg = f"{num_masks} masks need allow_of: one mask number per query"
                raise ValueError(msg)
        else:
            allow_of = torch.as_tensor(allow_of)
            if allow_of.dtype != torch.int64 or allow_of.shape != (nq,):
                msg = f"allow_of should be an int64 vector with one mask number per query ({nq}): {allow_of.dtype}, {tuple(allow_of.shape)}"
                raise ValueError(msg)
            allow_of = allow_of.to(self.embeddings.device).contiguous()
        return self.cell_mask(allow), allow_of

    def cell_blocked(self) -> torch.Tensor:
        """The catalog ordered by cell (``row_of``; padding rows zero) in the blocked layout of ``mf_topk_small``
        (``mf_topk_blocked_build`` on the padded matrix), built once: what the cell search reads where the few-query scan
        reads ``blocked()``.  (``blocked()`` itself stays the parent's, in row order, and is only built if ``path="scan"`` or an
        exact search of a few queries asks for it.)"""
        if self._cells is None:
            lib = _lib.lib()
            npad, d = self.row_of.numel(), self.embeddings.shape[1]
            padded = self.embeddings[self.row_of.clamp(min=0)]
            padded.masked_fill_((self.row_of < 0).unsqueeze(1), 0.0)
            out = torch.empty(lib.mf_topk_blocked_bytes(npad, d) // 4, dtype=torch.float32, device=padded.device)
            _lib.check(lib.mf_topk_blocked_build(padded.data_ptr(), npad, d, out.data_ptr(), _lib.stream_ptr()))
            self._cells = out
        return self._cells

    def refresh(self) -> None:
        """Forget the derived copies (the cell-ordered one too); the cells stay as they are -- ``rebuild()`` for new ones."""
        super().refresh()
        self._cells = None

    def rebuild(self) -> None:
        """Run the build again on the rows as they are now (an index from ``from_assignment`` keeps its cells and only
        forgets the derived copies)."""
        self.refresh()
        self._masks.clear()
        if self._build_args is not None:
            b = self._build_args
            self._install(*self._kmeans(b["num_partitions"], b["iters"], b["seed"]))

    def _top_k(self, top_k: int, search: str) -> int:
        top_k = int(top_k)
        if not 1 <= top_k <= self.TILE_MAX_K:
            msg = f"the {search} search returns 1..{self.TILE_MAX_K} rows per query: {top_k = }"
            raise ValueError(msg)
        return top_k

    def _nprobe(self, nprobe: int | None) -> int:
        nprobe = self.num_probes if nprobe is None else int(nprobe)
        if not 1 <= nprobe <= min(self.num_partitions, self.MAX_PROBES):
            msg = f"nprobe must be in 1..{min(self.num_partitions, self.MAX_PROBES)}: {nprobe = }"
            raise ValueError(msg)
        return nprobe

    def _plan(self, export, num_queries: int, nprobe: int, depth: int) -> dict[str, int]:
        """The four words of a plan export (``mf_ivf_plan``, ``mf_pq_plan``: one rule, csrc/mf_cells.h) for lists of ``depth``."""
        out = (ctypes.c_int64 * 4)()
        _lib.check(export(int(num_queries), nprobe, depth, self.max_cell_blocks, out))
        return {"slices": out[0], "lists": out[1], "workgroups": out[2], "bytes": out[3]}

    def plan(self, num_queries: int, top_k: int = TOP_K, nprobe: int | None = None, path: str = "cells") -> dict[str, int]:
        """The geometry ``search`` runs with (``mf_ivf_plan``; ``path="cells_deep"``: ``mf_ivf_deep_plan``): slices per cell, partial
        lists per query, workgroups."""
        export = _lib.lib().mf_ivf_deep_plan if path == "cells_deep" else _lib.lib().mf_ivf_plan
        return self._plan(export, num_queries, self.num_probes if nprobe is None else int(nprobe), int(top_k))

    def default_path(self, top_k: int) -> str:
        """The cell scan that serves ``top_k``: a list per wavefront up to ``TILE_MAX_K`` rows, the deep scan beyond."""
        return "cells" if int(top_k) <= self.TILE_MAX_K else "cells_deep"

    def _deep_top_k(self, top_k: int, nprobe: int) -> int:
        """``path="cells_deep"``'s depth: 1..``DEEP_MAX_K``, and a list per probe at least within the deep merge's keys."""
        top_k = int(top_k)
        if not 1 <= top_k <= self.DEEP_MAX_K:
            msg = f"the deep partitioned search returns 1..{self.DEEP_MAX_K} rows per query: {top_k = }"
            raise ValueError(msg)
        if nprobe * top_k > MERGE_DEEP_MAX_KEYS:
            msg = f"nprobe * top_k must not exceed {MERGE_DEEP_MAX_KEYS} (the keys the merge of the lists holds): {nprobe = }, {top_k = }"
            raise ValueError(msg)
        return top_k

    def search(self, queries: torch.Tensor, top_k: int = TOP_K, *, exclude: Sequence[Sequence[int]] | None = None,
               exclude_csr: tuple[torch.Tensor, torch.Tensor] | None = None, nprobe: int | None = None,
               path: str = "cells", where=None, allow=None, allow_of=None) -> tuple[torch.Tensor, torch.Tensor]:
        """``ItemIndex.search``'s inputs and result -- shapes, dtypes, the -inf / -1 tail -- over the rows of the ``nprobe``
        cells (default ``num_probes``) whose centroids score best against each query (exact, lowest cell on ties).
        ``path="cells"``: three launches' worth of stages, none with a host read -- the cells (the exact engines on the centroid
        matrix), the scan (``mf_ivf_scan``), the merge (``mf_topk_merge_packed``).  ``path="exact"`` is the parent's search over
        the whole catalog ("auto"); any other path is passed to the parent as it is.  ``where``: as in the parent -- the view
        keeps the cells, so the probes are the same and the result is this search's with the inadmissible rows excluded; for a
        filter without the view's copy, its host read and its per-filter grouping, see ``allow``.  ``path="cells_deep"``: the same
        contract and the same three stages for ``1 <= top_k <= DEEP_MAX_K`` (``mf_ivf_scan_deep``, ``mf_topk_merge_packed_deep``;
        ``"cells"`` stops at ``TILE_MAX_K``, a list per wavefront) with ``nprobe * top_k`` within ``MERGE_DEEP_MAX_KEYS`` -- bit for
        bit ``ItemIndex.search(path="deep")`` with the rows outside the probed cells excluded.  ``allow`` (the two cell paths
        only): a ``CellMask`` or anything ``cell_mask`` takes -- the scan filters in place (``mf_ivf_scan_allow``), the same
        result bit for bit; with several masks ``allow_of`` (``int64 [Q]``, host or device) names each query's, and a number
        outside ``[0, F)`` admits nothing for that query."""
        self._allow_route(allow, allow_of, where, path, ("cells", "cells_deep"))
        if where is not None:
            kw = {"nprobe": nprobe, "path": path}
            if _is_filter_sequence(where):
                return self._search_groups(self._queries(queries), int(top_k), where, exclude, exclude_csr, kw)
            return self.filtered(where).search(queries, top_k, exclude=exclude, exclude_csr=exclude_csr, **kw)
        if path not in ("cells", "cells_deep"):
            return super().search(queries, top_k, exclude=exclude, exclude_csr=exclude_csr, path="auto" if path == "exact" else path)
        deep = path == "cells_deep"
        nprobe = self._nprobe(nprobe)
        top_k = self._deep_top_k(top_k, nprobe) if deep else self._top_k(top_k, "partitioned")
        q = self._queries(queries)
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        mask, allow_of = self._allow_masks(allow, allow_of, nq)
        off, ids = exclude_csr if exclude_csr is not None else _csr(exclude, nq, q.device)
        _, probes = self.coarse.search(q, nprobe)
        lib = _lib.lib()
        scores = torch.empty(nq, top_k, dtype=torch.float32, device=q.device)
        rows = torch.empty(nq, top_k, dtype=torch.int64, device=q.device)
        ws_bytes, scan_plain, scan_allow, merge = (
            (lib.mf_ivf_deep_ws_bytes, lib.mf_ivf_scan_deep, lib.mf_ivf_scan_deep_allow, lib.mf_topk_merge_packed_deep) if deep else
            (lib.mf_ivf_ws_bytes, lib.mf_ivf_scan, lib.mf_ivf_scan_allow, lib.mf_topk_merge_packed))
        ws = self._workspace((path, nq, nprobe, top_k), ws_bytes(nq, nprobe, top_k, self.max_cell_blocks))
        lists = PartitionedIndex.plan(self, nq, top_k, nprobe, path)["lists"]      # (this scan's plan, whatever a subclass plans by default)
        scan = (q.data_ptr(), nq, self.cell_blocked().data_ptr(), self.cell_blk.data_ptr(), self.row_of.data_ptr(), self.row_of.numel(), n,
                self.num_partitions, d, self.max_cell_blocks, probes.data_ptr(), nprobe, top_k, 0, _lib.ptr(off), _lib.ptr(ids), self.idx_base)
        if mask is None:
            _lib.check(scan_plain(*scan, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        else:
            _lib.check(scan_allow(*scan, mask.words.data_ptr(), mask.num_masks, _lib.ptr(allow_of), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        _lib.check(merge(ws.data_ptr(), lists, nq, top_k, scores.data_ptr(), rows.data_ptr(), _lib.stream_ptr()))
        return scores, rows


class QuantizedIndex(PartitionedIndex):
    """A ``PartitionedIndex`` whose cells are searched through a product quantiser and refined exactly -- the reference's
    ``IVF_PQ`` index with ``num_sub_vectors = embedding_dim // 8`` and ``search(...).nprobes(num_probes).refine_factor(4)``
    (data/lightning.py:162-165, 203-204, 222-229, 250-259).  Every cell-ordered row keeps ``num_sub_vectors`` one-byte codes of
    its residual to the cell's centroid (``codes()``: ``Npad * M`` bytes, where the parent's ``cell_blocked()`` holds
    ``Npad * D * 4``); a query ranks the rows of its probed cells by a score read from its lookup tables, and the
    ``refine_factor * top_k`` best are scored again on the original matrix with the canonical chain.  The scores returned are
    exact chain scores of the rows returned; which rows are returned is the approximation (on top of the parent's probing).
    The arithmetic -- residuals, codes, tables, approximate keys, the seeded codebook build -- is fixed to the bit:
    csrc/mf_pq.hip, DESIGN.md "Quantised cells".  ``path="cells"`` and ``path="exact"`` stay the parent's."""

    MAX_CANDIDATES = 256       # refine_factor * top_k: a thread each in mf_pq_refine
    DEEP_MAX_CANDIDATES = 1024  # the same on path="pq_deep": mf_pq_scan_deep's lists, four candidates a thread in mf_pq_refine_deep
    SUB_LENGTHS = (4, 8, 16)   # channels per sub-vector
    MAX_SUB_VECTORS = 64       # 64 KiB of lookup tables
    TRAIN_ROWS = 65536         # rows the codebooks are trained on

    def __init__(self, embeddings: torch.Tensor, centroids: torch.Tensor, assign: torch.Tensor, codebooks: torch.Tensor, *,
                 refine_factor: int = 4, idx_base: int = 0, num_probes: int = 8) -> None:
        super().__init__(embeddings, centroids, assign, idx_base=idx_base, num_probes=num_probes)
        self.refine_factor = self._refine_factor(refine_factor)
        self._pq_args: dict | None = None                # how ``build`` trained the codebooks: ``rebuild`` runs it again
        books = _lib.dev_f32(codebooks.detach(), "codebooks")
        d = self.embeddings.shape[1]
        if books.dim() != 3 or books.shape[1] != 256 or books.shape[0] * books.shape[2] != d:
            msg = f"codebooks should be (num_sub_vectors, 256, {d} // num_sub_vectors): {tuple(books.shape) = }"
            raise ValueError(msg)
        self.num_sub_vectors, self.dsub = self._geometry(d, books.shape[0])
        self.codebooks = books.contiguous()

    @classmethod
    def from_codebooks(cls, embeddings: torch.Tensor, centroids: torch.Tensor, assign: torch.Tensor, codebooks: torch.Tensor, *,
                       refine_factor: int = 4, idx_base: int = 0, num_probes: int = 8) -> "QuantizedIndex":
        """The index over given cells and ``codebooks [M, 256, D // M]`` (D the stored width): the rows are encoded, nothing
        is trained."""
        return cls(embeddings, centroids, assign, codebooks, refine_factor=refine_factor, idx_base=idx_base, num_probes=num_probes)

    @classmethod
    def build(cls, embeddings: torch.Tensor, num_partitions: int | None = None, *, num_sub_vectors: int | None = None,
              refine_factor: int = 4, pq_iters: int = 10, iters: int = 10, seed: int = 0, num_probes: int = 8,
              idx_base: int = 0) -> "QuantizedIndex":
        """The parent's seeded cells, then seeded codebooks, the same for the same rows and seed.  The training rows are the
        residuals of all rows up to ``TRAIN_ROWS`` of them, else of the rows at the first ``TRAIN_ROWS`` places of a permutation
        drawn on the host; codeword j of every sub-space starts as the residual sub-vector of training row ``j mod T``; an
        iteration encodes the training rows (``mf_pq_encode``) and replaces every codeword by the mean of its sub-vectors,
        added in training-row order (``mf_ivf_cell_mean``, no normalisation); an empty codeword keeps its value.
        ``num_sub_vectors=None``: the stored width // 8, as in the reference."""
        d = _lib.padded_width(embeddings.shape[1])
        geometry = cls._geometry(d, d // 8 if num_sub_vectors is None else int(num_sub_vectors))
        refine_factor = cls._refine_factor(refine_factor)
        if pq_iters < 0:
            msg = f"pq_iters must not be negative: {pq_iters = }"
            raise ValueError(msg)
        index = super().build(embeddings, num_partitions, iters=iters, seed=seed, num_probes=num_probes, idx_base=idx_base)
        index.refine_factor = refine_factor
        index.num_sub_vectors, index.dsub = geometry
        index._pq_args = {"pq_iters": int(pq_iters), "seed": int(seed)}
        index.codebooks = index._train(int(pq_iters), int(seed))
        return index

    def default_path(self, top_k: int) -> str:  # noqa: ARG002
        """``"pq"``: the quantiser's own search at every depth it serves (``refine_factor * top_k <= MAX_CANDIDATES``)."""
        return "pq"

    def serving_path(self, top_k: int) -> str:
        """``"pq"`` up to ``TILE_MAX_K`` rows (where ``default_path`` and every limit stay what they were), ``"pq_deep"`` beyond."""
        return "pq" if int(top_k) <= self.TILE_MAX_K else "pq_deep"

    @classmethod
    def _geometry(cls, d: int, m: int) -> tuple[int, int]:
        if m < 1 or d % m or d // m not in cls.SUB_LENGTHS or m > cls.MAX_SUB_VECTORS:
            msg = (f"num_sub_vectors must divide the stored width {d} into sub-vectors of 4, 8 or 16 channels, "
                   f"at most {cls.MAX_SUB_VECTORS} of them: {m = }")
            raise ValueError(msg)
        return m, d // m

    @classmethod
    def _refine_factor(cls, refine_factor) -> int:
        if int(refine_factor) < 1:
            msg = f"refine_factor must be at least 1: {refine_factor = }"
            raise ValueError(msg)
        return int(refine_factor)

    def _train(self, pq_iters: int, seed: int) -> torch.Tensor:
        emb, dev = self.embeddings, self.embeddings.device
        n, d = emb.shape
        m, dsub = self.num_sub_vectors, self.dsub
        if n <= self.TRAIN_ROWS:
            train = emb - self.centroids[self.assign]
        else:
            picked = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[: self.TRAIN_ROWS].to(dev)
            train = emb[picked] - self.centroids[self.assign[picked]]
        train = train.contiguous()
        t = train.shape[0]
        books = train[torch.arange(256, device=dev) % t].reshape(256, m, dsub).permute(1, 0, 2).contiguous()
        lib = _lib.lib()
        edges = torch.arange(257, dtype=torch.int64, device=dev)
        codes = torch.empty(t, m, dtype=torch.uint8, device=dev)
        mean = torch.zeros(256, d, dtype=torch.float32, device=dev)
        for _ in range(pq_iters):
            _lib.check(lib.mf_pq_encode(train.data_ptr(), t, d, None, None, books.data_ptr(), dsub, None, t, codes.data_ptr(), _lib.stream_ptr()))
            for j in range(m):
                # the rows of codeword c of sub-space j as a "cell": mf_ivf_cell_mean adds them in training-row order and
                # leaves the row of an empty one as it is -- so it starts as the codebook; only columns j are read back
                cells, order = torch.sort(codes[:, j].to(torch.int64), stable=True)
                cell_off = torch.searchsorted(cells, edges)
                mean[:, j * dsub : (j + 1) * dsub] = books[j]
                _lib.check(lib.mf_ivf_cell_mean(train.data_ptr(), t, d, order.data_ptr(), cell_off.data_ptr(), 256, 0, mean.data_ptr(),
                                                _lib.stream_ptr()))
                books[j] = mean[:, j * dsub : (j + 1) * dsub]
        return books

    def _install(self, centroids: torch.Tensor, assign: torch.Tensor) -> None:
        super()._install(centroids, assign)
        self._codes = None

    def filtered(self, where, *, cache: bool = True) -> "FilteredView":  # noqa: ARG002
        """Not implemented: the candidate stage ranks by approximate scores, and that "a view's search equals the search with
        the other rows excluded" has only been argued for exact scores."""
        msg = f"{type(self).__name__} takes no filter: its candidates are ranked by approximate scores"
        raise NotImplementedError(msg)

    def codes(self) -> torch.Tensor:
        """The rows' codes in cell order, ``Npad * M`` bytes in the layout ``mf_pq_scan`` reads (include/mf_hip.h:
        ``[64-row block][M / 4][64]`` 32-bit words, lane = row; padding positions hold code 0), built once."""
        if self._codes is None:
            npad, (n, d) = self.row_of.numel(), self.embeddings.shape
            out = torch.empty(npad * self.num_sub_vectors, dtype=torch.uint8, device=self.embeddings.device)
            _lib.check(_lib.lib().mf_pq_encode(self.embeddings.data_ptr(), n, d, self.centroids.data_ptr(), self.assign.data_ptr(),
                                               self.codebooks.data_ptr(), self.dsub, self.row_of.data_ptr(), npad, out.data_ptr(),
                                               _lib.stream_ptr()))
            self._codes = out
        return self._codes

    def refresh(self) -> None:
        """Forget the derived copies, the codes among them (encoded again from the rows as they are then, with the same
        cells and codebooks); ``rebuild()`` for new cells and codebooks."""
        super().refresh()
        self._codes = None

    def rebuild(self) -> None:
        """Run the build again on the rows as they are now: cells and codebooks (an index from ``from_codebooks`` keeps both
        and only forgets the derived copies)."""
        super().rebuild()
        if self._pq_args is not None:
            self.codebooks = self._train(self._pq_args["pq_iters"], self._pq_args["seed"])

    def _candidates_of(self, top_k: int, refine_factor: int | None) -> int:
        rf = self.refine_factor if refine_factor is None else self._refine_factor(refine_factor)
        top_k = self._top_k(top_k, "quantised")
        if rf * top_k > self.MAX_CANDIDATES:
            msg = f"refine_factor * top_k must not exceed {self.MAX_CANDIDATES}: {rf = }, {top_k = }"
            raise ValueError(msg)
        return rf * top_k

    def _deep_candidates_of(self, top_k: int, refine_factor: int | None, nprobe: int) -> int:
        """``path="pq_deep"``'s candidate depth: ``top_k`` in 1..``DEEP_MAX_K``, ``refine_factor * top_k`` within
        ``DEEP_MAX_CANDIDATES``, and a list per probe at least within the deep merge's keys."""
        rf = self.refine_factor if refine_factor is None else self._refine_factor(refine_factor)
        top_k = int(top_k)
        if not 1 <= top_k <= self.DEEP_MAX_K:
            msg = f"the deep quantised search returns 1..{self.DEEP_MAX_K} rows per query: {top_k = }"
            raise ValueError(msg)
        if rf * top_k > self.DEEP_MAX_CANDIDATES:
            msg = f"refine_factor * top_k must not exceed {self.DEEP_MAX_CANDIDATES} on path='pq_deep': {rf = }, {top_k = }"
            raise ValueError(msg)
        if nprobe * rf * top_k > MERGE_DEEP_MAX_KEYS:
            msg = (f"nprobe * refine_factor * top_k must not exceed {MERGE_DEEP_MAX_KEYS} (the keys the merge of the lists holds): "
                   f"{nprobe = }, {rf = }, {top_k = }")
            raise ValueError(msg)
        return rf * top_k

    def plan(self, num_queries: int, top_k: int = TOP_K, nprobe: int | None = None, refine_factor: int | None = None,
             path: str = "pq") -> dict[str, int]:
        """The geometry ``search`` runs with (``mf_pq_plan`` for ``refine_factor * top_k`` candidates; ``path="pq_deep"``:
        ``mf_pq_deep_plan``; ``path="cells"``: the parent's): slices per cell, partial lists per query, workgroups."""
        if path not in ("pq", "pq_deep"):
            return super().plan(num_queries, top_k, nprobe, "cells_deep" if path == "cells_deep" else "cells")
        if path == "pq_deep":
            nprobe = self._nprobe(nprobe)
            r = self._deep_candidates_of(top_k, refine_factor, nprobe)
        else:
            r, nprobe = self._candidates_of(top_k, refine_factor), self._nprobe(nprobe)
        if int(num_queries) < 1:
            msg = f"num_queries must be at least 1: {num_queries = }"
            raise ValueError(msg)
        return self._plan(_lib.lib().mf_pq_deep_plan if path == "pq_deep" else _lib.lib().mf_pq_plan, num_queries, nprobe, r)

    def candidates(self, queries: torch.Tensor, num_candidates: int, *, exclude: Sequence[Sequence[int]] | None = None,
                   exclude_csr: tuple[torch.Tensor, torch.Tensor] | None = None,
                   nprobe: int | None = None, slices: int | None = None, allow=None,
                   allow_of=None, path: str = "pq") -> tuple[torch.Tensor, torch.Tensor]:
        """``(approximate scores [Q, R] fp32, GLOBAL rows [Q, R] int64)``: the ``R = num_candidates`` (1..``MAX_CANDIDATES``)
        admissible rows of the probed cells that the quantiser ranks first -- approximate score descending, row ascending,
        the -inf / -1 tail --, what ``search`` refines.  Three stages, none with a host read: the cells, ``mf_pq_scan``,
        ``mf_topk_merge_packed_deep``.  ``slices``: into how many workgroups a probed cell is cut (None: the plan's number;
        1..the largest cell's blocks, ``nprobe * slices * R`` within the merge's ``MERGE_DEEP_MAX_KEYS``) -- the lists are the
        same for every value.  ``allow`` / ``allow_of``: as in ``search`` (``mf_pq_scan_allow``) -- the candidates of the same call
        with every inadmissible row on every query's exclusion list.  ``path="pq_deep"``: the same lists for ``R`` in
        1..``DEEP_MAX_CANDIDATES`` from ``mf_pq_scan_deep`` -- for an ``R`` both paths take, the same bits."""
        r = int(num_candidates)
        if path not in ("pq", "pq_deep"):
            msg = f"candidates come from the quantised scans, path in ('pq', 'pq_deep'): {path = }"
            raise ValueError(msg)
        deep = path == "pq_deep"
        most = self.DEEP_MAX_CANDIDATES if deep else self.MAX_CANDIDATES
        if not 1 <= r <= most:
            msg = f"num_candidates must be in 1..{most}: {r = }"
            raise ValueError(msg)
        nprobe = self._nprobe(nprobe)
        if slices is not None and (not 1 <= int(slices) <= self.max_cell_blocks or nprobe * int(slices) * r > MERGE_DEEP_MAX_KEYS):
            msg = (f"slices must be in 1..{self.max_cell_blocks} with nprobe * slices * num_candidates <= {MERGE_DEEP_MAX_KEYS}: "
                   f"{slices = }, {nprobe = }, {r = }")
            raise ValueError(msg)
        q = self._queries(queries)
        self._allow_route(allow, allow_of, None, "pq", ("pq",))
        mask, allow_of = self._allow_masks(allow, allow_of, q.shape[0])
        off, ids = exclude_csr if exclude_csr is not None else _csr(exclude, q.shape[0], q.device)
        return self._candidates(q, r, nprobe, off, ids, 0 if slices is None else int(slices), mask, allow_of, deep)

    def _candidates(self, q: torch.Tensor, r: int, nprobe: int, off, ids, slices: int = 0, mask: CellMask | None = None,
                    allow_of: torch.Tensor | None = None, deep: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        base, probes = self.coarse.search(q, nprobe)
        lib = _lib.lib()
        plan, ws_bytes, scan_plain, scan_allow = (
            (lib.mf_pq_deep_plan, lib.mf_pq_deep_ws_bytes, lib.mf_pq_scan_deep, lib.mf_pq_scan_deep_allow) if deep else
            (lib.mf_pq_plan, lib.mf_pq_ws_bytes, lib.mf_pq_scan, lib.mf_pq_scan_allow))
        planned = self._plan(plan, nq, nprobe, r)["lists"]
        lists = nprobe * slices if slices else planned
        ws = self._workspace(("pq_deep" if deep else "pq", nq, nprobe, r, slices),
                             max(lists * nq * r * 8, ws_bytes(nq, nprobe, r, self.max_cell_blocks)))
        approx = torch.empty(nq, r, dtype=torch.float32, device=q.device)
        rows = torch.empty(nq, r, dtype=torch.int64, device=q.device)
        scan = (q.data_ptr(), nq, self.codes().data_ptr(), self.codebooks.data_ptr(), self.dsub, self.cell_blk.data_ptr(), self.row_of.data_ptr(),
                self.row_of.numel(), n, self.num_partitions, d, self.max_cell_blocks, probes.data_ptr(), base.data_ptr(), nprobe, r, slices,
                _lib.ptr(off), _lib.ptr(ids), self.idx_base)
        if mask is None:
            _lib.check(scan_plain(*scan, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        else:
            _lib.check(scan_allow(*scan, mask.words.data_ptr(), mask.num_masks, _lib.ptr(allow_of), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        _lib.check(lib.mf_topk_merge_packed_deep(ws.data_ptr(), lists, nq, r, approx.data_ptr(), rows.data_ptr(), _lib.stream_ptr()))
        return approx, rows

    def search(self, queries: torch.Tensor, top_k: int = TOP_K, *, exclude: Sequence[Sequence[int]] | None = None,
               exclude_csr: tuple[torch.Tensor, torch.Tensor] | None = None, nprobe: int | None = None,
               refine_factor: int | None = None, path: str = "pq", where=None, allow=None,
               allow_of=None) -> tuple[torch.Tensor, torch.Tensor]:
        """``ItemIndex.search``'s inputs and result.  ``path="pq"``: the ``refine_factor * top_k`` (default: the index's
        factor; at most ``MAX_CANDIDATES``) best rows of the ``nprobe`` probed cells by the quantiser's approximate score,
        scored again with the chain on the original rows and ordered exactly -- four stages, none with a host read: the
        cells, the scan (``mf_pq_scan``), the merge (``mf_topk_merge_packed_deep``), the refine (``mf_pq_refine``); the
        cell-ordered fp32 copy is not built.  ``path="cells"`` and ``path="exact"`` (and the exact engines' names) are the
        parent's.  ``where``: refused (``filtered``) -- the filter this index takes is ``allow``: a ``CellMask`` or anything
        ``cell_mask`` takes (``allow_of``: each query's mask among several), on ``path="pq"`` (``mf_pq_scan_allow``: a row the
        mask does not admit never becomes a candidate, so the refine only sees admitted rows) and on the parent's
        ``path="cells"`` -- bit for bit the same search with the inadmissible rows on every query's exclusion list.
        ``path="pq_deep"``: the same contract and the same four stages for ``1 <= top_k <= DEEP_MAX_K`` with ``refine_factor *
        top_k`` within ``DEEP_MAX_CANDIDATES`` and ``nprobe`` times that within ``MERGE_DEEP_MAX_KEYS`` (``mf_pq_scan_deep`` /
        ``mf_pq_scan_deep_allow``, ``mf_pq_refine_deep``) -- where ``"pq"`` takes the shape too, the same bits.
        ``serving_path(top_k)`` names the one of the two that serves a depth."""
        self._allow_route(allow, allow_of, where, path, ("pq", "pq_deep", "cells", "cells_deep"))
        if where is not None:
            self.filtered(where)
        if path not in ("pq", "pq_deep"):
            return super().search(queries, top_k, exclude=exclude, exclude_csr=exclude_csr, nprobe=nprobe, path=path, allow=allow,
                                  allow_of=allow_of)
        deep = path == "pq_deep"
        if deep:
            nprobe = self._nprobe(nprobe)
            r = self._deep_candidates_of(top_k, refine_factor, nprobe)
        else:
            r = self._candidates_of(top_k, refine_factor)
            nprobe = self._nprobe(nprobe)
        top_k = int(top_k)
        q = self._queries(queries)
        nq, n, d = q.shape[0], self.num_items, self.embeddings.shape[1]
        mask, allow_of = self._allow_masks(allow, allow_of, nq)
        off, ids = exclude_csr if exclude_csr is not None else _csr(exclude, nq, q.device)
        _, cand = self._candidates(q, r, nprobe, off, ids, 0, mask, allow_of, deep)
        scores = torch.empty(nq, top_k, dtype=torch.float32, device=q.device)
        rows = torch.empty(nq, top_k, dtype=torch.int64, device=q.device)
        refine = _lib.lib().mf_pq_refine_deep if deep else _lib.lib().mf_pq_refine
        _lib.check(refine(q.data_ptr(), nq, self.embeddings.data_ptr(), n, d, cand.data_ptr(), r, top_k, self.idx_base, scores.data_ptr(),
                          rows.data_ptr(), _lib.stream_ptr()))
        return scores, rows


class FilteredView:
    """The rows of an index that a filter admits, as an index of their own (``ItemIndex.filtered``): ``rows`` (``int64 [M]``, the
    admissible local rows in ascending order -- ``mf_filter_rows``), and ``index``, an index of the parent's class over a bit copy
    of those rows (``mf_gather_rows`` at the stored width) with ``idx_base = 0``; None when ``M == 0``.  ``search`` and
    ``positions`` take the parent's arguments and return GLOBAL rows: exclusion lists are mapped into the view on the device
    (``mf_filter_lists``), targets likewise (``mf_filter_remap``), result rows back (``mf_filter_unmap``), and the engines run
    untouched on ``M`` rows -- ``path=`` and the ``top_k`` limits are theirs.  Ascending compaction keeps "score descending, row
    ascending" and the copied rows give the same chain scores, so the result is, bit for bit, the parent's search with every
    inadmissible row on every query's exclusion list.  A snapshot of the rows and tags at its build, like the index itself."""

    def __init__(self, parent: ItemIndex, words: torch.Tensor, where: TagFilter) -> None:
        lib = _lib.lib()
        emb = parent.embeddings
        n, d = emb.shape
        dev = emb.device
        if words.data_ptr() % 16:
            words = words.clone()
        rows = torch.empty(n, dtype=torch.int64, device=dev)
        self.rank = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        ws = _lib.workspace(lib.mf_filter_ws_bytes(n), dev)
        _lib.check(lib.mf_filter_rows(words.data_ptr(), n, where.any_of, where.all_of, where.none_of, ws.data_ptr(), ws.numel(),
                                      rows.data_ptr(), self.rank.data_ptr(), count.data_ptr(), _lib.stream_ptr()))
        m = int(count.item())                       # the one host read: it sizes the copy
        self.parent, self.where = parent, where
        self.rows = rows[:m].clone()
        self.index: ItemIndex | None = None
        self._ws: dict = {}
        if m:
            sub = torch.empty(m, d, dtype=torch.float32, device=dev)
            _lib.check(lib.mf_gather_rows(emb.data_ptr(), n, d, self.rows.data_ptr(), m, 0, sub.data_ptr(), None, _lib.stream_ptr()))
            self.index = parent._sub_index(sub, self.rows)

    @property
    def num_items(self) -> int:
        return self.rows.numel()

    def _lists(self, nq: int, exclude, exclude_csr, device):
        """The exclusion lists inside the view: a device CSR of slots (``mf_filter_lists``), or None without lists."""
        off, ids = exclude_csr if exclude_csr is not None else _csr(exclude, nq, device)
        if off is None:
            return None
        off, ids = _lib.dev_i64(off, "exclusion offsets"), _lib.dev_i64(ids, "exclusion rows")
        if off.numel() != nq + 1:
            msg = f"one exclusion list per query expected: {off.numel() = }, {nq = }"
            raise ValueError(msg)
        lib = _lib.lib()
        entries = ids.numel()
        if entries == 0:       # keep the pointer valid
            ids = torch.zeros(1, dtype=torch.int64, device=device)
        need = lib.mf_filter_lists_ws_bytes(nq)
        ws = self._ws.get("lists")
        if ws is None or ws.numel() < need:
            ws = self._ws["lists"] = _lib.workspace(need, device)
        out_off = torch.empty(nq + 1, dtype=torch.int64, device=device)
        out_ids = torch.empty(max(entries, 1), dtype=torch.int64, device=device)
        _lib.check(lib.mf_filter_lists(off.data_ptr(), ids.data_ptr(), entries, nq, self.parent.idx_base, self.rank.data_ptr(),
                                       self.parent.num_items, ws.data_ptr(), ws.numel(), out_off.data_ptr(), out_ids.data_ptr(),
                                       _lib.stream_ptr()))
        return out_off, out_ids

    def _unmap(self, rows: torch.Tensor) -> torch.Tensor:
        _lib.check(_lib.lib().mf_filter_unmap(rows.data_ptr(), rows.numel(), self.rows.data_ptr(), self.num_items, self.parent.idx_base,
                                              rows.data_ptr(), _lib.stream_ptr()))
        return rows

    def search(self, queries: torch.Tensor, top_k: int = TOP_K, *, exclude: Sequence[Sequence[int]] | None = None,
               exclude_csr: tuple[torch.Tensor, torch.Tensor] | None = None, **kw) -> tuple[torch.Tensor, torch.Tensor]:
        """The parent's ``search`` over the admissible rows: its arguments (``path=``, ``nprobe=`` as the parent takes them), its
        result with GLOBAL rows.  An empty view answers -inf / -1 without an engine."""
        q = self.parent._queries(queries)
        nq = q.shape[0]
        if self.index is None:
            if exclude is not None and len(exclude) != nq:
                msg = f"one exclusion list per query expected: {len(exclude) = }, {nq = }"
                raise ValueError(msg)
            return (torch.full((nq, int(top_k)), -math.inf, dtype=torch.float32, device=q.device),
                    torch.full((nq, int(top_k)), -1, dtype=torch.int64, device=q.device))
        scores, rows = self.index.search(q, top_k, exclude_csr=self._lists(nq, exclude, exclude_csr, q.device), **kw)
        return scores, self._unmap(rows)

    def positions(self, queries: torch.Tensor, targets_csr: tuple[torch.Tensor, torch.Tensor], *,
                  exclude: Sequence[Sequence[int]] | None = None,
                  exclude_csr: tuple[torch.Tensor, torch.Tensor] | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The parent's ``positions`` among the admissible rows: a target the filter does not admit reads -1 / -inf, like one
        that is excluded or outside the catalog."""
        q = self.parent._queries(queries)
        nq = q.shape[0]
        t_off, t_ids, nt = self.parent._targets(nq, targets_csr, q.device)
        if self.index is None:
            return (torch.full((nt,), -1, dtype=torch.int64, device=q.device),
                    torch.full((nt,), -math.inf, dtype=torch.float32, device=q.device),
                    torch.zeros(nq, dtype=torch.int64, device=q.device))
        slots = torch.empty(max(nt, 1), dtype=torch.int64, device=q.device)
        _lib.check(_lib.lib().mf_filter_remap(t_ids.data_ptr(), nt, self.parent.idx_base, self.rank.data_ptr(), self.parent.num_items,
                                              slots.data_ptr(), _lib.stream_ptr()))
        return self.index.positions(q, (t_off, slots[:nt]), exclude_csr=self._lists(nq, exclude, exclude_csr, q.device))


def merge_topk(part_scores: torch.Tensor, part_rows: torch.Tensor, top_k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Merge per-shard results ``[G, Q, k]`` (global rows, each list ordered as ``search`` returns it) into the global top-k:
    ``mf_topk_merge`` up to ``ItemIndex.TILE_MAX_K``, ``mf_topk_merge_deep`` for deeper lists (``top_k`` up to
    ``ItemIndex.DEEP_MAX_K``, ``G * top_k`` up to ``MERGE_DEEP_MAX_KEYS``) -- the same bits either way."""
    ps = _lib.dev_f32(part_scores, "part_scores")
    pr = _lib.dev_i64(part_rows, "part_rows")
    g, nq, k = ps.shape
    if k != top_k:
        msg = f"partial results must hold top_k entries: {k = }, {top_k = }"
        raise ValueError(msg)
    scores = torch.empty(nq, k, dtype=torch.float32, device=ps.device)
    rows = torch.empty(nq, k, dtype=torch.int64, device=ps.device)
    merge = _lib.lib().mf_topk_merge_deep if top_k > ItemIndex.TILE_MAX_K else _lib.lib().mf_topk_merge
    _lib.check(merge(ps.data_ptr(), pr.data_ptr(), g, nq, k, scores.data_ptr(), rows.data_ptr(), _lib.stream_ptr()))
    return scores, rows


MERGE_DEEP_MAX_KEYS = _lib.MF_TOPK_MERGE_DEEP_MAX_KEYS      # ``G * top_k`` the deep merges take: a query's keys sit in 128 KiB of LDS


class ItemProcessor:
    """The retrieval half of ``xfmr_rec.data.lightning.ItemProcessor`` (:154-259): ``get_index``
    embeds the catalog with the item tower, ``search`` answers one query like the reference
    (numpy ``[1, d]`` in, ``pandas.DataFrame`` out with ``movie_rn``, ``movie_id``, ``score``)."""

    idx_col: str = ITEM_IDX_COL
    id_col: str = ITEM_ID_COL

    INDEX_TYPES = ("exact", "partitioned", "quantized")
    FILTER_MODES = ("view", "mask")

    @classmethod
    def check_filter_mode(cls, filter_mode: str, index_type: str) -> None:
        if filter_mode not in cls.FILTER_MODES:
            msg = f"filter_mode must be 'view' or 'mask': {filter_mode!r}"
            raise ValueError(msg)
        if filter_mode == "mask" and index_type not in ("partitioned", "quantized"):
            msg = f"filter_mode='mask' filters the cell scans: index_type must be 'partitioned' or 'quantized', not {index_type!r}"
            raise ValueError(msg)

    def __init__(self, item_ids: Sequence[int] | torch.Tensor | None = None, *, index_type: str = "exact",
                 num_partitions: int | None = None, num_probes: int = 8, index_seed: int = 0, num_sub_vectors: int | None = None,
                 refine_factor: int = 4, filter_mode: str = "view") -> None:
        """``index_type="partitioned"``: ``get_index`` / ``set_index`` / ``append`` build a ``PartitionedIndex`` --
        ``num_partitions`` cells (None: the reference's default for the catalog's size), ``num_probes`` of them visited per
        query, k-means seeded with ``index_seed`` -- and ``search`` probes it.  ``index_type="quantized"``: a
        ``QuantizedIndex`` over the same cells -- the reference's ``num_sub_vectors`` one-byte codes per row (None: the stored
        width // 8) and its ``refine_factor``: ``refine_factor * top_k`` candidates per query are scored exactly.
        ``filter_mode``: how ``search(where=...)`` filters -- "view": through the index's ``where=`` (a cached copy of the
        admissible rows; a quantised index refuses it); "mask": through its ``allow=`` (an allow bitmap over the cells, no
        copy; partitioned and quantised indexes only)."""
        if index_type not in self.INDEX_TYPES:
            msg = f"index_type must be 'exact', 'partitioned' or 'quantized': {index_type!r}"
            raise ValueError(msg)
        self.check_filter_mode(filter_mode, index_type)
        self.filter_mode = filter_mode
        if num_sub_vectors is not None and int(num_sub_vectors) < 1:
            msg = f"num_sub_vectors must be None (the stored width // 8) or at least 1: {num_sub_vectors = }"
            raise ValueError(msg)
        self.item_ids = None if item_ids is None else torch.as_tensor(item_ids, dtype=torch.int64).cpu()
        self.index_type, self.num_partitions, self.num_probes, self.index_seed = index_type, num_partitions, int(num_probes), int(index_seed)
        self.num_sub_vectors = None if num_sub_vectors is None else int(num_sub_vectors)
        self.refine_factor = QuantizedIndex._refine_factor(refine_factor)
        self.index: ItemIndex | None = None
        self._row_of_id: dict[int, int] | None = None
        self.tags: torch.Tensor | None = None            # int64 [rows] on the host: the items' tag words (set_tags)
        self.tag_vocabulary: list[str] | None = None     # name of bit i

    def set_tags(self, tags, vocabulary: Sequence[str] | None = None) -> None:
        """The items' tag words (``data.item_tag_bits``: ``int64 [rows]``, one per item row) and the names of their bits: what
        ``search(where=...)`` filters on.  Kept here and handed to every index this processor builds."""
        t = torch.as_tensor(tags)
        if t.dtype != torch.int64 or t.dim() != 1:
            msg = f"tags should be an int64 vector, one word per item row: {t.dtype}, {tuple(t.shape)}"
            raise ValueError(msg)
        if self.index is not None and t.numel() != self.index.num_items:
            msg = f"one tag word per item row: {t.numel()} != {self.index.num_items}"
            raise ValueError(msg)
        if vocabulary is not None and (len(vocabulary) > 64 or len(set(vocabulary)) != len(vocabulary)):  # noqa: PLR2004
            msg = f"a vocabulary names at most 64 distinct bits: {len(vocabulary)} names"
            raise ValueError(msg)
        self.tags = t.detach().cpu().contiguous()
        self.tag_vocabulary = None if vocabulary is None else [str(v) for v in vocabulary]
        if self.index is not None:
            self.index.set_tags(self.tags)

    def tag_filter(self, any_of: Sequence[str] = (), all_of: Sequence[str] = (), none_of: Sequence[str] = ()) -> TagFilter:
        """A ``TagFilter`` from names of the vocabulary (``KeyError`` for a name it does not hold)."""
        if self.tag_vocabulary is None:
            msg = "tag names need a vocabulary: set_tags(tags, vocabulary)"
            raise ValueError(msg)
        bit = {name: i for i, name in enumerate(self.tag_vocabulary)}

        def mask(names) -> int:
            names = [names] if isinstance(names, str) else list(names)
            unknown = [n for n in names if n not in bit]
            if unknown:
                msg = f"unknown tag names: {unknown}"
                raise KeyError(msg)
            return sum({1 << bit[n] for n in names})

        return TagFilter(any_of=mask(any_of), all_of=mask(all_of), none_of=mask(none_of))

    def _where(self, where):
        """``where`` as the index takes it: a ``TagFilter`` / allow-mask as it is, a dict of name lists through ``tag_filter``."""
        return self.tag_filter(**where) if isinstance(where, dict) else where

    def _install_tags(self) -> None:
        """Hand the tags to a newly built index when they still have one word per row; forget them otherwise."""
        if self.tags is not None and self.index is not None:
            if self.tags.numel() == self.index.num_items:
                self.index.set_tags(self.tags)
            else:
                self.tags = None

    def _make_index(self, embeddings: torch.Tensor) -> ItemIndex:
        if self.index_type == "exact":
            return ItemIndex(embeddings)
        c = self.num_partitions if self.num_partitions is not None else default_num_partitions(embeddings.shape[0])
        c = max(1, min(int(c), embeddings.shape[0]))
        num_probes = min(self.num_probes, c, PartitionedIndex.MAX_PROBES)
        if self.index_type == "quantized":
            return QuantizedIndex.build(embeddings, c, num_sub_vectors=self.num_sub_vectors, refine_factor=self.refine_factor,
                                        seed=self.index_seed, num_probes=num_probes)
        return PartitionedIndex.build(embeddings, c, seed=self.index_seed, num_probes=num_probes)

    @torch.inference_mode()
    def get_index(self, model: torch.nn.Module, subset: str = "predict") -> ItemIndex:  # noqa: ARG002
        tower = model.towers["item"] if hasattr(model, "towers") else model
        rows = torch.arange(tower.num_embeddings, device=tower.weight.device)
        self.index = self._make_index(tower(rows))
        if self.item_ids is None:
            self.item_ids = torch.arange(tower.num_embeddings)
        self._row_of_id = {int(i): r for r, i in enumerate(self.item_ids.tolist())}
        self._install_tags()
        return self.index

    def set_index(self, embeddings: torch.Tensor) -> ItemIndex:
        """Install a prebuilt (loaded) item matrix; row r belongs to ``item_ids[r]``."""
        self.index = self._make_index(embeddings)
        if self.item_ids is None:
            self.item_ids = torch.arange(embeddings.shape[0])
        self._row_of_id = {int(i): r for r, i in enumerate(self.item_ids.tolist())}
        self._install_tags()
        return self.index

    def append(self, item_ids, embeddings: torch.Tensor, tags=None) -> ItemIndex:
        """Add items to a built index: their rows follow the existing ones (the index is rebuilt, the id map extended).
        ``tags``: the new rows' tag words (0 when tags are set and none are given)."""
        if self.index is None or self.item_ids is None:
            msg = "`index` must be intialised first"
            raise ValueError(msg)
        ids = torch.as_tensor(item_ids, dtype=torch.int64).cpu().reshape(-1)
        if ids.numel() != embeddings.shape[0]:
            msg = f"one embedding per item id: {ids.numel()} != {embeddings.shape[0]}"
            raise ValueError(msg)
        if set(ids.tolist()) & set(self._row_of_id or {}) or len(set(ids.tolist())) != ids.numel():
            msg = "item ids must be new and distinct"
            raise ValueError(msg)
        if tags is not None:
            new_tags = torch.as_tensor(tags)
            if self.tags is None or new_tags.dtype != torch.int64 or new_tags.shape != (ids.numel(),):
                msg = "tags of appended items: one int64 word per new item, on a processor whose tags are set"
                raise ValueError(msg)
        if self.tags is not None:
            self.tags = torch.cat([self.tags, torch.zeros(ids.numel(), dtype=torch.int64) if tags is None else new_tags.cpu()])
        old = self.index.embeddings[:, : self.index.dim]
        self.item_ids = torch.cat([self.item_ids, ids])
        return self.set_index(torch.cat([old, embeddings.to(old.device, torch.float32)]))

    def row_of(self, item_id: int) -> int:
        if self._row_of_id is None or int(item_id) not in self._row_of_id:
            msg = f"unknown item id: {item_id = }"
            raise KeyError(msg)
        return self._row_of_id[int(item_id)]

    def search(self, embedding, exclude_item_ids: list[int] | None = None, top_k: int = TOP_K, where=None):
        """``where``: only items it admits are returned -- a ``TagFilter``, a ``bool [rows]`` allow-mask, or a dict of name
        lists (``tag_filter``'s arguments); the reference's ``.where(filter, prefilter=True)``.  It reaches the index as
        ``where=`` or, with ``filter_mode="mask"``, as ``allow=``."""
        import pandas as pd

        if self.index is None:
            msg = "`index` must be intialised first"  # message kept from data/lightning.py:244
            raise ValueError(msg)
        q = torch.as_tensor(np.asarray(embedding), dtype=torch.float32).reshape(1, -1).to(self.index.embeddings.device)
        rows = [self._row_of_id[i] for i in (exclude_item_ids or []) if i in self._row_of_id]
        path = self.index.serving_path(top_k)          # (the deep cell scan / the deep quantised search beyond 64 rows)
        if where is None:
            scores, idx = self.index.search(q, top_k, exclude=[rows], path=path)
        elif self.filter_mode == "mask":
            scores, idx = self.index.search(q, top_k, exclude=[rows], path=path, allow=self._where(where))
        else:
            scores, idx = self.index.search(q, top_k, exclude=[rows], path=path, where=self._where(where))
        idx = idx[0].cpu()
        keep = idx >= 0
        idx = idx[keep]
        return pd.DataFrame(
            {
                self.idx_col: idx.numpy(),
                self.id_col: self.item_ids[idx].numpy(),
                "score": scores[0].cpu()[keep].numpy(),
            }
        )


METRIC_NAMES = ("RetrievalNormalizedDCG", "RetrievalRecall", "RetrievalPrecision", "RetrievalMAP", "RetrievalHitRate",
                "RetrievalMRR")


def _all_ranks(total: torch.Tensor | None, n: int, width: int, comm):
    """A metric's running ``(sums [width] fp64, queries)``, added over the ranks of ``comm`` (one gather of ``width + 1``
    numbers); as they are without one.  A rank that has seen no query contributes zeros."""
    if comm is None:
        return total, n
    if total is None:
        total = torch.zeros(width, dtype=torch.float64)
    mine = torch.cat([total, torch.tensor([float(n)], dtype=torch.float64, device=total.device)])
    every = comm.gather(mine).reshape(comm.world, width + 1).sum(dim=0)
    return every[:width], int(every[width].item())


class RetrievalMetrics:
    """The reference's ``MetricCollection`` of six retrieval metrics @top_k
    (xfmr_rec/lightning.py:289-306), fed with whole batches of top-k results instead of one
    ``update`` per example (``update_metrics`` :149-187).  ``compute()`` returns
    ``{prefix + class name: mean over all queries seen}`` like ``MetricCollection.compute``."""

    def __init__(self, top_k: int = TOP_K, prefix: str = "") -> None:
        self.top_k, self.prefix = int(top_k), prefix
        self.reset()

    def reset(self) -> None:
        self._sum, self._n = None, 0

    @torch.no_grad()
    def update(self, topk_idx: torch.Tensor, target_offsets: torch.Tensor, target_idx: torch.Tensor,
               target_rating: torch.Tensor) -> torch.Tensor:
        """``topk_idx`` [Q, top_k] retrieved item ids, best first (``ItemIndex.search``); the targets of query q
        are ``target_idx / target_rating[target_offsets[q] : target_offsets[q + 1]]``.  Returns [Q, 6]."""
        ti = _lib.dev_i64(topk_idx, "topk_idx")
        q, k = ti.shape
        if k != self.top_k:
            msg = f"expected top_k = {self.top_k} columns: {k = }"
            raise ValueError(msg)
        off = _lib.dev_i64(target_offsets, "target_offsets")
        ids = _lib.dev_i64(target_idx, "target_idx")
        rel = _lib.dev_f32(target_rating, "target_rating")
        if off.numel() != q + 1 or ids.numel() != rel.numel():
            msg = f"target CSR does not match the queries: {off.numel() = }, {q = }, {ids.numel() = }, {rel.numel() = }"
            raise ValueError(msg)
        if ids.numel() == 0:       # keep the pointers valid
            ids, rel = torch.zeros(1, dtype=torch.int64, device=ti.device), torch.zeros(1, device=ti.device)
        out = torch.empty(q, 6, dtype=torch.float32, device=ti.device)
        _lib.check(_lib.lib().mf_retrieval_metrics(ti.data_ptr(), q, k, off.data_ptr(), ids.data_ptr(), rel.data_ptr(),
                                                   out.data_ptr(), _lib.stream_ptr()))
        tot = out.sum(dim=0, dtype=torch.float64)
        self._sum = tot if self._sum is None else self._sum + tot
        self._n += q
        return out

    def compute(self, comm=None) -> dict[str, torch.Tensor]:
        """``comm`` (``distributed.TorchComm`` / ``RcclComm``; every rank calls): the means over ALL ranks' queries."""
        total, n = _all_ranks(self._sum, self._n, len(METRIC_NAMES), comm)
        if not n:
            return {self.prefix + name: torch.tensor(0.0) for name in METRIC_NAMES}
        mean = (total / n).to(torch.float32)
        return {self.prefix + name: mean[j] for j, name in enumerate(METRIC_NAMES)}


POSITION_METRIC_NAMES = ("MRR", "MeanPosition", "AUC")
MAX_EVAL_KS = 8       # cut-offs one mf_position_metrics launch serves


class PositionMetrics:
    """The six metrics of ``RetrievalMetrics`` at one or several cut-offs, and three uncut ones, from the targets' exact
    positions (``ItemIndex.positions``) instead of a top-k list: no deepest k, one launch for all cut-offs.  ``compute()``
    returns the first k's values under the names ``RetrievalMetrics`` uses, further ks' under ``name@k``, and ``MRR``,
    ``MeanPosition`` and ``AUC`` over the relevant targets that have a position -- means over all queries seen."""

    def __init__(self, top_k: int | Sequence[int] = TOP_K, prefix: str = "") -> None:
        ks = (int(top_k),) if isinstance(top_k, (int, np.integer)) else tuple(int(k) for k in top_k)
        if not 1 <= len(ks) <= MAX_EVAL_KS or min(ks) < 1 or len(set(ks)) != len(ks):
            msg = f"1 to {MAX_EVAL_KS} distinct cut-offs >= 1 expected: {ks = }"
            raise ValueError(msg)
        self.ks, self.top_k, self.prefix = ks, ks[0], prefix
        self.names = tuple(name if j == 0 else f"{name}@{k}" for j, k in enumerate(ks) for name in METRIC_NAMES) + POSITION_METRIC_NAMES
        self.reset()

    def reset(self) -> None:
        self._sum, self._n = None, 0

    @torch.no_grad()
    def update(self, pos: torch.Tensor, target_offsets: torch.Tensor, target_rating: torch.Tensor, ncand: torch.Tensor) -> torch.Tensor:
        """``pos`` [T] and ``ncand`` [Q] as ``ItemIndex.positions`` returns them; the targets of query q are entries
        ``target_offsets[q] : target_offsets[q + 1]`` of ``pos`` / ``target_rating``.  Returns [Q, 6 * len(ks) + 3]."""
        p = _lib.dev_i64(pos, "pos")
        off = _lib.dev_i64(target_offsets, "target_offsets")
        rel = _lib.dev_f32(target_rating, "target_rating")
        nc = _lib.dev_i64(ncand, "ncand")
        q = nc.numel()
        if off.numel() != q + 1 or p.numel() != rel.numel():
            msg = f"target CSR does not match the queries: {off.numel() = }, {q = }, {p.numel() = }, {rel.numel() = }"
            raise ValueError(msg)
        if p.numel() == 0:       # keep the pointers valid
            p, rel = torch.zeros(1, dtype=torch.int64, device=nc.device), torch.zeros(1, device=nc.device)
        out = torch.empty(q, len(self.names), dtype=torch.float32, device=nc.device)
        ks = (ctypes.c_int32 * len(self.ks))(*self.ks)
        _lib.check(_lib.lib().mf_position_metrics(p.data_ptr(), off.data_ptr(), rel.data_ptr(), nc.data_ptr(), q, ks, len(self.ks),
                                                  out.data_ptr(), _lib.stream_ptr()))
        tot = out.sum(dim=0, dtype=torch.float64)
        self._sum = tot if self._sum is None else self._sum + tot
        self._n += q
        return out

    def compute(self, comm=None) -> dict[str, torch.Tensor]:
        """``comm`` (``distributed.TorchComm`` / ``RcclComm``; every rank calls): the means over ALL ranks' queries."""
        total, n = _all_ranks(self._sum, self._n, len(self.names), comm)
        if not n:
            return {self.prefix + name: torch.tensor(0.0) for name in self.names}
        mean = (total / n).to(torch.float32)
        return {self.prefix + name: mean[j] for j, name in enumerate(self.names)}
