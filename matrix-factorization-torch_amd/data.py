"""Batch layout of the hot path (the ids-only part of ``xfmr_rec/data``).

What the loss path consumes is fixed by the reference's collate
(``InteractionProcessor.collate``, xfmr_rec/data/lightning.py:335-342, batch type
``InteractionBatchType`` :72-76): ``target[B]`` int64 ratings, ``user.pos_idx[B, P]``
int64 right-padded with 0 (``pad_tensors`` / ``collate_tensor_fn``,
xfmr_rec/data/load.py:38-75), ``item.idx[B]`` 1-based item rows (``movie_rn``,
prepare.py:85) and ``neg_item.idx[B]`` uniform negatives (:344-354).  The towers here
are embedding tables, so ``user`` carries ``idx`` (``user_rn``) where the reference
carries ``text``.

The reference's text ETL (polars / parquet / LanceDB, prepare.py, load.py:78-141) is out of
scope; its ids-only core is here: :func:`split_ratings` (the per-user temporal
80/20 split and the val / test user split, prepare.py:160-194), :class:`InteractionTable` (train
pairs, per-user train positives, the 4-week rolling history of every rating, prepare.py:229-243, and
the evaluation sets of ``process_users``, :272-310) and :class:`DeviceInteractionSampler` (the batch
producer on the GPU).  :class:`SyntheticInteractions` produces MovieLens-*shaped* batches (no MovieLens
files are available offline) for tests and benchmarks.
"""
from __future__ import annotations

from typing import Iterable, Iterator, TypedDict

import torch
import torch.nn.functional as F  # noqa: N812

from .params import BATCH_SIZE, PADDING_IDX


class ItemBatchType(TypedDict):
    idx: torch.Tensor


class UserBatchType(TypedDict, total=False):
    idx: torch.Tensor
    pos_idx: torch.Tensor                 # the reference's padded positives [B, P] ...
    pos_csr: tuple                        # ... or (user idx [B], pos_off [U + 1], pos_items): the lists in place (no padding)


class InteractionBatchType(TypedDict):
    target: torch.Tensor
    user: UserBatchType
    item: ItemBatchType
    neg_item: ItemBatchType


def pad_tensors(batch: Iterable[torch.Tensor], dim: int = -1, *, pad_start: bool = False,
                pad_value: int = PADDING_IDX) -> torch.Tensor:
    """Stack ragged tensors, padding ``dim`` to the longest (same contract as load.py:38-55,
    whose 12 shape cases are replayed in tests/test_host_cpu.py)."""
    tensors = list(batch)
    size = max(t.size(dim) for t in tensors)
    nd = tensors[0].dim()
    axis = dim % nd
    out = []
    for t in tensors:
        pad = [0, 0] * nd
        # F.pad lists dimensions last-to-first; [2j] pads before, [2j + 1] after
        pad[2 * (nd - 1 - axis) + (0 if pad_start else 1)] = size - t.size(dim)
        out.append(F.pad(t, pad, value=pad_value))
    return torch.stack(out)


def collate_interactions(examples: list[dict]) -> InteractionBatchType:
    """List of ``{"target", "user": {"idx", "pos_idx"}, "item": {"idx"}, "neg_item": {"idx"}}``
    -> batch (ragged ``pos_idx`` rows are 0-padded on the right)."""
    as_t = lambda xs: torch.as_tensor(xs, dtype=torch.int64)  # noqa: E731
    return {
        "target": as_t([e["target"] for e in examples]),
        "user": {
            "idx": as_t([e["user"]["idx"] for e in examples]),
            "pos_idx": pad_tensors([as_t(e["user"]["pos_idx"]) for e in examples], dim=-1),
        },
        "item": {"idx": as_t([e["item"]["idx"] for e in examples])},
        "neg_item": {"idx": as_t([e["neg_item"]["idx"] for e in examples])},
    }


class SyntheticInteractions:
    """MovieLens-shaped synthetic interactions: Zipf(s) item popularity, log-normal user
    activity, ratings uniform in 1..5, each user's positives a fixed random item set
    (SURVEY.md 8d).  Rows are 1-based; row 0 is the padding row of both tables."""

    def __init__(self, num_users: int, num_items: int, *, max_positives: int = 64, zipf_s: float = 1.0,
                 seed: int = 0, user_range: tuple[int, int] | None = None) -> None:
        self.num_users, self.num_items, self.max_positives = num_users, num_items, max_positives
        self.gen = torch.Generator().manual_seed(seed)
        self.item_w = 1.0 / torch.arange(1, num_items, dtype=torch.float64) ** zipf_s
        lo, hi = user_range if user_range is not None else (1, num_users)
        self.user_lo = lo
        self.user_w = torch.exp(torch.randn(hi - lo, generator=self.gen, dtype=torch.float64))

    def item_probability(self) -> torch.Tensor:
        """Sampling probability of each item row as a batch column (positives ~ Zipf, negatives ~ uniform)."""
        p = 0.5 * self.item_w / self.item_w.sum() + 0.5 / (self.num_items - 1)
        return torch.cat([torch.zeros(1, dtype=torch.float64), p]).to(torch.float32)

    def batch(self, batch_size: int = BATCH_SIZE) -> InteractionBatchType:
        g, p = self.gen, self.max_positives
        user = torch.multinomial(self.user_w, batch_size, replacement=True, generator=g) + self.user_lo
        item = torch.multinomial(self.item_w, batch_size, replacement=True, generator=g) + 1
        neg = torch.randint(1, self.num_items, (batch_size,), generator=g)       # uniform negatives (:344-354)
        target = torch.randint(1, 6, (batch_size,), generator=g)
        n_pos = torch.randint(min(8, p), p + 1, (batch_size,), generator=g)
        pos = torch.multinomial(self.item_w, batch_size * p, replacement=True, generator=g).reshape(batch_size, p) + 1
        pos[:, 0] = item
        pos[torch.arange(p)[None, :] >= n_pos[:, None]] = PADDING_IDX
        return {"target": target, "user": {"idx": user, "pos_idx": pos}, "item": {"idx": item},
                "neg_item": {"idx": neg}}

    def __iter__(self) -> Iterator[InteractionBatchType]:
        while True:
            yield self.batch()


FOUR_WEEKS = 4 * 7 * 24 * 3600       # polars "4w", in the seconds of a MovieLens timestamp


def _segment_layout(keys_sorted: torch.Tensor):
    """(segment id of every position, first position of every segment, length of every segment) of a sorted key vector."""
    n = keys_sorted.numel()
    new = torch.ones(n, dtype=torch.bool, device=keys_sorted.device)
    new[1:] = keys_sorted[1:] != keys_sorted[:-1]
    seg = torch.cumsum(new.to(torch.int64), 0) - 1
    start = torch.nonzero(new).flatten()
    length = torch.diff(torch.cat([start, torch.tensor([n], device=start.device)]))
    return seg, start, length


def _rank_min(values_sorted: torch.Tensor, group_start_of_pos: torch.Tensor) -> torch.Tensor:
    """polars ``rank("min")`` (1-based; ties share the lowest rank) of values that are sorted inside their groups:
    position of the first element of the tie run, relative to its group's first position."""
    n = values_sorted.numel()
    pos = torch.arange(n, device=values_sorted.device)
    run_new = torch.ones(n, dtype=torch.bool, device=values_sorted.device)
    run_new[1:] = (values_sorted[1:] != values_sorted[:-1]) | (group_start_of_pos[1:] != group_start_of_pos[:-1])
    run_start = torch.cummax(torch.where(run_new, pos, torch.zeros_like(pos)), 0).values
    return run_start - group_start_of_pos + 1


def split_ratings(user: torch.Tensor, timestamp: torch.Tensor, *, train_prop: float = 0.8, val_prop: float = 0.2):
    """``train_test_split`` of the reference (xfmr_rec/data/prepare.py:160-194) on id / time vectors: per user the first
    ``train_prop`` of its ratings IN TIME are train (``p = (rank_min(datetime) - 1) / count < train_prop``); of the users
    that own non-train ratings, those with the largest ``val_prop`` share of such ratings (``(rank_min(len) - 1) /
    n_users >= 1 - val_prop``) are validation users, the others test users.  Returns bool vectors
    ``is_train, is_val, is_test`` aligned with the input."""
    n = user.numel()
    o1 = torch.argsort(timestamp, stable=True)
    order = o1[torch.argsort(user[o1], stable=True)]                 # by (user, time), ties in input order
    su, st = user[order], timestamp[order]
    seg, start, length = _segment_layout(su)
    rank = _rank_min(st, start[seg])
    p = (rank - 1).to(torch.float64) / length[seg].to(torch.float64)
    train_sorted = p < train_prop
    is_train = torch.empty(n, dtype=torch.bool, device=user.device)
    is_train[order] = train_sorted
    # users_split: over the users with at least one non-train rating
    nontrain = torch.zeros(start.numel(), dtype=torch.int64, device=user.device)
    nontrain.index_add_(0, seg, (~train_sorted).to(torch.int64))
    has = nontrain > 0
    lens = nontrain[has]
    lo = torch.argsort(lens, stable=True)
    r = _rank_min(lens[lo], torch.zeros_like(lens))
    pv = torch.empty(lens.numel(), dtype=torch.float64, device=user.device)
    pv[lo] = (r - 1).to(torch.float64) / max(lens.numel(), 1)
    val_user = torch.zeros(start.numel(), dtype=torch.bool, device=user.device)
    val_user[has] = pv >= 1.0 - val_prop
    val_sorted = (~train_sorted) & val_user[seg]
    is_val = torch.empty_like(is_train)
    is_val[order] = val_sorted
    return is_train, is_val, (~is_train) & (~is_val)


class InteractionTable:
    """The ids-only interaction tables a training / evaluation run needs, built once from the ratings
    (``user``, ``item`` -- the 1-based ``movie_rn`` -- , ``rating``, ``timestamp`` in seconds), all torch ops (the tensors
    may live on the GPU).  Follows ``prepare_movielens`` (prepare.py:313-325) for everything that is not text:

    * ``is_train / is_val / is_test`` -- :func:`split_ratings`;
    * ``pair_user / pair_item / pair_target`` -- the train ratings (``ratings.parquet`` filtered by ``is_train``,
      data/lightning.py:344-354), sorted by (user, time);
    * ``pos_off / pos_items`` -- every user's train items in time order: the ``target`` of a train row
      (``gather_history``, prepare.py:236-241) whose item rows become ``pos_idx`` (``UserProcessor.process``,
      data/lightning.py:274-280);
    * ``history_lo / history_hi`` -- per rating (in (user, time) order, ``order`` maps back to the input): its rolling
      4-week history is ``sorted_item[history_lo : history_hi]`` -- the user's ratings with ``t - 4w < t' < t``
      (``rolling("datetime", period="4w", closed="none")``, prepare.py:230-234);
    * ``eval_sets(split)`` -- per user of the split (``process_users``, :272-310): ``history`` = its train items
      (excluded from retrieval), ``target`` = its non-train items with their ratings."""

    def __init__(self, user, item, rating, timestamp, *, train_prop: float = 0.8, val_prop: float = 0.2) -> None:
        user, item = torch.as_tensor(user, dtype=torch.int64), torch.as_tensor(item, dtype=torch.int64)
        timestamp = torch.as_tensor(timestamp, dtype=torch.int64).to(user.device)
        rating = torch.as_tensor(rating).to(user.device)
        self.is_train, self.is_val, self.is_test = split_ratings(user, timestamp, train_prop=train_prop, val_prop=val_prop)
        o1 = torch.argsort(timestamp, stable=True)
        self.order = o1[torch.argsort(user[o1], stable=True)]
        su, st = user[self.order], timestamp[self.order]
        self.sorted_user, self.sorted_item, self.sorted_time = su, item[self.order], st
        self.sorted_rating = rating[self.order]
        self.sorted_train = self.is_train[self.order]
        self.sorted_val, self.sorted_test = self.is_val[self.order], self.is_test[self.order]
        self.num_user_rows = int(user.max()) + 1
        # rolling 4-week window of every rating: a slice of the (user, time)-sorted rows.  One composite key orders
        # (user, time) pairs; its offset form turns "t - 4w < t' < t inside the same user" into two searchsorted calls.
        span = int(st.max() - st.min()) + FOUR_WEEKS + 2
        key = su * span + (st - st.min())
        self.history_lo = torch.searchsorted(key, key - FOUR_WEEKS, right=True)        # first t' > t - 4w ...
        seg, start, _ = _segment_layout(su)
        self.history_lo = torch.maximum(self.history_lo, start[seg])                   # ... of the same user
        self.history_hi = torch.searchsorted(key, key, right=False)                    # first t' >= t
        # train pairs and per-user positives
        tr = self.sorted_train
        self.pair_user, self.pair_item = su[tr], self.sorted_item[tr]
        self.pair_target = self.sorted_rating[tr].to(torch.float32)
        counts = torch.bincount(self.pair_user, minlength=self.num_user_rows)
        self.pos_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=user.device), torch.cumsum(counts, 0)])
        self.pos_items = self.pair_item

    def eval_sets(self, split: str):
        """``(users, history_csr, target_csr)`` of ``split`` in {"val", "test"}: ``users`` ascending; ``history_csr`` =
        (offsets, train item rows) to exclude; ``target_csr`` = (offsets, item rows, ratings) to retrieve -- the shapes
        ``MatrixFactorizationLitModule.update_metrics`` consumes."""
        flag = {"val": self.sorted_val, "test": self.sorted_test}[split]
        users = torch.unique(self.sorted_user[flag])
        dev = users.device
        is_eval_user = torch.zeros(self.num_user_rows, dtype=torch.bool, device=dev)
        is_eval_user[users] = True
        slot = torch.full((self.num_user_rows,), -1, dtype=torch.int64, device=dev)
        slot[users] = torch.arange(users.numel(), device=dev)

        def csr(mask):
            rows = slot[self.sorted_user[mask]]                       # already grouped by user, ascending
            off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(rows, minlength=users.numel()), 0)])
            return off, mask

        h_off, h_mask = csr(self.sorted_train & is_eval_user[self.sorted_user])
        t_off, t_mask = csr((~self.sorted_train) & is_eval_user[self.sorted_user])
        return (users, (h_off, self.sorted_item[h_mask]),
                (t_off, self.sorted_item[t_mask], self.sorted_rating[t_mask].to(torch.float32)))

    def sampler(self, *, num_items: int, batch_size: int = BATCH_SIZE, seed: int = 0, device="cuda", pos_pad: int | None = None,
                user_range: tuple[int, int] | None = None, history: bool = False) -> "DeviceInteractionSampler":
        """``history=True``: batches also carry ``user.history = (start, end, sorted_item)``, the rolling window of every
        example (``history_lo / history_hi`` of the train pairs) -- the input of ``models.HistoryPoolingTower``."""
        hist = {}
        if history:
            tr = self.sorted_train
            hist = {"pair_hist_lo": self.history_lo[tr], "pair_hist_hi": self.history_hi[tr], "hist_items": self.sorted_item}
        return DeviceInteractionSampler(self.pair_user, self.pair_item, self.pair_target, self.pos_off, self.pos_items,
                                        num_items=num_items, batch_size=batch_size, pos_pad=pos_pad, seed=seed, device=device,
                                        user_range=user_range, **hist)


class DeviceInteractionSampler:
    """The training batches, produced on the GPU from HBM-resident interactions (``mf_sample_batch``):
    the counterpart of ``InteractionProcessor.get_batch_data`` (xfmr_rec/data/lightning.py:311-363) for
    id-only towers.  ``pair_user / pair_item / pair_target``: one entry per rating; the positive list
    of user u is ``pos_items[pos_off[u] : pos_off[u + 1]]`` (``UserProcessor.process``, :274-280).
    ``batch(step)`` is example positions ``step * batch_size ...`` of a stream that is reshuffled
    every epoch; the same (seed, step) always gives the same batch.

    Positives.  The reference passes ALL of a user's targets and pads to the longest list of the batch
    (data/lightning.py:275-279, load.py:38-55).  Default (``pos_pad=None``): **no padded tensor at all** -- a batch carries
    ``user.pos_csr = (user idx, pos_off, pos_items)``, the sampler's own HBM-resident lists, and the mask kernels read them
    in place (``mf_loss_fwd_csr``): nothing is ever dropped, and a user with 30,000 ratings costs 30,000 list reads, not a
    30,000-column matrix.  ``pos_pad=P``: the reference's layout, ``user.pos_idx[B, P]`` 0-padded on the right; a P shorter
    than the longest list of the data would silently turn positives into negatives and is refused unless
    ``truncate_positives=True`` says that this is wanted.  ``user_range=(lo, hi)`` keeps only the pairs of users
    ``lo <= u < hi``: the per-rank stream of a user-partitioned job (``distributed.ShardedTrainer(user_mode="partitioned")``).

    History.  ``pair_hist_lo / pair_hist_hi`` (one window per pair) and ``hist_items``: every batch also carries
    ``user.history = (start [B], end [B], hist_items)`` -- the window of the pair in each row (``mf_sample_history``, the same
    permutation as ``mf_sample_batch``); ``user_range`` filters the windows with their pairs."""

    def __init__(self, pair_user, pair_item, pair_target, pos_off, pos_items, *, num_items: int,
                 batch_size: int = BATCH_SIZE, pos_pad: int | None = None, seed: int = 0, device="cuda",
                 user_range: tuple[int, int] | None = None, truncate_positives: bool = False, pair_hist_lo=None, pair_hist_hi=None,
                 hist_items=None) -> None:
        from . import _lib

        self._lib = _lib
        i64 = lambda t: torch.as_tensor(t, dtype=torch.int64).to(device).contiguous()  # noqa: E731
        self.pair_user, self.pair_item = i64(pair_user), i64(pair_item)
        self.pair_target = torch.as_tensor(pair_target, dtype=torch.float32).to(device).contiguous()
        given = [t is not None for t in (pair_hist_lo, pair_hist_hi, hist_items)]
        if any(given) and not all(given):
            msg = "pair_hist_lo, pair_hist_hi and hist_items go together"
            raise ValueError(msg)
        self.pair_hist_lo = self.pair_hist_hi = self.hist_items = None
        if all(given):
            self.pair_hist_lo, self.pair_hist_hi, self.hist_items = i64(pair_hist_lo), i64(pair_hist_hi), i64(hist_items)
            if not (self.pair_hist_lo.numel() == self.pair_hist_hi.numel() == self.pair_user.numel()):
                msg = (f"one history window per pair: {self.pair_hist_lo.numel() = }, {self.pair_hist_hi.numel() = }, "
                       f"{self.pair_user.numel() = }")
                raise ValueError(msg)
            if self.pair_hist_lo.numel() and (int(self.pair_hist_lo.min()) < 0 or int(self.pair_hist_hi.max()) > self.hist_items.numel()
                                              or bool((self.pair_hist_hi < self.pair_hist_lo).any())):
                msg = f"history windows must satisfy 0 <= lo <= hi <= len(hist_items) = {self.hist_items.numel()}"
                raise ValueError(msg)
            if self.hist_items.numel() == 0:
                self.hist_items = torch.zeros(1, dtype=torch.int64, device=device)
        if user_range is not None:
            keep = (self.pair_user >= user_range[0]) & (self.pair_user < user_range[1])
            self.pair_user, self.pair_item, self.pair_target = (self.pair_user[keep].contiguous(), self.pair_item[keep].contiguous(),
                                                                self.pair_target[keep].contiguous())
            if self.pair_hist_lo is not None:
                self.pair_hist_lo, self.pair_hist_hi = self.pair_hist_lo[keep].contiguous(), self.pair_hist_hi[keep].contiguous()
        self.pos_off, self.pos_items = i64(pos_off), i64(pos_items)
        if self.pos_items.numel() == 0:
            self.pos_items = torch.zeros(1, dtype=torch.int64, device=device)
        n = self.pair_user.numel()
        if not (self.pair_item.numel() == n == self.pair_target.numel()) or n == 0:
            msg = "pair_user, pair_item and pair_target must have the same, non-zero length"
            raise ValueError(msg)
        # one-time checks on the data (host syncs at construction, none per batch)
        if int(self.pair_user.min()) < 0 or int(self.pair_user.max()) + 1 >= self.pos_off.numel():
            msg = f"every user id needs a row in pos_off: {int(self.pair_user.max()) = }, {self.pos_off.numel() = }"
            raise ValueError(msg)
        longest = int((self.pos_off[1:] - self.pos_off[:-1]).max()) if self.pos_off.numel() > 1 else 0
        if pos_pad is None:
            pos_pad = 0                      # CSR mode: batches carry the lists themselves
        elif longest > pos_pad and not truncate_positives:
            msg = (f"pos_pad = {pos_pad} would drop positives (longest list: {longest}); the dropped items would enter the "
                   "losses as negatives.  Pass pos_pad=None (sized from the data) or truncate_positives=True")
            raise ValueError(msg)
        self.longest_positive_list = longest
        self.num_items, self.batch_size, self.pos_pad, self.seed = int(num_items), int(batch_size), int(pos_pad), int(seed)

    @property
    def steps_per_epoch(self) -> int:
        return -(-self.pair_user.numel() // self.batch_size)

    def batch(self, step: int) -> InteractionBatchType:
        b, p, dev = self.batch_size, self.pos_pad, self.pair_user.device
        user = torch.empty(b, dtype=torch.int64, device=dev)
        item = torch.empty(2 * b, dtype=torch.int64, device=dev)
        target = torch.empty(b, dtype=torch.float32, device=dev)
        pos = torch.empty(b, p, dtype=torch.int64, device=dev) if p > 0 else None
        lib = self._lib
        lib.check(lib.lib().mf_sample_batch(self.pair_user.data_ptr(), self.pair_item.data_ptr(), self.pair_target.data_ptr(),
                                            self.pair_user.numel(), self.pos_off.data_ptr(), self.pos_items.data_ptr(),
                                            self.num_items, self.seed, int(step) * b, b, p, user.data_ptr(), item.data_ptr(),
                                            target.data_ptr(), None if pos is None else pos.data_ptr(), lib.stream_ptr()))
        ub = {"idx": user, "pos_idx": pos} if pos is not None else {"idx": user, "pos_csr": (user, self.pos_off, self.pos_items)}
        if self.pair_hist_lo is not None:
            h_start = torch.empty(b, dtype=torch.int64, device=dev)
            h_end = torch.empty(b, dtype=torch.int64, device=dev)
            lib.check(lib.lib().mf_sample_history(self.pair_hist_lo.data_ptr(), self.pair_hist_hi.data_ptr(), self.pair_user.numel(),
                                                  self.seed, int(step) * b, b, h_start.data_ptr(), h_end.data_ptr(), lib.stream_ptr()))
            ub["history"] = (h_start, h_end, self.hist_items)
        return {"target": target, "user": ub, "item": {"idx": item[:b]}, "neg_item": {"idx": item[b:]}}

    def __iter__(self) -> Iterator[InteractionBatchType]:
        step = 0
        while True:
            yield self.batch(step)
            step += 1


# ------------------------------------------------------------------ MovieLens ratings files (ids only) ---
def _read_id_column(path, sep: str, skip_header: bool):
    """First field of every line of an ids file (movies.dat / users.dat / movies.csv): the reference numbers its rows
    ``movie_rn`` / ``user_rn`` in FILE order from 1 (``with_row_index(..., offset=1)``, prepare.py:85,121)."""
    import numpy as np

    ids = []
    with open(path, encoding="iso-8859-1") as f:
        if skip_header:
            next(f, None)
        for line in f:
            if line.strip():
                ids.append(int(line.split(sep, 1)[0]))
    return np.asarray(ids, dtype=np.int64)


def read_ratings(path) -> dict[str, torch.Tensor]:
    """A MovieLens ratings file as id vectors: ``ml-1m/ratings.dat`` (``UserID::MovieID::Rating::Timestamp``, the file
    ``load_ratings`` reads, xfmr_rec/data/prepare.py:132-152) or ``ml-25m/ratings.csv`` (``userId,movieId,rating,timestamp``
    with a header; half-star ratings).  Returns ``user_id``, ``movie_id``, ``timestamp`` (int64) and ``rating`` (float32)."""
    import io
    import pathlib

    import numpy as np
    import pandas as pd

    path = pathlib.Path(path)
    if path.suffix == ".dat":           # "::" is not a single-character separator: rewrite it and let the C parser run
        raw = path.read_bytes().replace(b"::", b",")
        df = pd.read_csv(io.BytesIO(raw), header=None, names=["user_id", "movie_id", "rating", "timestamp"],
                         dtype={"user_id": np.int64, "movie_id": np.int64, "rating": np.float32, "timestamp": np.int64})
    else:
        df = pd.read_csv(path, header=0, names=["user_id", "movie_id", "rating", "timestamp"],
                         dtype={"user_id": np.int64, "movie_id": np.int64, "rating": np.float32, "timestamp": np.int64})
    return {k: torch.from_numpy(df[k].to_numpy().copy()) for k in ("user_id", "movie_id", "rating", "timestamp")}


def find_movielens(root=None):
    """The first MovieLens ratings file under ``root`` (default: ``$MF_MOVIELENS_DIR``, then ``./data``): the reference's
    ``data/ml-1m/ratings.dat``, or ``ml-25m/ratings.csv`` / ``ml-latest*/ratings.csv``.  ``None`` when there is none
    (there is no network here: benchmarks and fixtures never depend on the files)."""
    import os
    import pathlib

    roots = [root] if root is not None else [os.environ.get("MF_MOVIELENS_DIR"), "data"]
    for r in roots:
        if not r:
            continue
        r = pathlib.Path(r)
        for rel in ("ml-25m/ratings.csv", "ratings.csv", "ml-1m/ratings.dat", "ratings.dat", "ml-20m/ratings.csv",
                    "ml-latest/ratings.csv", "ml-latest-small/ratings.csv", "ml-100k/ratings.csv"):
            if (r / rel).is_file():
                return r / rel
    return None


def movielens_interactions(ratings_path, *, train_prop: float = 0.8, val_prop: float = 0.2):
    """``(InteractionTable, meta)`` of a MovieLens ratings file.  Item rows are the reference's ``movie_rn``: the 1-based
    position of the movie in ``movies.dat`` / ``movies.csv`` next to the ratings file (file order, prepare.py:85); users
    likewise from ``users.dat``; without those files, the rank of the id among the ids that occur (the same numbers whenever
    the side files are sorted by id and complete, as ML-1M's are).  Row 0 of both tables stays the padding row."""
    import pathlib

    import numpy as np

    ratings_path = pathlib.Path(ratings_path)
    r = read_ratings(ratings_path)

    def row_numbers(ids: torch.Tensor, side_files):
        for name, sep, header in side_files:
            f = ratings_path.parent / name
            if f.is_file():
                order = _read_id_column(f, sep, header)
                break
        else:
            order = np.unique(ids.numpy())
        lut = np.full(int(max(order.max(), int(ids.max()))) + 1, -1, dtype=np.int64)
        lut[order] = np.arange(1, order.size + 1)
        rn = lut[ids.numpy()]
        if (rn < 0).any():
            msg = f"{ratings_path}: ids without a row in the side file"
            raise ValueError(msg)
        return torch.from_numpy(rn), int(order.size) + 1

    item, num_items = row_numbers(r["movie_id"], (("movies.dat", "::", False), ("movies.csv", ",", True)))
    user, num_users = row_numbers(r["user_id"], (("users.dat", "::", False),))
    table = InteractionTable(user, item, r["rating"], r["timestamp"], train_prop=train_prop, val_prop=val_prop)
    meta = {"path": str(ratings_path), "num_users": num_users, "num_items": num_items, "ratings": int(user.numel()),
            "train_pairs": int(table.pair_user.numel())}
    return table, meta


def to_device(batch, device):
    if isinstance(batch, dict):
        return {k: to_device(v, device) for k, v in batch.items()}
    if isinstance(batch, (tuple, list)):             # ``pos_csr`` / ``history`` triples
        return type(batch)(to_device(v, device) for v in batch)
    return batch.to(device) if isinstance(batch, torch.Tensor) else batch


# ---------------------------------------------------------------------------------------- feature bags ----
# The reference embeds each entity's ATTRIBUTES, not its id: an item is the JSON of {"title", "genres"}, a user the JSON of
# {"gender", "age", "occupation", "zipcode"} (xfmr_rec/data/prepare.py:69-127), read by one shared text encoder
# (xfmr_rec/lightning.py:60-74).  Here those attributes become hashed tokens, one row each of a bucket table
# (models.FeatureBagTower): the classic EmbeddingBag tower of matrix-factorization recommenders.


class FeatureBags:
    """Bags of ``(token, weight)`` pairs as a CSR: entity e's bag is ``tokens[off[e]:off[e + 1]]`` with
    ``weights[off[e]:off[e + 1]]`` (``None``: every weight is 1).  ``max_len`` (the longest bag) is fixed here, on the host,
    so that the GPU kernels are sized without reading anything back.  Weights must be finite and >= 0."""

    def __init__(self, off, tokens, weights=None) -> None:
        self.off = torch.as_tensor(off, dtype=torch.int64)
        self.tokens = torch.as_tensor(tokens, dtype=torch.int64)
        self.weights = None if weights is None else torch.as_tensor(weights, dtype=torch.float32)
        if self.off.dim() != 1 or self.off.numel() < 1 or self.tokens.dim() != 1:
            msg = f"a bag CSR is off [n + 1] and tokens [nnz]: {tuple(self.off.shape) = }, {tuple(self.tokens.shape) = }"
            raise ValueError(msg)
        off_cpu = self.off.cpu()
        if int(off_cpu[0]) != 0 or int(off_cpu[-1]) != self.tokens.numel() or bool((off_cpu[1:] < off_cpu[:-1]).any()):
            msg = "bag offsets must start at 0, be non-decreasing and end at len(tokens)"
            raise ValueError(msg)
        if self.weights is not None:
            if self.weights.shape != self.tokens.shape:
                msg = f"one weight per token: {tuple(self.weights.shape)} != {tuple(self.tokens.shape)}"
                raise ValueError(msg)
            w = self.weights.cpu()
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                msg = "bag weights must be finite and >= 0"
                raise ValueError(msg)
        self.max_len = int((off_cpu[1:] - off_cpu[:-1]).max()) if off_cpu.numel() > 1 else 0

    @classmethod
    def from_lists(cls, lists, weights=None) -> "FeatureBags":
        """From per-entity token lists (and optional per-entity weight lists of the same lengths)."""
        lens = [len(x) for x in lists]
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        tokens = [int(t) for x in lists for t in x]
        w = None
        if weights is not None:
            if [len(x) for x in weights] != lens:
                msg = "one weight per token: weight lists must have the lengths of the token lists"
                raise ValueError(msg)
            w = [float(v) for x in weights for v in x]
        return cls(off, tokens, w)

    def __len__(self) -> int:
        return self.off.numel() - 1

    @property
    def device(self) -> torch.device:
        return self.tokens.device

    def to(self, device) -> "FeatureBags":
        out = object.__new__(FeatureBags)
        out.off, out.tokens = self.off.to(device), self.tokens.to(device)
        out.weights = None if self.weights is None else self.weights.to(device)
        out.max_len = self.max_len
        return out

    def lists(self) -> list[list[int]]:
        off, tok = self.off.tolist(), self.tokens.tolist()
        return [tok[off[e]:off[e + 1]] for e in range(len(self))]


class FeatureHasher:
    """Attributes -> hashed bucket tokens.  An entity is the reference's JSON text (or the dict it encodes): a list value
    gives one token per element (``genres=Comedy``), a field of ``text_fields`` one token per lowercase ``[a-z0-9]+`` word
    (``title=toy``, ``title=story``, ``title=1995``), any other value one ``field=value`` token.  ``id_field``: the entity's
    own id (passed to :meth:`bags`) is one more token.  Bucket = ``1 + blake2b(b"field=value", 8-byte digest, key = seed as
    8 little-endian bytes) mod (num_buckets - 1)``: never 0 (padding), and the same in every process (``hash()`` is not)."""

    def __init__(self, num_buckets: int, seed: int = 0, text_fields=("title",), id_field: str | None = None) -> None:
        if num_buckets < 2:  # noqa: PLR2004
            msg = f"num_buckets must be >= 2 (bucket 0 is padding): {num_buckets = }"
            raise ValueError(msg)
        if not 0 <= seed < 2**64:
            msg = f"seed must fit in 8 bytes: {seed = }"
            raise ValueError(msg)
        self.num_buckets, self.seed = int(num_buckets), int(seed)
        self.text_fields, self.id_field = tuple(text_fields), id_field
        self._key = self.seed.to_bytes(8, "little")

    def bucket(self, field: str, value) -> int:
        import hashlib

        h = hashlib.blake2b(f"{field}={value}".encode(), digest_size=8, key=self._key).digest()
        return 1 + int.from_bytes(h, "little") % (self.num_buckets - 1)

    def features(self, entity) -> list[str]:
        """The ``field=value`` strings of one entity (JSON text, dict, or ``None`` / ``""`` for an empty bag)."""
        import json
        import re

        if entity is None or entity == "":
            return []
        if isinstance(entity, str):
            entity = json.loads(entity)
        out = []
        for field, value in entity.items():
            if value is None:
                continue
            if isinstance(value, (list, tuple)):
                out += [f"{field}={v}" for v in value if v is not None]
            elif field in self.text_fields:
                out += [f"{field}={w}" for w in re.findall(r"[a-z0-9]+", str(value).lower())]
            else:
                out.append(f"{field}={value}")
        return out

    def tokens(self, entity, entity_id=None) -> list[int]:
        feats = self.features(entity)
        toks = [self.bucket(*f.split("=", 1)) for f in feats]
        if self.id_field is not None and entity_id is not None:
            toks.append(self.bucket(self.id_field, entity_id))
        return toks

    def bags(self, texts, ids=None) -> FeatureBags:
        """One bag per entity of ``texts``; ``ids`` (with ``id_field``) adds each entity's id token."""
        texts = list(texts)
        if self.id_field is not None and ids is not None and len(ids) != len(texts):
            msg = f"one id per entity: {len(ids)} != {len(texts)}"
            raise ValueError(msg)
        return FeatureBags.from_lists([self.tokens(t, None if ids is None else int(ids[k])) for k, t in enumerate(texts)])

    def config(self) -> dict:
        return {"num_buckets": self.num_buckets, "seed": self.seed, "text_fields": list(self.text_fields), "id_field": self.id_field}


def _json_text(obj: dict) -> str:
    """polars' ``struct.json_encode`` layout (prepare.py:86-87, 118-121): compact, non-ASCII kept."""
    import json

    return json.dumps(obj, separators=(",", ":"), ensure_ascii=False)


def read_movielens_features(ratings_path):
    """``(item_texts, user_texts)``: the reference's JSON texts of every item (``{"title", "genres"}``, prepare.py:69-92)
    and user (``{"gender", "age", "occupation", "zipcode"}``, :95-127), indexed by the rows :func:`movielens_interactions`
    assigns (file order from 1; entry 0, the padding row, is ``None``: an empty bag).  Read from ``movies.dat`` /
    ``movies.csv`` and ``users.dat`` next to the ratings file; a list is ``None`` when its file is absent (ML-25M has no
    ``users.dat``)."""
    import csv
    import pathlib

    root = pathlib.Path(ratings_path).parent
    items = None
    if (root / "movies.dat").is_file():
        items = [None]
        with open(root / "movies.dat", encoding="iso-8859-1") as f:
            for line in f:
                if line.strip():
                    _, title, genres = line.rstrip("\r\n").split("::", 2)
                    items.append(_json_text({"title": title, "genres": genres.split("|")}))
    elif (root / "movies.csv").is_file():
        items = [None]
        with open(root / "movies.csv", encoding="utf-8", newline="") as f:
            rows = csv.reader(f)
            next(rows, None)
            for row in rows:
                if row:
                    items.append(_json_text({"title": row[1], "genres": row[2].split("|")}))
    users = None
    if (root / "users.dat").is_file():
        users = [None]
        with open(root / "users.dat", encoding="iso-8859-1") as f:
            for line in f:
                if line.strip():
                    _, gender, age, occupation, zipcode = line.rstrip("\r\n").split("::")[:5]
                    users.append(_json_text({"gender": gender, "age": int(age), "occupation": int(occupation), "zipcode": zipcode}))
    return items, users


def synthetic_item_features(num_items: int, num_genres: int = 20, vocab: int = 5000, seed: int = 0):
    """``(texts, genre)``: MovieLens-shaped item JSON texts for probes and tests (row 0 = ``None``, the padding row).
    Item i has 1-3 genres from a skewed (Zipf-like) distribution -- ``genre[i]`` is its first -- and a title of 1-12 words
    from a ``vocab``-word vocabulary plus a year, as ``"w12 w7 (1994)"``."""
    import numpy as np

    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, num_genres + 1) ** 1.1
    p /= p.sum()
    genre = np.zeros(num_items, dtype=np.int64)
    texts = [None]
    for i in range(1, num_items):
        k = int(rng.integers(1, 4))
        gs = list(dict.fromkeys(rng.choice(num_genres, size=k, p=p).tolist()))
        genre[i] = gs[0]
        words = " ".join(f"w{int(w)}" for w in rng.integers(0, vocab, int(rng.integers(1, 13))))
        texts.append(_json_text({"title": f"{words} ({int(rng.integers(1920, 2020))})", "genres": [f"g{g}" for g in gs]}))
    return texts, torch.from_numpy(genre)


def item_tag_bits(item_texts, field: str = "genres"):
    """``(tags int64 [rows], vocabulary list[str])``: the values of ``field`` in the items' JSON texts
    (:func:`read_movielens_features`, :func:`synthetic_item_features`) as 64 boolean attributes per row -- what
    ``retrieval.ItemIndex.set_tags`` takes and a ``retrieval.TagFilter`` is evaluated on.  The names are sorted; bit i of row
    r is set iff the row carries name i (a list value: each element; any other value: itself).  ``None`` / ``""`` (row 0, the
    padding row) and a row without the field give 0.  More than 64 names: ``ValueError``."""
    import json

    import numpy as np

    rows = []
    for text in item_texts:
        entity = json.loads(text) if isinstance(text, str) and text else (text or {})
        value = entity.get(field)
        values = value if isinstance(value, (list, tuple)) else ([] if value is None else [value])
        rows.append([str(v) for v in values if v is not None])
    vocabulary = sorted({v for r in rows for v in r})
    if len(vocabulary) > 64:  # noqa: PLR2004
        msg = f"at most 64 attributes fit a tag word: {field!r} has {len(vocabulary)} values"
        raise ValueError(msg)
    bit = {name: i for i, name in enumerate(vocabulary)}
    tags = np.zeros(len(rows), dtype=np.uint64)
    for r, names in enumerate(rows):
        for name in names:
            tags[r] |= np.uint64(1) << np.uint64(bit[name])
    return torch.from_numpy(tags.view(np.int64)), vocabulary
