"""GPU: positions over a row-sharded catalog (``mf_target_words`` + ``mf_key_positions``, ``ItemIndex.target_words`` /
``key_positions``, ``ShardedIndex.positions``).  All but the last test use the shard-on-one-card form: the S shards of one
catalog are indexed on one device, the two exports are called per shard, and the results are combined with ``torch.max`` /
``sum`` -- against ``mf_target_positions`` on the unsharded catalog and the numpy spec (tests/_sharded_position_spec.py).
Positions and counts are compared as integers, scores as uint32 views: no tolerance anywhere."""
from __future__ import annotations

import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import _position_spec as spec
from tests import _sharded_position_spec as sspec
from tests import test_distributed_cpu as tdc
from tests import test_gpu_distributed as tgd
from tests import test_gpu_positions as tgp
from tests import test_sharded_positions_cpu as tsc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_dev, _bits, _unit, _same = tgp._dev, tgp._bits, tgp._unit, tgp._same
LAYOUTS = [(s, deal) for deal in (sspec.round_robin, sspec.contiguous) for s in (1, 2, 3, 8)]
LENGTHS = (0, 1, 4, 5, 16, 17, 1024, 1025)      # the three register-count instantiations, the sorted-bin path, two passes


class Shards:
    """The two exports per shard through the C ABI, on buffers that are kept (graph capture) and poisoned before every call."""

    def __init__(self, mf, q, items, layout, t_off, t_ids, excl=None, ws="preferred"):
        self.mf, self.lib, self.layout = mf, mf._lib.lib(), layout
        self.q = q.to(DEV).contiguous()
        self.nq, self.d = self.q.shape
        self.items = [items[torch.from_numpy(sspec.rows_of(sh))].to(DEV).contiguous() for sh in layout]
        # local exclusion rows: -1 for the other shards' rows, as ShardedIndex._localise writes them
        self.excl = [mf.retrieval._csr(None if excl is None else [[sspec.local_row(g, sh) for g in ex] for ex in excl], self.nq, DEV)
                     for sh in layout]
        self.t_off, self.nt = _dev(t_off, torch.int64), len(t_ids)
        self.t_ids = _dev(t_ids if self.nt else [0], torch.int64)
        size = self.lib.mf_key_positions_ws_bytes if ws == "preferred" else self.lib.mf_key_positions_min_ws_bytes
        self.nbytes = [size(self.nq, sh[2], self.d) for sh in layout]
        self.ws = torch.empty(max(self.nbytes), dtype=torch.uint8, device=DEV)       # one slab, shard after shard
        s, t = len(layout), max(self.nt, 1)
        self.words = torch.empty(s, t, dtype=torch.int64, device=DEV)
        self.wmax = torch.empty(t, dtype=torch.int64, device=DEV)
        self.above = torch.empty(s, t, dtype=torch.int64, device=DEV)
        self.score = torch.empty(s, t, dtype=torch.float32, device=DEV)
        self.ncand = torch.empty(s, self.nq, dtype=torch.int64, device=DEV)

    def poison(self, word=0xA5):
        self.ws.fill_(word)
        for t in (self.words, self.wmax, self.above, self.ncand):
            t.fill_(-7777)
        self.score.fill_(float("nan"))
        if self.nt == 0:
            self.words.fill_(0)                               # (one unused word: the maximum below reads it)

    def launch_words(self):
        stream = self.mf._lib.stream_ptr()
        for s, (stride, offset, n) in enumerate(self.layout):
            self.mf._lib.check(self.lib.mf_target_words(self.q.data_ptr(), self.nq, self.items[s].data_ptr(), n, self.d, self.t_off.data_ptr(),
                                                        self.t_ids.data_ptr(), self.nt, stride, offset, self.words[s].data_ptr(), stream))

    def launch(self):
        p, stream = self.mf._lib.ptr, self.mf._lib.stream_ptr()
        self.launch_words()
        torch.amax(self.words, dim=0, out=self.wmax)          # at most one shard holds a row
        for s, (stride, offset, n) in enumerate(self.layout):
            self.mf._lib.check(self.lib.mf_key_positions(
                self.q.data_ptr(), self.nq, self.items[s].data_ptr(), n, self.d, self.t_off.data_ptr(), self.t_ids.data_ptr(), self.wmax.data_ptr(),
                self.nt, stride, offset, p(self.excl[s][0]), p(self.excl[s][1]), self.ws.data_ptr(), self.nbytes[s], self.above[s].data_ptr(),
                self.score[s].data_ptr(), self.ncand[s].data_ptr(), stream))

    def result(self):
        above, score = self.above[:, : self.nt], self.score[:, : self.nt]
        none = (above < 0).any(dim=0)
        pos = torch.where(none, torch.full_like(above[0], -1), above.sum(dim=0))
        score = torch.where(none, torch.full_like(score[0], float("-inf")), score[0])
        return pos.cpu().numpy(), score.cpu().numpy(), self.ncand.sum(dim=0).cpu().numpy()

    def __call__(self, word=0xA5):
        self.poison(word)
        self.launch()
        return self.result()


@functools.lru_cache(maxsize=None)
def _world(nq, n, d, first=0, excl_lists=True):
    """Queries, catalog, exclusion lists (global rows, some outside the catalog) and target lists of every length of LENGTHS in
    turn -- random rows, some outside the catalog, an excluded one and a duplicate among them; computed once and shared."""
    g = torch.Generator().manual_seed(1000 * d + n + nq)
    rng = np.random.default_rng(1000 * d + n + nq)
    q, items = _unit(nq, d, g), _unit(n, d, g)
    items[10] = items[3]                                      # an exact score tie in every query
    excl = [sorted(set(rng.integers(-3, n + 3, int(rng.integers(1, 60))).tolist())) for _ in range(nq)] if excl_lists else None
    lists = []
    for r in range(nq):
        m = LENGTHS[(first + r) % len(LENGTHS)]
        own = rng.integers(-2, n + 2, m).tolist()
        if m >= 4:
            own[0], own[1], own[2] = 3, 10, own[3]            # the tied pair; a duplicate
            inside = [y for y in excl[r] if 0 <= y < n] if excl_lists else []
            if inside:
                own[3] = inside[0]                            # an excluded row
        lists.append(own)
    t_off = np.cumsum([0] + [len(x) for x in lists])
    t_ids = np.array([y for x in lists for y in x], dtype=np.int64)
    return q, items, excl, t_off, t_ids


def _layout(n, k):
    s, deal = LAYOUTS[k % len(LAYOUTS)]
    return deal(n, s)


# ------------------------------------------------------------------------------------------------------- the cases ----
@pytest.mark.parametrize("nq", [1, 33, 70])
@pytest.mark.parametrize("n", [33, 1000, 2500])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_sharded_positions_equal_the_unsharded_call_and_the_spec(mf, d, n, nq):
    """Every shape meets another layout (S in 1, 2, 3, 8; round-robin and contiguous; uneven shard sizes), one query another list
    length; 70 queries run on the minimum workspace: three query blocks."""
    k = (d // 32).bit_length() + 4 * (n // 1000) + 3 * (nq // 33)
    q, items, excl, t_off, t_ids = _world(nq, n, d, first=k if nq == 1 else 0)
    layout = _layout(n, k)
    if nq == 70:
        lib, plan = mf._lib.lib(), (ctypes.c_int64 * 3)()
        assert lib.mf_topk_deep_plan(nq, layout[0][2], d, 1, lib.mf_key_positions_min_ws_bytes(nq, layout[0][2], d), plan) == 0
        assert (plan[0], plan[1]) == (32, 3)
    got = Shards(mf, q, items, layout, t_off, t_ids, excl, ws="minimum" if nq == 70 else "preferred")()
    want = tgp.Call(mf, q, items, t_off, t_ids, excl)()
    _same(got, want, layout)
    if nq > 1:
        assert (want[0] == -1).any() and (want[0] >= 0).any()
    if n <= 1000:
        _same(got, spec.positions(q.numpy(), items.numpy(), t_off, t_ids, excl), "spec")
        _same(got, sspec.sharded_positions(q.numpy(), items.numpy(), layout, t_off, t_ids, excl), "sharded spec")


def test_every_layout_covers_the_catalog_and_is_used():
    used = {(d // 32).bit_length() + 4 * (n // 1000) + 3 * (nq // 33) for d in (32, 64, 128, 256) for n in (33, 1000, 2500) for nq in (1, 33, 70)}
    assert {k % len(LAYOUTS) for k in used} == set(range(len(LAYOUTS)))
    for n in (33, 1000, 2500):
        for s, deal in LAYOUTS:
            layout = deal(n, s)
            assert sorted(np.concatenate([sspec.rows_of(sh) for sh in layout]).tolist()) == list(range(n))
            assert s == 1 or n % s == 0 or len({sh[2] for sh in layout}) > 1       # uneven shard sizes


@pytest.mark.parametrize("k", range(len(LAYOUTS)), ids=lambda k: f"{LAYOUTS[k][1].__name__}-{LAYOUTS[k][0]}")
def test_every_list_length_on_every_layout(mf, k):
    q, items, excl, t_off, t_ids = _world(len(LENGTHS), 2500, 64)
    assert np.diff(t_off).tolist() == list(LENGTHS)
    _same(Shards(mf, q, items, _layout(2500, k), t_off, t_ids, excl)(), tgp.Call(mf, q, items, t_off, t_ids, excl)(), k)


@pytest.mark.parametrize("deal", [sspec.round_robin, sspec.contiguous], ids=lambda f: f.__name__)
def test_a_shard_of_one_row(mf, deal):
    n, d = 9, 32
    g = torch.Generator().manual_seed(9)
    q, items = _unit(3, d, g), _unit(n, d, g)
    items[8] = items[0]                                       # round-robin: both on shard 0, the only one with two rows
    layout = deal(n, 8)
    assert min(sh[2] for sh in layout) == 1
    excl = [[], [4, 8], [0, 1, 2, 3]]
    t_ids = list(range(-1, n + 1)) * 3
    t_off = [0, n + 2, 2 * (n + 2), 3 * (n + 2)]
    got = Shards(mf, q, items, layout, t_off, t_ids, excl)()
    _same(got, spec.positions(q.numpy(), items.numpy(), t_off, t_ids, excl), "spec")
    _same(got, tgp.Call(mf, q, items, t_off, t_ids, excl)(), "unsharded")
    assert sorted(got[0][1: n + 1].tolist()) == list(range(n)) and got[2].tolist() == [9, 7, 5]


# ----------------------------------------------------------------------------------------------------------- ties ----
@pytest.mark.parametrize("k", [3, 6], ids=["round_robin-8", "contiguous-3"])
def test_a_run_of_identical_rows_spans_the_shards(mf, k):
    g = torch.Generator().manual_seed(5)
    n, d = 1500, 64
    q, items = _unit(3, d, g), 0.3 * _unit(n, d, g)
    run = torch.randperm(n, generator=g)[:300].sort().values
    items[run] = 0.5 * q[0]
    layout = _layout(n, k)
    owners = {s for s, sh in enumerate(layout) for y in run.tolist() if sspec.local_row(y, sh) >= 0}
    assert owners == set(range(len(layout)))                  # the run is spread over all shards
    t_ids = run[[0, 1, 150, 298, 299]].tolist() + run.tolist() + [int(run[7])] * 3
    t_off = [0, 5, 5 + 300, len(t_ids)]
    want = spec.positions(q.numpy(), items.numpy(), t_off, t_ids)
    first = want[0][0]
    assert want[0][:5].tolist() == [first, first + 1, first + 150, first + 298, first + 299]      # consecutive places, ascending global rows
    _same(Shards(mf, q, items, layout, t_off, t_ids)(), want)


@pytest.mark.parametrize("k", [1, 2, 7])
def test_a_zero_query_places_every_row_at_its_own_number(mf, k):
    n, d = 1100, 32
    items = _unit(n, d, torch.Generator().manual_seed(6))
    excl = [[0, 2, 5], []]
    t_ids = [1, 3, 4, 6, n - 1, 2] + list(range(0, n, 3))
    t_off = [0, 6, len(t_ids)]
    pos, score, ncand = Shards(mf, torch.zeros(2, d), items, _layout(n, k), t_off, t_ids, excl)()
    assert pos[:6].tolist() == [0, 1, 2, 3, n - 4, -1] and pos[6:].tolist() == list(range(0, n, 3)) and ncand.tolist() == [n - 3, n]
    assert (_bits(score[:5]) == 0).all() and np.isneginf(score[5]) and (_bits(score[6:]) == 0).all()      # +0.0


# ------------------------------------------------------------------------------------------------- exclusion lists ----
def test_shards_without_targets_shards_without_rows_and_three_rows_left(mf):
    g = torch.Generator().manual_seed(7)
    n, d = 2000, 64
    q, items = _unit(4, d, g), _unit(n, d, g)
    layout = sspec.contiguous(n, 3)                           # rows 0 .. 666, 667 .. 1333, 1334 .. 1999
    left = [17, 1203, 1999]
    excl = [[y for y in range(n) if y not in left],           # all but three rows, one on every shard
            list(range(n)),                                   # nothing admissible
            list(range(667, 1334)),                           # the middle shard has every row excluded
            []]
    t_ids = left + [5] + left + list(range(20)) + [700, 1999] + list(range(10))         # query 3: shard 0 holds every target
    t_off = [0, 4, 7, 29, 39]
    want = spec.positions(q.numpy(), items.numpy(), t_off, t_ids, excl)
    assert sorted(want[0][:3].tolist()) == [0, 1, 2] and want[0][3:7].tolist() == [-1] * 4 and want[2].tolist() == [3, 0, n - 667, n]
    call = Shards(mf, q, items, layout, t_off, t_ids, excl)
    got = call()
    _same(got, want)
    _same(got, tgp.Call(mf, q, items, t_off, t_ids, excl)(), "unsharded")
    assert call.ncand.cpu()[:, 2].tolist() == [667, 0, 666] and call.ncand.cpu()[:, 0].tolist() == [1, 1, 1]
    held = (call.words[:, t_off[3]: t_off[4]] != 0).any(dim=1).cpu().tolist()      # query 3's targets: all on shard 0
    assert held == [True, False, False] and (call.above[1:, t_off[3]: t_off[4]] >= 0).all()


def test_no_exclusion_lists_at_all(mf):
    q, items, _, t_off, t_ids = _world(33, 1000, 128, excl_lists=False)
    want = spec.positions(q.numpy(), items.numpy(), t_off, t_ids)
    assert (want[2] == 1000).all()
    for k in (2, 5):
        _same(Shards(mf, q, items, _layout(1000, k), t_off, t_ids, None)(), want, k)


# --------------------------------------------------------------------------------------- the engine it must agree with ----
@pytest.mark.parametrize("shape", [(33, 1000, 64, 3), (70, 2500, 128, 6)], ids=lambda s: "x".join(map(str, s)))
def test_positions_below_1024_are_the_deep_searchs_columns(mf, shape):
    nq, n, d, k = shape
    q, items, excl, t_off, t_ids = _world(nq, n, d)
    pos, score, ncand = Shards(mf, q, items, _layout(n, k), t_off, t_ids, excl)()
    s, rows = mf.retrieval.ItemIndex(items.to(DEV)).search(q.to(DEV), 1024, exclude=excl, path="deep")
    s, rows = s.cpu().numpy(), rows.cpu().numpy()
    assert np.array_equal((rows >= 0).sum(axis=1), np.minimum(ncand, 1024))
    inside = 0
    for r in range(nq):
        listed = set(rows[r][rows[r] >= 0].tolist())
        for e in range(t_off[r], t_off[r + 1]):
            if 0 <= pos[e] < 1024:
                inside += 1
                assert rows[r, pos[e]] == t_ids[e] and _bits(s[r, pos[e]]) == _bits(score[e]), (r, e)
            else:
                assert int(t_ids[e]) not in listed, (r, e)
    assert inside >= len(t_ids) / 4 and len(t_ids) > 1000, (inside, len(t_ids))


# ---------------------------------------------------------------------------------------------------- words alone ----
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_target_words_are_the_chain_scores_words(mf, d):
    nq, n = 5, 333
    q, items, _, _, _ = _world(nq, n, d)
    rng = np.random.default_rng(d)
    lists = [rng.integers(-3, n + 3, m).tolist() for m in (1500, 0, 1, 300, 40)]     # more than one pass of the workgroups; an empty list
    t_off, t_ids = np.cumsum([0] + [len(x) for x in lists]), np.array([y for x in lists for y in x], dtype=np.int64)
    layout = _layout(n, {32: 1, 64: 2, 128: 3, 256: 6}[d])    # round-robin 2, 3, 8; contiguous 3
    call = Shards(mf, q, items, layout, t_off, t_ids)
    call.poison()
    call.launch_words()
    got = call.words.cpu().numpy()
    held = 0
    for s, sh in enumerate(layout):
        scores = spec.chain.scores(q.numpy(), np.ascontiguousarray(items.numpy()[sspec.rows_of(sh)]))
        want = sspec.shard_words(scores, t_off, t_ids, sh)
        assert np.array_equal(got[s], want), (d, s)
        held += int((want != 0).sum())
    assert held == int(((t_ids >= 0) & (t_ids < n)).sum())    # every row of the catalog on exactly one shard, 0 elsewhere
    assert (got >= 0).all() and (got < 2**32).all()


# ------------------------------------------------------------------------------------- determinism, capture, poison ----
def test_repeat_calls_capture_and_poisoned_buffers(mf):
    q, items, excl, t_off, t_ids = _world(70, 2500, 128)
    call = Shards(mf, q, items, _layout(2500, 2), t_off, t_ids, excl)
    first = call(0xA5)
    _same(first, tgp.Call(mf, q, items, t_off, t_ids, excl)())       # nothing of the poison is left: -7777 and NaN are no answers
    _same(call(0x00), first)
    _same(call(0xFF), first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # both exports of every shard, and the maximum between them
        call.launch()
    for word in (0x5A, 0x00):
        call.poison(word)
        graph.replay()
        torch.cuda.synchronize()
        _same(call.result(), first)


# -------------------------------------------------------------------------------------------------------- surface ----
def test_item_index_methods_take_the_searches_checks_and_padding(mf):
    g = torch.Generator().manual_seed(3)
    q, items = _unit(6, 48, g), _unit(700, 48, g)             # dim 48: padded to 64 by ItemIndex
    rng = np.random.default_rng(3)
    excl = [sorted(set(rng.integers(0, 700, 30).tolist())) for _ in range(6)]
    t_off, t_ids = np.arange(0, 6 * 25 + 1, 25), rng.integers(-2, 702, 150)
    pad = lambda x: torch.nn.functional.pad(x, (0, 16)).numpy()   # noqa: E731
    want = spec.positions(pad(q), pad(items), t_off, t_ids, excl)
    csr = (_dev(t_off, torch.int64), _dev(t_ids, torch.int64))
    layout = sspec.round_robin(700, 3)
    shards = [mf.retrieval.ItemIndex(items[torch.from_numpy(sspec.rows_of(sh))].to(DEV)) for sh in layout]
    words = torch.stack([ix.target_words(q.to(DEV), csr, stride=sh[0], offset=sh[1]) for ix, sh in zip(shards, layout)])
    assert words.dtype == torch.int64 and words.shape == (3, 150) and int((words != 0).sum(dim=0).max()) == 1
    wmax = words.max(dim=0).values
    parts = [ix.key_positions(q.to(DEV), csr, wmax, stride=sh[0], offset=sh[1],
                              exclude_local_csr=mf.retrieval._csr([[sspec.local_row(y, sh) for y in ex] for ex in excl], 6, DEV))
             for ix, sh in zip(shards, layout)]
    _same(sspec.combine([tuple(t.cpu().numpy() for t in p) for p in parts]), want)
    assert ("positions", 6) in shards[0]._ws                  # the workspace is kept, and shared with positions()
    whole = mf.retrieval.ItemIndex(items.to(DEV))             # stride 1, offset 0, no lists: the unsharded call
    one = whole.key_positions(q.to(DEV), csr, whole.target_words(q.to(DEV), csr))
    assert all(torch.equal(a, b) for a, b in zip(one, whole.positions(q.to(DEV), csr)))
    ix, (stride, offset, _) = shards[1], layout[1]
    none = (torch.zeros(7, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert ix.target_words(q.to(DEV), none, stride=stride, offset=offset).numel() == 0
    empty = ix.key_positions(q.to(DEV), none, torch.zeros(0, dtype=torch.int64, device=DEV), stride=stride, offset=offset)
    assert empty[0].numel() == 0 and empty[1].numel() == 0 and empty[2].tolist() == [layout[1][2]] * 6
    with pytest.raises(ValueError, match="queries should be"):
        ix.target_words(torch.zeros(6, 64, device=DEV), csr)
    with pytest.raises(ValueError, match="queries should be"):
        ix.key_positions(torch.zeros(6, 64, device=DEV), csr, wmax)
    with pytest.raises(ValueError, match="one target list per query"):
        ix.target_words(q[:5].to(DEV), csr)
    with pytest.raises(ValueError, match="one target list per query"):
        ix.key_positions(q[:5].to(DEV), csr, wmax)
    with pytest.raises(ValueError, match="one word per target entry"):
        ix.key_positions(q.to(DEV), csr, wmax[:-1])
    for bad in (dict(stride=0), dict(offset=-1)):
        with pytest.raises(ValueError, match="stride >= 1 and offset >= 0"):
            ix.target_words(q.to(DEV), csr, **bad)
        with pytest.raises(ValueError, match="stride >= 1 and offset >= 0"):
            ix.key_positions(q.to(DEV), csr, wmax, **bad)
    with pytest.raises(mf.MfHipError, match="no CPU path"):
        ix.target_words(q, csr)
    with pytest.raises(mf.MfHipError, match="no CPU path"):
        ix.key_positions(q, csr, wmax)


# -------------------------------------------------------------------------------------------------------- world 2 ----
def _gpu_positions_case(rank: int, world: int, out_dir: str) -> None:
    mf = importlib.import_module("matrix-factorization-torch_amd")
    mfd = mf.distributed
    items, q, excl, lists, _ = tsc._case_inputs(rank)
    (e_off, e_ids), (t_off, t_ids) = tsc._csr(excl), tsc._csr(lists)
    index = mfd.ShardedIndex(items[rank::world].contiguous().to(DEV), rank, tdc.N_ITEMS, stride=world, comm=tgd._relay_comm(mfd))
    assert isinstance(index.ops, mfd.HipOps)
    exact = index.positions(q.to(DEV), (t_off.to(DEV), t_ids.to(DEV)), exclude_csr=(e_off.to(DEV), e_ids.to(DEV)))
    capped = index.positions(q.to(DEV), (t_off.to(DEV), t_ids.to(DEV)), exclude_csr=(e_off.to(DEV), e_ids.to(DEV)), exclude_capacity=40,
                             target_capacity=40)
    torch.cuda.synchronize()
    torch.save({"exact": tuple(t.cpu() for t in exact), "capped": tuple(t.cpu() for t in capped)}, f"{out_dir}/gpos_{rank}.pt")


def _worker(rank: int, world: int, port: int, fn: str, out_dir: str) -> None:
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        globals()[fn](rank, world, out_dir)
    finally:
        dist.destroy_process_group()


def test_sharded_index_positions_world_2_with_hip_kernels(tmp_path):
    """Two ranks sharing one card, the catalog dealt round-robin, target and exclusion lists gathered at exact lengths and in
    capacity-padded blocks: the whole catalog's positions, counts and score bits."""
    import torch.multiprocessing as mp

    mp.spawn(_worker, args=(2, tdc._free_port(), "_gpu_positions_case", str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        items, q, excl, lists, _ = tsc._case_inputs(r)
        off, ids = (t.numpy() for t in tsc._csr(lists))
        want = spec.positions(q.numpy(), items.numpy(), off, ids, excl)
        assert (want[0] == -1).any() and (want[0] >= 0).sum() > 20
        got = torch.load(f"{tmp_path}/gpos_{r}.pt")
        for mode in ("exact", "capped"):
            _same(tuple(t.numpy() for t in got[mode]), want, (r, mode))
