"""GPU: the bf16 retrieval prefilter (csrc/mf_topk_bf3.hip, ``ItemIndex.search(path="bf16")`` and what "auto" picks for almost
every batched call) at the plan geometries its first tests never met: several query workgroups, workgroups that own several
blocks (the LDS ring wraps from the third), catalogs beyond one window of the exclusion-word prep, the sampled seed bound with
exclusion lists, all twelve (d, XT, lists) instantiations of the scans.  The cases and their data are tests/_bf3_cases.py;
every case asserts its cell through ``mf_topk_bf3_plan`` before it searches.  Per case: all queries against the fp32 tile
engine on the same index and against "auto", a sample (or all) of them against the CPU oracle -- rows as integers, scores as
bit patterns: equal, never close."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import chain
from tests import _bf3_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8                # result rows in front of and behind the Q real ones: they keep their fill
FILL_S, FILL_I = 7.0, -7


def _bits(s):
    return np.ascontiguousarray(s.cpu().numpy() if isinstance(s, torch.Tensor) else s).view(np.uint32)


def _same(got, want, what, queries=None):
    """Rows and score bits equal; a failure names the first queries that differ."""
    (gs, gi), (ws, wi) = got, want
    gi, wi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (gi, wi))
    bad = np.flatnonzero((gi != wi).any(axis=1) | (_bits(gs) != _bits(ws)).any(axis=1))
    names = bad if queries is None else np.asarray(queries)[bad]
    assert bad.size == 0, (what, f"{bad.size} queries differ, first: {names[:8].tolist()}",
                           gi[bad[0]].tolist(), wi[bad[0]].tolist())


def _bf3_guarded(mf, index, q, k, off, ids):
    """mf_topk_bf3 through the C ABI on result buffers with GUARD filled rows on either side of the Q real ones."""
    lib = mf._lib.lib()
    nq, (n, d) = q.shape[0], index.embeddings.shape
    s = torch.full((nq + 2 * GUARD, k), FILL_S, device=DEV)
    i = torch.full((nq + 2 * GUARD, k), FILL_I, dtype=torch.int64, device=DEV)
    ws = mf._lib.workspace(lib.mf_topk_bf3_ws_bytes(nq, n, d, k), DEV)
    mf._lib.check(lib.mf_topk_bf3(q.data_ptr(), nq, index.embeddings.data_ptr(), index.bf16_index().data_ptr(), n, d, k,
                                  mf._lib.ptr(off), mf._lib.ptr(ids), index.idx_base, ws.data_ptr(), ws.numel(),
                                  s[GUARD:].data_ptr(), i[GUARD:].data_ptr(), mf._lib.stream_ptr()))
    torch.cuda.synchronize()
    for part in (slice(0, GUARD), slice(nq + GUARD, None)):
        assert bool((s[part] == FILL_S).all()) and bool((i[part] == FILL_I).all()), "written outside the Q result rows"
    return s[GUARD: nq + GUARD], i[GUARD: nq + GUARD]


def _check(mf, name, case, sample_all=False):
    lib = mf._lib.lib()
    p = bc.plan(lib, case.nq, case.n, case.d)
    bc.check_cell(case, p)                                               # the cell first: then the search
    data = bc.build(name, case, p)
    q = data.q.to(DEV).contiguous()
    index = mf.retrieval.ItemIndex(data.items.to(DEV), idx_base=case.idx_base)
    off, ids = mf.retrieval._csr(data.excl, case.nq, DEV)
    csr = None if data.excl is None else (off, ids)
    tiles = index.search(q, case.k, exclude_csr=csr, path="tiles")
    got = _bf3_guarded(mf, index, q, case.k, off, ids)
    _same(got, tiles, "bf16 against the fp32 tile engine")
    engines = []
    run = index._run
    index._run = lambda engine, *a, **kw: (engines.append(engine), run(engine, *a, **kw))[1]
    auto = index.search(q, case.k, exclude_csr=csr)
    assert engines == ["bf16"], engines                                  # what "auto" picks, and it was not refused
    _same(auto, got, "auto against bf16")
    sel = list(range(case.nq)) if sample_all else bc.oracle_sample(case, p, data.special)
    assert set(data.special.values()) <= set(sel) and (sample_all or len(sel) <= 32)
    ws, wi = chain.topk(data.q[sel].numpy(), data.items.numpy(), case.k, data.local_lists(case, sel))
    want = (ws, np.where(wi >= 0, wi + case.idx_base, -1))
    pick = torch.tensor(sel, device=DEV)
    _same((got[0][pick], got[1][pick]), want, "bf16 against the CPU oracle", sel)
    _same((tiles[0][pick], tiles[1][pick]), want, "the tile engine against the CPU oracle", sel)
    return data, got


@pytest.mark.parametrize("inst", bc.INSTANTIATIONS, ids=lambda c: f"d{c[0]}-Q{c[1]}-{'lists' if c[2] else 'nolists'}")
def test_all_instantiations(mf, inst):
    """The twelve (d, XT, exclusion lists) instantiations of the two scan kernels on a catalog of 18 blocks; three of them
    -- (64, 4, no lists), (128, 4, lists), (256, 2, no lists) -- no other test launches.  The oracle answers every query."""
    d, nq, lists = inst
    _check(mf, f"all_instantiations_{d}_{nq}_{int(lists)}", bc.instantiation(d, nq, lists), sample_all=True)


@pytest.mark.parametrize("name", [n for n in bc.CASES if n != "seams"])
def test_plan_cell(mf, name):
    _check(mf, name, bc.CASES[name])


def test_seams(mf):
    """Three blocks per workgroup of the full scan (the ring wraps), two per seed workgroup, two prep windows, XT = 4 with lists
    at d = 128, and planted rows at every seam (tests/_bf3_cases.py; test_topk_bf3_plan_cpu.py shows by the oracle alone that
    they sit where they should)."""
    case = bc.CASES["seams"]
    data, (s, i) = _check(mf, "seams", case)
    rows = i.cpu().numpy()
    for x in range(case.nq):                                            # no excluded row anywhere, whatever the reference says
        assert not set(rows[x].tolist()) & set(data.excl[x]), x
    seam = bc.WINDOW_ROWS
    assert seam - 1 not in rows[2] and seam not in rows[2] and {seam - 2, seam + 1} <= set(rows[2].tolist())
    assert case.n - 1 not in rows[3] and rows[3][0] == case.n - 2
