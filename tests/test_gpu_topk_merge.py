"""GPU: the sharded index's exchange format (``mf_topk_pack`` + ``mf_topk_merge_packed``) against ``mf_topk_merge`` and the
oracle's merge, and the metrics kernel on both sides of k = 64.  Scores are compared as uint32 views and rows as integers:
equal, never close."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import retrieval as oretr

from tests import _metrics_seam_cases as seam
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = 5


def _parts(G, k, layout):
    """Per-shard results ``[G, Q, k]``, each ordered (score descending, row ascending) with a -inf / -1 tail, and the
    shards' (stride, offset).  Query 0 is full in every shard, 1 empty in every shard, 2 draws its scores from four values
    (-0.0 among them) so that shards tie, 3 from three (0.0 among them; the oracle's order holds -0.0 and 0.0 equal, the
    keys do not, so no query has both), the rest are normal with random fill."""
    g = np.random.default_rng(100 * G + k)
    n_local = 4 * k + 7
    scores = np.full((G, Q, k), -np.inf, np.float32)
    local = np.full((G, Q, k), -1, np.int64)
    for sh in range(G):
        for q in range(Q):
            m = k if q == 0 else 0 if q == 1 else int(g.integers(0, k + 1))
            r = np.sort(g.choice(n_local, m, replace=False))
            if q == 2:
                s = g.choice(np.array([-1.5, -0.0, 0.25, 3.0], np.float32), m)
            elif q == 3:
                s = g.choice(np.array([-2.0, 0.0, 1.0], np.float32), m)
            else:
                s = g.standard_normal(m).astype(np.float32)
            order = np.lexsort((r, -s.astype(np.float64)))
            scores[sh, q, :m], local[sh, q, :m] = s[order], r[order]
    where = [(G, sh) if layout == "interleaved" else (1, sh * n_local) for sh in range(G)]
    return scores, local, where


@pytest.mark.parametrize("layout", ["interleaved", "contiguous"])
@pytest.mark.parametrize(("G", "k"), [(1, 1), (1, 20), (1, 64), (3, 1), (3, 20), (3, 64), (128, 64)])    # (128, 64): 64 KiB of keys, the most
def test_pack_and_merge_packed_match_merge_and_oracle(mf, G, k, layout):
    lib, L = mf._lib.lib(), mf._lib
    scores, local, where = _parts(G, k, layout)
    glob = np.stack([np.where(local[sh] >= 0, local[sh] * st + o, -1) for sh, (st, o) in enumerate(where)])
    want_s, want_i = oretr.merge_topk(scores, glob, k)
    assert (want_i[1] == -1).all() and (want_i[0] >= 0).all()

    ds, dl = torch.from_numpy(scores).to(DEV), torch.from_numpy(local).to(DEV)
    packed = torch.empty(G, Q, k, dtype=torch.int64, device=DEV)
    for sh, (st, o) in enumerate(where):
        L.check(lib.mf_topk_pack(ds[sh].data_ptr(), dl[sh].data_ptr(), Q * k, st, o, packed[sh].data_ptr(), L.stream_ptr()))
    bits = (scores.view(np.uint32).astype(np.uint64) << np.uint64(32)) | glob.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    assert np.array_equal(packed.cpu().numpy(), np.where(glob >= 0, bits.view(np.int64), -1))

    def same(got, what):
        gs, gi = (x.cpu().numpy() for x in got)
        assert np.array_equal(gi, want_i), what
        assert np.array_equal(gs.view(np.uint32), want_s.view(np.uint32)), what

    out = torch.empty(Q, k, device=DEV), torch.empty(Q, k, dtype=torch.int64, device=DEV)
    L.check(lib.mf_topk_merge_packed(packed.data_ptr(), G, Q, k, out[0].data_ptr(), out[1].data_ptr(), L.stream_ptr()))
    same(out, "mf_topk_merge_packed")
    same(mf.retrieval.merge_topk(ds, torch.from_numpy(glob).to(DEV), k), "mf_topk_merge")


@pytest.fixture(scope="module")
def seam_golden():
    return np.load(GOLDEN / "retrieval_metrics_seam.npz")


@pytest.mark.parametrize("k", seam.KS)
def test_metrics_on_both_sides_of_64(mf, seam_golden, k):
    topk, off, ids, rel, targets = seam.seam_case(k)
    if k in (65, 128):                                        # the missed targets of query 2 take ranks 60 .. min(69, k - 1)
        assert (topk[2] >= 0).sum() == 60 and sum(i not in set(topk[2].tolist()) for i in targets[2]) == 10
    got = mf.retrieval.RetrievalMetrics(top_k=k).update(*(torch.from_numpy(x).to(DEV) for x in (topk, off, ids, rel))).cpu().numpy()
    want = oretr.retrieval_metrics(topk, targets, k)
    print(f"k = {k}: largest |got - want| = {np.abs(got - want).max():.3g}")
    assert not got[0].any() and want[3, 1] == 1.0
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    if k in seam.GOLDEN_KS:                                   # one rank per lane: the bits of the kernel that held only that case
        assert np.array_equal(got.view(np.uint32), seam_golden[f"k{k}"].view(np.uint32))
