"""CPU: the host side of the position path -- ``mf_target_positions`` (csrc/mf_topk_deep.hip) and ``mf_position_metrics``
(csrc/mf_topk.hip): exports, workspace sizes, every refusal (all decided before any launch, so never-dereferenced fake pointers
do), the new kernels' resources, the numpy spec (tests/_position_spec.py) against itself and against the list oracle, and the
module's two config fields."""
from __future__ import annotations

import ctypes
import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import retrieval as oretr
from tests import _position_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
BIG = ctypes.c_size_t(2**40)
EXPORTS = ("mf_target_positions_ws_bytes", "mf_target_positions_min_ws_bytes", "mf_target_positions", "mf_position_metrics")


def test_exports_are_declared_bound_and_present(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    for name in EXPORTS:
        assert hasattr(lib, name) and name in mf._lib.SIGNATURES and name + "(" in header, name


def test_workspace_is_the_deep_engines(mf):
    lib = mf._lib.lib()
    for q in (1, 31, 32, 33, 1024, 65_536):
        for n in (1, 31, 33, 62_423, 8_400_000):
            for d in (32, 64, 128, 256):
                pref, low = lib.mf_target_positions_ws_bytes(q, n, d), lib.mf_target_positions_min_ws_bytes(q, n, d)
                assert pref >= low > 0 and low == 32 * (-(-n // 32) * 32) * 4, (q, n, d, pref, low)
                for k in (1, 100, 1024):                      # k is out of the picture
                    assert pref == lib.mf_topk_deep_ws_bytes(q, n, d, k) and low == lib.mf_topk_deep_min_ws_bytes(q, n, d, k), (q, n, d, k)
    for q, n, d in ((0, 10, 64), (-1, 10, 64), (4, 0, 64), (4, 10, 48), (4, 1 << 31, 64), (4, 40_000_000, 64)):
        assert lib.mf_target_positions_ws_bytes(q, n, d) == 0 and lib.mf_target_positions_min_ws_bytes(q, n, d) == 0, (q, n, d)


@pytest.fixture
def call(mf):
    lib = mf._lib.lib()

    def run(q=FAKE, Q=4, items=FAKE, N=1000, d=64, to=FAKE, ti=FAKE, nt=10, eo=None, ei=None, base=0, ws=FAKE, wsb=BIG, op=FAKE, os_=FAKE,
            oc=FAKE):
        rc = lib.mf_target_positions(q, Q, items, N, d, to, ti, nt, eo, ei, base, ws, wsb, op, os_, oc, None)
        return rc, (lib.mf_last_error() if rc else b"")

    return run


@pytest.mark.parametrize("kw", [dict(q=None), dict(items=None), dict(to=None), dict(ti=None), dict(ws=None), dict(op=None), dict(os_=None),
                                dict(oc=None), dict(Q=0), dict(Q=-3), dict(N=0), dict(N=-1), dict(nt=-1)], ids=str)
def test_positions_refuses_bad_arguments(mf, call, kw):
    rc, msg = call(**kw)
    assert rc == mf._lib.MF_EINVAL and msg.startswith(b"mf_target_positions: bad argument"), (kw, rc, msg)


@pytest.mark.parametrize("kw,code,text", [
    (dict(d=48), "MF_EINVAL", b"mf_target_positions: embedding width 48 not in {32,64,128,256}"),
    (dict(d=16), "MF_EINVAL", b"mf_target_positions: embedding width 16 not in {32,64,128,256}"),
    (dict(eo=FAKE), "MF_EINVAL", b"mf_target_positions: excl_off/excl_idx mismatch"),
    (dict(ei=FAKE), "MF_EINVAL", b"mf_target_positions: excl_off/excl_idx mismatch"),
    (dict(N=1 << 31), "MF_ENOTSUP", b"mf_target_positions: item indices must fit 32 bits"),
    (dict(base=-1), "MF_ENOTSUP", b"mf_target_positions: item indices must fit 32 bits"),
    (dict(N=1000, base=(1 << 32) - 999), "MF_ENOTSUP", b"mf_target_positions: item indices must fit 32 bits"),
    (dict(N=40_000_000), "MF_ENOTSUP", b"mf_target_positions: a 32-query score slab of 40000000 columns exceeds the descriptor limit"),
    (dict(wsb=ctypes.c_size_t(0)), "MF_ENOSPC", b"mf_target_positions: workspace too small"),
], ids=lambda x: str(x) if isinstance(x, dict) else None)
def test_positions_refusals_have_the_searches_codes(mf, call, kw, code, text):
    rc, msg = call(**kw)
    assert rc == getattr(mf._lib, code) and msg.startswith(text), (kw, rc, msg)


def test_positions_refusal_order_and_the_workspace_floor(mf, call):
    E, lib = mf._lib, mf._lib.lib()
    low = lib.mf_target_positions_min_ws_bytes(4, 1000, 64)
    rc, msg = call(wsb=ctypes.c_size_t(low - 1))
    assert rc == E.MF_ENOSPC and msg.startswith(b"mf_target_positions: workspace too small")
    # pointers and sizes, width, 32-bit rows, the exclusion pair, geometry, workspace: the searches' order
    for kw, code, text in ((dict(q=None, d=48), E.MF_EINVAL, b"bad argument"), (dict(nt=-1, N=1 << 31), E.MF_EINVAL, b"bad argument"),
                           (dict(d=48, N=1 << 31), E.MF_EINVAL, b"embedding width 48"), (dict(base=-1, eo=FAKE), E.MF_ENOTSUP, b"must fit 32 bits"),
                           (dict(eo=FAKE, wsb=ctypes.c_size_t(0)), E.MF_EINVAL, b"excl_off/excl_idx mismatch"),
                           (dict(N=40_000_000, wsb=ctypes.c_size_t(0)), E.MF_ENOTSUP, b"descriptor limit")):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (kw, rc, msg)


def test_position_metrics_refusals(mf):
    lib, E = mf._lib.lib(), mf._lib

    def run(pos=FAKE, off=FAKE, rel=FAKE, nc=FAKE, Q=4, ks=(20,), nk=None, out=FAKE):
        arr = (ctypes.c_int32 * max(len(ks), 1))(*ks) if ks is not None else None
        rc = lib.mf_position_metrics(pos, off, rel, nc, Q, arr, len(ks) if nk is None else nk, out, None)
        return rc, (lib.mf_last_error() if rc else b"")

    for kw in (dict(pos=None), dict(off=None), dict(rel=None), dict(nc=None), dict(out=None), dict(ks=None, nk=1), dict(Q=0), dict(Q=-1)):
        rc, msg = run(**kw)
        assert rc == E.MF_EINVAL and msg.startswith(b"mf_position_metrics: bad argument"), (kw, rc, msg)
    for nk in (0, -1, 9):
        rc, msg = run(ks=(1,) * 9, nk=nk)
        assert rc == E.MF_ENOTSUP and msg.startswith(b"mf_position_metrics: %d cut-offs outside 1..8" % nk), (nk, rc, msg)
    for ks in ((0,), (20, -3), (1, 2, 3, 4, 5, 6, 7, 0)):
        rc, msg = run(ks=ks)
        assert rc == E.MF_EINVAL and msg.startswith(b"mf_position_metrics: k = "), (ks, rc, msg)


def test_new_kernels_have_no_spill_and_no_scratch():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    mine = {n: r for n, r in kr.kernel_resources().items() if "target_positions_kernel" in n or "position_metrics_kernel" in n}
    assert len(mine) == 2, sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 64 * 1024, (name, r)


# ------------------------------------------------------------------------------------------------- the spec itself ----
def _world(seed=0, nq=6, n=300):
    """Random fp32 scores with planted ties, exclusion lists, and target lists whose entries are all admissible."""
    rng = np.random.default_rng(seed)
    scores = rng.standard_normal((nq, n)).astype(np.float32)
    scores[:, 40:60] = scores[:, 40:41]                      # a run of equal scores: the row decides
    excl = [sorted(rng.choice(n, size=int(rng.integers(0, 40)), replace=False).tolist()) for _ in range(nq)]
    excl[2] = [y for y in range(n) if y % 29]                # 11 admissible rows: fewer than k
    targets = []
    for r in range(nq):
        free = np.setdiff1d(np.arange(n), excl[r])
        own = rng.choice(free, size=min(free.size, int(rng.integers(1, 25))), replace=False)
        targets.append(dict(zip(own.tolist(), rng.integers(0, 6, own.size).astype(float).tolist())))
    targets[4] = {}
    return scores, excl, targets


def _csr(targets):
    off = np.cumsum([0] + [len(t) for t in targets])
    return off, np.array([y for t in targets for y in t], dtype=np.int64), np.array([v for t in targets for v in t.values()], dtype=np.float64)


@pytest.mark.parametrize("k", [1, 5, 20, 100, 5000])
def test_spec_metrics_equal_the_list_oracle_when_every_target_is_admissible(k):
    scores, excl, targets = _world()
    off, ids, rel = _csr(targets)
    pos, sc, ncand = spec.positions_from_scores(scores, off, ids, excl)
    assert (pos >= 0).all() and np.array_equal(ncand, [scores.shape[1] - len(e) for e in excl])
    topk = np.full((len(targets), k), -1, dtype=np.int64)
    for r, order in enumerate(spec.orders(scores, excl)):
        topk[r, : min(k, order.size)] = order[:k]
    want = oretr.retrieval_metrics(topk, targets, k)
    got = spec.metrics(pos, off, rel, ncand, (k,))
    assert np.abs(got[:, :6] - want).max() <= 1e-12
    several = spec.metrics(pos, off, rel, ncand, (3, k, 7))
    assert np.array_equal(several[:, 6:12], got[:, :6]) and np.array_equal(several[:, 18:], got[:, 6:])


def test_spec_positions_are_the_places_in_the_order():
    scores, excl, targets = _world(seed=1)
    off, ids, _ = _csr(targets)
    pos, sc, _ = spec.positions_from_scores(scores, off, ids, excl, idx_base=0)
    for r, order in enumerate(spec.orders(scores, excl)):
        k = spec.keys(scores[r])[order]
        assert (k[:-1] > k[1:]).all()                        # a total order: keys are unique
        for e in range(off[r], off[r + 1]):
            assert order[pos[e]] == ids[e] and sc[e] == scores[r, ids[e]]
    tied = spec.orders(scores, None)[0]
    run = [y for y in tied.tolist() if 40 <= y < 60]
    assert run == list(range(40, 60))                        # equal scores: ascending rows
    # global rows: the same places behind an idx_base, and rows outside [base, base + N) are not admissible
    p7, _, _ = spec.positions_from_scores(scores, off, ids + 7, [[y + 7 for y in e] for e in excl], idx_base=7)
    assert np.array_equal(p7, pos)
    p0, s0, _ = spec.positions_from_scores(scores, [0, 2, 2, 2, 2, 2, 2], [6, 7 + scores.shape[1]], None, idx_base=7)
    assert p0.tolist() == [-1, -1] and np.isneginf(s0).all()


def test_spec_hand_worked_rows():
    log2 = np.log2
    # five queries over a catalog of 10 admissible rows (ncand = 10 but for the last)
    cases = [
        ([0], [3.0]),                                        # one target at position 0
        ([4, 5], [2.0, 1.0]),                                # two targets with tied scores: neighbours, the lower row first
        ([1, 6], [0.0, 4.0]),                                # a rating-0 target above a relevant one
        ([2, -1], [1.0, 5.0]),                               # an inadmissible target: counts in recall's and IDCG's denominators
        ([], []),                                            # an empty list
    ]
    off = np.cumsum([0] + [len(p) for p, _ in cases])
    pos = np.array([x for p, _ in cases for x in p], dtype=np.int64)
    rel = np.array([x for _, r in cases for x in r])
    got = spec.metrics(pos, off, rel, [10, 10, 10, 10, 3], (5,))
    want = np.zeros((5, 9))
    want[0] = [1, 1, 1 / 5, 1, 1, 1, 1, 0, 1]
    ideal = 2 / log2(2) + 1 / log2(3)
    want[1] = [(2 / log2(6)) / ideal, 1 / 2, 1 / 5, 1 / 5, 1, 1 / 5, 1 / 5, 4.5, 1 - (4 + 4) / (2 * 8)]
    want[2] = [0, 0, 0, 0, 0, 0, 1 / 7, 6, 1 - 6 / 9]
    want[3] = [(1 / log2(4)) / (5 / log2(2) + 1 / log2(3)), 1 / 2, 1 / 5, 1 / 3, 1, 1 / 3, 1 / 3, 2, 1 - 2 / 9]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    at10 = spec.metrics(pos, off, rel, [10, 10, 10, 10, 3], (10,))
    np.testing.assert_allclose(at10[1, :6], [(2 / log2(6) + 1 / log2(7)) / ideal, 1, 2 / 10, (1 / 5 + 2 / 6) / 2, 1, 1 / 5], rtol=0, atol=1e-15)
    np.testing.assert_allclose(at10[2, :6], [(4 / log2(8)) / (4 / log2(2)), 1, 1 / 10, 1 / 7, 1, 1 / 7], rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------------ the surface ----
def test_position_metrics_names(mf):
    r = mf.retrieval
    one = r.PositionMetrics(top_k=20, prefix="val/")
    assert one.ks == (20,) and one.top_k == 20
    assert list(one.compute()) == ["val/" + n for n in r.METRIC_NAMES] + ["val/MRR", "val/MeanPosition", "val/AUC"]
    many = r.PositionMetrics((20, 100, 5000))
    assert list(many.compute()) == (list(r.METRIC_NAMES) + [f"{n}@100" for n in r.METRIC_NAMES] + [f"{n}@5000" for n in r.METRIC_NAMES]
                                    + ["MRR", "MeanPosition", "AUC"])
    assert tuple(spec.NAMES) == tuple(r.METRIC_NAMES) and tuple(spec.UNCUT) == tuple(r.POSITION_METRIC_NAMES)
    for bad in ((), (0,), (20, 20), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="cut-offs"):
            r.PositionMetrics(bad)


def test_config_fields(mf):
    cfg_cls = mf.lightning.MatrixFactorizationLitConfig
    base = {"num_users": 10, "num_items": 20}
    cfg = cfg_cls.model_validate(base)
    assert cfg.metrics_mode == "topk" and cfg.eval_ks is None
    with pytest.raises(ValueError, match="metrics_mode"):
        cfg_cls.model_validate({**base, "metrics_mode": "lists"})
    cfg = cfg_cls.model_validate({**base, "metrics_mode": "positions", "eval_ks": [100, 5000], "top_k": 20})
    dumped = cfg.model_dump()
    assert dumped["metrics_mode"] == "positions" and dumped["eval_ks"] == [100, 5000]
    assert cfg_cls.model_validate(dumped) == cfg
    module = mf.lightning.MatrixFactorizationLitModule(dumped)
    metrics = module.get_metrics()
    assert set(metrics) == {"val", "test"} and all(isinstance(m, mf.retrieval.PositionMetrics) for m in metrics.values())
    assert metrics["val"].ks == (20, 100, 5000) and metrics["val"].prefix == "val/"
    default = mf.lightning.MatrixFactorizationLitModule(base).get_metrics()
    assert all(type(m) is mf.retrieval.RetrievalMetrics and m.top_k == cfg_cls.model_validate(base).top_k for m in default.values())
