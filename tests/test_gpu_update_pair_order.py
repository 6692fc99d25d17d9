"""GPU: the two-table update launch whichever list is longer, and long runs laid out by hand, bit for bit.

1. Order: ``mf_update_pair`` / ``mf_update_pair_adagrad`` hand the longer list to the kernel first.  For A longer, B longer
   and the tie: tables and optimiser state ``torch.equal`` to the two single-table calls, no other row touched.
2. One bucket laid out by hand -- a run of seven chunks on the all-pairs path; a run of 500 followed by a run of 70 whose
   head is not on a multiple of 32 (two parked chunks in one 32-block) on the bitonic path; one run of 1025 (P = 2048); a
   run of 8000 in a bucket of 8192 -- with integer gradients against the int64 reference of tests/_update_cases.py, exact.
3. The loops that keep gradient rows in flight: runs of a first chunk of 32 - r rows, x whole chunks (x of LADDER_X) and a last
   chunk of 16 a + b rows, (a, b) in (1, -1), (1, 0), (1, 1), (2, 1), heads at residues r = 0, 1, 31, beside single-chunk runs
   of 11 .. 17 rows: Adam against the list of unique ids with the exact sums, as tests/test_gpu_update.py does.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _update_cases as uc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, WD, B1, B2, EPS = 0.05, 0.01, 0.9, 0.999, 1e-8
AG_EPS = 1e-10
KINDS = ("sgd", "adam", "adagrad")


def _ws(mf, n, d):
    return torch.full((max(int(mf._lib.lib().mf_update_ws_bytes(n, d)), 256),), 0xFF, dtype=torch.uint8, device=DEV)


def _state(w0):
    """[table, exp_avg (Adagrad: its first column is not used; `sum` is state[3]), exp_avg_sq, sum]"""
    return [w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0), torch.zeros(w0.shape[0], device=w0.device)]


def _single(mf, kind, st, idx, grad, normalized, ws, step=1, lr=LR, wd=WD):
    lib = mf._lib.lib()
    t, m, v, s = st
    rows, d = t.shape
    if kind == "adam":
        rc = lib.mf_update_adam(t.data_ptr(), m.data_ptr(), v.data_ptr(), rows, d, idx.data_ptr(), idx.numel(), grad.data_ptr(), normalized,
                                step, None, lr, B1, B2, EPS, wd, ws.data_ptr(), ws.numel(), None)
    elif kind == "sgd":
        rc = lib.mf_update_sgd(t.data_ptr(), rows, d, idx.data_ptr(), idx.numel(), grad.data_ptr(), normalized, lr, wd, ws.data_ptr(),
                               ws.numel(), None)
    else:
        rc = lib.mf_update_adagrad(t.data_ptr(), s.data_ptr(), rows, d, idx.data_ptr(), idx.numel(), grad.data_ptr(), normalized, lr, AG_EPS,
                                   wd, ws.data_ptr(), ws.numel(), None)
    mf._lib.check(rc)
    torch.cuda.synchronize()


def _pair(mf, kind, sa, ia, ga, norm_a, wsa, sb, ib, gb, norm_b, wsb, step=1):
    lib = mf._lib.lib()
    d = sa[0].shape[1]
    if kind == "adagrad":
        rc = lib.mf_update_pair_adagrad(d, sa[0].data_ptr(), sa[3].data_ptr(), sa[0].shape[0], ia.data_ptr(), ia.numel(), ga.data_ptr(), norm_a,
                                        wsa.data_ptr(), wsa.numel(), sb[0].data_ptr(), sb[3].data_ptr(), sb[0].shape[0], ib.data_ptr(),
                                        ib.numel(), gb.data_ptr(), norm_b, wsb.data_ptr(), wsb.numel(), LR, AG_EPS, WD, None)
    else:
        adam = kind == "adam"
        p = (lambda x: x.data_ptr()) if adam else (lambda x: None)
        rc = lib.mf_update_pair(int(adam), d, sa[0].data_ptr(), p(sa[1]), p(sa[2]), sa[0].shape[0], ia.data_ptr(), ia.numel(), ga.data_ptr(),
                                norm_a, wsa.data_ptr(), wsa.numel(), sb[0].data_ptr(), p(sb[1]), p(sb[2]), sb[0].shape[0], ib.data_ptr(),
                                ib.numel(), gb.data_ptr(), norm_b, wsb.data_ptr(), wsb.numel(), step, None, LR, B1, B2, EPS, WD, None)
    mf._lib.check(rc)
    torch.cuda.synchronize()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. order ----
ROWS_A, ROWS_B = 3000, 5000


def _order_inputs(n, rows, d, gen):
    idx = torch.randint(0, rows, (n,), generator=gen, device=DEV)
    if n > 100:
        idx[:100] = 7                                              # a run longer than a chunk
    grads = [torch.randn(n, d, generator=gen, device=DEV) for _ in range(2)]
    return idx, grads, torch.randn(rows, d, generator=gen, device=DEV)


@pytest.mark.parametrize("d", (32, 128))
@pytest.mark.parametrize("n_a,n_b", ((20, 8193), (8193, 20), (64, 64), (33, 32)))
def test_pair_equals_two_single_calls_whichever_list_is_longer(mf, n_a, n_b, d):
    gen = torch.Generator(device=DEV).manual_seed(1000 * n_a + n_b + d)
    ia, ga, wa0 = _order_inputs(n_a, ROWS_A, d, gen)
    ib, gb, wb0 = _order_inputs(n_b, ROWS_B, d, gen)
    wsa, wsb = _ws(mf, n_a, d), _ws(mf, n_b, d)
    for kind in KINDS:
        single_a, single_b, pa, pb = _state(wa0), _state(wb0), _state(wa0), _state(wb0)
        for step in (1, 2):                                          # (A normalised, B not)
            _single(mf, kind, single_a, ia, ga[step - 1], 1, wsa, step=step)
            _single(mf, kind, single_b, ib, gb[step - 1], 0, wsb, step=step)
            _pair(mf, kind, pa, ia, ga[step - 1], 1, wsa, pb, ib, gb[step - 1], 0, wsb, step=step)
            for which, both, single in (("A", pa, single_a), ("B", pb, single_b)):
                for name, x, y in zip(("table", "exp_avg", "exp_avg_sq", "sum"), both, single):
                    assert _same_bits(x, y), (kind, step, which, name, "the pair differs from the single call")
        for both, w0, idx in ((pa, wa0, ia), (pb, wb0, ib)):
            untouched = torch.ones(w0.shape[0], dtype=torch.bool, device=DEV)
            untouched[idx] = False
            assert _same_bits(both[0][untouched], w0[untouched]), (kind, "a row outside the ids was written")
            assert not bool(both[1][untouched].any()) and not bool(both[2][untouched].any()) and not bool(both[3][untouched].any())
            assert not _same_bits(both[0][~untouched], w0[~untouched])


# ------------------------------------------------------------------------------------- 2. hand-made buckets ----
# name -> run lengths of one bucket, in sorted order
LAYOUTS = {
    "m300-run200": [200, 25, 25, 25, 25],                           # all-pairs path, a run of seven chunks
    "m600-run500-then70": [500, 70] + [1] * 30,                     # bitonic 1024; the chunks at 480 and 500 share a 32-block
    "m1025-one-run": [1025],                                        # P = 2048
    "m8192-run8000": [8000, 29, 29, 29, 29, 29, 29, 18],            # P = 8192
}
PLANNED = {"m300-run200": ("rank",), "m600-run500-then70": ("bitonic", 1024), "m1025-one-run": ("bitonic", 2048),
           "m8192-run8000": ("bitonic", 8192)}


@pytest.mark.parametrize("d", (32, 128))
@pytest.mark.parametrize("name", tuple(LAYOUTS))
def test_layouts_are_exact_against_the_reference(mf, name, d):
    spec = uc._one(f"hand-{name}-d{d}", "hand", d, LAYOUTS[name], 0, 0, 7200 + d)
    assert spec.n == int(spec.counts().sum()) and uc.regime(spec.n) == PLANNED[name]
    inp = uc.build(spec, 1)
    idx, grad, w0 = (torch.from_numpy(inp[k] if k != "grads" else inp[k][0]).to(DEV) for k in ("idx", "grads", "w0"))
    uniq, sums = uc.reference(idx, grad, spec.n_rows)
    want = w0.clone()
    exact = w0[uniq].to(torch.int64) - sums
    assert int(exact.abs().max()) < uc.EXACT_LIMIT
    want[uniq] = exact.to(torch.float32)
    st = _state(w0)
    _single(mf, "sgd", st, idx, grad, 0, _ws(mf, spec.n, d), lr=1.0, wd=0.0)
    assert torch.equal(st[0], want), (name, d, "SGD at lr = 1 is not w0 - sum g")


# ------------------------------------------------------------------------------------- 3. rows in flight ----
TAILS = tuple(16 * a + b for a, b in ((1, -1), (1, 0), (1, 1), (2, 1)))
SHORT_RUNS = (11, 12, 13, 15, 16, 17)


def _flight_counts(x, tail, residue):
    p = uc._Placer()
    p.run(3)
    p.head_at(residue, (uc.RUN_CHUNK - residue) + x * uc.RUN_CHUNK + tail)
    for length in SHORT_RUNS:
        p.run(length)
    return p.counts


@pytest.mark.parametrize("residue", (0, 1, 31))
@pytest.mark.parametrize("d", (32, 256))
def test_rows_in_flight_at_every_boundary(mf, d, residue):
    gen = torch.Generator(device=DEV).manual_seed(7300 + d + residue)
    w0 = torch.randint(-uc.W0_MAX, uc.W0_MAX + 1, (uc.N_ROWS, d), generator=gen, device=DEV).float()
    w0[:, 0] = torch.where(w0[:, 0] == 0, torch.ones_like(w0[:, 0]), w0[:, 0])
    for x in uc.LADDER_X:
        for tail in TAILS:
            counts = _flight_counts(x, tail, residue)
            spec = uc._one(f"flight-x{x}-t{tail}-r{residue}-d{d}", "flight", d, counts, 0, 4, 7400 + x + 100 * tail)
            heads = spec.heads()
            assert heads[np.argmax(spec.counts())] % uc.RUN_CHUNK == residue
            idx_np = uc.indices(spec)
            idx = torch.from_numpy(idx_np).to(DEV)
            big = uc.magnitude(idx_np, spec.n_rows)
            bad = (idx < 0) | (idx >= spec.n_rows)
            grads = []
            for _ in range(2):
                g = torch.randint(-big, big + 1, (spec.n, d), generator=gen, device=DEV).float()
                g[bad] = float("nan")
                grads.append(g)
            refs = [uc.reference(idx, g, spec.n_rows) for g in grads]
            uniq = refs[0][0]
            ws, ws_pre = _ws(mf, spec.n, d), _ws(mf, len(uniq), d)
            dup, pre = _state(w0), _state(w0)
            for step in (1, 2):
                ids, g = uc.presummed(uniq, refs[step - 1][1], spec.n_rows)
                _single(mf, "adam", dup, idx, grads[step - 1], 0, ws, step=step)
                _single(mf, "adam", pre, ids, g.contiguous(), 0, ws_pre, step=step)
                for tensor, a, b in zip(("table", "exp_avg", "exp_avg_sq"), dup, pre):
                    assert torch.equal(a, b), (spec.name, step, tensor, "the list with duplicates against the pre-summed list")
