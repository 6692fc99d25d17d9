"""GPU: the sparse row update (csrc/mf_update.h, the update half of csrc/mf_embed.hip) on its own, driven through
``mf_update_sgd`` / ``mf_update_adam`` / ``mf_update_pair`` by the C ABI, on the run layouts of tests/_update_cases.py
(planned and pinned on the CPU by tests/test_update_cpu.py; which regime a case reaches is planned there through a mirror
of the bucket rules, not observed here).

Every gradient and every initial row is an integer, every partial sum stays below 2^24: a gradient row that is lost,
doubled or added to the wrong row or channel changes the result, whatever the order of the additions.  The workspace is
filled with 0xFF bytes and the gradient rows of out-of-range ids with NaN, so a read of something never written shows.

1. SGD at lr = 1, wd = 0: touched rows ``torch.equal`` to ``w0 - sum g`` of the int64 reference, every other row
   bit-identical to w0, a second call bit-identical.
2. Adam, normalised SGD, normalised Adam (lr 0.05, wd 0.01, steps 1 and 2, another gradient on step 2): the case's list
   against the list of its unique ids with the exact summed rows, through the same entry point (a multi-launch case's
   pre-summed list is padded with out-of-range ids to the same n): tables and both moments ``torch.equal``.
3. The row arithmetic of those pre-summed calls against ``oracle.embed`` in float64 (hyper-parameters at their fp32
   values, each step from the kernel's own state before it): with E the largest elementwise difference between the oracle
   in float32 and in float64, the kernel may differ from float64 by 4 E, floored at one fp32 ulp of the tensor's largest
   value.  The group butterfly, the reciprocal-then-multiply and the contraction order the roundings differently from
   torch; they do not add roundings: hence a margin of 4 and no more.  Per tensor: table, exp_avg, exp_avg_sq.
4. ``mf_update_pair`` ``torch.equal`` to the two single calls, and to the int64 reference for SGD.

  family      what                                                        widths
  bucket      one bucket of m = 1, 2, 32, 33, 511, 512 | 513, 1023,       32 64 128 256
              1024 | 1025, 2047, 2048 | 2049, 8191, 8192 | 8193 keys
              (rank | bitonic 1024 | 2048 | ... 8192 | global-memory
              sort), many runs above 33; m = 9000 as one run; two
              buckets over 8192 in one call of 65,536
  n           n = 1, 32 | 33, 64 | 65, 4096 | 4097, 8192 | 8193, 65535,   32 64 128 256
              65536 (1, 2, 4, 128, 256 buckets; the last one-launch n)
  placement   one sorted list of 2,496 keys: lengths 1..33 at residue    32 64 128 256
              0; 1, 2, 31, 32, 33, 63, 64, 65 at residues 0, 1, 31;
              heads at 1023 and 1024; a run across 2048 (list B: across
              1024); the first run; a run that ends on the last key and
              whose next chunk boundary is m
  ladder      runs of 1 + x chunks, x = NF-1, NF, NF+1, 2NF, 2NF+1 for    32 64 128 256
              NF = 12 and 16; + one row; with a first chunk of 27
  multi       n = 65537 over 32767 (packed sort) | 32768 rows (generic);  32 256
              131072 over 16383 (packed) | 40000 (generic): placement A
              in the global order, a run of 9,000, a run of exactly 32
              on a boundary, a run of 70 on the last valid position
              (out-of-range ids behind it; once none: it ends at n - 1)
  pair        n_a = 20 (one bucket), n_b = 8193 (256 buckets, one over    32 256
              8192), A's ids among B's
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import embed as oembed
from tests import _update_cases as uc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, WD, B1, B2, EPS = 0.05, 0.01, 0.9, 0.999, 1e-8
FAMILIES = (("adam", True, 0), ("sgd-normalised", False, 1), ("adam-normalised", True, 1))     # (name, adam, normalized)
MARGIN = 4
MAXIMA: dict = {}                   # (family, tensor) -> [largest E, largest kernel deviation, largest deviation / bound]


@pytest.fixture(scope="module", autouse=True)
def _report_maxima():
    """After the module: the largest E and the largest kernel deviation per family and tensor (the figures of DESIGN.md)."""
    yield
    for (family, name), (e, dev, ratio) in sorted(MAXIMA.items()):
        print(f"\nUPDATE-E-MAX {family} {name}: E {e:.3e} kernel {dev:.3e} largest kernel / bound {ratio:.3f}", end="")
    print()


def _f32(x: float) -> float:
    return float(np.float32(x))


def _ws(mf, n: int, d: int) -> torch.Tensor:
    nbytes = int(mf._lib.lib().mf_update_ws_bytes(n, d))
    return torch.full((max(nbytes, 256),), 0xFF, dtype=torch.uint8, device=DEV)


def _update(mf, adam, state, idx, grad, normalized, ws, step=1, lr=LR, wd=WD):
    """One call of the single-table entry point on state = [table, exp_avg, exp_avg_sq]."""
    lib = mf._lib.lib()
    t, m, v = state
    n_rows, d = t.shape
    assert idx.dtype == torch.int64 and grad.dtype == torch.float32 and grad.shape == (idx.numel(), d) and grad.is_contiguous()
    if adam:
        mf._lib.check(lib.mf_update_adam(t.data_ptr(), m.data_ptr(), v.data_ptr(), n_rows, d, idx.data_ptr(), idx.numel(), grad.data_ptr(),
                                         normalized, step, None, lr, B1, B2, EPS, wd, ws.data_ptr(), ws.numel(), None))
    else:
        mf._lib.check(lib.mf_update_sgd(t.data_ptr(), n_rows, d, idx.data_ptr(), idx.numel(), grad.data_ptr(), normalized, lr, wd,
                                        ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()


def _pair(mf, adam, sa, ia, ga, norm_a, wsa, sb, ib, gb, norm_b, wsb, step=1, lr=LR, wd=WD):
    lib = mf._lib.lib()
    p = (lambda x: x.data_ptr()) if adam else (lambda x: None)
    mf._lib.check(lib.mf_update_pair(int(adam), sa[0].shape[1], sa[0].data_ptr(), p(sa[1]), p(sa[2]), sa[0].shape[0], ia.data_ptr(), ia.numel(),
                                     ga.data_ptr(), norm_a, wsa.data_ptr(), wsa.numel(), sb[0].data_ptr(), p(sb[1]), p(sb[2]), sb[0].shape[0],
                                     ib.data_ptr(), ib.numel(), gb.data_ptr(), norm_b, wsb.data_ptr(), wsb.numel(), step, None, lr, B1, B2, EPS,
                                     wd, None))
    torch.cuda.synchronize()


def _inputs(spec, steps):
    inp = uc.build(spec, steps)
    return (torch.from_numpy(inp["idx"]).to(DEV), [torch.from_numpy(g).to(DEV) for g in inp["grads"]],
            torch.from_numpy(inp["w0"]).to(DEV))


def _state(w0):
    return [w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)]


def _where(spec, row: int) -> str:
    """The run of table row `row`: what to look at when a case fails."""
    for t in range(len(spec.targets)):
        at = np.nonzero(uc.target_ids(spec, t) == row)[0]
        if len(at):
            k = int(at[0])
            return (f"row {row}: run {k} of target {t} (bucket {spec.targets[t][0]}, m = {int(spec.counts(t).sum())}), head at sorted "
                    f"position {int(spec.heads(t)[k])}, length {int(spec.counts(t)[k])}")
    return f"row {row}: not in a target run (a filler or an untouched row)"


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.view(torch.int32)


def _assert_rows_equal(spec, got, want, what):
    if torch.equal(got, want):
        return
    rows = torch.nonzero((got != want).any(1)).flatten()
    r = int(rows[0])
    ch = int(torch.nonzero(got[r] != want[r])[0])
    raise AssertionError(f"{spec.name}: {what}: {len(rows)} rows differ, first {_where(spec, r)}, channel {ch}: got {float(got[r, ch])!r}, "
                         f"want {float(want[r, ch])!r}")


def _assert_untouched(spec, table, w0, uniq, what):
    mask = torch.ones(table.shape[0], dtype=torch.bool, device=table.device)
    mask[uniq] = False
    same = (_bits(table) == _bits(w0)).all(1)
    if not bool(same[mask].all()):
        r = int(torch.nonzero(mask & ~same)[0])
        raise AssertionError(f"{spec.name}: {what}: a row that no valid id names was written: {_where(spec, r)}")


def _sgd_exact_want(w0, uniq, sums):
    want = w0.clone()
    exact = w0[uniq].to(torch.int64) - sums
    assert int(exact.abs().max()) < uc.EXACT_LIMIT
    want[uniq] = exact.to(torch.float32)
    return want


@pytest.mark.parametrize("spec", uc.specs(), ids=lambda s: s.name)
def test_sgd_is_exact(mf, spec):
    idx, (grad,), w0 = _inputs(spec, 1)
    uniq, sums = uc.reference(idx, grad, spec.n_rows)
    want = _sgd_exact_want(w0, uniq, sums)
    ws = _ws(mf, spec.n, spec.d)
    first = _state(w0)
    _update(mf, False, first, idx, grad, 0, ws, lr=1.0, wd=0.0)
    _assert_untouched(spec, first[0], w0, uniq, "SGD")
    _assert_rows_equal(spec, first[0], want, "SGD, lr = 1: w0 - sum g")
    again = _state(w0)
    _update(mf, False, again, idx, grad, 0, _ws(mf, spec.n, spec.d), lr=1.0, wd=0.0)
    assert torch.equal(_bits(again[0]), _bits(first[0])), (spec.name, "a second call on fresh copies differs")


def _oracle_step(adam, normalized, rows, g, step, dtype):
    """One step of oracle.embed on compact rows (row k of each tensor belongs to unique id k) in `dtype`."""
    t, m, v = (x.to(dtype).clone() for x in rows)
    g = g.to(dtype)
    ids = torch.arange(t.shape[0])
    if normalized:
        g = oembed.normalize_backward(t[ids], g)
    if adam:
        oembed.adam_update(t, m, v, ids, g, step=step, lr=_f32(LR), beta1=_f32(B1), beta2=_f32(B2), eps=_f32(EPS), weight_decay=_f32(WD))
    else:
        oembed.sgd_update(t, ids, g, _f32(LR), _f32(WD))
    return t, m, v


def _check_row_arithmetic(spec, family, adam, normalized, before, after, sums, step):
    """Check 3 of the module docstring, on the touched rows (compact, on the CPU)."""
    g = sums.cpu().double()
    o64 = _oracle_step(adam, normalized, before, g, step, torch.float64)
    o32 = _oracle_step(adam, normalized, before, g, step, torch.float32)
    for name, k64, k32, got in zip(("table", "exp_avg", "exp_avg_sq")[: 3 if adam else 1], o64, o32, after):
        e = float((k32.double() - k64).abs().max())
        dev = float((got.double() - k64).abs().max())
        ulp = float(np.spacing(np.float32(float(k64.abs().max()))))
        bound = max(MARGIN * e, ulp)
        print(f"UPDATE-E {family} {spec.name} step {step} {name}: E {e:.3e} kernel {dev:.3e} ulp {ulp:.3e} kernel/E {dev / max(e, 1e-300):.2f}")
        top = MAXIMA.setdefault((family, name), [0.0, 0.0, 0.0])
        top[:] = [max(top[0], e), max(top[1], dev), max(top[2], dev / bound)]
        assert dev <= bound, (spec.name, family, step, name, f"kernel {dev:.3e} > max(4 E = {MARGIN * e:.3e}, ulp = {ulp:.3e})")


@pytest.mark.parametrize("spec", uc.specs(), ids=lambda s: s.name)
def test_duplicates_equal_the_presummed_list_and_rows_match_fp64(mf, spec):
    idx, grads, w0 = _inputs(spec, 2)
    refs = [uc.reference(idx, g, spec.n_rows) for g in grads]
    uniq = refs[0][0]
    lists = [uc.presummed(uniq, sums, spec.n_rows, pad_to=spec.n if spec.multi else 0) for _, sums in refs]
    assert all((len(ids) > uc.FUSED_MAX_N) == spec.multi for ids, _ in lists)                   # the same path
    ws, ws_pre = _ws(mf, spec.n, spec.d), _ws(mf, len(lists[0][0]), spec.d)
    zero = torch.zeros_like(w0)
    for family, adam, normalized in FAMILIES:
        dup, pre = _state(w0), _state(w0)
        for step in (1, 2):
            before = [x[uniq].cpu() for x in pre]
            _update(mf, adam, dup, idx, grads[step - 1], normalized, ws, step=step)
            _update(mf, adam, pre, lists[step - 1][0], lists[step - 1][1].contiguous(), normalized, ws_pre, step=step)
            for name, a, b in zip(("table", "exp_avg", "exp_avg_sq"), dup, pre):
                _assert_rows_equal(spec, a, b, f"{family}, step {step}, {name}: the list with duplicates against the pre-summed list")
            _assert_untouched(spec, dup[0], w0, uniq, family)
            if adam:
                _assert_untouched(spec, dup[1], zero, uniq, f"{family}, exp_avg")
                _assert_untouched(spec, dup[2], zero, uniq, f"{family}, exp_avg_sq")
            _check_row_arithmetic(spec, family, adam, normalized, before, [x[uniq].cpu() for x in pre], refs[step - 1][1], step)


@pytest.mark.parametrize("pair", uc.pair_specs(), ids=lambda p: p[0].name.replace("pair-a-", "pair-"))
def test_pair_equals_two_single_calls(mf, pair):
    a, b = pair
    (ia, ga, wa0), (ib, gb, wb0) = _inputs(a, 2), _inputs(b, 2)
    assert set(torch.unique(ia[(ia >= 0) & (ia < a.n_rows)]).tolist()) <= set(torch.unique(ib).tolist())      # the same ids ...
    assert not torch.equal(wa0, wb0)                                                                        # ... other tables, other gradients
    wsa, wsb = _ws(mf, a.n, a.d), _ws(mf, b.n, b.d)
    # SGD, exact: the pair, the two single calls and the int64 reference
    single_a, single_b, pa, pb = _state(wa0), _state(wb0), _state(wa0), _state(wb0)
    _update(mf, False, single_a, ia, ga[0], 0, wsa, lr=1.0, wd=0.0)
    _update(mf, False, single_b, ib, gb[0], 0, wsb, lr=1.0, wd=0.0)
    _pair(mf, False, pa, ia, ga[0], 0, wsa, pb, ib, gb[0], 0, wsb, lr=1.0, wd=0.0)
    for spec, idx, grad, w0, single, both in ((a, ia, ga[0], wa0, single_a, pa), (b, ib, gb[0], wb0, single_b, pb)):
        uniq, sums = uc.reference(idx, grad, spec.n_rows)
        want = _sgd_exact_want(w0, uniq, sums)
        _assert_untouched(spec, both[0], w0, uniq, "pair SGD")
        _assert_rows_equal(spec, both[0], want, "pair SGD against the reference")
        _assert_rows_equal(spec, single[0], want, "single SGD against the reference")
        assert torch.equal(_bits(both[0]), _bits(single[0]))
    # Adam (A normalised, B not), two steps: the pair against the two single calls
    single_a, single_b, pa, pb = _state(wa0), _state(wb0), _state(wa0), _state(wb0)
    for step in (1, 2):
        _update(mf, True, single_a, ia, ga[step - 1], 1, wsa, step=step)
        _update(mf, True, single_b, ib, gb[step - 1], 0, wsb, step=step)
        _pair(mf, True, pa, ia, ga[step - 1], 1, wsa, pb, ib, gb[step - 1], 0, wsb, step=step)
        for spec, single, both in ((a, single_a, pa), (b, single_b, pb)):
            for name, x, y in zip(("table", "exp_avg", "exp_avg_sq"), both, single):
                _assert_rows_equal(spec, x, y, f"pair Adam, step {step}, {name}: against the single call")
