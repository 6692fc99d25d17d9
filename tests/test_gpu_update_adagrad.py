"""GPU: the row-wise Adagrad row update on its own, driven through ``mf_update_adagrad`` / ``mf_update_pair_adagrad`` by the C
ABI on the run layouts of tests/_update_cases.py -- every sort regime, bucket count, chunk ladder, run placement and the
multi-launch path, like tests/test_gpu_update.py for SGD and Adam (see its table of families).

Gradients and initial rows are integers (every partial sum below 2^24: exact in any order), the initial ``sum`` is a small
integer per row, the workspace is filled with 0xFF bytes and the gradient rows of out-of-range ids with NaN.  For plain and
normalised Adagrad, each with wd = 0.01 and wd = 0 (lr 0.05, eps 1e-10), two steps with another gradient on the second:

1. Duplicates: the case's list and the list of its unique ids with the exact summed rows, through the same entry point,
   give ``torch.equal`` tables and ``sum``; every untouched row and untouched ``sum`` entry keeps its initial bits; a
   second run from the same start is bit-identical.
2. Row arithmetic: the pre-summed call against the specification (tests/_adagrad_spec.py) in fp64 -- with E the largest
   elementwise difference between the specification in fp32 and in fp64, the kernel may differ from fp64 by 4 E, floored at
   one fp32 ulp of the tensor's largest value; per tensor (table, ``sum``).  The margin is tests/test_gpu_update.py's: the
   group butterfly and the operation order move roundings, they add none.
3. The hand-worked row (g_c = +-4, lr 0.5, eps 4: s = 16, w_c = -+0.25) exactly, on every width and both launch paths.
4. ``mf_update_pair_adagrad`` ``torch.equal`` to the two single calls.

Largest figures over all cases (MI355X; printed at the end of the module as UPDATE-ADAGRAD-E-MAX): see DESIGN.md, "What the
sparse row update is held to".
"""
from __future__ import annotations

import pytest
import torch

from tests import _adagrad_spec as spec
from tests import _update_cases as uc
from tests import test_gpu_update as tgu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, WD, EPS = 0.05, 0.01, 1e-10
FAMILIES = (("adagrad", 0, WD), ("adagrad-wd0", 0, 0.0), ("adagrad-normalised", 1, WD), ("adagrad-normalised-wd0", 1, 0.0))
MARGIN = 4
MAXIMA: dict = {}                   # (family, tensor) -> [largest E, largest kernel deviation, largest deviation / bound]


@pytest.fixture(scope="module", autouse=True)
def _report_maxima():
    yield
    for (family, name), (e, dev, ratio) in sorted(MAXIMA.items()):
        print(f"\nUPDATE-ADAGRAD-E-MAX {family} {name}: E {e:.3e} kernel {dev:.3e} largest kernel / bound {ratio:.3f}", end="")
    print()


def _update(mf, state, idx, grad, normalized, ws, lr=LR, eps=EPS, wd=WD):
    """One call of the single-table entry point on state = [table, sum]."""
    t, s = state
    n_rows, d = t.shape
    assert idx.dtype == torch.int64 and grad.dtype == torch.float32 and grad.shape == (idx.numel(), d) and grad.is_contiguous()
    assert s.shape == (n_rows,) and s.dtype == torch.float32
    mf._lib.check(mf._lib.lib().mf_update_adagrad(t.data_ptr(), s.data_ptr(), n_rows, d, idx.data_ptr(), idx.numel(), grad.data_ptr(),
                                                  normalized, lr, eps, wd, ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()


def _pair(mf, sa, ia, ga, norm_a, wsa, sb, ib, gb, norm_b, wsb, lr=LR, eps=EPS, wd=WD):
    mf._lib.check(mf._lib.lib().mf_update_pair_adagrad(
        sa[0].shape[1], sa[0].data_ptr(), sa[1].data_ptr(), sa[0].shape[0], ia.data_ptr(), ia.numel(), ga.data_ptr(), norm_a, wsa.data_ptr(),
        wsa.numel(), sb[0].data_ptr(), sb[1].data_ptr(), sb[0].shape[0], ib.data_ptr(), ib.numel(), gb.data_ptr(), norm_b, wsb.data_ptr(),
        wsb.numel(), lr, eps, wd, None))
    torch.cuda.synchronize()


def _sum0(spec_):
    """The initial state: a small integer per row (zero among them), seeded by the case."""
    gen = torch.Generator().manual_seed(spec_.seed + 5)
    return torch.randint(0, 10, (spec_.n_rows,), generator=gen).to(torch.float32).to(DEV)


def _state(w0, s0):
    return [w0.clone(), s0.clone()]


def _check_row_arithmetic(case, family, normalized, wd, before, after, sums, step):
    rows = spec.check_4e(before[0], before[1], sums.cpu().double(), after[0], after[1], normalized=bool(normalized), lr=LR, eps=EPS, wd=wd,
                         margin=MARGIN)
    for name, e, dev, bound in rows:
        print(f"UPDATE-ADAGRAD-E {family} {case.name} step {step} {name}: E {e:.3e} kernel {dev:.3e} bound {bound:.3e} "
              f"kernel/E {dev / max(e, 1e-300):.2f}")
        top = MAXIMA.setdefault((family, name), [0.0, 0.0, 0.0])
        top[:] = [max(top[0], e), max(top[1], dev), max(top[2], dev / bound)]
    for name, e, dev, bound in rows:
        assert dev <= bound, (case.name, family, step, name, f"kernel {dev:.3e} > max(4 E = {MARGIN * e:.3e}, one ulp) = {bound:.3e}")


@pytest.mark.parametrize("case", uc.specs(), ids=lambda s: s.name)
def test_duplicates_equal_the_presummed_list_and_rows_match_fp64(mf, case):
    idx, grads, w0 = tgu._inputs(case, 2)
    s0 = _sum0(case)
    refs = [uc.reference(idx, g, case.n_rows) for g in grads]
    uniq = refs[0][0]
    lists = [uc.presummed(uniq, sums, case.n_rows, pad_to=case.n if case.multi else 0) for _, sums in refs]
    assert all((len(ids) > uc.FUSED_MAX_N) == case.multi for ids, _ in lists)                   # the same path
    ws, ws_pre = tgu._ws(mf, case.n, case.d), tgu._ws(mf, len(lists[0][0]), case.d)
    for family, normalized, wd in FAMILIES:
        dup, pre = _state(w0, s0), _state(w0, s0)
        for step in (1, 2):
            before = [x[uniq].cpu() for x in pre]
            _update(mf, dup, idx, grads[step - 1], normalized, ws, wd=wd)
            _update(mf, pre, lists[step - 1][0], lists[step - 1][1].contiguous(), normalized, ws_pre, wd=wd)
            tgu._assert_rows_equal(case, dup[0], pre[0], f"{family}, step {step}, table: the list with duplicates against the pre-summed list")
            tgu._assert_rows_equal(case, dup[1][:, None], pre[1][:, None], f"{family}, step {step}, sum: duplicates against pre-summed")
            tgu._assert_untouched(case, dup[0], w0, uniq, family)
            tgu._assert_untouched(case, dup[1][:, None], s0[:, None], uniq, f"{family}, sum")
            if step == 1:
                again = _state(w0, s0)
                _update(mf, again, idx, grads[0], normalized, tgu._ws(mf, case.n, case.d), wd=wd)
                assert torch.equal(tgu._bits(again[0]), tgu._bits(dup[0])) and torch.equal(tgu._bits(again[1]), tgu._bits(dup[1])), (
                    case.name, family, "a second run from the same start differs")
            _check_row_arithmetic(case, family, normalized, wd, before, [x[uniq].cpu() for x in pre], refs[step - 1][1], step)


@pytest.mark.parametrize("multi", [False, True], ids=["one-launch", "multi-launch"])
@pytest.mark.parametrize("d", uc.WIDTHS)
def test_the_hand_worked_row_is_exact(mf, d, multi):
    """w0 = 0, s0 = 0, summed gradient +-4 per channel (row 5: two rows of +-2; row 9: one row), lr 0.5, eps 4, wd 0:
    s = (1 / d) * d * 16 = 16, w_c = -+ 0.5 * 4 / (sqrt(16) + 4) = -+0.25 -- every operation exact."""
    n_rows = 20
    pattern = torch.tensor([4.0, -4.0], device=DEV).repeat(d // 2)
    ids = [5, -1, 9, 5, n_rows] + ([-1, n_rows + 3] * 32800 if multi else [])
    idx = torch.tensor(ids, dtype=torch.int64, device=DEV)
    grad = torch.full((len(ids), d), float("nan"), device=DEV)
    grad[0], grad[3], grad[2] = pattern / 2, pattern / 2, pattern
    assert (len(ids) > uc.FUSED_MAX_N) == multi
    state = [torch.zeros(n_rows, d, device=DEV), torch.zeros(n_rows, device=DEV)]
    _update(mf, state, idx, grad, 0, tgu._ws(mf, len(ids), d), lr=0.5, eps=4.0, wd=0.0)
    want_t, want_s = torch.zeros(n_rows, d, device=DEV), torch.zeros(n_rows, device=DEV)
    want_t[5] = want_t[9] = -pattern / 16
    want_s[5] = want_s[9] = 16.0
    assert torch.equal(state[0], want_t) and torch.equal(state[1], want_s)
    # wd = 0.5 on w0 = 2 with g = 3 adds exactly 1: s = 16, w = 2 - 0.5 * 4 / 8 = 1.75
    state = [torch.full((n_rows, d), 2.0, device=DEV), torch.zeros(n_rows, device=DEV)]
    grad[0], grad[3], grad[2] = 1.0, 2.0, 3.0
    _update(mf, state, idx, grad, 0, tgu._ws(mf, len(ids), d), lr=0.5, eps=4.0, wd=0.5)
    want_t = torch.full((n_rows, d), 2.0, device=DEV)
    want_t[5] = want_t[9] = 1.75
    assert torch.equal(state[0], want_t) and torch.equal(state[1], want_s)


@pytest.mark.parametrize("pair", uc.pair_specs(), ids=lambda p: p[0].name.replace("pair-a-", "pair-"))
def test_pair_equals_two_single_calls(mf, pair):
    a, b = pair
    (ia, ga, wa0), (ib, gb, wb0) = tgu._inputs(a, 2), tgu._inputs(b, 2)
    sa0, sb0 = _sum0(a), _sum0(b)
    wsa, wsb = tgu._ws(mf, a.n, a.d), tgu._ws(mf, b.n, b.d)
    single_a, single_b, pa, pb = _state(wa0, sa0), _state(wb0, sb0), _state(wa0, sa0), _state(wb0, sb0)
    for step in (1, 2):                                                 # A normalised, B not
        _update(mf, single_a, ia, ga[step - 1], 1, wsa)
        _update(mf, single_b, ib, gb[step - 1], 0, wsb)
        _pair(mf, pa, ia, ga[step - 1], 1, wsa, pb, ib, gb[step - 1], 0, wsb)
        for case, single, both, w0, s0, idx in ((a, single_a, pa, wa0, sa0, ia), (b, single_b, pb, wb0, sb0, ib)):
            tgu._assert_rows_equal(case, both[0], single[0], f"pair Adagrad, step {step}, table: against the single call")
            tgu._assert_rows_equal(case, both[1][:, None], single[1][:, None], f"pair Adagrad, step {step}, sum: against the single call")
            uniq = torch.unique(idx[(idx >= 0) & (idx < case.n_rows)])
            tgu._assert_untouched(case, both[0], w0, uniq, "pair Adagrad")
            tgu._assert_untouched(case, both[1][:, None], s0[:, None], uniq, "pair Adagrad, sum")
    assert not torch.equal(pa[0], wa0) and not torch.equal(pb[1], sb0)
