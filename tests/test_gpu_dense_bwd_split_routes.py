"""GPU: the split backward sweeps of the dense loss (csrc/mf_bf_split.h, loss_bwd_dense_kernel's SPLIT variants) on every route
that reaches them, where tests/test_gpu_dense_bwd_split.py looks at one: forced mode 2, a single-kind loss object with padded
positives, d = 128 exactly, B >= 256.

1. the DEFAULT switch (mode 1): which path serves either side of N = 8192, at batches of 24 .. 300 rows -- where the operand
   images have room of their own and dV's splits hold padding only -- against float64; d = 64 and a mined loss never split;
2. the other routes into mf_loss_bwd: fused_losses (one and several trained kinds), CSR positives, prepared masks, widths
   padded to 128, a logQ table, a non-unit grad_out, a step replayed from a captured graph;
3. the switches flipped between a forward and its backward, and a retained graph differentiated under modes 0, 2, 0;
4. mf_loss_fwd / mf_loss_bwd through the C ABI on a workspace filled with 0x00, 0xFF, 0xA5 or another call's leftovers;
5. the no-worse-than-fp32 comparison where the column plan weights G' (factor from the CPU emulation of
   tests/_bwd_split_cases.py), and at (24, 8192) under mode 1.

Every case asserts the bits of ``mf_loss_bwd_path`` on the workspace its backward used, and both switches are restored by a
fixture.  References are oracle.losses.loss in float64 (tests/_dense_cases.py: ``reference``), bars those of that module."""
from __future__ import annotations

import math

import pytest
import torch

from oracle import losses as ol
from tests import _bwd_split_cases as sc
from tests import _dense_cases as dc
from tests import test_gpu_dense_dedup as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = sc.D
INFONCE, LOGISTIC, HINGE = sc.INFONCE, sc.LOGISTIC, sc.HINGE
COLS, SPLIT, RECOMP = sc.PATH_COLS, sc.PATH_SPLIT, sc.PATH_RECOMP
FAMILIES = (("random", ol.KINDS, dc.SMOOTH), ("lattice", dc.HINGE, dc.HINGE))
NO_MARGIN = ("AlignmentLoss", INFONCE, "MutualInformationNeuralEstimationLoss")
LOCATE = {"tps_u": 1, "tps_v": 1, "nsplit_u": 0, "nsplit_v": 0}               # (only names rows in a failure message)


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


@pytest.fixture()
def switches(mf):
    """both process-wide switches at their defaults before and after"""
    lib = mf._lib.lib()
    lib.mf_set_dense_bwd_split(1)
    lib.mf_set_dense_dedup(1)
    yield lib
    lib.mf_set_dense_bwd_split(1)
    lib.mf_set_dense_dedup(1)


def _modes(lib, split, dedup):
    lib.mf_set_dense_bwd_split(split)
    lib.mf_set_dense_dedup(dedup)


def _to_dev(t):
    return {k: x.to(DEV) for k, x in t.items() if isinstance(x, torch.Tensor)}


def _case(family, b, n, d=D):
    return dc.random_case(b, n, d) if family == "random" else dc.lattice_case(b, n, d)


def _workspace_of(val):
    """the workspace of the forward behind ``val`` (kept by the loss's autograd node)"""
    node = val.grad_fn
    while not hasattr(node, "saved_tensors"):
        node = node.next_functions[0][0]
    return node.saved_tensors[2]


def _forward(mf, kind, t, dev, k=0, **route):
    """(value, u, v, workspace); ``route``: keywords of the loss call that replace the padded positives / the logQ vector"""
    u, v = dev["u"].clone().requires_grad_(), dev["v"].clone().requires_grad_()
    fn = getattr(mf.losses, kind)(num_negatives=k, sigma=t["sigma"], margin=t["margin"][kind])
    kw = dict(item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], logq=dev.get("logq"))
    kw.update(route)
    val = fn(u, v, dev["target"], **kw)
    return val, u, v, _workspace_of(val)


def _backward(mf, val, u, v, ws, retain=False, scale=None):
    """(du, dv, path of this backward)"""
    u.grad = v.grad = None
    (val if scale is None else scale * val).backward(retain_graph=retain)
    return u.grad.clone(), v.grad.clone(), mf._lib.lib().mf_loss_bwd_path(ws.data_ptr())


def _run(mf, kind, t, dev, k=0, scale=None, **route):
    """(loss, du, dv, path)"""
    val, u, v, ws = _forward(mf, kind, t, dev, k, **route)
    return (val.detach().clone(),) + _backward(mf, val, u, v, ws, scale=scale)


def _same_bits(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("loss", "du", "dv")):
        assert torch.equal(x, y), (what, name)


def _check_grads(got, want, t, what, p=LOCATE, scale=1.0):
    _, du, dv = got[:3]
    dc.assert_grads_close_located(du.cpu().numpy(), scale * want[1], t["sigma"], what, "du", p, floor_scale=abs(scale))
    dc.assert_grads_close_located(dv.cpu().numpy(), scale * want[2], t["sigma"], what, "dv", p, floor_scale=abs(scale))


def _check_families(mf, lib, b, n, d, path_ok, what0):
    """all seven kinds on the random family (values; gradients of the smooth kinds), the hinge kinds on the lattice, against
    float64; ``path_ok(path)`` for every kind that sweeps"""
    p = dc.plan(lib, b, n, mf._lib.padded_width(d))
    for family, kinds, grad_kinds in FAMILIES:
        t = _case(family, b, n, d)
        dev = _to_dev(t)
        got = {kind: _run(mf, kind, t, dev) for kind in kinds}
        want = dc.reference(t, kinds, grad_kinds)
        for kind in kinds:
            what = f"{what0} {family} {kind} B={b} N={n} d={d}"
            val, du, dv, path = got[kind]
            if kind != "AlignmentLoss":                   # (no sweep runs for it)
                assert path_ok(path), (what, f"path = {path}", f"bit 0 (distinct columns) = {path & COLS}")
            assert du.shape == (b, d) and dv.shape == (n, d), (what, du.shape, dv.shape)
            dc.assert_value_close(float(val.cpu()), want[kind][0], t["sigma"], t["target"].numpy(), what)
            if kind in grad_kinds:
                _check_grads(got[kind], want[kind], t, what, p)


def _split_served(path):
    return path & SPLIT and path & RECOMP


# --------------------------------------------------------- 1. the default switch (mode 1) ---
@pytest.mark.parametrize("shape", list(sc.SERVED), ids=lambda s: f"{s[0]}x{s[1]}")
def test_default_switch_serves_from_8192_columns(mf, switches, shape):
    """nothing forced: N >= 8192 at d = 128 takes the split sweeps, at batches where the images get room of their own
    (Bp = 128) and three of dV's four splits contract a zero image against the G' of padded rows"""
    b, n = shape
    want_u, want_v, own_room, what = sc.SERVED[shape]
    sc.assert_geometry(switches, b, n, want_u, want_v, own_room)
    _check_families(mf, switches, b, n, D, _split_served, "default switch")


@pytest.mark.parametrize("row", list(sc.UNSERVED), ids=lambda r: "x".join(map(str, r)))
def test_default_switch_leaves_the_rest_to_the_fp32_sweeps(mf, switches, row):
    """one column below the threshold, d = 64, a mined loss: the path bits say so, and the results are those of mode 0"""
    b, n, d, k = row
    lib = switches
    want_path, what = sc.UNSERVED[row]
    assert dc.plan(lib, b, n, d, k)["mined"] == (1 if k else 0)
    t = dc.random_case(b, n, d)
    dev = _to_dev(t)
    for kind in (INFONCE, LOGISTIC):
        lib.mf_set_dense_bwd_split(1)
        auto = _run(mf, kind, t, dev, k)
        lib.mf_set_dense_bwd_split(0)
        off = _run(mf, kind, t, dev, k)
        assert auto[3] == want_path and off[3] == want_path, (row, what, kind, auto[3], off[3])
        assert not auto[3] & (SPLIT | RECOMP)
        _same_bits(auto, off, (row, kind))
        assert torch.isfinite(auto[1]).all() and torch.isfinite(auto[2]).all()


# ------------------------------------------------------------------------------ 2. routes ---
@pytest.fixture()
def split_always(switches):
    switches.mf_set_dense_bwd_split(2)
    return switches


def _fused(mf, t, dev, margin, train_loss):
    u, v = dev["u"].clone().requires_grad_(), dev["v"].clone().requires_grad_()
    out = mf.losses.fused_losses(u, v, dev["target"], item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], sigma=t["sigma"],
                                 margin=margin, logq=dev.get("logq"), kinds=ol.KINDS, train_loss=train_loss)
    return out, u, v, _workspace_of(out[INFONCE])


@pytest.mark.parametrize("kind,family", [(INFONCE, "random"), (LOGISTIC, "random"), (HINGE, "lattice")], ids=lambda x: x[:8])
def test_fused_losses_with_one_trained_kind(mf, split_always, kind, family):
    """the forward runs without MF_LOSS_ROWC (all statistics, no row coefficients): the backward's rowc_kernel feeds the sweeps"""
    b, n = sc.ROUTE_SHAPE
    t = _case(family, b, n)
    dev = _to_dev(t)
    out, u, v, ws = _fused(mf, t, dev, t["margin"][kind], kind)
    got = (out[kind].detach(),) + _backward(mf, out[kind], u, v, ws)
    assert got[3] == SPLIT | RECOMP, got[3]
    want = dc.reference(t, ol.KINDS, (kind,))
    for other in ol.KINDS:                                 # (one margin per fused call: the kinds this one is right for)
        if other in NO_MARGIN or t["margin"][other] == t["margin"][kind]:
            dc.assert_value_close(float(out[other].detach()), want[other][0], t["sigma"], t["target"].numpy(), f"fused {family} {other}")
    _check_grads(got, want[kind], t, f"fused, trained {kind} {family}", dc.plan(split_always, b, n, D))


def test_fused_losses_with_several_trained_kinds(mf, split_always):
    """two backwards on one workspace, each rebuilding the images inside the G' stash"""
    b, n = sc.ROUTE_SHAPE
    t = dc.random_case(b, n, D)
    dev = _to_dev(t)
    out, u, v, ws = _fused(mf, t, dev, 0.25, None)
    total = sum(c * out[kind] for kind, c in sc.COMBINATION)
    got = (total.detach(),) + _backward(mf, total, u, v, ws)
    assert got[3] == SPLIT | RECOMP, got[3]
    kinds = tuple(kind for kind, _ in sc.COMBINATION)
    ref = dc.reference(t, kinds, kinds)
    want = tuple(sum(c * ref[kind][i] for kind, c in sc.COMBINATION) for i in range(3))
    bar = sum(abs(c) * dc.value_bar(ref[kind][0], t["sigma"], t["target"].numpy()) for kind, c in sc.COMBINATION)
    assert abs(float(total.detach()) - want[0]) <= bar, (float(total.detach()), want[0], bar)
    _check_grads(got, want, t, "fused, 0.75 InfoNCE - 1.5 PairwiseLogistic", dc.plan(split_always, b, n, D))


def test_csr_positives(mf, split_always):
    b, n = sc.ROUTE_SHAPE
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = _case(family, b, n)
        dev = _to_dev(t)
        csr = tuple(x.to(DEV) for x in sc.csr_of_padded(t["pos_idx"]))
        got = _run(mf, kind, t, dev, pos_idx=None, pos_csr=csr)
        padded = _run(mf, kind, t, dev)
        assert got[3] == padded[3] == SPLIT | RECOMP, (got[3], padded[3])
        _same_bits(got, padded, ("csr against padded positives", kind))       # the same masks: the same bits
        want = dc.reference(t, (kind,), (kind,))[kind]
        dc.assert_value_close(float(got[0]), want[0], t["sigma"], t["target"].numpy(), f"csr {kind}")
        _check_grads(got, want, t, f"csr {family} {kind}")


def test_prepared_masks_refuse_the_column_plan_and_keep_the_split(mf, split_always):
    b, n = sc.ROUTE_SHAPE
    lib = split_always
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = sc.heavy_case(family, b, n)                    # copies the plan would compact
        dev = _to_dev(t)
        lib.mf_set_dense_dedup(0)
        plain = _run(mf, kind, t, dev)
        lib.mf_set_dense_dedup(2)
        served = _run(mf, kind, t, dev)
        fn = getattr(mf.losses, kind)(num_negatives=0, sigma=t["sigma"], margin=t["margin"][kind])
        prepared = fn.prepare_masks(dev["item_idx"], dev["pos_idx"], batch_size=b, embedding_dim=D)
        got = _run(mf, kind, t, dev, prepared=prepared)
        assert (plain[3], served[3], got[3]) == (SPLIT | RECOMP, COLS | SPLIT | RECOMP, SPLIT | RECOMP), (plain[3], served[3], got[3])
        _same_bits(got, plain, ("prepared masks against the unprepared plan-off run", kind))
        want = dc.reference(t, (kind,), (kind,))[kind]
        dc.assert_value_close(float(got[0]), want[0], t["sigma"], t["target"].numpy(), f"prepared {kind}")
        _check_grads(got, want, t, f"prepared {family} {kind}")


@pytest.mark.parametrize("d", sc.PADDED_WIDTHS)
def test_widths_padded_to_128(mf, split_always, d):
    """65 <= d <= 127 runs at 128: the images hold zero features, the returned gradients have d columns"""
    b, n = sc.ROUTE_SHAPE
    _check_families(mf, split_always, b, n, d, lambda path: path == SPLIT | RECOMP, "padded width")


def test_int64_targets_with_a_logq_table(mf, split_always):
    b, n = sc.ROUTE_SHAPE
    t, table = sc.table_case(b, n)
    dev = _to_dev(t)
    assert dev["target"].dtype == torch.int64
    table_dev = table.to(DEV)
    got = {kind: _run(mf, kind, t, dev, logq=None, logq_table=table_dev) for kind in ol.KINDS}
    want = dc.reference(t, ol.KINDS, dc.SMOOTH)
    for kind in ol.KINDS:
        what = f"logq table {kind}"
        if kind != "AlignmentLoss":
            assert got[kind][3] == SPLIT | RECOMP, (what, got[kind][3])
        dc.assert_value_close(float(got[kind][0]), want[kind][0], t["sigma"], t["target"].numpy(), what)
        if kind in dc.SMOOTH:
            _check_grads(got[kind], want[kind], t, what)
    vector = _run(mf, INFONCE, t, dev)                     # the same values passed per column
    _same_bits(got[INFONCE], vector, "logq table against the logq vector")


@pytest.mark.parametrize("g", sc.GRAD_OUTS, ids=lambda g: f"{g:g}")
def test_grad_out_is_folded_into_g_before_the_split(mf, split_always, g):
    b, n = sc.ROUTE_SHAPE
    for kind, family in ((INFONCE, "random"), (LOGISTIC, "random"), (HINGE, "lattice")):
        t = _case(family, b, n)
        dev = _to_dev(t)
        got = _run(mf, kind, t, dev, scale=g)
        assert got[3] == SPLIT | RECOMP, got[3]
        want = dc.reference(t, (kind,), (kind,))[kind]
        _check_grads(got, want, t, f"grad_out = {g} {family} {kind}", scale=g)


@pytest.mark.parametrize("plan", ["plan-served", "plan-off"])
def test_captured_step_equals_the_eager_one(mf, split_always, plan):
    """the body of tests/test_gpu_dense_dedup.py's test, with the split sweeps inside the captured step: replays on OTHER
    batches than the captured one equal the eager steps bit for bit"""
    lib = split_always
    lib.mf_set_dense_dedup(2 if plan == "plan-served" else 0)
    want_path = SPLIT | RECOMP | (COLS if plan == "plan-served" else 0)
    g = torch.Generator().manual_seed(3)
    b, users, items = 256, 400, 300

    def batch():
        item = torch.cat([torch.randint(1, 40, (b,), generator=g), torch.randint(1, items, (b,), generator=g)])
        pos = torch.randint(0, items, (b, 4), generator=g)
        pos[:, 0] = item[:b]
        return {k: x.to(DEV) for k, x in dict(user=torch.randint(1, users, (b,), generator=g), item=item,
                                              target=torch.randint(1, 6, (b,), generator=g), pos=pos).items()}

    batches = [batch() for _ in range(3)]
    results = []
    for captured in (False, True):
        torch.manual_seed(0)
        towers = mf.models.init_towers(mf.models.ModelConfig(num_users=users, num_items=items, hidden_size=D), device=DEV)
        opt = mf.optim.SparseSGD(list(towers.parameters()), lr=0.05)
        fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)
        one = torch.ones((), device=DEV)
        paths = []

        def step(bt):
            loss = fn(towers["user"](bt["user"]), towers["item"](bt["item"]), bt["target"], item_idx=bt["item"], pos_idx=bt["pos"])
            ws = _workspace_of(loss)
            loss.backward(one)
            paths.append(lib.mf_loss_bwd_path(ws.data_ptr()))      # (host side: decided when the backward is issued)
            opt.step()
            return loss.detach()

        if captured:
            run = mf.graph.CapturedStep(step, batches[0], optimizers=[opt], warmup=3)
        else:
            for _ in range(3):              # the capture's three warm-up steps are real steps on batch 0
                step(batches[0])
            run = step
        assert paths and all(p == want_path for p in paths), (plan, captured, paths)
        losses = [run(bt).clone() for bt in batches[1:]]
        results.append((losses, [p.detach().clone() for p in towers.parameters()]))
    (l0, p0), (l1, p1) = results
    assert all(torch.equal(x, y) for x, y in zip(l0, l1)), (l0, l1)
    assert all(torch.equal(x, y) for x, y in zip(p0, p1))


# ---------------------------------------- 3. switches flipped between forward and backward ---
def test_split_switch_is_read_by_the_backward(mf, switches):
    """the split is decided when the backward runs: a forward under one mode and a backward under the other give the bits of
    a run wholly under the backward's mode"""
    lib = switches
    b, n = sc.ROUTE_SHAPE
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = _case(family, b, n)
        dev = _to_dev(t)
        whole = {}
        for mode in (0, 2):
            lib.mf_set_dense_bwd_split(mode)
            whole[mode] = _run(mf, kind, t, dev)
        assert (whole[0][3], whole[2][3]) == (0, SPLIT | RECOMP), (whole[0][3], whole[2][3])
        for before, after in ((0, 2), (2, 0)):
            lib.mf_set_dense_bwd_split(before)
            val, u, v, ws = _forward(mf, kind, t, dev)
            lib.mf_set_dense_bwd_split(after)
            got = (val.detach(),) + _backward(mf, val, u, v, ws)
            assert got[3] == whole[after][3], (kind, before, after, got[3])
            _same_bits(got, whole[after], (kind, f"forward under mode {before}, backward under mode {after}"))


@pytest.mark.parametrize("split", [2, 0], ids=["split-on", "split-off"])
def test_column_plan_of_the_forward_holds_for_its_backward(mf, switches, split):
    """the column plan is decided by the forward and remembered per workspace, whatever the switch says by then"""
    lib = switches
    b, n = sc.ROUTE_SHAPE
    want_path = COLS | (SPLIT | RECOMP if split else 0)
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = sc.heavy_case(family, b, n)
        dev = _to_dev(t)
        _modes(lib, split, 2)
        whole = _run(mf, kind, t, dev)
        val, u, v, ws = _forward(mf, kind, t, dev)
        lib.mf_set_dense_dedup(0)
        got = (val.detach(),) + _backward(mf, val, u, v, ws)
        assert whole[3] == want_path and got[3] == want_path, (kind, whole[3], got[3])
        _same_bits(got, whole, (kind, "forward under plan mode 2, backward under plan mode 0"))


@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
def test_retained_graph_under_modes_0_2_0(mf, switches, plan):
    """dU's G' stash (fp32 sweeps) and the operand images (split sweeps) share the same bytes: three backwards of one graph"""
    lib = switches
    b, n = sc.STREAM_SHAPE
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    cols = COLS if served else 0
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = sc.heavy_case(family, b, n) if served else _case(family, b, n)
        dev = _to_dev(t)
        lib.mf_set_dense_bwd_split(2)
        fresh = _run(mf, kind, t, dev)
        lib.mf_set_dense_bwd_split(0)
        val, u, v, ws = _forward(mf, kind, t, dev)
        runs = []
        for i, mode in enumerate((0, 2, 0)):
            lib.mf_set_dense_bwd_split(mode)
            runs.append((val.detach(),) + _backward(mf, val, u, v, ws, retain=i < 2))
        assert [r[3] for r in runs] == [cols, cols | SPLIT | RECOMP, cols] and fresh[3] == cols | SPLIT | RECOMP, [r[3] for r in runs]
        _same_bits(runs[0], runs[2], (kind, plan, "first and third backward (mode 0)"))
        _same_bits(runs[1], fresh, (kind, plan, "second backward (mode 2) against a fresh mode-2 run"))


# ------------------------------------------------- 4. poisoned workspace, through the C ABI ---
def _abi_run(mf, kind, t, dev, ws, b, n):
    """mf_loss_fwd + mf_loss_bwd on the caller's workspace as it is; du and dv start as NaN"""
    lib, L = mf._lib.lib(), mf._lib
    ki = ol.KINDS.index(kind)
    out = torch.empty(len(ol.KINDS), dtype=torch.float32, device=DEV)
    u, v, lq = dev["u"], dev["v"], dev.get("logq")
    assert dev["target"].dtype == torch.int64 and u.is_contiguous() and v.is_contiguous()
    st = torch.cuda.current_stream().cuda_stream
    nbytes = lib.mf_loss_ws_bytes(b, n, D, dc.P, 0)
    assert 0 < nbytes <= ws.numel()
    L.check(lib.mf_loss_fwd(b, n, D, dc.P, 0, t["sigma"], t["margin"][kind], 1 << ki, u.data_ptr(), v.data_ptr(), dev["target"].data_ptr(),
                            dev["item_idx"].data_ptr(), dev["pos_idx"].data_ptr(), L.ptr(lq), 0, L.LOSS_TARGET_I64 | L.LOSS_ROWC,
                            ws.data_ptr(), nbytes, out.data_ptr(), None, st))
    du, dv = torch.full_like(u, float("nan")), torch.full_like(v, float("nan"))
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    L.check(lib.mf_loss_bwd(b, n, D, dc.P, 0, t["sigma"], t["margin"][kind], ki, u.data_ptr(), v.data_ptr(), L.LOSS_ROWC, ws.data_ptr(),
                            nbytes, one.data_ptr(), du.data_ptr(), dv.data_ptr(), st))
    return out[ki].clone(), du, dv, lib.mf_loss_bwd_path(ws.data_ptr())


POISON_CASES = {
    "small-split": (sc.SMALL_SHAPE, "plain", 2, 0, SPLIT | RECOMP),           # images in their own room, dV over padding only
    "route-split": (sc.ROUTE_SHAPE, "plain", 2, 0, SPLIT | RECOMP),
    "heavy-plan-split": (sc.ROUTE_SHAPE, "heavy", 2, 2, COLS | SPLIT | RECOMP),   # N' < N: image tiles past N' keep the poison
    "route-fp32": (sc.ROUTE_SHAPE, "plain", 0, 0, 0),
    "heavy-plan-fp32": (sc.ROUTE_SHAPE, "heavy", 0, 2, COLS),
}


@pytest.mark.parametrize("name", list(POISON_CASES))
def test_results_do_not_depend_on_what_the_workspace_held(mf, switches, name):
    """The loss takes its workspace from torch.empty and from a pool of used blocks, and the forward documents no word the
    caller must clear: so nothing is cleared here.  The split sweeps read memory nobody may have written -- image tiles of
    padding rows, tiles past N' under the column plan, rowc of padded users in dV's recompute."""
    lib = switches
    (b, n), ids, split, dedup, want_path = POISON_CASES[name]
    nbytes = lib.mf_loss_ws_bytes(b, n, D, dc.P, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        if ids == "heavy":
            t, other = sc.heavy_case(family, b, n), dd.build_case(family, "heavy", b, n, seed=977)
        else:
            t, other = _case(family, b, n), dd.build_case(family, "half", b, n, seed=977)
        dev, other_dev = _to_dev(t), _to_dev(other)
        _modes(lib, split, dedup)
        module = _run(mf, kind, t, dev)
        assert module[3] == want_path, (name, kind, module[3])
        runs = {}
        for fill in (0x00, 0xFF, 0xA5):
            ws.fill_(fill)
            runs[f"0x{fill:02X}"] = _abi_run(mf, kind, t, dev, ws, b, n)
        _modes(lib, 0 if split else 2, dedup)               # another case's forward and backward in the OTHER split mode
        left = _abi_run(mf, kind, other, other_dev, ws, b, n)
        assert bool(left[3] & SPLIT) != bool(split) and torch.isfinite(left[1]).all() and torch.isfinite(left[2]).all()
        _modes(lib, split, dedup)
        runs["leftovers"] = _abi_run(mf, kind, t, dev, ws, b, n)
        for fill, got in runs.items():
            assert got[3] == want_path, (name, kind, fill, got[3])
            assert torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all(), (name, kind, fill)
            _same_bits(got, module, (name, kind, f"workspace filled with {fill} against the module route"))


def test_path_of_a_backward_without_a_dense_sweep_is_zero(mf, split_always):
    """mf_loss_bwd_path answers for the LAST backward on the workspace: an alignment backward after a split one reports 0"""
    b, n = sc.SMALL_SHAPE
    t = dc.random_case(b, n, D)
    dev = _to_dev(t)
    ws = torch.empty(split_always.mf_loss_ws_bytes(b, n, D, dc.P, 0), dtype=torch.uint8, device=DEV)
    assert _abi_run(mf, INFONCE, t, dev, ws, b, n)[3] == SPLIT | RECOMP
    val, du, dv, path = _abi_run(mf, "AlignmentLoss", t, dev, ws, b, n)
    assert path == 0
    want = dc.reference(t, ("AlignmentLoss",), ("AlignmentLoss",))["AlignmentLoss"]
    dc.assert_value_close(float(val), want[0], t["sigma"], t["target"].numpy(), "alignment")
    _check_grads((val, du, dv), want, t, "alignment")


# ------------------------------------------------------ 5. precision where the plan weights G' ---
def _excess_by_mode(mf, lib, t, kinds, modes):
    """{kind: {mode: (E(du), E(dv))}}, E = the worst error against float64 in units of the gradient bar"""
    dev = _to_dev(t)
    want = dc.reference(t, kinds, kinds)
    out = {}
    for kind in kinds:
        out[kind] = {}
        for mode in modes:
            lib.mf_set_dense_bwd_split(mode)
            _, du, dv, path = _run(mf, kind, t, dev)
            assert bool(path & SPLIT) == (mode != 0), (kind, mode, path)
            out[kind][mode] = tuple(float(dc.grad_excess(g.cpu().numpy(), w, t["sigma"]).max())
                                    for g, w in ((du, want[kind][1]), (dv, want[kind][2])))
    return out


def test_split_is_no_worse_than_fp32_where_the_plan_weights_g(mf, switches):
    """The plan-served "heavy" case: one distinct column of weight ~700, and G' x weight is what dU splits.  E as in
    tests/test_gpu_dense_bwd_split.py.  The CPU emulation of the scheme on THESE inputs (tests/_bwd_split_cases.py: torch's
    fp32 G', bf16 casts, G' weighted by the copy counts; rerun by tests/test_bwd_split_routes_cpu.py) gives
    r6 = E(six products) / E(fp32 matmul) = 1.10 at the most and r5 = E(any five) / E(fp32 matmul) = 3.52 at the least: the
    factor is their geometric mean, 1.97."""
    lib = switches
    assert abs(sc.FACTOR - math.sqrt(sc.R6 * sc.R5)) <= 0.005 and sc.R5 >= 2 * sc.R6
    b, n = sc.PRECISION_SHAPE
    lib.mf_set_dense_dedup(2)
    t = sc.heavy_case("random", b, n)
    err = _excess_by_mode(mf, lib, t, (INFONCE, LOGISTIC), (0, 2))
    bad = []
    for kind, by_mode in err.items():
        for side, e_fp32, e_split in zip(("du", "dv"), by_mode[0], by_mode[2]):
            print(f"{kind} {side}: E(fp32) = {e_fp32:.4g}, E(split) = {e_split:.4g}")
            if not (e_fp32 > 0 and e_split <= sc.FACTOR * e_fp32):
                bad.append((kind, side, f"E(split) = {e_split:.6g}", f"E(fp32) = {e_fp32:.6g}"))
    assert not bad, bad


def test_split_is_no_worse_than_fp32_at_24_rows_under_the_default_switch(mf, switches):
    """test_split_gradients_are_no_worse_than_the_fp32_sweeps (plan off, the same input family, its factor of 2) at
    (24, 8192), the split sweeps served by mode 1"""
    lib = switches
    lib.mf_set_dense_dedup(0)
    b, n = 24, 8192
    err = _excess_by_mode(mf, lib, dc.random_case(b, n, D), (INFONCE, LOGISTIC), (0, 1))
    bad = []
    for kind, by_mode in err.items():
        for side, e_fp32, e_split in zip(("du", "dv"), by_mode[0], by_mode[1]):
            print(f"{kind} {side}: E(fp32) = {e_fp32:.4g}, E(split) = {e_split:.4g}")
            if not (e_fp32 > 0 and e_split <= 2 * e_fp32):
                bad.append((kind, side, f"E(split) = {e_split:.6g}", f"E(fp32) = {e_fp32:.6g}"))
    assert not bad, bad
