"""GPU: the split forward sweep of the dense loss at d = 128 (csrc/mf_bf_split.h, loss_fwd_dense_kernel's SPLIT variant)
against oracle.losses.loss in float64, against the fp32 forward, and against itself.

The score tile runs on the bf16 matrix cores: the item tile arrives as its image of three bf16 pieces, the user fragment is
split in registers, six piece products are accumulated in fp32.  Unless a test says otherwise the forward's switch is forced
to mode 2 (serve wherever d = 128 and the loss is dense) and every case asserts the bits of ``mf_loss_fwd_path`` on the
workspace its forward used: a silent return to the fp32 forward fails the test.  All switches are restored by a fixture.
Shapes and the emulation behind the precision factor: tests/_fwd_split_cases.py; bars and input families:
tests/_dense_cases.py; the route helpers are those of tests/test_gpu_dense_bwd_split_routes.py."""
from __future__ import annotations

import ctypes
import functools
import math

import pytest
import torch

from oracle import losses as ol
from tests import _bwd_split_cases as sc
from tests import _dense_cases as dc
from tests import _fwd_split_cases as fc
from tests import test_gpu_dense_bwd_split_routes as br
from tests import test_gpu_dense_dedup as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = fc.D
INFONCE, LOGISTIC, HINGE = sc.INFONCE, sc.LOGISTIC, sc.HINGE
COLS, SPLIT = fc.PATH_COLS, fc.PATH_SPLIT
FAMILIES = (("random", ol.KINDS, dc.SMOOTH), ("lattice", dc.HINGE, dc.HINGE))


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


@pytest.fixture()
def switches(mf):
    """the three process-wide switches at their defaults before and after"""
    lib = mf._lib.lib()

    def defaults():
        lib.mf_set_dense_fwd_split(1)
        lib.mf_set_dense_bwd_split(1)
        lib.mf_set_dense_dedup(1)
    defaults()
    yield lib
    defaults()


@pytest.fixture()
def fwd_always(switches):
    switches.mf_set_dense_fwd_split(2)
    return switches


def _run(mf, kind, t, dev, k=0, **route):
    """(loss, du, dv, path of the forward, path of the backward)"""
    val, u, v, ws = br._forward(mf, kind, t, dev, k, **route)
    fpath = mf._lib.lib().mf_loss_fwd_path(ws.data_ptr())
    return (val.detach().clone(),) + br._backward(mf, val, u, v, ws)[:2] + (fpath, mf._lib.lib().mf_loss_bwd_path(ws.data_ptr()))


def _served_ids(n):
    return "heavy" if n >= 1024 else "half"               # (heavy marks 700 columns with one id: it needs more than that)


@functools.lru_cache(maxsize=2)
def _served_case(family, b, n):
    return dd.build_case(family, _served_ids(n), b, n, seed=11 + b + n)


def _check_families(mf, lib, t_of, b, n, want_fpath, what0, d=D):
    """all seven kinds on the random family (values; gradients of the smooth kinds), the hinge kinds on the lattice, against
    float64 at the bars of tests/_dense_cases.py"""
    p = dc.plan(lib, b, n, mf._lib.padded_width(d))
    for family, kinds, grad_kinds in FAMILIES:
        t = t_of(family)
        dev = br._to_dev(t)
        got = {kind: _run(mf, kind, t, dev) for kind in kinds}
        want = dc.reference(t, kinds, grad_kinds)
        for kind in kinds:
            what = f"{what0} {family} {kind} B={b} N={n} d={d}"
            val, du, dv, fpath, _ = got[kind]
            if kind != "AlignmentLoss":                   # (no sweep runs for it)
                assert fpath == want_fpath, (what, fpath)
            else:
                assert fpath == 0, (what, fpath)
            assert du.shape == (b, d) and dv.shape == (n, d), (what, du.shape, dv.shape)
            dc.assert_value_close(float(val.cpu()), want[kind][0], t["sigma"], t["target"].numpy(), what)
            if kind in grad_kinds:
                br._check_grads(got[kind], want[kind], t, what, p)


# ------------------------------------------------------------------------ 1. the float64 oracle ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
@pytest.mark.parametrize("shape", list(fc.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_forward_matches_float64_oracle(mf, fwd_always, shape, plan):
    """every shape of tests/_fwd_split_cases.py, all seven kinds, with the column plan off and on (N' < N; from 1024 columns
    on the "heavy" ids: one distinct column of weight ~700)"""
    b, n = shape
    lib = fwd_always
    fc.assert_geometry(lib, b, n)
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    t_of = (lambda family: _served_case(family, b, n)) if served else (lambda family: br._case(family, b, n))
    _check_families(mf, lib, t_of, b, n, SPLIT | (COLS if served else 0), f"split forward {plan}")
    if served:
        t = _served_case("lattice", b, n)
        ws = br._forward(mf, HINGE, t, br._to_dev(t))[3]
        out9 = (ctypes.c_int64 * 9)()
        assert lib.mf_loss_cols_info(ws.data_ptr(), out9) == 0
        assert out9[0] == 1 and 0 < out9[1] < n, list(out9)          # N' < N: rows past N' of the image are zeros, tiles past NT' unread


# -------------------------------------------------------------- 2. the fused forward, bit for bit ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
def test_fused_forward_equals_the_single_kind_forwards(mf, fwd_always, plan):
    """the all-statistics instantiation and the four single-statistic ones compute the same score tiles and statistics"""
    lib = fwd_always
    b, n = fc.RING_SHAPE
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    t = _served_case("random", b, n) if served else dc.random_case(b, n, D)
    dev = br._to_dev(t)
    out, u, v, ws = br._fused(mf, t, dev, 0.25, None)
    assert lib.mf_loss_fwd_path(ws.data_ptr()) == SPLIT | (COLS if served else 0)
    for kind in ol.KINDS:
        val, _, _, ws1 = br._forward(mf, kind, t, dev)
        if kind != "AlignmentLoss":
            assert lib.mf_loss_fwd_path(ws1.data_ptr()) == SPLIT | (COLS if served else 0), kind
        assert torch.equal(val.detach(), out[kind].detach()), (plan, kind, float(val), float(out[kind]))


# ------------------------------------------------------------------------------ 3. routes ---
def test_csr_positives_equal_the_padded_route(mf, fwd_always):
    b, n = fc.ROUTE_SHAPE
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = br._case(family, b, n)
        dev = br._to_dev(t)
        csr = tuple(x.to(DEV) for x in sc.csr_of_padded(t["pos_idx"]))
        got = _run(mf, kind, t, dev, pos_idx=None, pos_csr=csr)
        padded = _run(mf, kind, t, dev)
        assert got[3] == padded[3] == SPLIT, (got[3], padded[3])
        br._same_bits(got, padded, ("csr against padded positives", kind))
        want = dc.reference(t, (kind,), (kind,))[kind]
        dc.assert_value_close(float(got[0]), want[0], t["sigma"], t["target"].numpy(), f"csr {kind}")
        br._check_grads(got, want, t, f"csr {family} {kind}")


def test_prepared_masks_refuse_the_column_plan_and_keep_the_split_forward(mf, fwd_always):
    b, n = fc.ROUTE_SHAPE
    lib = fwd_always
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = sc.heavy_case(family, b, n)
        dev = br._to_dev(t)
        lib.mf_set_dense_dedup(0)
        plain = _run(mf, kind, t, dev)
        lib.mf_set_dense_dedup(2)
        served = _run(mf, kind, t, dev)
        fn = getattr(mf.losses, kind)(num_negatives=0, sigma=t["sigma"], margin=t["margin"][kind])
        prepared = fn.prepare_masks(dev["item_idx"], dev["pos_idx"], batch_size=b, embedding_dim=D)
        got = _run(mf, kind, t, dev, prepared=prepared)
        assert (plain[3], served[3], got[3]) == (SPLIT, COLS | SPLIT, SPLIT), (plain[3], served[3], got[3])
        br._same_bits(got, plain, ("prepared masks against the unprepared plan-off run", kind))
        want = dc.reference(t, (kind,), (kind,))[kind]
        dc.assert_value_close(float(got[0]), want[0], t["sigma"], t["target"].numpy(), f"prepared {kind}")
        br._check_grads(got, want, t, f"prepared {family} {kind}")


@pytest.mark.parametrize("d", fc.PADDED_WIDTHS)
def test_widths_padded_to_128(mf, fwd_always, d):
    """65 <= d <= 127 runs at 128: image and user fragment hold zero features"""
    b, n = fc.ROUTE_SHAPE
    fwd_always.mf_set_dense_dedup(0)
    _check_families(mf, fwd_always, lambda family: br._case(family, b, n, d), b, n, SPLIT, "padded width", d=d)


def test_int64_targets_with_a_logq_table(mf, fwd_always):
    b, n = fc.ROUTE_SHAPE
    fwd_always.mf_set_dense_dedup(0)
    t, table = sc.table_case(b, n)
    dev = br._to_dev(t)
    assert dev["target"].dtype == torch.int64
    table_dev = table.to(DEV)
    got = {kind: _run(mf, kind, t, dev, logq=None, logq_table=table_dev) for kind in ol.KINDS}
    want = dc.reference(t, ol.KINDS, dc.SMOOTH)
    for kind in ol.KINDS:
        what = f"logq table {kind}"
        assert got[kind][3] == (0 if kind == "AlignmentLoss" else SPLIT), (what, got[kind][3])
        dc.assert_value_close(float(got[kind][0]), want[kind][0], t["sigma"], t["target"].numpy(), what)
        if kind in dc.SMOOTH:
            br._check_grads(got[kind], want[kind], t, what)
    vector = _run(mf, INFONCE, t, dev)
    br._same_bits(got[INFONCE], vector, "logq table against the logq vector")


@pytest.mark.parametrize("plan", ["plan-served", "plan-off"])
def test_captured_step_equals_the_eager_one(mf, fwd_always, plan):
    """the split forward and its image launch inside a captured step: replays on OTHER batches than the captured one equal
    the eager steps bit for bit"""
    lib = fwd_always
    lib.mf_set_dense_dedup(2 if plan == "plan-served" else 0)
    want_path = SPLIT | (COLS if plan == "plan-served" else 0)
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
            paths.append(lib.mf_loss_fwd_path(br._workspace_of(loss).data_ptr()))      # (host side: decided when the forward is issued)
            loss.backward(one)
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


@pytest.mark.parametrize("shape", fc.GATE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_default_switch_on_both_sides_of_the_gate(mf, switches, shape):
    """nothing forced: mode 1 serves from 2048 x 4096 scores upward (profiles/fwd_split_threshold.json)"""
    b, n = shape
    lib = switches
    t = dc.random_case(b, n, D)
    dev = br._to_dev(t)
    got = _run(mf, INFONCE, t, dev)
    assert bool(got[3] & SPLIT) == fc.default_serves(b, n, D, 0), (shape, got[3])
    want = dc.reference(t, (INFONCE,), (INFONCE,))[INFONCE]
    dc.assert_value_close(float(got[0]), want[0], t["sigma"], t["target"].numpy(), f"default switch {shape}")
    br._check_grads(got, want, t, f"default switch {shape}", dc.plan(lib, b, n, D))
    lib.mf_set_dense_fwd_split(0)
    off = _run(mf, INFONCE, t, dev)
    assert not off[3] & SPLIT
    if not got[3] & SPLIT:
        br._same_bits(got, off, ("below the gate: the bits of mode 0", shape))


@pytest.mark.parametrize("row", [(64, 8192, 64, 0), (64, 8192, 128, 4)], ids=lambda r: "x".join(map(str, r)))
def test_other_widths_and_mined_losses_are_never_served(mf, switches, row):
    b, n, d, k = row
    lib = switches
    t = dc.random_case(b, n, d)
    dev = br._to_dev(t)
    for kind in (INFONCE, LOGISTIC):
        lib.mf_set_dense_fwd_split(2)
        forced = _run(mf, kind, t, dev, k)
        lib.mf_set_dense_fwd_split(0)
        off = _run(mf, kind, t, dev, k)
        assert not forced[3] & SPLIT and not off[3] & SPLIT, (row, kind, forced[3], off[3])
        br._same_bits(forced, off, (row, kind))
        assert torch.isfinite(forced[1]).all() and torch.isfinite(forced[2]).all()


# ------------------------------------------------------------ 4. forward mode x backward mode ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
def test_every_forward_mode_feeds_every_backward_mode(mf, switches, plan):
    """the backward reads the logit stash whichever way the forward filled it; a forward's bits do not depend on the
    backward's switch, and a retained graph differentiates twice after a split forward (the backward's image launch has
    overwritten the forward's image by then)"""
    lib = switches
    b, n = fc.STREAM_SHAPE
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    cols = COLS if served else 0
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = sc.heavy_case(family, b, n) if served else br._case(family, b, n)
        dev = br._to_dev(t)
        want = dc.reference(t, (kind,), (kind,))[kind]
        runs = {}
        for fmode in (0, 2):
            for bmode in (0, 2):
                lib.mf_set_dense_fwd_split(fmode)
                lib.mf_set_dense_bwd_split(bmode)
                got = runs[fmode, bmode] = _run(mf, kind, t, dev)
                what = f"forward mode {fmode}, backward mode {bmode} {plan} {kind}"
                assert got[3] == cols | (SPLIT if fmode else 0), (what, got[3])
                assert bool(got[4] & sc.PATH_SPLIT) == bool(bmode) and bool(got[4] & COLS) == served, (what, got[4])
                dc.assert_value_close(float(got[0]), want[0], t["sigma"], t["target"].numpy(), what)
                br._check_grads(got, want, t, what, dc.plan(lib, b, n, D))
        for fmode in (0, 2):
            assert torch.equal(runs[fmode, 0][0], runs[fmode, 2][0]), (kind, fmode, "the forward does not read the backward's switch")
        for bmode in (0, 2):
            lib.mf_set_dense_fwd_split(2)
            lib.mf_set_dense_bwd_split(bmode)
            val, u, v, ws = br._forward(mf, kind, t, dev)
            first = br._backward(mf, val, u, v, ws, retain=True)
            second = br._backward(mf, val, u, v, ws)
            for x, y, name in zip(first[:2], second[:2], ("du", "dv")):
                assert torch.equal(x, y), (kind, plan, bmode, name, "second backward on a retained graph")
            br._same_bits((val.detach(),) + first, runs[2, bmode], (kind, plan, bmode, "against a fresh run"))


# ------------------------------------------------- 5. poisoned workspace, through the C ABI ---
POISON_CASES = {
    "small": (sc.SMALL_SHAPE, "plain", 0, SPLIT),                 # Bp = 128: the image lies in the backward images' own room
    "route": (fc.ROUTE_SHAPE, "plain", 0, SPLIT),                 # the image lies inside the G' stash
    "heavy-plan": (fc.ROUTE_SHAPE, "heavy", 2, COLS | SPLIT),     # N' < N: rows past N' of the last streamed tile are zeros
}


@pytest.mark.parametrize("bmode", [0, 2], ids=["bwd-fp32", "bwd-split"])
@pytest.mark.parametrize("name", list(POISON_CASES))
def test_results_do_not_depend_on_what_the_workspace_held(mf, switches, name, bmode):
    """nothing is cleared by the caller: image rows of padding, and of a packed v' past N', are written by the image kernel"""
    lib = switches
    (b, n), ids, dedup, want_path = POISON_CASES[name]
    nbytes = lib.mf_loss_ws_bytes(b, n, D, dc.P, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        if ids == "heavy":
            t, other = sc.heavy_case(family, b, n), dd.build_case(family, "heavy", b, n, seed=977)
        else:
            t, other = br._case(family, b, n), dd.build_case(family, "half", b, n, seed=977)
        dev, other_dev = br._to_dev(t), br._to_dev(other)

        def modes(fmode):
            lib.mf_set_dense_fwd_split(fmode)
            lib.mf_set_dense_bwd_split(bmode)
            lib.mf_set_dense_dedup(dedup)
        modes(2)
        module = _run(mf, kind, t, dev)
        assert module[3] == want_path, (name, kind, module[3])
        runs = {}
        for fill in (0x00, 0xFF, 0xA5):
            ws.fill_(fill)
            runs[f"0x{fill:02X}"] = br._abi_run(mf, kind, t, dev, ws, b, n) + (lib.mf_loss_fwd_path(ws.data_ptr()),)
        modes(0)                                            # another case's forward and backward with the fp32 forward
        left = br._abi_run(mf, kind, other, other_dev, ws, b, n)
        assert lib.mf_loss_fwd_path(ws.data_ptr()) == (COLS if dedup else 0) and torch.isfinite(left[1]).all() and torch.isfinite(left[2]).all()
        modes(2)
        runs["leftovers"] = br._abi_run(mf, kind, t, dev, ws, b, n) + (lib.mf_loss_fwd_path(ws.data_ptr()),)
        for fill, got in runs.items():
            assert got[4] == want_path, (name, kind, fill, got[4])
            assert torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all(), (name, kind, fill)
            br._same_bits(got, module, (name, kind, f"workspace filled with {fill} against the module route"))


# ---------------------------------------------------------------------------- 6. repeatability ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
def test_split_forward_is_repeatable(mf, fwd_always, plan):
    lib = fwd_always
    b, n = fc.RING_SHAPE
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = _served_case(family, b, n) if served else br._case(family, b, n)
        dev = br._to_dev(t)
        first, again = _run(mf, kind, t, dev), _run(mf, kind, t, dev)
        assert first[3] == again[3] == SPLIT | (COLS if served else 0), (first[3], again[3])
        br._same_bits(first, again, (kind, plan, "second forward + backward"))


# ------------------------------------------------------------------------------- 7. precision ---
def test_split_forward_is_no_worse_than_the_fp32_forward(mf, switches):
    """E = the worst error of a gradient against float64 in units of the gradient bar (_dense_cases.grad_excess), split
    forward against fp32 forward, both under the fp32 backward so that only the forward differs, on the sharp-softmax case of
    tests/_fwd_split_cases.py.  The CPU emulation on THESE inputs (rerun by tests/test_dense_fwd_split_cpu.py) gives
    r6 = E(six products) / E(fp32 matmul) = 1.00 at the most and r5 = E(any five) / E(fp32 matmul) = 3.05 at the least: the
    factor is their geometric mean, 1.75."""
    lib = switches
    assert abs(fc.FACTOR - math.sqrt(fc.R6 * fc.R5)) <= 0.005 and fc.R5 >= 2 * fc.R6
    lib.mf_set_dense_dedup(0)
    lib.mf_set_dense_bwd_split(0)
    t = fc.precision_case()
    dev = br._to_dev(t)
    want = dc.reference(t, (INFONCE,), (INFONCE,))[INFONCE]
    err = {}
    for fmode in (0, 2):
        lib.mf_set_dense_fwd_split(fmode)
        got = _run(mf, INFONCE, t, dev)
        assert got[3] == (SPLIT if fmode else 0) and got[4] == 0, (fmode, got[3], got[4])
        err[fmode] = tuple(float(dc.grad_excess(g.cpu().numpy(), w, t["sigma"]).max()) for g, w in ((got[1], want[1]), (got[2], want[2])))
    bad = []
    for side, e_fp32, e_split in zip(("du", "dv"), err[0], err[2]):
        print(f"InfoNCE {side}: E(fp32 forward) = {e_fp32:.4g}, E(split forward) = {e_split:.4g}")
        if not (e_fp32 > 0 and e_split <= fc.FACTOR * e_fp32):
            bad.append((side, f"E(split) = {e_split:.6g}", f"E(fp32) = {e_fp32:.6g}"))
    assert not bad, bad
