"""CPU: the host side of streaming logQ -- ``mf_logq_update`` / ``mf_logq_lookup`` (csrc/mf_logq.hip): exports, every refusal
(all decided before any launch, so never-dereferenced fake pointers do), the kernels' resources; the numpy rule
(tests/_logq_spec.py) against hand-worked rows, its closed form and a sampled stream; ``logq_from_counts``; the module's
config fields; no CPU path."""
from __future__ import annotations

import ctypes
import importlib.util
import pathlib

import numpy as np
import pytest
import torch

from oracle import embed as oembed
from tests import _logq_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
EXPORTS = ("mf_logq_update", "mf_logq_lookup")


def test_exports_are_declared_bound_and_present(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    for name in EXPORTS:
        assert hasattr(lib, name) and name in mf._lib.SIGNATURES and name + "(" in header, name
    assert "mf_logq.hip" in (ROOT / "matrix-factorization-torch_amd" / "csrc" / "Makefile").read_text()
    assert mf.StreamingLogQ is mf.logq.StreamingLogQ and mf.logq_from_counts is mf.logq.logq_from_counts


@pytest.fixture
def update(mf):
    lib = mf._lib.lib()

    def run(last=FAKE, gap=FAKE, nb=100, H=0, seed=0, ids=FAKE, n=10, t=1, t_dev=None, alpha=0.01, table=None, out=None):
        rc = lib.mf_logq_update(last, gap, nb, H, seed, ids, n, t, t_dev, alpha, table, out, None)
        return rc, (lib.mf_last_error() if rc else b"")

    return run


@pytest.fixture
def lookup(mf):
    lib = mf._lib.lib()

    def run(gap=FAKE, nb=100, H=0, seed=0, ids=FAKE, n=10, out=FAKE):
        rc = lib.mf_logq_lookup(gap, nb, H, seed, ids, n, out, None)
        return rc, (lib.mf_last_error() if rc else b"")

    return run


@pytest.mark.parametrize("kw", [dict(last=None), dict(gap=None), dict(ids=None), dict(n=-1), dict(nb=0), dict(nb=-5), dict(H=-1), dict(H=5),
                                dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=float("inf")),
                                dict(t=0), dict(t=-7), dict(table=FAKE, H=1), dict(table=FAKE, H=4)], ids=str)
def test_update_refuses_bad_arguments(mf, update, kw):
    rc, msg = update(**kw)
    assert rc == mf._lib.MF_EINVAL and msg.startswith(b"mf_logq_update: "), (kw, rc, msg)


@pytest.mark.parametrize("kw", [dict(t=1 << 31), dict(t=1 << 40), dict(nb=1 << 31), dict(nb=1 << 40, H=2)], ids=str)
def test_update_refuses_what_does_not_fit_31_bits(mf, update, kw):
    rc, msg = update(**kw)
    assert rc == mf._lib.MF_ENOTSUP and msg.startswith(b"mf_logq_update: ") and b"31 bits" in msg, (kw, rc, msg)


def test_update_accepts_the_edges_without_a_launch(mf, update):
    """n == 0 is MF_OK with nothing launched (fake pointers are never dereferenced, no GPU here), ids may then be null; a
    device step makes the host t irrelevant -- but is still only read on the device."""
    for kw in (dict(n=0), dict(n=0, ids=None), dict(n=0, alpha=1.0), dict(n=0, t=(1 << 31) - 1), dict(n=0, H=4, nb=(1 << 31) - 1),
               dict(n=0, t=0, t_dev=FAKE), dict(n=0, t=1 << 31, t_dev=FAKE), dict(n=0, table=FAKE), dict(n=0, out=FAKE)):
        rc, msg = update(**kw)
        assert rc == mf._lib.MF_OK, (kw, rc, msg)


def test_lookup_refusals(mf, lookup):
    E = mf._lib
    for kw in (dict(gap=None), dict(ids=None), dict(out=None), dict(n=-1), dict(nb=0), dict(H=-1), dict(H=5)):
        rc, msg = lookup(**kw)
        assert rc == E.MF_EINVAL and msg.startswith(b"mf_logq_lookup: "), (kw, rc, msg)
    rc, msg = lookup(nb=1 << 31)
    assert rc == E.MF_ENOTSUP and msg.startswith(b"mf_logq_lookup: "), (rc, msg)
    for kw in (dict(n=0), dict(n=0, ids=None, out=None)):
        assert lookup(**kw)[0] == E.MF_OK, kw


def test_new_kernels_have_no_spill_and_no_scratch():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    mine = {n: r for n, r in kr.kernel_resources().items() if "logq_update_kernel" in n or "logq_read_kernel" in n}
    assert len(mine) == 2, sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (name, r)


# ----------------------------------------------------------------------------------------------------- the rule ----
def test_splitmix_known_answer_and_bucket_range():
    assert int(spec.splitmix64(spec.GOLDEN_GAMMA)) == 0xE220A8397B1DCDAF          # (tests/test_host_cpu.py pins the same word)
    b = spec.hash_buckets([0, 1, 2**39 - 1], 4, 7, 17)
    assert b.shape == (3, 4) and b.min() >= 0 and b.max() < 17
    assert int(spec.hash_buckets([0], 1, 0, 2**31 - 1)[0, 0]) == 0xE220A8397B1DCDAF % (2**31 - 1)


def test_hand_worked_rows():
    s = spec.Spec(4, alpha=0.5)
    got = []
    for t in (3, 5, 6, 10):
        s.update([2], t)
        got.append(float(s.gap[2]))
    assert got == [3.0, 2.5, 1.75, 2.875] and s.last_seen.tolist() == [0, 0, 10, 0]
    assert s.logq([2, 0])[0] == -np.log(2.875) and s.logq([2, 0])[1] == 0.0


@pytest.mark.parametrize("alpha", [0.01, 0.05, 0.5, 1.0])
def test_closed_form(alpha):
    """An item seen every g steps from t0 has D_n = g + (1 - alpha)^n (t0 - g)."""
    g, t0 = 7, 5
    s = spec.Spec(1, alpha=alpha)
    worst = 0.0
    for n in range(200):
        s.update([0], t0 + n * g)
        want = g + (1.0 - float(np.float32(alpha))) ** n * (t0 - g)
        worst = max(worst, abs(float(s.gap[0]) - want))
    print(f"LOGQ-CLOSED-FORM alpha {alpha}: largest |fp32 recursion - closed form| {worst:.3e}")
    assert worst <= 1e-4
    if alpha == 1.0:
        assert worst == 0.0


def test_duplicates_count_once_and_same_t_is_idempotent():
    a, b = spec.Spec(8, alpha=0.5), spec.Spec(8, alpha=0.5)
    for t, ids in ((1, [3, 3, 3, 5]), (4, [3, 5, 5, 5, 5, 9, -1]), (9, [3] * 100)):
        a.update(ids, t)
        b.update(sorted(set(ids)), t)
        assert np.array_equal(a.gap, b.gap) and np.array_equal(a.last_seen, b.last_seen)
    before = (a.gap.copy(), a.last_seen.copy())
    first = a.logq([3, 5, 0])
    again = a.update([3, 5, 0], 9)                          # 3 was seen at 9: untouched; 5 and 0 are new sightings at 9
    assert a.gap[3] == before[0][3] and a.last_seen[5] == 9 and a.last_seen[0] == 9
    state = (a.gap.copy(), a.last_seen.copy())
    assert np.array_equal(a.update([3, 5, 0], 9), again) and np.array_equal(a.gap, state[0]) and np.array_equal(a.last_seen, state[1])
    assert first[2] == 0.0 and again[2] == -np.log(9.0)


def test_hashed_maximum_rule_and_never_seen():
    table = {10: [0, 1], 11: [0, 2], 12: [3, 3]}
    s = spec.Spec(4, alpha=1.0, num_hashes=2, bucket_fn=lambda ids, H, seed, nb: np.array([table[int(i)] for i in ids]))
    table[0] = [0, 0]                                      # (the stand-in id of an ignored negative one)
    assert s.logq([10, 11, 12]).tolist() == [0.0, 0.0, 0.0]
    s.update([10], 2)                                      # hash 0 bucket 0, hash 1 bucket 1: gap 2
    assert s.logq([10])[0] == -np.log(2.0) and s.logq([11])[0] == 0.0      # 11 shares hash 0's bucket, its other one is unseen
    s.update([11], 5)                                      # hash 0 bucket 0: gap 3; hash 1 bucket 2: gap 5
    assert s.gap.tolist() == [[3.0, 0.0, 0.0, 0.0], [0.0, 2.0, 5.0, 0.0]]
    assert s.logq([10])[0] == -np.log(3.0) and s.logq([11])[0] == -np.log(5.0) and s.logq([12, -4]).tolist() == [0.0, 0.0]
    s.update([10, 11, -4], 6)                              # 10 and 11 share hash 0's bucket: ONE sighting there
    assert s.gap.tolist() == [[1.0, 0.0, 0.0, 0.0], [0.0, 4.0, 1.0, 0.0]]
    assert s.logq([10])[0] == -np.log(4.0) and s.logq([11])[0] == 0.0 - np.log(1.0)


def test_a_gap_above_2_pow_24_rounds_to_nearest_even():
    s = spec.Spec(2, alpha=0.5)
    s.update([0, 1], 1)
    s.update([0], 2 + (1 << 24))                           # t - old = 2^24 + 1: not a float32, ties to even = 2^24
    s.update([1], 4 + (1 << 24))                           # 2^24 + 3 -> 2^24 + 4
    # fl(0.5 + 2^23) = 2^23 and fl(0.5 + 2^23 + 2) = 2^23 + 2 (ties to even again); with g = 2^24 + 3 truncated the latter would be 2^23 + 1
    assert float(s.gap[0]) == float(1 << 23) and float(s.gap[1]) == float((1 << 23) + 2)


def test_mixture_stream_estimates_the_inclusion_probability():
    """M = 2000 Zipf(1) positives, 64 + 64 columns per step, 4000 steps, alpha = 0.01: 1 / gap over the true inclusion
    probability has its median in [0.9, 1.2]."""
    m, b, steps = 2000, 64, 4000
    p = 1.0 / np.arange(1, m + 1)
    p /= p.sum()
    rng = np.random.default_rng(0)
    s = spec.Spec(m, alpha=0.01)
    for t in range(1, steps + 1):
        pos = rng.choice(m, b, p=p)
        neg = rng.integers(0, m, b)
        s.update(np.concatenate([pos, neg]), t)
    assert bool((s.gap > 0).all())                         # all 2000 items seen
    ratio = (1.0 / s.gap.astype(np.float64)) / spec.inclusion_probability(p, b, b)
    med, lo, hi = np.median(ratio), np.percentile(ratio, 5), np.percentile(ratio, 95)
    print(f"LOGQ-MIXTURE median {med:.3f}, 5th-95th percentile {lo:.3f}-{hi:.3f}")
    assert 0.9 <= med <= 1.2


# ------------------------------------------------------------------------------------------------------- python ----
def test_logq_from_counts_is_the_oracles(mf):
    g = torch.Generator().manual_seed(0)
    for counts in (torch.randint(0, 1000, (5000,), generator=g), torch.zeros(7), torch.tensor([0.0, 0.5, 3.0, 1e9]),
                   torch.randint(0, 5, (33,), generator=g).to(torch.int32)):
        got, want = mf.logq_from_counts(counts), oembed.logq_from_counts(counts)
        assert got.dtype == torch.float32 and torch.equal(got, want)


def test_config_validation_and_round_trip(mf):
    cfg_cls = mf.lightning.MatrixFactorizationLitConfig
    base = {"num_users": 30, "num_items": 40}
    d = cfg_cls(**base)
    assert (d.logq_mode, d.logq_alpha, d.logq_buckets, d.logq_hashes) == ("table", 0.01, 0, 2)
    for bad in (dict(logq_mode="streaming"), dict(logq_mode="streaming", use_logq=False), dict(logq_mode="ema", use_logq=True),
                dict(logq_alpha=0.0), dict(logq_alpha=1.01), dict(logq_alpha=float("nan")), dict(logq_buckets=-1), dict(logq_buckets=1 << 31),
                dict(logq_hashes=0), dict(logq_hashes=5)):
        with pytest.raises(ValueError):
            cfg_cls(**base, **bad)
    ok = cfg_cls(**base, use_logq=True, logq_mode="streaming", logq_alpha=1.0, logq_buckets=1024, logq_hashes=4)
    assert cfg_cls.model_validate(ok.model_dump()) == ok
    m = mf.lightning.MatrixFactorizationLitModule(base)
    assert m.logq_estimator is None and m.config.logq_mode == "table"


def test_estimator_arguments_state_and_no_cpu_path(mf):
    for bad in (dict(num_buckets=0), dict(num_buckets=1 << 31), dict(alpha=0.0), dict(alpha=float("nan")), dict(alpha=1.5), dict(num_hashes=-1),
                dict(num_hashes=5)):
        with pytest.raises(ValueError):
            mf.StreamingLogQ(**{"num_buckets": 10, **bad})
    est = mf.StreamingLogQ(10, alpha=0.5)
    assert set(est.state_dict()) == {"last_seen", "gap", "step", "table"} and est.table.tolist() == [0.0] * 10
    assert est.last_seen.dtype == torch.int32 and est.gap.dtype == torch.float32 and est.step.dtype == torch.int64 and est.step.shape == (1,)
    hashed = mf.StreamingLogQ(16, num_hashes=3, seed=5)
    assert set(hashed.state_dict()) == {"last_seen", "gap", "step"} and hashed.gap.shape == (3, 16)
    with pytest.raises(AttributeError, match="no table"):
        hashed.table
    for e in (est, hashed):
        with pytest.raises(mf.MfHipError):
            e.update(torch.tensor([1, 2, 3]))
        with pytest.raises(mf.MfHipError):
            e.lookup(torch.tensor([1, 2, 3]))
        assert int(e.step) == 0                             # a refused update does not advance the step
