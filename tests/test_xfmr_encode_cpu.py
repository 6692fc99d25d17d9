"""No GPU: the serving encode's (mf_xfmr_encode, HistoryTransformerTower.encode) argument checks -- all decided on the host
before any GPU call --, the resources of its kernel, the module constant and the refusal of CPU tensors."""
from __future__ import annotations

import ctypes
import importlib.util
import pathlib

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
LDS_BYTES = 160 * 1024


def _call(mf, **over):
    """The export on host addresses that are never read: a valid call up to the first GPU call, which ``over`` keeps it from."""
    lib = mf._lib.lib()
    buf = (ctypes.c_int64 * 16)()
    prm = (ctypes.c_void_p * 68)(*[ctypes.addressof(buf)] * 68)
    a = ctypes.addressof(buf)
    args = {"table": a, "n_rows": 300, "h": 64, "seg_start": a, "seg_end": a, "items": a, "n_items": 16, "B": 2, "max_history": 16,
            "layers": 1, "heads": 4, "intermediate": 64, "act": 0, "mode": 0, "norm_item": 1, "norm_user": 1, "params": prm, "out_u": a,
            "stream": None}
    assert set(over) <= set(args)
    args.update(over)
    return lib.mf_xfmr_encode(*args.values()), lib.mf_last_error().decode()


def test_export_is_declared_and_bound(mf):
    header = (ROOT / "include" / "mf_hip.h").read_text()
    assert "mf_xfmr_encode(" in header and "mf_xfmr_encode" in mf._lib.SIGNATURES
    assert len(mf._lib.SIGNATURES["mf_xfmr_encode"][1]) == 19  # noqa: PLR2004
    assert mf._lib.lib().mf_version() >= 101  # noqa: PLR2004


@pytest.mark.parametrize(("over", "why"), [({"h": 48}, "hidden size"), ({"heads": 16}, "head width"), ({"intermediate": 48}, "intermediate"),
                                           ({"intermediate": 288}, "intermediate"), ({"layers": 5}, "layers"), ({"layers": 0}, "layers"),
                                           ({"max_history": 65}, "max_history"), ({"max_history": 0}, "max_history"),
                                           ({"heads": 3}, "heads"), ({"n_rows": (1 << 20) + 1}, "table rows")])
def test_unsupported_shapes(mf, over, why):
    rc, msg = _call(mf, **over)
    assert rc == mf._lib.MF_ENOTSUP and msg.startswith("mf_xfmr_encode") and why in msg, (rc, msg)


@pytest.mark.parametrize("over", [{"table": None}, {"seg_start": None}, {"seg_end": None}, {"items": None}, {"params": None}, {"out_u": None},
                                  {"B": 0}, {"B": -3}, {"act": 4}, {"act": -1}, {"mode": 3}, {"mode": -1}])
def test_bad_arguments(mf, over):
    rc, msg = _call(mf, **over)
    assert rc == mf._lib.MF_EINVAL and msg.startswith("mf_xfmr_encode"), (rc, msg)


def test_null_parameter(mf):
    buf = (ctypes.c_int64 * 16)()
    prm = (ctypes.c_void_p * 68)(*[ctypes.addressof(buf)] * 68)
    prm[4 + 16 + 3] = None                                       # the second layer's bk
    rc, msg = _call(mf, params=prm, layers=2)
    assert rc == mf._lib.MF_EINVAL and "parameter 23" in msg


def test_encode_kernels_fit(mf):
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    mine = {k: v for k, v in kr.kernel_resources().items() if "xfmr_encode_kernel" in k}
    for h in (32, 64, 128):
        assert any(f"xfmr_encode_kernel<{h}>" in k for k in mine), sorted(mine)
    for k, v in mine.items():
        print(k, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["group_segment_fixed_size"] <= LDS_BYTES, (k, v)
        assert v["vgpr_count"] + v["agpr_count"] <= 512, (k, v)  # noqa: PLR2004


def test_module_constant(mf):
    limit = mf.models.XFMR_ENCODE_FUSED_MAX_USERS
    assert limit is None or (isinstance(limit, int) and not isinstance(limit, bool) and limit > 0)


def test_cpu_tensors_are_refused(mf):
    item = mf.models.EmbeddingTower(50, 32)
    user = mf.models.HistoryTransformerTower(item, max_history=8)
    for path in ("auto", "fused", "forward"):
        with pytest.raises(mf._lib.MfHipError):
            user.encode(torch.zeros(2, 4, dtype=torch.int64), path=path)
        with pytest.raises(mf._lib.MfHipError):
            user.encode((torch.zeros(2, dtype=torch.int64), torch.ones(2, dtype=torch.int64), torch.ones(4, dtype=torch.int64)), path=path)
    with pytest.raises(ValueError, match="path"):
        user.encode(torch.zeros(2, 4, dtype=torch.int64), path="quick")
    mixed = mf.models.HistoryTransformerTower(item, max_history=8, precision="bf16-mixed")
    with pytest.raises(ValueError, match="fp32"):
        mixed.encode(torch.zeros(2, 4, dtype=torch.int64), path="fused")
