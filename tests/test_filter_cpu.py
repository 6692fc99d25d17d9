"""CPU: the host side of filtered retrieval (csrc/mf_filter.hip, ``retrieval.TagFilter``, ``data.item_tag_bits``,
``ItemProcessor.tag_filter``) -- the exports and their argument types, every refusal on calls that never launch (fake pointers
are never dereferenced), the workspace sizes, the kernels' resources from the code object's notes, the numpy spec against
hand-worked rows, and a save without tags."""
from __future__ import annotations

import ctypes
import importlib.util
import json
import pathlib

import numpy as np
import pytest
import torch

from tests import _filter_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
EXPORTS = {"mf_filter_ws_bytes": "size_t", "mf_filter_rows": "int", "mf_filter_remap": "int", "mf_filter_lists_ws_bytes": "size_t",
           "mf_filter_lists": "int", "mf_filter_unmap": "int"}


def test_exports_are_declared_bound_documented_and_present(mf):
    lib, L = mf._lib.lib(), mf._lib
    header = (ROOT / "include" / "mf_hip.h").read_text()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for name, ret in EXPORTS.items():
        assert hasattr(lib, name) and name in L.SIGNATURES and f"{ret} {name}(" in header and name in guide, name
    assert "mf_filter.hip" in (ROOT / "matrix-factorization-torch_amd" / "csrc" / "Makefile").read_text()
    vp, i64, u64, sz = L.c_vp, L.c_i64, L.c_u64, L.c_sz
    assert L.SIGNATURES["mf_filter_ws_bytes"] == (sz, [i64]) and L.SIGNATURES["mf_filter_lists_ws_bytes"] == (sz, [i64])
    assert L.SIGNATURES["mf_filter_rows"] == (L.c_int, [vp, i64, u64, u64, u64, vp, sz, vp, vp, vp, vp])
    assert L.SIGNATURES["mf_filter_remap"] == (L.c_int, [vp, i64, i64, vp, i64, vp, vp])
    assert L.SIGNATURES["mf_filter_lists"] == (L.c_int, [vp, vp, i64, i64, i64, vp, i64, vp, sz, vp, vp, vp])
    assert L.SIGNATURES["mf_filter_unmap"] == (L.c_int, [vp, i64, vp, i64, i64, vp, vp])


# ------------------------------------------------------------------------------------------------------ refusals ----
def _rows(lib, **kw):
    a = dict(tags=FAKE, N=1000, ws=FAKE, ws_bytes=1 << 20, rows=FAKE, rank=FAKE, count=FAKE)
    a.update(kw)
    rc = lib.mf_filter_rows(a["tags"], a["N"], 1, 2, 4, a["ws"], a["ws_bytes"], a["rows"], a["rank"], a["count"], None)
    return rc, (lib.mf_last_error() if rc else b"")


def _remap(lib, **kw):
    a = dict(ids=FAKE, n=10, base=0, rank=FAKE, N=1000, out=FAKE)
    a.update(kw)
    rc = lib.mf_filter_remap(a["ids"], a["n"], a["base"], a["rank"], a["N"], a["out"], None)
    return rc, (lib.mf_last_error() if rc else b"")


def _unmap(lib, **kw):
    a = dict(idx=FAKE, n=10, rows=FAKE, M=100, base=0, out=FAKE)
    a.update(kw)
    rc = lib.mf_filter_unmap(a["idx"], a["n"], a["rows"], a["M"], a["base"], a["out"], None)
    return rc, (lib.mf_last_error() if rc else b"")


def _lists(lib, **kw):
    a = dict(off=FAKE, ids=FAKE, entries=10, Q=4, base=0, rank=FAKE, N=1000, ws=FAKE, ws_bytes=1 << 20, out_off=FAKE, out_ids=FAKE)
    a.update(kw)
    rc = lib.mf_filter_lists(a["off"], a["ids"], a["entries"], a["Q"], a["base"], a["rank"], a["N"], a["ws"], a["ws_bytes"], a["out_off"],
                             a["out_ids"], None)
    return rc, (lib.mf_last_error() if rc else b"")


def test_every_refusal_and_its_code(mf):
    lib, E = mf._lib.lib(), mf._lib
    for call, name, bad in ((_rows, b"mf_filter_rows", [dict(tags=None), dict(ws=None), dict(rows=None), dict(rank=None), dict(count=None),
                                                        dict(N=-1), dict(rank=ctypes.c_void_p(0x1004))]),
                            (_remap, b"mf_filter_remap", [dict(ids=None), dict(rank=None), dict(out=None), dict(n=-1), dict(N=0), dict(N=-5)]),
                            (_unmap, b"mf_filter_unmap", [dict(idx=None), dict(out=None), dict(rows=None), dict(n=-1), dict(M=-1)]),
                            (_lists, b"mf_filter_lists", [dict(off=None), dict(ids=None), dict(rank=None), dict(ws=None), dict(out_off=None),
                                                          dict(out_ids=None), dict(entries=-1), dict(Q=-1), dict(N=0)])):
        for kw in bad:
            rc, msg = call(lib, **kw)
            assert rc == E.MF_EINVAL and name + b": bad argument" in msg, (name, kw, rc, msg)
    for call, kw in ((_rows, dict(N=2**31)), (_remap, dict(N=2**31)), (_unmap, dict(M=2**31)), (_lists, dict(N=2**31)), (_lists, dict(Q=2**31))):
        rc, msg = call(lib, **kw)
        assert rc == E.MF_ENOTSUP and (b"32 bits" in msg or b"exceed one launch" in msg), (kw, rc, msg)
    for call, kw in ((_rows, dict(ws_bytes=lib.mf_filter_ws_bytes(1000) - 1)), (_lists, dict(ws_bytes=lib.mf_filter_lists_ws_bytes(4) - 1))):
        rc, msg = call(lib, **kw)
        assert rc == E.MF_ENOSPC and b"workspace too small" in msg, (kw, rc, msg)
    # a fault further up wins: bad argument, then the range, then the workspace
    assert _rows(lib, tags=None, N=2**31)[0] == E.MF_EINVAL and _rows(lib, N=2**31, ws_bytes=0)[0] == E.MF_ENOTSUP
    assert _lists(lib, off=None, N=2**31)[0] == E.MF_EINVAL and _lists(lib, N=2**31, ws_bytes=0)[0] == E.MF_ENOTSUP


def test_a_zero_count_is_ok_and_launches_nothing(mf):
    lib = mf._lib.lib()               # (fake pointers and no GPU: a launch would fail)
    assert _rows(lib, N=0, ws_bytes=0)[0] == 0 and _remap(lib, n=0)[0] == 0 and _unmap(lib, n=0)[0] == 0 and _lists(lib, Q=0, ws_bytes=0)[0] == 0
    assert _unmap(lib, n=0, rows=None, M=0)[0] == 0


def test_workspace_sizes(mf):
    lib = mf._lib.lib()
    for size in (lib.mf_filter_ws_bytes, lib.mf_filter_lists_ws_bytes):
        assert size(0) == 0 and size(-1) == 0 and size(2**31) == 0 and size(1) > 0 and size(2**31 - 1) > 0
        seen = [size(n) for n in (1, 2, 33, 2047, 2048, 2049, 4097, 5000, 62423, 2**22, 2**31 - 1)]
        assert seen == sorted(seen) and all(s % 256 == 0 for s in seen)
    # two ballot words per wave of 128 rows and a count per 2048 rows; a count per query
    assert lib.mf_filter_ws_bytes(2**22) <= 2**22 // 8 + 2**22 // 2048 * 4 + 512
    assert lib.mf_filter_lists_ws_bytes(1024) == 1024 * 8


def test_the_new_kernels_have_no_spill_and_no_scratch():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    mine = {n: r for n, r in kr.kernel_resources().items() if "filter_" in n and "mf_filter" not in n}
    assert len(mine) == 10, sorted(mine)      # mark x 2, pack, remap x 2, unmap x 2, lists count / scan / write
    for name, r in mine.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


# ---------------------------------------------------------------------------------------------------- TagFilter ----
def test_tag_filter_validation(mf):
    F = mf.retrieval.TagFilter
    f = F(any_of=1, all_of=2, none_of=4)
    assert (f.any_of, f.all_of, f.none_of) == (1, 2, 4) and F() == F(0, 0, 0) and hash(F(1, 2, 4)) == hash(f) and {f: 1}[F(1, 2, 4)] == 1
    assert F(any_of=2**64 - 1, none_of=0).any_of == 2**64 - 1 and F(all_of=np.int64(8)).all_of == 8
    with pytest.raises(Exception):
        f.any_of = 3                                             # frozen
    for kw in (dict(any_of=-1), dict(all_of=2**64), dict(none_of=1.0), dict(any_of="1"), dict(any_of=None), dict(all_of=True),
               dict(all_of=0b110, none_of=0b010)):
        with pytest.raises(ValueError):
            F(**kw)


# ------------------------------------------------------------------------------------------------ item_tag_bits ----
TEXTS = [None,
         '{"title":"Toy Story (1995)","genres":["Animation","Children\'s","Comedy"]}',
         '{"title":"Heat (1995)","genres":["Action","Crime","Thriller"]}',
         "",
         '{"title":"Sabrina (1995)","genres":["Comedy","Romance"]}',
         '{"title":"No genres"}']


def test_item_tag_bits_on_hand_written_texts(mf):
    tags, vocab = mf.data.item_tag_bits(TEXTS)
    assert vocab == ["Action", "Animation", "Children's", "Comedy", "Crime", "Romance", "Thriller"]
    assert tags.dtype == torch.int64 and tags.tolist() == [0, 0b0001110, 0b1010001, 0, 0b0101000, 0]
    assert mf.data.item_tag_bits([None])[0].tolist() == [0] and mf.data.item_tag_bits([None])[1] == []
    titles, names = mf.data.item_tag_bits(TEXTS, field="title")
    assert len(names) == 4 and titles.tolist() == [0, 8, 1, 0, 4, 2]
    many = [None] + [json.dumps({"genres": [f"g{i:02d}"]}) for i in range(64)]
    tags, vocab = mf.data.item_tag_bits(many)
    assert len(vocab) == 64 and int(tags[64]) == -2**63 and int(tags[1]) == 1                 # bit 63 is the sign bit of the word
    with pytest.raises(ValueError, match="at most 64"):
        mf.data.item_tag_bits(many + [json.dumps({"genres": ["one more"]})])
    texts, first = mf.data.synthetic_item_features(50, num_genres=6, seed=1)
    tags, vocab = mf.data.item_tag_bits(texts)
    assert int(tags[0]) == 0 and all(int(tags[i]) >> vocab.index(f"g{int(first[i])}") & 1 for i in range(1, 50))


def test_item_processor_tag_names(mf):
    proc = mf.retrieval.ItemProcessor()
    with pytest.raises(ValueError, match="vocabulary"):
        proc.tag_filter(any_of=["Comedy"])
    tags, vocab = mf.data.item_tag_bits(TEXTS)
    proc.set_tags(tags, vocab)
    F = mf.retrieval.TagFilter
    assert proc.tag_filter(any_of=["Comedy", "Crime"]) == F(any_of=0b11000)
    assert proc.tag_filter(all_of=["Action"], none_of=("Romance", "Romance")) == F(all_of=1, none_of=0b100000)
    assert proc.tag_filter(any_of="Comedy") == F(any_of=0b1000) and proc.tag_filter() == F()
    assert proc._where({"any_of": ["Comedy"]}) == F(any_of=0b1000) and proc._where(F(any_of=1)) == F(any_of=1)
    with pytest.raises(KeyError, match="Western"):
        proc.tag_filter(any_of=["Comedy", "Western"])
    with pytest.raises(ValueError):
        proc.tag_filter(all_of=["Comedy"], none_of=["Comedy"])
    for bad in (tags.to(torch.int32), tags.reshape(2, 3)):
        with pytest.raises(ValueError, match="tags should be"):
            proc.set_tags(bad)
    with pytest.raises(ValueError, match="at most 64"):
        proc.set_tags(tags, [str(i) for i in range(65)])


# ------------------------------------------------------------------------------------------------------ the spec ----
def test_the_spec_on_hand_worked_rows():
    tags = np.array([0b0000, 0b0001, 0b0011, 0b0111, 0b1001, 0b0110, -2**63, -2**63 | 0b0001], dtype=np.int64)
    assert spec.admits(tags, any_of=0b0110, all_of=0b0001, none_of=0b1000).tolist() == [False, False, True, True, False, False, False, False]
    assert spec.admits(tags, all_of=0b0001).tolist() == [False, True, True, True, True, False, False, True]           # any_of = 0: no demand
    assert spec.admits(tags).all()
    assert spec.admits(tags, any_of=1 << 63).tolist() == [False] * 6 + [True, True]
    assert spec.admits(tags, all_of=(1 << 63) | 1).tolist() == [False] * 7 + [True]
    assert spec.admits(tags, none_of=1 << 63).tolist() == [True] * 6 + [False, False]
    ok = spec.admits(tags, all_of=0b0001)
    rows, rank = spec.compact(ok)
    assert rows.tolist() == [1, 2, 3, 4, 7] and rank.tolist() == [-1, 0, 1, 2, 3, -1, -1, 4] and rank.dtype == np.int32
    assert spec.remap([99, 100, 101, 107, 108, 105, 101], 100, rank).tolist() == [-1, -1, 0, 4, -1, -1, 0]
    off, ids = spec.map_lists([0, 3, 3, 7], [100, 101, 104, 99, 102, 102, 108], 100, rank)
    assert off.tolist() == [0, 2, 2, 4] and ids.tolist() == [0, 3, 1, 1]
    assert spec.unmap([4, -1, 0, 2], rows, 100).tolist() == [107, -1, 101, 103]
    assert spec.extended_lists([[5], []], 2, ok, 100) == [[5, 100, 105, 106], [100, 105, 106]]
    assert spec.extended_lists(None, 1, ok, 0) == [[0, 5, 6]]
    empty = spec.compact(np.zeros(4, bool))
    assert empty[0].size == 0 and empty[1].tolist() == [-1] * 4


# ------------------------------------------------------------------------------------------------------ the module ----
def test_a_save_without_tags_writes_no_new_file_and_no_new_key(mf, tmp_path):
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": 10, "num_items": 12, "hidden_size": 32})
    m.configure_model(device="cpu")
    m.save(tmp_path / "plain")
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["processors.json", "towers.safetensors"]
    assert sorted(json.loads((tmp_path / "plain" / "processors.json").read_text())) == ["config", "history"]
    tags, vocab = mf.data.item_tag_bits([None] + ['{"genres":["a","b"]}'] * 11)
    m.set_item_tags(tags, vocab)
    m.save(tmp_path / "tagged")
    assert sorted(p.name for p in (tmp_path / "tagged").iterdir()) == ["item_tags.safetensors", "processors.json", "towers.safetensors"]
    proc = json.loads((tmp_path / "tagged" / "processors.json").read_text())
    assert sorted(proc) == ["config", "history", "item_tag_vocabulary"] and proc["item_tag_vocabulary"] == ["a", "b"]
    assert (tmp_path / "tagged" / "towers.safetensors").read_bytes() == (tmp_path / "plain" / "towers.safetensors").read_bytes()
    proc.pop("item_tag_vocabulary")
    assert json.dumps(proc, indent=2) == (tmp_path / "plain" / "processors.json").read_text()


def test_the_digest_record_shows_no_existing_kernel_changed():
    """profiles/filter_digest_{parent,branch}.json: ``tools/kernel_resources.py --text-digest`` of the parent's library and of
    this one, for the 203 kernels of the four top-k units, mf_ivf.hip and mf_embed.hip (one kernel per line).  The two records
    are equal: same kernels, same instruction text, same resource figures."""
    parent = json.loads((ROOT / "profiles" / "filter_digest_parent.json").read_text())
    branch = json.loads((ROOT / "profiles" / "filter_digest_branch.json").read_text())
    assert len(parent) == 203 and branch == parent and all(len(v["text_sha256"]) == 64 for v in parent.values())
    for unit in ("topk_small_scan_kernel", "bf3_scan_kernel", "topk_deep", "ivf_scan_kernel", "gather_rows_kernel", "select_kernel"):
        assert any(unit in k for k in parent), unit
