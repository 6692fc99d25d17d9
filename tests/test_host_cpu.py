"""CPU: the C ABI loads and exports what include/mf_hip.h declares; host-side logic
(batch layout, error behaviour, no silent CPU fallback)."""
from __future__ import annotations

import pathlib
import re

import pytest
import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_library_exports_every_declared_symbol(mf):
    header = (ROOT / "include" / "mf_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", header))
    assert {"mf_loss_fwd", "mf_loss_bwd", "mf_gather_rows", "mf_update_sgd", "mf_update_adam", "mf_topk",
            "mf_topk_merge", "mf_topk_bf3_plan"} <= declared
    lib = mf._lib.lib()
    for name in declared:
        assert hasattr(lib, name), f"libmf_hip.so lacks {name}"
    assert declared == set(mf._lib.SIGNATURES), declared ^ set(mf._lib.SIGNATURES)
    assert lib.mf_version() >= 100


def test_workspace_queries_need_no_gpu(mf):
    lib = mf._lib.lib()
    assert lib.mf_loss_ws_bytes(8192, 16384, 128, 64, 0) > 2 * 8192 * 16384 * 4  # logits stash + G' stash
    assert lib.mf_loss_ws_bytes(8192, 16384, 128, 64, 4) < 512 * 2**20           # mined: no stash
    assert lib.mf_loss_ws_bytes(4, 2, 128, 0, 0) == 0                            # N < B is invalid
    assert lib.mf_topk_ws_bytes(1024, 62423, 128, 20) > 0
    assert lib.mf_update_ws_bytes(16384, 128) >= 16384 * 128 * 4


def test_descriptor_limits_are_enforced_on_the_host(mf):
    """Tiles are staged through 32-bit buffer descriptors (csrc/mf_stream.h): a workgroup's share of a catalog, and the
    exclusion words of a query block, must stay below ~4 GiB or rows would silently arrive as zeros.  Both
    limits are decided by host arithmetic before any launch, so they are testable without a GPU."""
    import ctypes

    lib = mf._lib.lib()
    rows = ctypes.c_int64()
    # fp32 tile engine: every chunk of every plan fits one descriptor, also when few chunks would do for occupancy
    for q, n, d in ((1024, 62_423, 128), (65_536, 8_400_000, 256), (8_192, 100_000_000, 128), (1, 2_000_000_000, 32)):
        chunks = lib.mf_topk_chunks(q, n, d, 20, ctypes.byref(rows))
        assert chunks >= 1 and rows.value * chunks >= n
        assert rows.value * d * 4 <= 0xFFF00000, (q, n, d, chunks, rows.value)
    assert lib.mf_topk_chunks(65_536, 8_400_000, 256, 20, ctypes.byref(rows)) >= 3       # one chunk would be 8 GiB
    # bf16 prefilter with exclusion lists: a query block's words beyond 4 GiB are refused (MF_ENOTSUP), nothing is launched
    fake = ctypes.c_void_p(0x1000)           # never dereferenced: the geometry check comes first
    n_big = 150_000_000                      # 4.7 M tiles x 256 queries x 4 bytes > 4 GiB
    rc = lib.mf_topk_bf3(fake, 8192, fake, fake, n_big, 64, 20, fake, fake, 0, fake, ctypes.c_size_t(2**62), fake, fake, None)
    assert rc == mf._lib.MF_ENOTSUP and b"exclusion words" in lib.mf_last_error()


def test_mining_prefilter_plan_holds_what_its_kernels_write(mf):
    """The split-bf16 mining prefilter (csrc/mf_mine_bf.h) is planned on the host, and its limits are host arithmetic: the
    rescoring wave's key array must hold the copy-expansion pool (the k winners and, behind the winner at position t, up to
    k - 1 - t copies: k (k + 1) / 2 keys -- more than the lists hold once the batch is large enough for few item chunks),
    its LDS must fit one workgroup, and a scan hit packs its column into 24 bits.  Swept over the batch sizes the default
    mode serves (B >= 4096) up to 2^20, ragged ones included, and catalogs on both sides of 2^24."""
    import ctypes

    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 8)()
    bs = [1 << e for e in range(8, 21)] + [300, 4100, 5000, 12_289, 33_000, 70_001, 131_000, 600_000]
    served = {"near 2^24": 0, "few chunks, k > 16": 0}
    for b in bs:
        for n in (b, 2 * b, (1 << 24) - 32, (1 << 24) + 32):
            for d in (64, 128):
                for k in range(1, 33):
                    assert lib.mf_mining_prefilter_plan(b, n, d, k, out) == 0
                    ok, pays, nchunk, tpc, lpc, nlists, keys_cap, lds = out
                    what = dict(B=b, N=n, d=d, k=k, plan=list(out))
                    assert pays == (ok and b >= 4096), what
                    if n >= 1 << 24:
                        assert not ok, what               # columns would alias in the scan's 24-bit hit words
                    if not ok:
                        continue
                    assert nchunk * tpc * 32 >= n and lpc == (4 if k > 16 else 2) and nlists == lpc * nchunk <= 64, what
                    assert keys_cap >= 16 * nlists + 128 + 1, what          # the lists, the spill list, a diagonal's stand-in
                    assert keys_cap >= k * (k + 1) // 2, what               # the copy-expansion pool
                    assert lds <= 64 * 1024 and lds >= keys_cap * 8, what
                    served["near 2^24"] += n == (1 << 24) - 32
                    served["few chunks, k > 16"] += nchunk < 16 and k > 16
    assert all(served.values()), served                  # (the sweep reaches the cases it is about)
    # the geometries the GPU tests (tests/test_gpu_mining_prefilter.py) rely on
    for b, d, k, nchunk, lpc in ((16_384, 128, 32, 8, 4), (32_768, 64, 32, 4, 4), (65_536, 64, 24, 2, 4), (65_536, 64, 32, 2, 4),
                                 (8_192, 128, 4, 16, 2)):
        assert lib.mf_mining_prefilter_plan(b, b if b > 8192 else 2 * b, d, k, out) == 0
        assert out[0] == 1 and out[2] == nchunk and out[4] == lpc, (b, d, k, list(out))
    assert lib.mf_mining_prefilter_plan(8192, 16384, 32, 4, out) == 0 and out[0] == 0     # d = 32: never served


def test_loss_plan_tells_how_many_tiles_a_workgroup_streams(mf):
    """mf_loss_plan is host arithmetic on the launch geometry of the dense sweeps (split_geometry, as csrc/mf_loss_ws.h
    applies it for the sweeps of csrc/mf_loss_dense.hip).
    What a workgroup does depends on its tile count, so the tests that are about the multi-tile paths
    (tests/test_gpu_dense_sweeps.py) assert through it that they reach them -- and this one, that the dense cases of
    the older tests never did: one tile per workgroup up to Bp * Np = 2^21."""
    import ctypes

    from tests import _dense_cases as dc

    lib = mf._lib.lib()
    for d in dc.WIDTHS:
        for (b, n), (fu, dv, _) in dc.SHAPES.items():
            p = dc.plan(lib, b, n, d)
            nt, bt = -(-n // 128) * 4, -(-b // 128) * 4
            assert p["mined"] == 0 and (p["tps_f"], p["last_f"]) == (p["tps_u"], p["last_u"]) == fu, (b, n, d, p)
            assert (p["tps_v"], p["last_v"]) == dv, (b, n, d, p)
            assert p["nsplit_f"] == p["nsplit_u"] == -(-nt // fu[0]) and p["nsplit_v"] == -(-bt // dv[0]), (b, n, d, p)
        for b, n in dc.OLD_SHAPES + ((64, 64), (4, 8), (33, 95), (100, 260)):
            p = dc.plan(lib, b, n, d)
            assert p["tps_f"] == p["tps_u"] == p["tps_v"] == p["last_f"] == p["last_u"] == p["last_v"] == 1, (b, n, d, p)
        assert dc.plan(lib, 1024, 2048 + 1, d)["tps_f"] == 2                  # the first shape past the threshold
        p = dc.plan(lib, 8192, 16384, d)                                      # the full-size training step
        assert (p["nsplit_f"], p["tps_f"], p["nsplit_v"], p["tps_v"], p["last_f"], p["last_v"]) == (8, 64, 4, 64, 64, 64)
        assert dc.plan(lib, 8192, 16384, d, num_negatives=4)["mined"] == 1    # mining: no dense sweep runs
        assert dc.plan(lib, 8192, 16384, d, num_negatives=16384)["mined"] == 0
    out = (ctypes.c_int64 * 8)()
    for b, n, d in ((4, 2, 128), (0, 8, 64), (-1, 8, 64), (8, 16, 48)):      # what mf_loss_ws_bytes answers with 0; a bad width
        assert lib.mf_loss_plan(b, n, d, 0, out) == mf._lib.MF_EINVAL and b"mf_loss_plan" in lib.mf_last_error(), (b, n, d)
    assert lib.mf_loss_ws_bytes(4, 2, 128, 0, 0) == 0 and lib.mf_loss_ws_bytes(0, 8, 64, 0, 0) == 0
    assert lib.mf_loss_plan(8, 16, 64, 0, None) == mf._lib.MF_EINVAL


def test_no_product_kernel_spills():
    """vgpr_spill_count == 0 and no scratch for every kernel of the training step, its set-up and the retrieval paths
    (read from the code objects' notes: tools/kernel_resources.py).  Spills in update_fused_kernel<*, Adam> and
    prep_kernel<256> went unnoticed for a round."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = kr.kernel_resources()
    assert len(res) > 100
    watched = ("loss_fwd_dense_kernel", "loss_bwd_dense_kernel", "select_kernel", "select_seed_kernel", "gather_rows_kernel",
               "gather_hashed_kernel", "update_fused_kernel", "update_rows_kernel", "prep_kernel", "finish_kernel", "sum_parts_kernel",
               "hits_kernel", "gt_insert_kernel", "mask_sweep_kernel", "mined_rows_kernel", "mined_bwd_kernel", "topk_small_scan_kernel",
               "topk_small_select_kernel", "bf3_scan_kernel", "bf3_bound_kernel", "step_small_kernel")
    seen = set()
    for name, r in res.items():
        hit = [w for w in watched if w in name]
        if not hit:
            continue
        seen.update(hit)
        # (SGPR "spills" go to VGPR lanes -- v_writelane / v_readlane, no memory: the one-query scan keeps a whole query
        # in scalar registers on purpose -- so the bar is: no VGPR spill and not a byte of scratch)
        if "step_small_kernel" in name:
            # one workgroup of 1024 threads (128 registers per lane) running every phase of a step: latency-bound by design;
            # its Adam variants keep <= 8 registers in scratch around the inlined update body (the SGD variants none)
            assert r["vgpr_spill_count"] <= 8 and r["private_segment_fixed_size"] <= 32, (name, r)
            continue
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert {"loss_fwd_dense_kernel", "loss_bwd_dense_kernel", "update_fused_kernel", "prep_kernel", "bf3_scan_kernel"} <= seen


def test_no_cpu_fallback(mf):
    """The product path raises on CPU tensors instead of computing somewhere else."""
    fn = mf.losses.InfomationNoiseContrastiveEstimationLoss()
    with pytest.raises(mf.MfHipError, match="no CPU path"):
        fn(torch.randn(4, 32), torch.randn(8, 32), torch.ones(4), item_idx=torch.arange(8), pos_idx=None)
    with pytest.raises(mf.MfHipError):
        mf.retrieval.ItemIndex(torch.randn(10, 32))


def test_check_inputs_raise_like_reference(mf):
    fn = mf.losses.PairwiseHingeLoss(num_negatives=4, sigma=2.0, margin=0.5)
    assert (fn.num_negatives, fn.sigma, fn.margin) == (4, 2.0, 0.5)
    u, v = torch.randn(4, 32), torch.randn(8, 32)
    with pytest.raises(ValueError, match="2 dimensions"):
        fn(u[0], v, torch.ones(4), item_idx=torch.arange(8), pos_idx=None)
    with pytest.raises(ValueError, match="dimension 1"):
        fn(u, v[:, :16], torch.ones(4), item_idx=torch.arange(8), pos_idx=None)
    with pytest.raises(ValueError, match="dimension 0"):
        fn(u, v, torch.ones(5), item_idx=torch.arange(8), pos_idx=None)


def test_losses_the_kernels_do_not_know_are_refused(mf):
    """Upstream a subclass supplies its own phi through ``score_loss_fn`` (xfmr_rec/losses.py:342,348-359) or its own
    ``loss`` (:81-90); here the seven are compiled code.  A renamed subclass of a known loss is that loss; anything whose
    arithmetic the kernels cannot honour raises NotImplementedError naming the class -- before any GPU work."""
    L = mf.losses

    class Renamed(L.PairwiseHingeLoss):
        pass

    class OwnPhi(L.PairwiseEmbeddingLoss):
        def score_loss_fn(self, score):
            return score.exp()

    class OverriddenPhi(L.PairwiseLogisticLoss):
        def score_loss_fn(self, score):
            return score.relu() ** 2

    class Foreign(L.EmbeddingLoss):
        pass

    assert Renamed(num_negatives=4).kind == L.KINDS.index("PairwiseHingeLoss")
    u, v = torch.randn(4, 32), torch.randn(8, 32)
    for cls, text in ((OwnPhi, "not one of the seven"), (Foreign, "not one of the seven"), (OverriddenPhi, "score_loss_fn differs")):
        with pytest.raises(NotImplementedError, match=text):
            cls()(u, v, torch.ones(4), item_idx=torch.arange(8), pos_idx=None)
    patched = L.PairwiseHingeLoss()
    patched.score_loss_fn = lambda score: score * 0
    with pytest.raises(NotImplementedError, match="score_loss_fn differs"):
        patched(u, v, torch.ones(4), item_idx=torch.arange(8), pos_idx=None)

    class TorchLoss(L.EmbeddingLoss):                      # the upstream extension point that still works: plain torch code
        def loss(self, user_embed, item_embed, target, **_):
            return (user_embed.sum() + item_embed.sum()) * target.sum()

    assert float(TorchLoss()(u, v, torch.ones(4), item_idx=torch.arange(8))) == pytest.approx(float((u.sum() + v.sum()) * 4))


def test_loss_class_names_and_order(mf):
    module = mf.lightning.MatrixFactorizationLitModule({"num_users": 10, "num_items": 10, "hidden_size": 32})
    with pytest.raises(ValueError, match="`loss_fns` must be initialised first"):
        module.compute_losses({})
    with pytest.raises(ValueError, match="`model` must be initialised first"):
        module(torch.zeros(1, dtype=torch.long))
    names = [type(f).__name__ for f in module.get_loss_fns()]
    assert names == list(mf.losses.KINDS)
    assert module.config.train_loss == "PairwiseHingeLoss" and module.config.num_negatives == 4
    assert module.config.learning_rate == 1e-4 and module.config.top_k == 20


@pytest.mark.parametrize(
    ("batch_sizes", "dim", "pad_start", "expected_size"),
    [
        ([(1,), (3,)], 0, False, (2, 3)), ([(1,), (3,)], -1, False, (2, 3)),
        ([(3, 2), (5, 2)], 0, False, (2, 5, 2)), ([(2, 3), (2, 5)], 1, False, (2, 2, 5)),
        ([(2, 3), (2, 5)], -1, False, (2, 2, 5)), ([(3, 2), (5, 2)], -2, False, (2, 5, 2)),
        ([(1,), (3,)], 0, True, (2, 3)), ([(1,), (3,)], -1, True, (2, 3)),
        ([(3, 2), (5, 2)], 0, True, (2, 5, 2)), ([(2, 3), (2, 5)], 1, True, (2, 2, 5)),
        ([(2, 3), (2, 5)], -1, True, (2, 2, 5)), ([(3, 2), (5, 2)], -2, True, (2, 5, 2)),
    ],
)
def test_pad_tensors(mf, batch_sizes, dim, pad_start, expected_size):
    """The reference's only unit test (tests/data/test_load.py:5-29: 12 shape cases), plus values."""
    batch = [torch.rand(size) + 1.0 for size in batch_sizes]
    padded = mf.data.pad_tensors(batch, dim=dim, pad_start=pad_start)
    assert padded.size() == expected_size
    small = batch[0]
    region = padded[0]
    sl = [slice(None)] * region.dim()
    n = small.size(dim)
    sl[dim % region.dim()] = slice(region.size(dim) - n, None) if pad_start else slice(0, n)
    assert torch.equal(region[tuple(sl)], small) and int((region != 0).sum()) == small.numel()


def test_collate_and_synthetic_batches(mf):
    ex = [{"target": 5, "user": {"idx": 1, "pos_idx": [4, 9, 2]}, "item": {"idx": 4}, "neg_item": {"idx": 7}},
          {"target": 1, "user": {"idx": 2, "pos_idx": [3]}, "item": {"idx": 3}, "neg_item": {"idx": 8}}]
    b = mf.data.collate_interactions(ex)
    assert b["user"]["pos_idx"].tolist() == [[4, 9, 2], [3, 0, 0]] and b["target"].dtype == torch.int64
    syn = mf.data.SyntheticInteractions(100, 50, max_positives=8, seed=1).batch(16)
    assert syn["user"]["pos_idx"].shape == (16, 8) and (syn["user"]["pos_idx"][:, 0] == syn["item"]["idx"]).all()
    assert int(syn["item"]["idx"].min()) >= 1 and int(syn["neg_item"]["idx"].max()) < 50


def test_hash_bucket_known_answer_and_range():
    """The hash of the bloom towers is pinned by SplitMix64's published first output (state 0)."""
    from oracle import embed as oembed

    assert int(oembed.hash_buckets(torch.tensor([0]), 1, 0, 1 << 62)[0, 0]) == 0xE220A8397B1DCDAF % (1 << 62)
    ids = torch.tensor([0, 1, 2, 62_423, 10**12, -5])
    b = oembed.hash_buckets(ids, 3, 7, 1000)
    assert b.shape == (6, 3) and int(b.min()) >= 0 and int(b.max()) < 1000
    assert len({tuple(r) for r in b.tolist()}) == 6          # distinct ids -> distinct bucket triples here
    assert torch.equal(b, oembed.hash_buckets(ids, 3, 7, 1000))


def test_oracle_retrieval_metrics_hand_example():
    """k = 4, retrieved [7, 3, 9, 5]; targets {3: 5, 5: 2, 8: 4} (8 was missed)."""
    from oracle import retrieval as oretr

    m = oretr.retrieval_metrics(np.array([[7, 3, 9, 5]]), [{3: 5.0, 5: 2.0, 8: 4.0}], 4)[0]
    dcg = 5 / np.log2(3) + 2 / np.log2(5)
    idcg = 5 / np.log2(2) + 4 / np.log2(3) + 2 / np.log2(4)
    want = [dcg / idcg, 2 / 3, 2 / 4, (1 / 2 + 2 / 4) / 2, 1.0, 1 / 2]
    assert np.allclose(m, want)
    assert not oretr.retrieval_metrics(np.array([[1, 2, 3, 4]]), [{}], 4).any()          # no target: all 0


def test_metric_convention_for_unretrieved_targets_and_where_it_differs_from_the_reference():
    """The reference scores a target the search did NOT retrieve with -U(0, 1) (xfmr_rec/lightning.py:170-175) and lets
    torchmetrics rank everything by score; here (oracle.retrieval.retrieval_metrics, mf_retrieval_metrics) an unretrieved target
    ranks below every retrieved item.  The two agree for ANY draw whenever every retrieved score is >= 0 (cosine scores of the
    top k of a trained model); they can differ when a retrieved score is negative -- a tiny catalog, or untrained towers --
    because the reference may then lift a missed target above a retrieved item.  Pinned here so that nobody reads the numbers
    of such a run as the reference's ("deviations")."""
    from oracle import retrieval as oretr

    def reference_convention(scores, idx, tgt, k, draws):
        """HitRate@k and Recall@k under the reference's scoring: retrieved items keep their scores, missed targets get -draw."""
        pred = {int(i): float(s) for i, s in zip(idx, scores)}
        missed = [i for i in tgt if i not in pred]
        for i, u in zip(missed, draws):
            pred[i] = -float(u)
        order = sorted(pred, key=lambda i: -pred[i])[:k]
        hits = sum(1 for i in order if tgt.get(i, 0) > 0)
        return float(hits > 0), hits / sum(1 for v in tgt.values() if v > 0)

    k, idx, tgt = 4, np.array([7, 3, 9, 5]), {3: 5.0, 8: 4.0}          # 8 was missed
    ours = oretr.retrieval_metrics(idx[None, :], [tgt], k)[0]
    for draws in ([0.01], [0.5], [0.99]):                                # every retrieved score >= 0: the same for any draw
        hr, rec = reference_convention([0.9, 0.5, 0.2, 0.0], idx, tgt, k, draws)
        assert hr == ours[4] and rec == ours[1]
    # negative retrieved scores: a draw of 0.05 puts the missed target 8 above the retrieved item 5 (score -0.3)
    hr, rec = reference_convention([0.9, 0.5, -0.1, -0.3], idx, tgt, k, [0.05])
    assert rec == 1.0 and ours[1] == 0.5                                 # the documented deviation: ours never promotes a missed target


def test_oracle_epoch_permutation_is_a_bijection():
    from oracle import data as odata

    for n in (1, 2, 7, 100, 1000):
        for epoch in (0, 1):
            assert sorted(odata.feistel_perm(x, n, epoch, 9) for x in range(n)) == list(range(n))
    assert [odata.feistel_perm(x, 100, 0, 9) for x in range(100)] != [odata.feistel_perm(x, 100, 1, 9) for x in range(100)]


def test_interaction_table_split_and_histories_match_the_reference_semantics():
    """data.split_ratings / InteractionTable against a plain-Python restatement of the reference's polars expressions
    (train_test_split, prepare.py:160-194; gather_history's rolling 4-week window, :229-243; process_users' per-user
    history / target, :272-310) on ratings with timestamp ties, single-rating users and bursts inside one window."""
    import importlib

    from oracle import data as odata

    mf_data = importlib.import_module("matrix-factorization-torch_amd.data")
    g = torch.Generator().manual_seed(0)
    n_users, n_items, n = 23, 40, 400
    user = torch.randint(1, n_users, (n,), generator=g)
    user[:3] = torch.tensor([20, 21, 22])                           # three users with a single rating
    user[user >= 20] = torch.where(torch.arange(n)[user >= 20] < 3, user[user >= 20], torch.tensor(1))
    item = torch.randint(1, n_items, (n,), generator=g)
    rating = torch.randint(1, 6, (n,), generator=g)
    ts = 978_300_000 + torch.randint(0, 20 * 7 * 24 * 3600, (n,), generator=g)
    ts[50:60] = ts[50]                                              # ties in time (also across users)
    ts[100:140] = ts[100] + torch.arange(40) * 3600                 # a burst inside one 4-week window
    tab = mf_data.InteractionTable(user, item, rating, ts)
    want_train, want_val, want_test = odata.split_ratings(user.tolist(), ts.tolist())
    assert tab.is_train.tolist() == want_train and tab.is_val.tolist() == want_val and tab.is_test.tolist() == want_test
    assert 0.7 < sum(want_train) / n < 0.9 and any(want_val) and any(want_test)
    # rolling history of every rating (as sets: the reference's window has no order among equal timestamps)
    hist = odata.rolling_history(user.tolist(), item.tolist(), ts.tolist(), mf_data.FOUR_WEEKS)
    order = tab.order.tolist()
    for pos, r in enumerate(order):
        got = tab.sorted_item[int(tab.history_lo[pos]): int(tab.history_hi[pos])].tolist()
        assert sorted(got) == sorted(hist[r]), (pos, r)
    # train pairs + positives: a user's pos list = its train items
    for u in range(n_users):
        mine = sorted(int(item[r]) for r in range(n) if int(user[r]) == u and want_train[r])
        assert sorted(tab.pos_items[int(tab.pos_off[u]): int(tab.pos_off[u + 1])].tolist()) == mine
    assert tab.pair_user.numel() == sum(want_train)
    # evaluation sets (process_users): history = train items, target = non-train items + ratings, per val / test user
    for split, flags in (("val", want_val), ("test", want_test)):
        users, (h_off, h_items), (t_off, t_items, t_rating) = tab.eval_sets(split)
        assert users.tolist() == sorted({int(user[r]) for r in range(n) if flags[r]})
        for s_, u in enumerate(users.tolist()):
            assert sorted(h_items[int(h_off[s_]): int(h_off[s_ + 1])].tolist()) == sorted(int(item[r]) for r in range(n) if int(user[r]) == u and want_train[r])
            tg = sorted((int(item[r]), float(rating[r])) for r in range(n) if int(user[r]) == u and not want_train[r])
            assert sorted(zip(t_items[int(t_off[s_]): int(t_off[s_ + 1])].tolist(), t_rating[int(t_off[s_]): int(t_off[s_ + 1])].tolist())) == tg


def test_bench_starts_its_own_ranks_and_reports_them():
    """`python bench.py --gpus 2` with no launcher around it: two fresh child processes (started before any GPU call), one
    JSON line with n_gpus = 2 and the transport fields; a rank count that differs from --gpus is an error, never a smaller
    job timed under the bigger name (--gpus used to be parsed and ignored).  Runs the launch / barrier /
    max-over-ranks plumbing on CPU (MF_BENCH_DRY_RUN: gloo, stub step, no kernels)."""
    import json
    import os
    import subprocess
    import sys

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["MF_BENCH_DRY_RUN"] = "1"
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout                       # rank 0 prints, rank 1 does not
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 4 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert {"metric", "value", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "config", "rccl_ranks",
            "transport"} <= set(line)
    # a failed RCCL self-test: every rank hands over to a FRESH child of itself on torch's collectives (new rendezvous port,
    # MF_COMM=torch) and exits with its code -- no continuation in the process whose RCCL is in an unknown state; one JSON
    # line, carrying the note (simulated on the CPU plumbing)
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                         env=dict(env, MF_BENCH_FAKE_COMM_FAILURE="1"), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    assert json.loads(lines[0])["n_gpus"] == 2 and "self-test failed" in json.loads(lines[0])["comm_note"]
    assert res.stderr.count("restarting this rank in a fresh process") == 2
    # under a launcher whose world differs from --gpus: exit 2, nothing printed
    bad = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="3", RANK="0"),
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "WORLD_SIZE=3" in bad.stderr and not bad.stdout.strip()
    # more ranks than GPUs (none here): refused before anything starts
    env.pop("MF_BENCH_DRY_RUN")
    if not torch.cuda.is_available():
        none = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120)
        assert none.returncode == 2 and "visible" in none.stderr


def test_movielens_ratings_reader(mf, tmp_path):
    """ids-only reader of the reference's inputs (xfmr_rec/data/prepare.py:132-152 reads ml-1m/ratings.dat; ml-25m ships
    ratings.csv): both layouts give the same interaction table; movie_rn / user_rn follow the side files' order."""
    rows = [(1, 10, 5, 100), (1, 30, 3, 200), (1, 20, 4, 300), (1, 50, 2, 400), (1, 40, 1, 500),
            (2, 30, 4, 150), (2, 10, 2, 250), (7, 50, 5, 50), (7, 20, 3, 60), (7, 30, 1, 70), (7, 10, 4, 80), (7, 40, 2, 90)]
    d1 = tmp_path / "ml-1m"
    d1.mkdir()
    (d1 / "ratings.dat").write_text("".join(f"{u}::{m}::{r}::{t}\n" for u, m, r, t in rows))
    (d1 / "movies.dat").write_text("".join(f"{m}::Title {m} (1999)::Drama|Comedy\n" for m in (10, 20, 25, 30, 40, 50)), encoding="iso-8859-1")
    (d1 / "users.dat").write_text("".join(f"{u}::F::25::3::12345\n" for u in (1, 2, 5, 7)))
    d2 = tmp_path / "ml-25m"
    d2.mkdir()
    (d2 / "ratings.csv").write_text("userId,movieId,rating,timestamp\n" + "".join(f"{u},{m},{r}.0,{t}\n" for u, m, r, t in rows))
    assert mf.data.find_movielens(tmp_path) == d2 / "ratings.csv"
    assert mf.data.find_movielens(d1.parent / "ml-1m") == d1 / "ratings.dat"
    raw = mf.data.read_ratings(d1 / "ratings.dat")
    assert raw["user_id"].tolist() == [r[0] for r in rows] and raw["rating"].dtype == torch.float32
    t1, m1 = mf.data.movielens_interactions(d1 / "ratings.dat")
    t2, m2 = mf.data.movielens_interactions(d2 / "ratings.csv")
    # side files: movie 25 has no rating but owns row 3; user 5 owns row 3
    assert (m1["num_items"], m1["num_users"]) == (7, 5) and (m2["num_items"], m2["num_users"]) == (6, 4)
    rn1 = {10: 1, 20: 2, 30: 4, 40: 5, 50: 6}
    assert sorted(t1.pair_item.tolist()) == sorted(rn1[m] for (u, m, r, t), tr in zip(rows, t1.is_train.tolist()) if tr)
    assert torch.equal(t1.is_train, t2.is_train) and torch.equal(t1.pos_off[[1, 2]], t2.pos_off[[1, 2]])
    # user 1: 5 ratings in time order 10, 30, 20, 50, 40 -> the first 80 % are train
    assert t1.pos_items[t1.pos_off[1]: t1.pos_off[2]].tolist() == [rn1[10], rn1[30], rn1[20], rn1[50]]
