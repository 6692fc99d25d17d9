#!/usr/bin/env python3
"""Times the transformer user tower (models.HistoryTransformerTower) at the history probe's world: the ML-25M-shaped
synthetic InteractionTable of tools/history_probe.py, batches of B = 8192 history windows.

    python tools/xfmr_probe.py [--out profiles/xfmr_probe.json] [--ratings 25000000]
    MF_HIP_LIB=path/to/parent/libmf_hip.so python tools/xfmr_probe.py --baseline-only --out profiles/xfmr_probe_parent.json

For (d, L, I) in (64, 32, 64), (128, 32, 128), (128, 64, 512), one layer, 4 heads, mean pooling: the step time (InfoNCE over
the batch's items, CSR positives, RowAdam on the table + AdamW on the encoder, through optim.TowerOptimizer), medians of
three timed regions after warm-up, and the mf_timing spans of the forward, the backward, the coalesce, the GEMM launches and
the attention.  For the GEMM spans: achieved fp32 matrix rate from the algorithmic flops 2 T (4 h^2 + 2 h I) per layer
forward, twice that backward, against 157.3 TFLOP/s.  Next to it the same step with user_tower="history" (mean);
``--baseline-only`` measures only that one, so that it can run against another build of the library (MF_HIP_LIB), whose
missing mf_xfmr_* exports are then left unbound.

    python tools/xfmr_probe.py --transformer-only --repeat 3 --dropout 0.1 0.1 --out profiles/xfmr_dropout_probe.json
    MF_HIP_LIB=path/to/parent/libmf_hip.so python tools/xfmr_probe.py --transformer-only --repeat 3 --out parent.json

``--dropout P_HIDDEN P_ATTN`` adds, per shape, the same step with the tower's training dropout (its spans, and the share of
the step that dropout adds: mask generation, the masked multiplies and the backward's masked copy); ``--repeat N`` repeats
every step measurement N times (``ms_per_step_runs``: the spread that a comparison between two libraries has to respect);
``--transformer-only`` skips the history-tower steps.  A library without the dropout exports (the parent commit's) still runs
the p = 0 step: the exports it lacks are left unbound.

    python tools/xfmr_probe.py --transformer-only --repeat 3 --precision bf16-mixed --out mixed.json

``--precision`` (default fp32) is passed to the tower; the GEMM spans' rate stays the algorithmic flops over the span time,
and its fraction stays the one of the fp32 matrix peak, so that the two precisions read on one scale.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import importlib.util
import json
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
_spec = importlib.util.spec_from_file_location("history_probe", ROOT / "tools" / "history_probe.py")
hp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(hp)

SHAPES = ((64, 32, 64), (128, 32, 128), (128, 64, 512))
PEAK_TFLOPS = 157.3
SPANS = ("xfmr_forward", "xfmr_backward", "xfmr_coalesce", "xfmr_gemm_fwd", "xfmr_gemm_bwd", "xfmr_attn_fwd", "xfmr_attn_bwd",
         "pool_forward", "pool_backward", "update_rows")


def median_ms(fn, regions: int = 3, warmup: int = 10, iters: int = 10) -> float:
    hp.time_ms(fn, warmup=warmup, iters=2)
    return statistics.median(hp.time_ms(fn, warmup=0, iters=iters) for _ in range(regions))


def spans(mf, lib, step, steps: int = 6) -> dict:
    lib.mf_timing_reset()
    lib.mf_timing_enable(1)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    lib.mf_timing_enable(0)
    out = {}
    for name in SPANS:
        tot = ctypes.c_double(0.0)
        n = lib.mf_timing_get(name.encode(), ctypes.byref(tot))
        if n:
            out[name] = {"spans_per_step": n / steps, "ms_per_step": tot.value / steps}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "xfmr_probe.json"))
    ap.add_argument("--ratings", type=int, default=25_000_000)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--transformer-only", action="store_true")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--dropout", type=float, nargs=2, metavar=("P_HIDDEN", "P_ATTN"))
    ap.add_argument("--precision", choices=("fp32", "bf16-mixed"), default="fp32")
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    have = ctypes.CDLL(str(mf._lib.LIB_PATH))   # another build of the library may not have the newest exports
    new = lambda n: "dropout" in n or "mixed" in n or "xfmr_dense" in n or "xfmr_encode" in n or (args.baseline_only and n.startswith("mf_xfmr_"))  # noqa: E731
    missing = [n for n in mf._lib.SIGNATURES if new(n) and not hasattr(have, n)]
    for name in missing:
        del mf._lib.SIGNATURES[name]
    if args.dropout and missing:
        raise SystemExit(f"--dropout needs the dropout exports, which {mf._lib.LIB_PATH} lacks")
    if args.precision != "fp32" and missing:
        raise SystemExit(f"--precision {args.precision} needs the mixed exports, which {mf._lib.LIB_PATH} lacks")
    lib = mf._lib.lib()
    torch.manual_seed(0)
    table = hp.synthetic_table(mf, args.ratings)
    sampler = table.sampler(num_items=hp.ITEMS, batch_size=hp.B, seed=0, device="cuda", history=True)
    batches = [sampler.batch(i) for i in range(8)]
    res = {"library": str(mf._lib.LIB_PATH), "shape": {"items": hp.ITEMS, "batch": hp.B, "ratings": int(table.sorted_user.numel())},
           "cases": []}
    loss_fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)
    variants = [("history", None)] * (not args.transformer_only) + [("transformer", None)] * (not args.baseline_only)
    if args.dropout and not args.baseline_only:
        variants.append(("transformer", tuple(args.dropout)))
    for d, L, inter in SHAPES:
        plain = None
        for user_tower, dropout in variants:
            kw = {"hidden_dropout_prob": dropout[0], "attention_probs_dropout_prob": dropout[1]} if dropout else {}
            if user_tower == "transformer" and args.precision != "fp32":
                kw["precision"] = args.precision
            cfg = mf.models.ModelConfig(num_items=hp.ITEMS, hidden_size=d, user_tower=user_tower, max_history=L, intermediate_size=inter,
                                        num_hidden_layers=1, num_attention_heads=4, **kw)
            towers = mf.models.init_towers(cfg, device="cuda")
            if user_tower == "transformer":
                opt = mf.optim.tower_optimizer(towers, "adam", 1e-3)
                opt.sparse.init_state()
            else:
                opt = mf.optim.RowAdam(towers.parameters(), lr=1e-3)
                opt.init_state()
            k = [0]

            def step():
                bt = batches[k[0] % len(batches)]
                k[0] += 1
                u = towers["user"](bt["user"]["history"])
                idx = torch.cat([bt["item"]["idx"], bt["neg_item"]["idx"]])
                loss = loss_fn(u, towers["item"](idx), bt["target"], item_idx=idx, pos_csr=bt["user"]["pos_csr"])
                loss.backward()
                opt.step()
                opt.zero_grad()

            runs = [median_ms(step) for _ in range(max(1, args.repeat))]
            case = {"user_tower": user_tower, "d": d, "L": L, "I": inter, "ms_per_step": statistics.median(runs), "ms_per_step_runs": runs,
                    "spans": spans(mf, lib, step)}
            if user_tower == "transformer":
                case["precision"] = args.precision
            if user_tower == "transformer" and dropout is None:
                plain = case
            if dropout:
                case["dropout"] = {"hidden_dropout_prob": dropout[0], "attention_probs_dropout_prob": dropout[1]}
                if plain:
                    case["dropout"]["share_of_step_added_by_dropout"] = 1.0 - plain["ms_per_step"] / case["ms_per_step"]
                    for name in ("xfmr_forward", "xfmr_backward"):
                        case["dropout"][f"{name}_ms_added"] = case["spans"][name]["ms_per_step"] - plain["spans"][name]["ms_per_step"]
            if user_tower == "transformer":
                st, en, items = batches[0]["user"]["history"]
                valid = (items >= 1) & (items < hp.ITEMS)
                csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), valid.cumsum(0)])
                tokens = float(torch.stack([(csum[en] - csum[st]).clamp(max=L) for _ in (0,)]).sum())
                flops = 2.0 * tokens * (4 * d * d + 2 * d * inter)
                case["tokens_batch0"] = tokens
                for name, mult in (("xfmr_gemm_fwd", 1.0), ("xfmr_gemm_bwd", 2.0)):
                    if name in case["spans"]:
                        tf = mult * flops / (case["spans"][name]["ms_per_step"] * 1e-3) / 1e12
                        case["spans"][name]["achieved_TFLOPs"] = tf
                        case["spans"][name]["fraction_of_fp32_matrix_peak"] = tf / PEAK_TFLOPS
            res["cases"].append(case)
            print(json.dumps(case))
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=2))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
