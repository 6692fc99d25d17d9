"""``MatrixFactorizationLitModule`` on the HIP hot path.

Mirrors the surface of ``xfmr_rec/lightning.py`` that the training loop touches:
``MatrixFactorizationLitConfig`` (:32-43, same defaults), ``forward`` (:60-74),
``recommend`` (:76-95), ``compute_losses`` (:97-147, same ``"{step}/{ClassName}"`` keys,
all seven losses per step), ``training_step`` (:189-192), ``configure_optimizers``
(:238-239), ``configure_model`` / ``get_loss_fns`` (:252-287) and the
``"... must be initialised first"`` guards (:61-63, :85-87, :100-102).

Differences, all dictated by the north-star: towers are embedding tables indexed by
``user_rn`` / ``movie_rn`` (``forward(idx, tower=...)`` instead of ``forward(text)``),
the optimiser is a sparse row optimiser, retrieval is exact brute force.  The class
derives from ``lightning.LightningModule`` when Lightning is installed (it is not in the
build image) and from ``torch.nn.Module`` otherwise, so ``Trainer.fit`` can drive it
unchanged where Lightning exists.  The retrieval metrics (``validation_step`` / ``test_step`` /
``predict_step``, on the device), ``save`` / ``load`` and the two id-based serving entry points ARE
implemented; callbacks, loggers and the CLI are the reference's control
plane and stay out of scope.
"""
from __future__ import annotations

import contextlib

import pydantic
import torch

from . import losses as mf_losses
from . import fused, models, optim
from .logq import StreamingLogQ
from .params import INDEX_PATH, LOGQ_PATH, PROCESSORS_JSON, TOP_K, TOWERS_PATH
from .retrieval import MERGE_DEEP_MAX_KEYS, ItemProcessor, PartitionedIndex, PositionMetrics, QuantizedIndex, RetrievalMetrics

FEATURE_BAGS_PATH = "feature_bags.safetensors"     # the feature towers' registered bags (save / load)
ITEM_TAGS_PATH = "item_tags.safetensors"           # the items' tag words, written only when tags are set

try:  # pragma: no cover - Lightning is absent from the build image
    from lightning import LightningModule as _Base
except ImportError:  # noqa: SIM105
    class _Base(torch.nn.Module):
        """Minimal stand-in: what this module uses of LightningModule."""

        def log_dict(self, *_, **__) -> None:
            return None

        @property
        def device(self) -> torch.device:
            return next(self.parameters()).device


METRICS_MODES = ("topk", "positions")
LOGQ_MODES = ("table", "streaming")


class MatrixFactorizationLitConfig(models.ModelConfig):
    hidden_size: int = 32          # xfmr_rec/lightning.py:33
    train_loss: str = "PairwiseHingeLoss"
    num_negatives: int = 4
    sigma: float = 1.0
    margin: float = 1.0
    learning_rate: float = 0.0001
    top_k: int = TOP_K
    optimizer: str = "adam"        # "adam" = row-wise AdamW (the reference's optimiser class), "sgd", "adagrad" = row-wise Adagrad
    fused_losses: bool = True      # all seven losses from one sweep instead of seven sweeps
    use_logq: bool = False         # logQ correction (absent upstream)
    # "topk": the metrics read a top_k list (top_k <= 1024); "positions": they read every target's exact place in the catalog
    # (ItemIndex.positions) -- any top_k, further cut-offs eval_ks in the same pass, and uncut MRR / MeanPosition / AUC
    metrics_mode: str = "topk"
    eval_ks: list[int] | None = None      # with "positions": cut-offs beside top_k (logged as name@k)
    # "table": the module's ``logq`` is assigned by the caller (logq.logq_from_counts); "streaming": logq.StreamingLogQ estimates
    # it from the training batches' item columns, on the device (needs use_logq)
    logq_mode: str = "table"
    logq_alpha: float = 0.01       # the estimator's step size: an error shrinks by 1 - alpha per sighting (a default, not tuned)
    logq_buckets: int = 0          # 0: direct, one bucket per item row; > 0: hashed into that many buckets per hash
    logq_hashes: int = 2           # 1..4, read only when logq_buckets > 0
    # the item index ``ItemProcessor`` builds: "exact" scans the catalog; "partitioned" = retrieval.PartitionedIndex, the
    # reference's inverted file (data/lightning.py:203, 222-229): num_partitions cells (None: its default for the catalog's
    # size), num_probes visited per query, k-means seeded with index_seed; "quantized" = retrieval.QuantizedIndex, those cells
    # with the reference's product quantiser and refine (:162-165, 203-204): num_sub_vectors codes per row (None: the stored
    # width // 8), refine_factor * top_k candidates scored exactly.  The saved files are the same whichever it is
    index_type: str = "exact"
    num_partitions: int | None = None
    num_probes: int = 8
    index_seed: int = 0
    num_sub_vectors: int | None = None
    refine_factor: int = 4
    # how recommend*(where=...) filters: "view" = a cached copy of the admissible rows (a quantised index refuses it), "mask" = an
    # allow bitmap the cell scans read in place (partitioned and quantised indexes)
    filter_mode: str = "view"

    @pydantic.model_validator(mode="after")
    def _index_fields(self):
        if self.index_type not in ItemProcessor.INDEX_TYPES:
            msg = f"index_type must be 'exact', 'partitioned' or 'quantized': {self.index_type!r}"
            raise ValueError(msg)
        ItemProcessor.check_filter_mode(self.filter_mode, self.index_type)
        if self.num_sub_vectors is not None and self.num_sub_vectors < 1:
            msg = f"num_sub_vectors must be None (the stored width // 8) or at least 1: {self.num_sub_vectors}"
            raise ValueError(msg)
        if not 1 <= self.refine_factor <= QuantizedIndex.MAX_CANDIDATES:
            msg = f"refine_factor must be in 1..{QuantizedIndex.MAX_CANDIDATES}: {self.refine_factor}"
            raise ValueError(msg)
        if self.index_type == "quantized" and self.top_k <= QuantizedIndex.TILE_MAX_K:
            if self.refine_factor * self.top_k > QuantizedIndex.MAX_CANDIDATES:
                msg = (f"a quantized index refines at most {QuantizedIndex.MAX_CANDIDATES} candidates per query: "
                       f"refine_factor * top_k = {self.refine_factor * self.top_k}")
                raise ValueError(msg)
        elif self.index_type == "quantized":         # beyond 64 rows: the deep search (QuantizedIndex.serving_path), its limits
            candidates = self.refine_factor * self.top_k
            if self.top_k > QuantizedIndex.DEEP_MAX_K:
                msg = f"a quantized index returns at most {QuantizedIndex.DEEP_MAX_K} rows per query: top_k = {self.top_k}"
                raise ValueError(msg)
            if candidates > QuantizedIndex.DEEP_MAX_CANDIDATES:
                msg = (f"a quantized index refines at most {QuantizedIndex.DEEP_MAX_CANDIDATES} candidates per query beyond "
                       f"{QuantizedIndex.TILE_MAX_K} rows: refine_factor * top_k = {candidates}")
                raise ValueError(msg)
            if self.num_probes * candidates > MERGE_DEEP_MAX_KEYS:
                msg = (f"a quantized index merges at most {MERGE_DEEP_MAX_KEYS} candidates of a query's probes: "
                       f"num_probes * refine_factor * top_k = {self.num_probes * candidates}")
                raise ValueError(msg)
        if self.num_partitions is not None and self.num_partitions < 1:
            msg = f"num_partitions must be None (the default for the catalog's size) or at least 1: {self.num_partitions}"
            raise ValueError(msg)
        if not 1 <= self.num_probes <= PartitionedIndex.MAX_PROBES:
            msg = f"num_probes must be in 1..{PartitionedIndex.MAX_PROBES}: {self.num_probes}"
            raise ValueError(msg)
        if self.index_seed < 0:
            msg = f"index_seed must not be negative: {self.index_seed}"
            raise ValueError(msg)
        return self

    @pydantic.model_validator(mode="after")
    def _streaming_logq_fields(self):
        if self.logq_mode not in LOGQ_MODES:
            msg = f"logq_mode must be 'table' or 'streaming': {self.logq_mode!r}"
            raise ValueError(msg)
        if self.logq_mode == "streaming" and not self.use_logq:
            msg = "logq_mode='streaming' estimates the table of the logQ correction: it needs use_logq=True"
            raise ValueError(msg)
        if not 0.0 < self.logq_alpha <= 1.0:
            msg = f"logq_alpha must be in (0, 1]: {self.logq_alpha}"
            raise ValueError(msg)
        if not 0 <= self.logq_buckets < 2**31:
            msg = f"logq_buckets must be 0 (direct) or a bucket count below 2^31: {self.logq_buckets}"
            raise ValueError(msg)
        if not 1 <= self.logq_hashes <= StreamingLogQ.MAX_HASHES:
            msg = f"logq_hashes must be in 1..{StreamingLogQ.MAX_HASHES}: {self.logq_hashes}"
            raise ValueError(msg)
        return self

    @pydantic.field_validator("metrics_mode")
    @classmethod
    def _known_metrics_mode(cls, v: str) -> str:
        if v not in METRICS_MODES:
            msg = f"metrics_mode must be 'topk' or 'positions': {v!r}"
            raise ValueError(msg)
        return v


HISTORY_TOWERS = ("history", "transformer")      # user towers whose input is the user's history, not its id


class MatrixFactorizationLitModule(_Base):
    def __init__(self, config: MatrixFactorizationLitConfig | dict) -> None:
        super().__init__()
        self.config = MatrixFactorizationLitConfig.model_validate(config)
        self.towers: torch.nn.ModuleDict | None = None
        self.loss_fns: torch.nn.ModuleList | None = None
        self.item_processor: ItemProcessor | None = None
        self.history: dict[int, list[int]] = {}      # user_rn -> item ids already consumed (recommend excludes them)
        self.logq: torch.Tensor | None = None         # [num_items] log sampling probability, when use_logq
        self.logq_estimator: StreamingLogQ | None = None      # logq_mode="streaming": produces ``logq`` (direct) or the batch's rows (hashed)
        self.metrics: dict[str, RetrievalMetrics | PositionMetrics] | None = None
        self._fused: fused.FusedSmallStep | None = None

    # ------------------------------------------------------------------ towers ---
    def forward(self, idx: torch.Tensor, *, tower: str = "user") -> torch.Tensor:
        if self.towers is None:
            msg = "`model` must be initialised first"
            raise ValueError(msg)
        return self.towers[tower](idx)

    @torch.inference_mode()
    def recommend(self, user_idx: int, *, top_k: int = TOP_K, exclude_item_ids: list[int] | None = None, where=None):
        if self.towers is None or self.item_processor is None or self.item_processor.index is None:
            msg = "`user_processor` and `item_processor` must be initialised first"
            raise ValueError(msg)
        exclude_item_ids = (exclude_item_ids or []) + list(self.history.get(int(user_idx), []))
        device = self.towers["user"].weight.device
        if self.config.user_tower in HISTORY_TOWERS:      # the user IS its history: pool it (xfmr_rec/lightning.py:89-90 excludes it)
            embed = self._pool_item_ids(list(self.history.get(int(user_idx), []))).cpu().numpy()
        else:
            with self._user_tower_eval():
                embed = self(torch.tensor([int(user_idx)], device=device)).cpu().numpy()
        return self.item_processor.search(embed, exclude_item_ids=exclude_item_ids, top_k=top_k, where=where)

    def set_item_tags(self, tags, vocabulary=None) -> None:
        """The items' tag words and the names of their bits (``data.item_tag_bits``), for ``recommend*(where=...)``: a
        ``retrieval.TagFilter``, or a dict of name lists ``{"any_of": [...], "all_of": [...], "none_of": [...]}``.  Saved with
        the module."""
        if self.item_processor is None:
            self.item_processor = self._item_processor()
        self.item_processor.set_tags(tags, vocabulary)

    @contextlib.contextmanager
    def _user_tower_eval(self):
        """The user tower in eval mode for one serving / metric call (a transformer tower with dropout never drops there),
        its mode restored afterwards; training steps run the tower in whatever mode the module is in."""
        tower = self.towers["user"]
        was = tower.training
        tower.eval()
        try:
            yield tower
        finally:
            tower.train(was)

    def _pool_item_ids(self, item_ids: list[int]) -> torch.Tensor:
        """``[1, d]`` history-tower query of a list of item ids (rows through the item index's id map when there is one)."""
        proc = self.item_processor
        rows = [proc.row_of(i) for i in item_ids] if (proc is not None and proc._row_of_id is not None) else [int(i) for i in item_ids]
        device = self.towers["item"].weight.device
        history = torch.tensor([rows or [0]], dtype=torch.int64, device=device)
        if isinstance(self.towers["user"], models.HistoryTransformerTower):      # its serving path: eval mode whatever the tower's
            return self.towers["user"].encode(history)
        with self._user_tower_eval() as tower:
            return tower(history)

    @torch.inference_mode()
    def recommend_with_history(self, item_ids: list[int], *, top_k: int = TOP_K, exclude_item_ids: list[int] | None = None,
                               where=None):
        """Serve a user who is in no table from the items they consumed (history tower only): the query is the pooled
        history and the history itself is excluded (xfmr_rec/lightning.py:89-90)."""
        if self.config.user_tower not in HISTORY_TOWERS:
            msg = ("recommend_with_history needs user_tower='history' or 'transformer' (a table user tower has no row for an "
                   "unseen user)")
            raise ValueError(msg)
        if self.towers is None or self.item_processor is None or self.item_processor.index is None:
            msg = "`user_processor` and `item_processor` must be initialised first"
            raise ValueError(msg)
        embed = self._pool_item_ids(list(item_ids)).cpu().numpy()
        exclude = [*(exclude_item_ids or []), *map(int, item_ids)]
        return self.item_processor.search(embed, exclude_item_ids=exclude, top_k=top_k, where=where)

    # ------------------------------------------------------------ feature towers ---
    def feature_hasher(self):
        """The tokenizer of the feature towers (its settings are part of the config, so they are saved with it)."""
        from .data import FeatureHasher

        cfg = self.config
        return FeatureHasher(cfg.feature_buckets, seed=cfg.feature_seed, text_fields=cfg.feature_text_fields)

    def _feature_tower(self, name: str, what: str) -> models.FeatureBagTower:
        if self.towers is None:
            msg = "`model` must be initialised first"
            raise ValueError(msg)
        tower = self.towers[name]
        if not isinstance(tower, models.FeatureBagTower):
            msg = f"{what} needs {name}_tower='features' (a {type(tower).__name__} does not read attributes)"
            raise ValueError(msg)
        return tower

    def _bags(self, x):
        from .data import FeatureBags

        return x if isinstance(x, FeatureBags) else self.feature_hasher().bags(x)

    def set_features(self, *, item=None, user=None) -> None:
        """Register every entity's attributes on the feature towers: ``data.FeatureBags``, or the reference's JSON texts
        indexed by row (``data.read_movielens_features``; row 0 = ``None``, the padding row)."""
        for name, x in (("item", item), ("user", user)):
            if x is not None:
                self._feature_tower(name, "set_features").set_bags(self._bags(x))

    @torch.no_grad()
    def add_items(self, item_ids, item_texts, tags=None) -> None:
        """Cold start: embed items that were not in the catalogue from their attributes (the reference's item JSON text)
        and append their rows and ids to the item index -- and to the item tower's bags, so a rebuilt index keeps them.
        ``tags``: their tag words (0 when the items have tags and none are given)."""
        from .data import FeatureBags

        tower = self._feature_tower("item", "add_items")
        if self.item_processor is None or self.item_processor.index is None:
            msg = "`user_processor` and `item_processor` must be initialised first"
            raise ValueError(msg)
        bags = self._bags(item_texts)
        if len(bags) != len(item_ids):
            msg = f"one text per item id: {len(item_ids)} != {len(bags)}"
            raise ValueError(msg)
        self.item_processor.append(item_ids, tower.embed(bags), tags=tags)
        if tower.bags is not None:
            old = tower.bags
            w = None
            if old.weights is not None or bags.weights is not None:
                w = torch.cat([old.weights.cpu() if old.weights is not None else torch.ones(old.tokens.numel()),
                               bags.weights.cpu() if bags.weights is not None else torch.ones(bags.tokens.numel())])
            off = torch.cat([old.off.cpu(), bags.off.cpu()[1:] + int(old.off[-1])])
            tower.set_bags(FeatureBags(off, torch.cat([old.tokens.cpu(), bags.tokens.cpu()]), w))

    @torch.inference_mode()
    def recommend_with_text(self, user_text, *, top_k: int = TOP_K, exclude_item_ids: list[int] | None = None, where=None):
        """Serve a user from their attributes alone (the reference's user JSON text, or a dict): the counterpart of
        ``recommend(text, ...)`` (xfmr_rec/lightning.py:76-95)."""
        tower = self._feature_tower("user", "recommend_with_text")
        if self.item_processor is None or self.item_processor.index is None:
            msg = "`user_processor` and `item_processor` must be initialised first"
            raise ValueError(msg)
        embed = tower.embed(self._bags([user_text])).cpu().numpy()
        return self.item_processor.search(embed, exclude_item_ids=exclude_item_ids, top_k=top_k, where=where)

    @torch.inference_mode()
    def recommend_with_item_id(self, item_id: int, *, top_k: int = TOP_K, exclude_item_ids: list[int] | None = None, where=None):
        """Items closest to item ``item_id`` -- the query is the item's own embedding and the item itself is
        excluded (``Service.recommend_with_item_id`` -> ``recommend_with_item``, xfmr_rec/bentoml/service.py:220-247)."""
        if self.item_processor is None or self.item_processor.index is None:
            msg = "`user_processor` and `item_processor` must be initialised first"
            raise ValueError(msg)
        row = self.item_processor.row_of(item_id)
        embed = self.item_processor.index.embeddings[row: row + 1, : self.config.hidden_size].cpu().numpy()
        return self.item_processor.search(embed, exclude_item_ids=[*(exclude_item_ids or []), int(item_id)], top_k=top_k, where=where)

    def recommend_with_user_id(self, user_idx: int, *, top_k: int = TOP_K, exclude_item_ids: list[int] | None = None, where=None):
        """``Service.recommend_with_user_id`` (service.py:286-311): the user's history is excluded."""
        return self.recommend(user_idx, top_k=top_k, exclude_item_ids=exclude_item_ids, where=where)

    def _item_processor(self, item_ids=None) -> ItemProcessor:
        cfg = self.config
        return ItemProcessor(item_ids, index_type=cfg.index_type, num_partitions=cfg.num_partitions, num_probes=cfg.num_probes,
                             index_seed=cfg.index_seed, num_sub_vectors=cfg.num_sub_vectors, refine_factor=cfg.refine_factor,
                             filter_mode=cfg.filter_mode)

    # ------------------------------------------------------------- save / load (f-3) ---
    def save(self, path) -> None:
        """The counterpart of ``save`` (xfmr_rec/lightning.py:312-328: ``transformer/`` + ``processors.json`` +
        ``lance_db/``): the two tables (``towers.safetensors``), ``processors.json`` (config, item ids,
        histories) and the built item index (``item_index.safetensors``: unit-norm item matrix + id map)."""
        import json
        import pathlib

        from safetensors.torch import save_file

        if self.towers is None:
            msg = "`model` must be initialised first"
            raise ValueError(msg)
        path = pathlib.Path(path)
        path.mkdir(parents=True, exist_ok=True)
        # (a history user tower has no table of its own: it shares the item table, which is written once)
        # feature towers: their bucket table as "features.weight" (shared by both towers, written once), their bags apart
        tables, bags = {}, {}
        for k, t in self.towers.items():
            if isinstance(t, models.FeatureBagTower):
                tables["features.weight"] = t.weight.detach().cpu().contiguous()   # (init_towers: at most one feature table)
                if t.bags is not None:
                    bags[f"{k}.off"], bags[f"{k}.tokens"] = t.bags.off.cpu().contiguous(), t.bags.tokens.cpu().contiguous()
                    if t.bags.weights is not None:
                        bags[f"{k}.weights"] = t.bags.weights.cpu().contiguous()
            elif isinstance(t, models.HistoryTransformerTower):      # the encoder's weights, next to the shared table
                tables.update({f"{k}.{name}": v.detach().cpu().contiguous() for name, v in t.state_dict().items()})
            elif not isinstance(t, models.HistoryPoolingTower):
                tables[f"{k}.weight"] = t.weight.detach().cpu().contiguous()
        save_file(tables, str(path / TOWERS_PATH))
        if bags:
            save_file(bags, str(path / FEATURE_BAGS_PATH))
        proc = {"config": self.config.model_dump(), "history": {str(k): list(map(int, v)) for k, v in self.history.items()}}
        if self.item_processor is not None and self.item_processor.tags is not None:      # (no tags: no file, no key)
            save_file({"tags": self.item_processor.tags.contiguous()}, str(path / ITEM_TAGS_PATH))
            proc["item_tag_vocabulary"] = self.item_processor.tag_vocabulary
        (path / PROCESSORS_JSON).write_text(json.dumps(proc, indent=2))
        if self.item_processor is not None and self.item_processor.index is not None:
            idx = self.item_processor.index
            save_file({"embeddings": idx.embeddings[:, : idx.dim].cpu().contiguous(),
                       "item_ids": self.item_processor.item_ids.contiguous()}, str(path / INDEX_PATH))
        if self.logq_estimator is not None:
            save_file({k: v.detach().cpu().contiguous() for k, v in self.logq_estimator.state_dict().items()}, str(path / LOGQ_PATH))

    @classmethod
    def load(cls, path, device="cuda") -> "MatrixFactorizationLitModule":
        """What serving loads (``bentoml/service.py`` builds its processors from the same three pieces)."""
        import json
        import pathlib

        from safetensors.torch import load_file

        path = pathlib.Path(path)
        proc = json.loads((path / PROCESSORS_JSON).read_text())
        module = cls(proc["config"])
        module.configure_model(device=device)
        weights = load_file(str(path / TOWERS_PATH))
        with torch.no_grad():
            for k, t in module.towers.items():
                if isinstance(t, models.FeatureBagTower):
                    t.weight.copy_(weights["features.weight"].to(device))
                elif isinstance(t, models.HistoryTransformerTower):
                    t.load_state_dict({name: weights[f"{k}.{name}"].to(device) for name in t.state_dict()})
                elif not isinstance(t, models.HistoryPoolingTower):
                    t.weight.copy_(weights[f"{k}.weight"].to(device))
        if (path / FEATURE_BAGS_PATH).exists():
            from .data import FeatureBags

            bags = load_file(str(path / FEATURE_BAGS_PATH))
            for k, t in module.towers.items():
                if f"{k}.off" in bags:
                    t.set_bags(FeatureBags(bags[f"{k}.off"], bags[f"{k}.tokens"], bags.get(f"{k}.weights")))
        if module.logq_estimator is not None and (path / LOGQ_PATH).exists():
            module.logq_estimator.load_state_dict(load_file(str(path / LOGQ_PATH)))      # (copies into the device buffers)
        module.history = {int(k): v for k, v in proc.get("history", {}).items()}
        if (path / INDEX_PATH).exists():
            idx = load_file(str(path / INDEX_PATH))
            module.item_processor = module._item_processor(idx["item_ids"])      # (a partitioned index: the same build, so the same cells)
            module.item_processor.set_index(idx["embeddings"].to(device))
        if (path / ITEM_TAGS_PATH).exists():
            module.set_item_tags(load_file(str(path / ITEM_TAGS_PATH))["tags"], proc.get("item_tag_vocabulary"))
        return module

    # ------------------------------------------------------------------ losses ---
    def compute_losses(self, batch, step_name: str = "train") -> dict[str, torch.Tensor]:
        if self.loss_fns is None:
            msg = "`loss_fns` must be initialised first"
            raise ValueError(msg)
        target = batch["target"]
        pos_idx = batch["user"].get("pos_idx")            # the reference's padded positives, or ...
        pos_csr = batch["user"].get("pos_csr")            # ... the producer's CSR lists (data.DeviceInteractionSampler)
        # history tower: the user vector is the pooled history of the example (data.DeviceInteractionSampler(history=True))
        user_embed = self(batch["user"]["history" if self.config.user_tower in HISTORY_TOWERS else "idx"], tower="user")
        # positives then sampled negatives, as xfmr_rec/lightning.py:133-134
        item_idx = torch.cat([batch["item"]["idx"], batch["neg_item"]["idx"]])
        item_embed = self(item_idx, tower="item")
        # streaming logQ: a training step's item columns are one more batch the estimator sees, before the loss reads it;
        # evaluation reads the estimate and advances nothing
        logq_rows = self._streaming_logq(item_idx, advance=step_name == "train" and self.training)
        # the logQ table is looked up by item_idx inside the kernel (no gather launch)
        logq_table = self.logq if (self.config.use_logq and self.logq is not None and logq_rows is None) else None
        cfg = self.config
        if cfg.fused_losses:
            vals = mf_losses.fused_losses(user_embed, item_embed, target, item_idx=item_idx, pos_idx=pos_idx,
                                          num_negatives=cfg.num_negatives, sigma=cfg.sigma, margin=cfg.margin,
                                          logq=logq_rows, logq_table=logq_table, pos_csr=pos_csr,
                                          train_loss=cfg.train_loss if step_name == "train" else None)
            return {f"{step_name}/{name}": v for name, v in vals.items()}
        return {
            f"{step_name}/{fn.__class__.__name__}": fn(user_embed=user_embed, item_embed=item_embed, target=target, item_idx=item_idx,
                                                       pos_idx=pos_idx, logq=logq_rows, logq_table=logq_table, pos_csr=pos_csr)
            for fn in self.loss_fns
        }

    def _streaming_logq(self, item_idx: torch.Tensor, *, advance: bool) -> torch.Tensor | None:
        """``logq_mode="streaming"``: feed the estimator the step's item columns (``advance``) and hand the loss its values --
        direct mode through ``self.logq`` (the estimator's table, updated in place: returns None), hashed mode as the rows of
        ``item_idx`` (returned).  Without an estimator: None, ``self.logq`` is the caller's."""
        est = self.logq_estimator
        if est is None:
            return None
        if est.num_hashes == 0:
            if advance:
                est.update(item_idx, rows=False)
            self.logq = est.table
            return None
        return est.update(item_idx) if advance else est.lookup(item_idx)

    # ------------------------------------------------------------------ metrics ---
    @torch.no_grad()
    def update_metrics(self, batch, step_name: str = "val") -> dict[str, torch.Tensor]:
        """Batched counterpart of ``update_metrics`` (xfmr_rec/lightning.py:149-187, one example per
        call upstream): top-k for all users of the batch with their histories excluded
        (``predict_step`` -> ``recommend``, :76-95), then the six retrieval metrics on the device.
        ``batch``: ``user.idx`` [Q]; ``history`` = (offsets [Q+1], item rows) to exclude; ``target`` =
        (offsets [Q+1], item rows, ratings) -- item rows are the index's ``movie_rn``."""
        if self.metrics is None:
            msg = "`metrics` must be initialised first"
            raise ValueError(msg)
        if self.item_processor is None or self.item_processor.index is None:
            msg = "`user_processor` and `item_processor` must be initialised first"
            raise ValueError(msg)
        queries = self._queries(batch)
        off, ids, rating = batch["target"]
        metric = self.metrics[step_name]
        if self.config.metrics_mode == "positions":      # no list: where each target stands among all admissible rows
            pos, _, ncand = self.item_processor.index.positions(queries, (off, ids), exclude_csr=batch.get("history"))
            metric.update(pos, off, rating, ncand)
            return metric.compute()
        index = self.item_processor.index
        _, rows = index.search(queries, self.config.top_k, exclude_csr=batch.get("history"), path=index.serving_path(self.config.top_k))
        metric.update(rows, off, ids, rating)
        return metric.compute()

    def _queries(self, batch) -> torch.Tensor:
        """The users' query vectors: their table rows, or (history tower) their pooled history -- the same CSR
        ``(offsets, item rows)`` that is excluded from retrieval (``InteractionTable.eval_sets``)."""
        if self.towers is not None and isinstance(self.towers["user"], models.HistoryTransformerTower):   # its serving path
            off, items = batch["history"]
            return self.towers["user"].encode((off[:-1], off[1:], items))
        with self._user_tower_eval():
            if self.config.user_tower not in HISTORY_TOWERS:
                return self(batch["user"]["idx"], tower="user")
            off, items = batch["history"]
            return self((off[:-1], off[1:], items), tower="user")

    def validation_step(self, batch, _: int = 0) -> None:
        self.log_dict(self.update_metrics(batch, step_name="val"))

    def test_step(self, batch, _: int = 0) -> None:
        self.log_dict(self.update_metrics(batch, step_name="test"))

    @torch.no_grad()
    def predict_step(self, batch, _: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
        """``(scores, item rows)`` [Q, top_k] of the batch's users, histories excluded."""
        queries = self._queries(batch)
        index = self.item_processor.index
        return index.search(queries, self.config.top_k, exclude_csr=batch.get("history"), path=index.serving_path(self.config.top_k))

    def training_step(self, batch, _: int = 0) -> torch.Tensor:
        losses = self.compute_losses(batch, step_name="train")
        self.log_dict(losses)
        return losses[f"train/{self.config.train_loss}"]

    def fused_training_step(self, batch, optimizer: torch.optim.Optimizer) -> torch.Tensor:
        """``training_step`` + ``loss.backward()`` + ``optimizer.step()`` (xfmr_rec/lightning.py:189-192 and Lightning's
        automatic optimisation around it) in ONE launch when the configuration is the reference's kind -- B <= 128 pairs,
        plain embedding towers, a mined loss, ``optim.SparseSGD`` / ``optim.RowAdam`` -- through ``fused.FusedSmallStep``
        (``mf_step_small``: bit-identical to the three calls); any other configuration (``optim.RowAdagrad`` among them) runs
        those three calls.  Returns
        the trained loss, detached (its gradient has been applied); logs all seven losses like ``training_step``."""
        if self.loss_fns is None or self.towers is None:
            msg = "`loss_fns` must be initialised first"
            raise ValueError(msg)
        cfg = self.config
        est = self.logq_estimator
        if est is not None and est.num_hashes > 0:      # hashed rows go to the loss as logq=: the three calls
            self._fused = None
        elif self._fused is None or self._fused.opt is not optimizer:
            fn = next(f for f in self.loss_fns if f.__class__.__name__ == cfg.train_loss)
            try:
                self._fused = fused.FusedSmallStep(self.towers, optimizer, fn, all_losses=True,
                                                   logq_table=self.logq if (cfg.use_logq and self.logq is not None) else None)
            except mf_losses._lib.MfHipError:        # hash towers, a foreign optimiser: the ordinary three calls
                self._fused = None
        if self._fused is not None:                  # the table of THIS step (it may be set / refreshed after the first one)
            self._fused.set_logq_table(self.logq if (cfg.use_logq and self.logq is not None) else None)
        if self._fused is None:
            loss = self.training_step(batch)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad(set_to_none=True)
            return loss.detach()
        flat = {"user": batch["user"]["idx"], "item": torch.cat([batch["item"]["idx"], batch["neg_item"]["idx"]]), "target": batch["target"]}
        if est is not None:                          # direct mode: the table the step reads is updated in place, ahead of it
            self._streaming_logq(flat["item"], advance=self.training)
        if batch["user"].get("pos_csr") is not None:
            flat["pos_csr"] = (flat["user"],) + tuple(batch["user"]["pos_csr"][1:])
        elif batch["user"].get("pos_idx") is not None:
            flat["pos"] = batch["user"]["pos_idx"]
        before = self._fused.fused_steps
        loss = self._fused(flat)
        if self._fused.fused_steps > before:       # (a fallback step evaluates the trained loss only)
            self.log_dict({f"train/{name}": self._fused.losses[i] for i, name in enumerate(mf_losses.KINDS)})
        return loss

    # ------------------------------------------------------------------- setup ---
    def configure_optimizers(self) -> torch.optim.Optimizer:
        # (a transformer tower: tables + the encoder's dense weights, one object steps both; otherwise the bare row optimiser)
        kind = self.config.optimizer if self.config.optimizer in ("sgd", "adagrad") else "adam"
        return optim.tower_optimizer(self.towers, kind, self.config.learning_rate)

    def configure_model(self, device=None) -> None:
        if self.towers is None:
            self.towers = self.get_model(device)
        if self.loss_fns is None:
            self.loss_fns = self.get_loss_fns()
        if self.item_processor is None:
            self.item_processor = self._item_processor()
        if self.metrics is None:
            self.metrics = self.get_metrics()
        cfg = self.config
        if self.logq_estimator is None and cfg.logq_mode == "streaming":
            where = device if device is not None else next(self.towers.parameters()).device
            hashed = cfg.logq_buckets > 0
            self.logq_estimator = StreamingLogQ(cfg.logq_buckets if hashed else cfg.num_items, alpha=cfg.logq_alpha,
                                                num_hashes=cfg.logq_hashes if hashed else 0, device=where)
            if not hashed:
                self.logq = self.logq_estimator.table

    def get_model(self, device=None) -> torch.nn.ModuleDict:
        return models.init_towers(self.config, device=device)

    def get_loss_fns(self) -> torch.nn.ModuleList:
        loss_classes = [
            mf_losses.AlignmentLoss,
            mf_losses.ContrastiveLoss,
            mf_losses.AlignmentContrastiveLoss,
            mf_losses.InfomationNoiseContrastiveEstimationLoss,
            mf_losses.MutualInformationNeuralEstimationLoss,
            mf_losses.PairwiseHingeLoss,
            mf_losses.PairwiseLogisticLoss,
        ]
        cfg = self.config
        return torch.nn.ModuleList(
            [cls(num_negatives=cfg.num_negatives, sigma=cfg.sigma, margin=cfg.margin) for cls in loss_classes]
        )

    def get_metrics(self) -> dict[str, RetrievalMetrics | PositionMetrics]:
        """NDCG / Recall / Precision / MAP / HitRate / MRR @top_k for "val" and "test" (lightning.py:289-306); with
        ``metrics_mode="positions"`` also @ every ``eval_ks`` and the uncut MRR / MeanPosition / AUC."""
        cfg = self.config
        if cfg.metrics_mode == "positions":
            return {step: PositionMetrics((cfg.top_k, *(cfg.eval_ks or ())), prefix=f"{step}/") for step in ("val", "test")}
        return {step: RetrievalMetrics(top_k=cfg.top_k, prefix=f"{step}/") for step in ("val", "test")}

    def on_validation_start(self) -> None:
        self.item_processor.get_index(self)
        self.metrics["val"].reset()

    def on_test_start(self) -> None:
        self.item_processor.get_index(self)
        self.metrics["test"].reset()
