"""Top-K recommendation on the device: score a catalogue of M items for U users, keep the K best.

The per-row paths (``FiBiNETTrainer.predict``, the drop-in module, ``predict.py``) score rows that
each carry their own candidate and history.  Scoring every (user, candidate) pair through them
re-gathers the history for every pair and re-runs the mm projection for every pair.  Here the pair's
fields are composed from two caches (csrc/recommend.hip):

* per candidate, once per catalogue: field 4 = ReLU(LN(mm_proj(item_emb_d128)))  (``refresh``)
* per user, once per call:           field 5 = masked mean of the history rows

and the rest of the forward (SENET, bilinear, MLP, head) is ``ops.forward``'s own launches on the pair
rows, chunk by chunk, so a score is what the eval forward gives for that pair.  ``topk`` feeds every
chunk's logits to ``fbn_rec_topk``, which carries each user's K best as integer keys: no score ever
reaches the host and the U x M matrix is never sorted.  ``rank`` counts, in the same order, how many
eligible items lie above one held-out item per user (``fbn_rec_rank`` on one sweep's logits), and
``evaluate`` turns such ranks into HR / NDCG / MRR@K through ``rank_metrics.RankMetrics``.

``score_lists`` / ``topk_lists`` / ``rank_lists`` do the same over a candidate list that is different
for each user -- ``candidates [U, C]`` of item ids or catalogue positions, a negative entry an empty
slot -- scoring only the listed pairs (``fbn_rec_fields_list`` reads the pair's catalogue position
through the list; the selection and rank keys carry the slot, so ties go to the caller's own order),
and ``evaluate_sampled`` ranks each held-out item against sampled negatives through them.

``similar_items`` / ``retrieve`` / ``recommend`` / ``evaluate_retrieval`` are the retrieval stage in
front of those lists (csrc/retrieve.hip): cosine similarity between L2-normalised item vectors of one
``space`` -- the content vectors, the item cache or the id table -- as exact f32 scores, chunk by chunk
into the same ``fbn_rec_topk`` / ``fbn_rec_rank``; a user's query is the normalised sum of its history
items' vectors, which ranks as the mean cosine to them does.

``diversify`` / ``list_diversity`` / ``evaluate_diversity`` (csrc/diversify.hip) re-rank a
user's list by greedy maximal marginal relevance -- relevance against the largest cosine to what is
already picked, in one of the retrieval spaces -- and measure the intra-list diversity of finished lists;
``recommend(lam=...)`` puts the re-ranking behind the retrieval stage.

Single device, bilinear "all"; a row-sharded table is out of scope.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib, ops
from ._lib import call, ptr

K_MAX = 256          # include/fibinet.h: fbn_rec_topk
L_MAX = 32
DEFAULT_CHUNK_ROWS = 131072
CATALOGUE_KEYS = ("item_id", "likes_level", "views_level", "item_emb_d128")
SPACES = ("content", "mm", "id")            # retrieval vector spaces
DEFAULT_KNN_CHUNK_BYTES = 64 << 20
Q_MAX = 65535                               # include/fibinet.h: fbn_knn_scores / fbn_rec_topk
MMR_MAX_C = _lib.FBN_MMR_MAX_C              # include/fibinet.h: fbn_mmr_select's list length


def _state_of(state) -> Dict[str, torch.Tensor]:
    if isinstance(state, dict):
        return state
    if hasattr(state, "state_dict"):
        if getattr(state, "world", 1) > 1:          # FiBiNETTrainer with a row-sharded table
            raise ValueError("Recommender serves one device: pass the assembled state_dict of a world > 1 trainer")
        return state.state_dict()
    raise TypeError(f"state must be a state_dict, a FiBiNETTrainer or the model module, not {type(state).__name__}")


def _check_calibrator(calibrator, logits: bool) -> None:
    if calibrator is not None and logits:
        raise ValueError("a calibrator maps probabilities; it cannot be combined with logits=True")


def _check_lists(item_seq, candidates, by: str, target_slot=None, k: Optional[int] = None):
    """The argument checks of the ``*_lists`` methods, before anything is launched: -> (U, C).  Shapes
    only, so it needs no device."""
    if by not in ("item_id", "index"):
        raise ValueError(f"by must be 'item_id' or 'index', not {by!r}")
    if k is not None and not 1 <= int(k) <= K_MAX:
        raise ValueError(f"k must be in 1..{K_MAX}")
    if item_seq is not None and item_seq.dim() != 2:
        raise ValueError("item_seq must be [U, L]")
    U = 1 if item_seq is None else int(item_seq.shape[0])
    if U < 1:
        raise ValueError("item_seq holds no user")
    if not isinstance(candidates, torch.Tensor) or candidates.dim() != 2 or candidates.is_floating_point():
        raise ValueError("candidates must be an integer tensor [U, C]")
    if int(candidates.shape[0]) != U or int(candidates.shape[1]) < 1:
        raise ValueError(f"candidates is {tuple(candidates.shape)} for {U} users: need [U, C] with C >= 1")
    if target_slot is not None and int(torch.as_tensor(target_slot).numel()) != U:
        raise ValueError(f"target_slot holds {int(torch.as_tensor(target_slot).numel())} slots for {U} users")
    return U, int(candidates.shape[1])


def _check_knn(space: str, n: Optional[int] = None, *, what: str = "n", by: Optional[str] = None, items=None,
               item_seq=None) -> int:
    """The argument checks of the retrieval methods, before anything is launched: -> the number of
    queries.  Shapes only, so it needs no device."""
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}, not {space!r}")
    if by is not None and by not in ("item_id", "index"):
        raise ValueError(f"by must be 'item_id' or 'index', not {by!r}")
    if n is not None and not 1 <= int(n) <= K_MAX:
        raise ValueError(f"{what} must be in 1..{K_MAX}")
    if items is not None:
        if not isinstance(items, torch.Tensor) or items.dim() != 1 or items.is_floating_point():
            raise ValueError("items must be an integer tensor [Q]")
        if not 1 <= int(items.shape[0]) <= Q_MAX:
            raise ValueError(f"items holds {int(items.shape[0])} queries: need 1..{Q_MAX} per call")
        return int(items.shape[0])
    if not isinstance(item_seq, torch.Tensor) or item_seq.dim() != 2 or item_seq.is_floating_point():
        raise ValueError("item_seq must be an integer tensor [U, L]")
    if not 1 <= int(item_seq.shape[0]) <= Q_MAX:
        raise ValueError(f"item_seq holds {int(item_seq.shape[0])} users: need 1..{Q_MAX} per call")
    return int(item_seq.shape[0])


def _check_lam(lam) -> float:
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:                  # NaN fails both comparisons
        raise ValueError(f"lam must be a number in [0, 1], not {lam!r}")
    return lam


def _check_diversify(item_seq, candidates, k, lam, space: str, relevance, by: str):
    """The argument checks of ``diversify``, before anything is launched: -> (U, C, lam).  Shapes only,
    so it needs no device."""
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}, not {space!r}")
    lam = _check_lam(lam)
    U, C = _check_lists(item_seq, candidates, by, k=k)
    if C > MMR_MAX_C:
        raise ValueError(f"candidates holds {C} slots per user: diversify takes at most {MMR_MAX_C}")
    if U > Q_MAX:
        raise ValueError(f"candidates holds {U} users: need 1..{Q_MAX} per call")
    if isinstance(relevance, torch.Tensor):
        if relevance.dtype != torch.float32 or tuple(relevance.shape) != (U, C):
            raise ValueError(f"relevance must be 'prob', 'logit' or a float32 tensor [{U}, {C}]")
    elif relevance not in ("prob", "logit"):
        raise ValueError(f"relevance must be 'prob', 'logit' or a float32 tensor [U, C], not {relevance!r}")
    return U, C, lam


def _check_positions(index, space: str):
    """The argument checks of ``list_diversity``: -> (U, K)."""
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}, not {space!r}")
    if not isinstance(index, torch.Tensor) or index.dim() != 2 or index.is_floating_point():
        raise ValueError("index must be an integer tensor [U, K] of catalogue positions")
    U, K = int(index.shape[0]), int(index.shape[1])
    if not 1 <= U <= Q_MAX or not 1 <= K <= K_MAX:
        raise ValueError(f"index is {tuple(index.shape)}: need 1..{Q_MAX} lists of 1..{K_MAX} positions")
    return U, K


def _knn_chunks(M: int, Q: int, chunk_bytes: int):
    """(first column, columns) of the score chunks [Q, Mc] f32 of at most chunk_bytes: Mc a multiple of
    1024 (fbn_rec_topk's segment) except in the last chunk, or whatever a smaller budget allows."""
    mc = max(1, int(chunk_bytes) // (4 * Q))
    if mc >= 1024:
        mc -= mc % 1024
    mc = min(mc, M, 0x7FFFFFFF // Q)
    return [(m0, min(mc, M - m0)) for m0 in range(0, M, mc)]


class Recommender:
    """Scores ``catalogue`` (a dict of ``item_id [M]``, ``likes_level [M]``, ``views_level [M]``,
    ``item_emb_d128 [M, 128]``) for user histories with the weights of ``state`` (an App. B
    ``state_dict``, a single-device ``FiBiNETTrainer`` or the drop-in module).  The compute dtype
    follows ``model_cfg`` exactly as ``build_model`` reads it.  At most ``chunk_rows`` (user, candidate)
    rows are live at a time.  Ids outside their tables never fault: they set a device flag that
    ``check_ids()`` turns into the reference's ``IndexError``."""

    def __init__(self, state, model_cfg: Dict, catalogue: Dict[str, torch.Tensor], *, device=None,
                 max_len: int = 20, chunk_rows: Optional[int] = None,
                 knn_chunk_bytes: int = DEFAULT_KNN_CHUNK_BYTES):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError(f"Recommender runs only on a HIP device, not {self.device} (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not 0 <= int(max_len) <= L_MAX:
            raise ValueError(f"max_len must be in 0..{L_MAX}")
        self.max_len = int(max_len)
        self.chunk_rows = int(chunk_rows) if chunk_rows is not None else DEFAULT_CHUNK_ROWS
        if self.chunk_rows < 1:
            raise ValueError("chunk_rows must be positive")
        self.knn_chunk_bytes = int(knn_chunk_bytes)
        if self.knn_chunk_bytes < 4:
            raise ValueError("knn_chunk_bytes must hold at least one score")
        self._knn: Dict[str, torch.Tensor] = {}            # space -> normalised [M, D], built on first use
        honour = bool(model_cfg.get("honour_config", False))
        btype = model_cfg.get("bilinear_type", "all") if honour else "all"
        if btype not in ("all", "each"):
            raise ValueError("bilinear_type must be 'all' or 'each'")
        if btype == "each":
            raise NotImplementedError("Recommender supports bilinear_type 'all' only ('each' keeps one W per field: "
                                      "score those models with FiBiNETTrainer.predict on expanded rows)")
        cdt = str(model_cfg.get("compute_dtype", "fp32")).lower()
        if cdt not in ("fp32", "float32", "bf16", "bfloat16", "bf16_fwd"):
            raise ValueError(f"compute_dtype must be 'fp32', 'bf16' or 'bf16_fwd', not {cdt!r}")
        self.d = int(model_cfg.get("embedding_dim", 64))
        self._bf16 = cdt in ("bf16", "bfloat16")
        self._fwd16 = cdt == "bf16_fwd"
        missing = [k for k in CATALOGUE_KEYS if k not in catalogue]
        if missing:
            raise KeyError(f"catalogue lacks {missing}")
        dev = self.device
        self.cat = {k: catalogue[k].to(dev).long().contiguous() for k in CATALOGUE_KEYS[:3]}
        self._x = catalogue["item_emb_d128"].to(dev).float().contiguous()
        self.M = int(self.cat["item_id"].shape[0])
        if self.M < 1 or any(int(t.shape[0]) != self.M for t in self.cat.values()) or \
                tuple(self._x.shape) != (self.M, 128):
            raise ValueError("catalogue columns must be [M] and item_emb_d128 [M, 128] with M >= 1")
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        # bit 0: a NaN logit reached the selection (it ranks below every number), or was a ranked target's
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._acts: Dict[int, Dict] = {}
        self._probe: Optional[Dict[str, list]] = None      # tools/recommend_bench.py: ops.forward's kernel probes
        self.refresh(state)

    # ------------------------------------------------------------------ weights + item cache
    @torch.no_grad()
    def refresh(self, state) -> None:
        """Take new weights and rebuild the item-side cache (field 4 of every catalogue row)."""
        sd = _state_of(state)
        dev, d = self.device, self.d
        if "bilinear.W" not in sd:
            raise NotImplementedError("Recommender supports bilinear_type 'all' only (state has no bilinear.W)")
        if tuple(sd["item_emb.weight"].shape[1:]) != (d,):
            raise ValueError(f"state has embedding_dim {sd['item_emb.weight'].shape[1]}, model_cfg says {d}")
        p = {}
        for k, v in sd.items():
            t = v.detach().to(dev, copy=True)      # never aliases a live module's parameters
            p[k] = (t.float() if t.is_floating_point() else t).contiguous()
        self.p = p
        self.V = int(p["item_emb.weight"].shape[0])
        self.cfg = ops.FwdConfig(d=d, L=0, training=False, p_drop=0.0, bf16=self._bf16, fwd16=self._fwd16,
                                 bilinear_each=False, R=int(p["senet.excitation.0.weight"].shape[0]))
        g16 = self._bf16 or self._fwd16
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            self.err.zero_()
            self._acts = {}
            self._knn.pop("mm", None)                      # the spaces made of weights; "content" stays
            self._knn.pop("id", None)
            self._wimg: Dict = {}
            self._w16 = None
            hmm = torch.empty((self.M, d), dtype=torch.float32, device=dev)
            if g16:
                # bf16 images of the GEMM weights, once; the catalogue's x image only for this GEMM
                w = ops.bf16_weights(p, d, self._wimg, st, x=self._x)
                ops.gemm(w["x"], w["Wp"], hmm, self.M, d, 128, 128, 128, d, False, True, bias=p["mm_proj.0.bias"],
                         bf16=True, stream=st)
                self._w16 = {k: v for k, v in w.items() if k != "x"}
                self._wimg.pop("w16_x", None)
            else:
                ops.gemm(self._x, p["mm_proj.0.weight"], hmm, self.M, d, 128, 128, 128, d, False, True,
                         bias=p["mm_proj.0.bias"], stream=st)
            self.cache = torch.empty((self.M, d), dtype=torch.float32, device=dev)
            call("fbn_rec_item_cache", ptr(self.cat["item_id"]), ptr(self.cat["likes_level"]),
                 ptr(self.cat["views_level"]), ptr(hmm), ptr(p["mm_proj.1.weight"]), ptr(p["mm_proj.1.bias"]),
                 ops.LN_EPS, int(p["cate_emb.weight"].shape[0]), self.V, ptr(self.cache), ptr(self.err), self.M, d, st)
            self._build_positions()

    def _build_positions(self) -> None:
        """self._pos [V] int32: id -> smallest catalogue position holding it, -1 for an id the catalogue
        lacks (torch ops on the device; a catalogue id outside [0, V) has no entry)."""
        ids = self.cat["item_id"]
        pos = torch.arange(self.M, dtype=torch.int64, device=self.device)
        ok = (ids >= 0) & (ids < self.V)
        ids, pos = ids[ok], pos[ok]
        ids, order = torch.sort(ids, stable=True)                 # equal ids stay in position order
        first = torch.ones_like(ids, dtype=torch.bool)
        first[1:] = ids[1:] != ids[:-1]
        self._pos = torch.full((self.V,), -1, dtype=torch.int32, device=self.device)
        self._pos[ids[first]] = pos[order][first].to(torch.int32)   # distinct indices: no write order to depend on

    def positions(self, item_ids: torch.Tensor) -> torch.Tensor:
        """Catalogue positions (int64, the shape of ``item_ids``) of item ids: the smallest position when
        the catalogue repeats an id, -1 for an id that is not in the catalogue or lies outside [0, V).
        No host sync, and no id faults."""
        ids = torch.as_tensor(item_ids).to(self.device).long()
        ok = (ids >= 0) & (ids < self.V)
        found = self._pos[ids.clamp(0, self.V - 1)].long()
        return torch.where(ok, found, torch.full_like(found, -1))

    def check_ids(self) -> None:
        """Raise the reference's IndexError if any id seen since construction (or the last refresh)
        lay outside its embedding table (one 4-byte read)."""
        if int(self.err.item()) & 1:
            raise IndexError("index out of range in self (item/likes/views id outside its embedding table)")

    # ------------------------------------------------------------------ the chunk loop
    def _hist(self, item_seq: Optional[torch.Tensor], st):
        dev, d = self.device, self.d
        if item_seq is None:
            seq, U, L = None, 1, 0
        else:
            if item_seq.dim() != 2:
                raise ValueError("item_seq must be [U, L]")
            seq = item_seq.to(dev).long()
            if seq.shape[1] > self.max_len:
                seq = seq[:, seq.shape[1] - self.max_len:]      # the collator keeps the last max_len
            seq = seq.contiguous()
            U, L = int(seq.shape[0]), int(seq.shape[1])
            if U < 1:
                raise ValueError("item_seq holds no user")
        hist = torch.empty((U, d), dtype=torch.float32, device=dev)
        call("fbn_rec_hist_pool", ptr(seq) if L else None, ptr(self.p["item_emb.weight"]), self.V, ptr(hist),
             ptr(self.err), U, L, d, st)
        return seq if L else None, hist, U, L

    def _chunks(self, U: int, n: Optional[int] = None):
        """(first column, columns) of the chunks over n columns: the catalogue (default), or a list's slots."""
        n = self.M if n is None else n
        mc = max(1, self.chunk_rows // U)
        for m0 in range(0, n, mc):
            yield m0, min(mc, n - m0)

    def _forward_chunk(self, hist, U, m0, Mc, cand: Optional[torch.Tensor] = None) -> Dict:
        """The eval forward's activations of one chunk: a["logits"] / a["probs"] [U * Mc], row u * Mc + j
        = user u, candidate m0 + j -- catalogue position m0 + j, or with ``cand`` ([U, C] positions) slot
        m0 + j of the user's own list; the buffers are reused by the next chunk of the same size."""
        p, c, dev = self.p, self.cat, self.device
        if cand is None:
            name, pairs = "fbn_rec_fields", (U, m0, Mc, self.d)
        else:
            name, pairs = "fbn_rec_fields_list", (U, ptr(cand), int(cand.shape[1]), m0, Mc, self.M, self.d)

        def fill(Vc, Vc16, cbuf, ldc, c_bf16, a_out, err, st):
            call(name, ptr(c["item_id"]), ptr(c["likes_level"]), ptr(c["views_level"]), ptr(self.cache),
                 ptr(hist), ptr(p["cate_emb.weight"]), int(p["cate_emb.weight"].shape[0]),
                 ptr(p["item_emb.weight"]), self.V, ptr(p["senet.excitation.0.weight"]),
                 ptr(p["senet.excitation.0.bias"]), ptr(p["senet.excitation.2.weight"]),
                 ptr(p["senet.excitation.2.bias"]), self.cfg.R, ptr(Vc), ptr(Vc16), ptr(cbuf), ldc, c_bf16,
                 ptr(a_out), ptr(err), *pairs, st)

        rows = U * Mc
        acts = self._acts.get(rows)
        if acts is None:
            if len(self._acts) >= 4:                 # a few shapes recur (full and ragged chunk)
                self._acts.clear()
            acts = self._acts[rows] = {}
        if self._w16 is not None:
            acts["w16"] = self._w16
        a = ops.forward(p, None, self.cfg, None, err=self.err, acts=acts, w16_ready=self._w16 is not None,
                        fields=ops.FieldsStage(rows, dev, fill), probe=self._probe)
        return a

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def score(self, item_seq: Optional[torch.Tensor], logits: bool = False, calibrator=None) -> torch.Tensor:
        """Probabilities (or logits) [U, M] of every (user, catalogue item) pair; ``item_seq=None``:
        one cold user whose history field is zero.  ``calibrator``: a metrics.IsotonicCalibrator applied
        to the probabilities in place (one more launch); not with ``logits=True``.  ``topk`` needs none:
        it ranks on logits and the map is monotone."""
        _check_calibrator(calibrator, logits)
        with torch.cuda.device(self.device):
            st = _lib.stream_handle(self.device)
            _, hist, U, _ = self._hist(item_seq, st)
            out = self._sweep(hist, U, logits)
            if calibrator is not None:
                calibrator.apply(out, out=out)
        return out

    def _sweep(self, hist, U: int, logits: bool, cand: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One sweep of the chunk loop collected into [U, M] (4 U M bytes) -- over the catalogue, or with
        ``cand`` ([U, C] positions) over the slots of the users' lists into [U, C]."""
        n = self.M if cand is None else int(cand.shape[1])
        out = torch.empty((U, n), dtype=torch.float32, device=self.device)
        for m0, Mc in self._chunks(U, n):
            a = self._forward_chunk(hist, U, m0, Mc, cand)
            out[:, m0:m0 + Mc].copy_((a["logits"] if logits else a["probs"]).view(U, Mc))
        return out

    @torch.no_grad()
    def topk(self, item_seq: Optional[torch.Tensor], k: int, exclude_history: bool = True) -> Dict[str, torch.Tensor]:
        """Each user's k best catalogue items, best first: ``index`` (catalogue position, int64),
        ``item_id``, ``logit``, ``prob``, all [U, k].  Ranked on logits; equal logits go to the smaller
        position.  exclude_history: items of the user's own history and padding items (id 0) are never
        returned.  With fewer than k eligible items the tail is index -1, item_id -1, logit -inf, prob 0.
        Nothing is copied to the host and nothing synchronises."""
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"k must be in 1..{K_MAX}")
        dev = self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            seq, hist, U, L = self._hist(item_seq, st)
            carry = torch.zeros((U, k), dtype=torch.int64, device=dev)
            out = {"index": torch.empty((U, k), dtype=torch.int64, device=dev),
                   "item_id": torch.empty((U, k), dtype=torch.int64, device=dev),
                   "logit": torch.empty((U, k), dtype=torch.float32, device=dev),
                   "prob": torch.empty((U, k), dtype=torch.float32, device=dev)}
            chunks = list(self._chunks(U))
            nws = int(_lib.lib().fbn_rec_topk_workspace_size(U, chunks[0][1], k))
            ws = torch.empty(max(1, (nws + 7) // 8), dtype=torch.int64, device=dev)
            for i, (m0, Mc) in enumerate(chunks):
                a = self._forward_chunk(hist, U, m0, Mc)
                last = i == len(chunks) - 1
                call("fbn_rec_topk", ptr(a["logits"]), U, m0, Mc, ptr(self.cat["item_id"]), ptr(seq), L,
                     int(bool(exclude_history)), k, ptr(carry), ptr(ws), nws,
                     ptr(out["index"]) if last else None, ptr(out["item_id"]) if last else None,
                     ptr(out["logit"]) if last else None, ptr(out["prob"]) if last else None, ptr(self.status), st)
        return out

    @torch.no_grad()
    def rank(self, item_seq: Optional[torch.Tensor], target: torch.Tensor, *, exclude_history: bool = True,
             by: str = "item_id", _status: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The rank of one held-out item per user among the eligible catalogue items, in ``topk``'s
        order: ``{"rank": int32 [U], "n_eligible": int32 [U]}``, rank 1 = ``topk``'s first place.
        ``target`` [U] holds item ids (``by="item_id"``, mapped by :meth:`positions`) or catalogue
        positions (``by="index"``); ``item_seq=None`` with one target is the cold user.  Eligibility is
        ``topk``'s rule (exclude_history: no padding items, no items of the user's own history) except
        that the target itself stays eligible when the history holds it.  A target that is not in the
        catalogue, or is the padding item, gets rank 0 ("not ranked").

        One catalogue sweep through the chunk loop into a [U, M] f32 buffer of logits -- 4 U M bytes,
        23 MB for 64 users x 91,718 items -- then one ``fbn_rec_rank`` call: only logits of the same
        sweep are compared.  Nothing is copied to the host and nothing synchronises; a
        NaN logit at a ranked target sets bit 0 of ``status``, as a NaN does in ``topk``."""
        if by not in ("item_id", "index"):
            raise ValueError(f"by must be 'item_id' or 'index', not {by!r}")
        dev = self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            seq, hist, U, L = self._hist(item_seq, st)
            tgt = torch.as_tensor(target).to(dev).long().reshape(-1)
            if tgt.numel() != U:
                raise ValueError(f"target holds {tgt.numel()} items for {U} users")
            pos = (self.positions(tgt) if by == "item_id" else tgt).contiguous()
            buf = self._sweep(hist, U, True)
            out = {"rank": torch.empty(U, dtype=torch.int32, device=dev),
                   "n_eligible": torch.empty(U, dtype=torch.int32, device=dev)}
            call("fbn_rec_rank", ptr(buf), self.M, U, self.M, ptr(self.cat["item_id"]), ptr(seq), L,
                 int(bool(exclude_history)), ptr(pos), ptr(out["rank"]), ptr(out["n_eligible"]),
                 ptr(self.status if _status is None else _status), st)
        return out

    @torch.no_grad()
    def evaluate(self, pairs, ks=(5, 10, 20), *, exclude_history: bool = True, max_users: Optional[int] = None,
                 users_per_block: int = 64) -> Dict:
        """HR@K, NDCG@K and MRR@K of ``topk`` over the full catalogue on held-out interactions.
        ``pairs``: an iterable of (batch, labels) as ``FiBiNETTrainer.evaluate`` takes it; every row
        with label 1 is one evaluation user with history ``batch["item_seq"]`` and held-out item
        ``batch["item_id"]``, taken in order until ``max_users``.  The users go ``users_per_block`` at
        a time through :meth:`rank` (4 * users_per_block * M bytes of logits) into a
        :class:`RankMetrics` record on the device.  Selecting a batch's positive rows synchronises once
        per batch; nothing else does until the record is read at the end.  Returns
        ``RankMetrics.compute(ks)``; raises ValueError when a ranked target's logit was NaN, and
        ``check_ids()``'s IndexError for an id outside its table."""
        from .rank_metrics import RankMetrics, _check_ks
        ks = _check_ks(ks)
        upb = int(users_per_block)
        if upb < 1:
            raise ValueError("users_per_block must be positive")
        left = None if max_users is None else int(max_users)
        dev = self.device
        metrics = RankMetrics(dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)     # this evaluation's own NaN flag
        for batch, labels in pairs:
            if left is not None and left <= 0:
                break
            rows = (labels.to(dev).reshape(-1) == 1).nonzero().reshape(-1)      # the per-batch sync
            if left is not None:
                rows = rows[:left]
                left -= int(rows.numel())
            if rows.numel() == 0:
                continue
            seq, tgt = batch["item_seq"].to(dev)[rows], batch["item_id"].to(dev).reshape(-1)[rows]
            for r0 in range(0, int(rows.numel()), upb):
                out = self.rank(seq[r0:r0 + upb], tgt[r0:r0 + upb], exclude_history=exclude_history, _status=status)
                metrics.update(out["rank"])
        self.status |= status
        if int(status.item()) & 1:
            raise ValueError("Recommender.evaluate: the logit of a ranked target is NaN")
        result = metrics.compute(ks)
        self.check_ids()
        return result

    # ------------------------------------------------------------------ per-user candidate lists
    def _lists(self, candidates: torch.Tensor, by: str) -> torch.Tensor:
        """candidates [U, C] -> catalogue positions [U, C] (int64, contiguous, on the device); an id
        the catalogue lacks becomes the empty slot -1."""
        cand = candidates.to(self.device).long()
        return (self.positions(cand) if by == "item_id" else cand).contiguous()

    @torch.no_grad()
    def score_lists(self, item_seq: Optional[torch.Tensor], candidates: torch.Tensor, *, by: str = "item_id",
                    logits: bool = False, calibrator=None) -> torch.Tensor:
        """Probabilities (or logits) [U, C] of every user's own candidate list: ``candidates`` [U, C]
        (int64) holds item ids (``by="item_id"``, mapped by :meth:`positions`) or catalogue positions
        (``by="index"``).  A negative entry, or an id the catalogue lacks, is an empty slot and reads
        probability 0 / logit -inf; a position >= M does too and sets the flag ``check_ids()`` raises
        on.  ``item_seq=None`` with one row of candidates is the cold user.  Only the U x C pairs are
        scored (chunked along the slots); nothing is copied to the host and nothing synchronises.
        ``calibrator``: as in :meth:`score`; an empty slot still reads 0."""
        _check_calibrator(calibrator, logits)
        U, _ = _check_lists(item_seq, candidates, by)
        with torch.cuda.device(self.device):
            st = _lib.stream_handle(self.device)
            pos = self._lists(candidates, by)
            _, hist, U, _ = self._hist(item_seq, st)
            out = self._sweep(hist, U, logits, pos)
            if calibrator is not None:
                calibrator.apply(out, out=out)
            live = (pos >= 0) & (pos < self.M)
            out = torch.where(live, out, torch.full_like(out, float("-inf") if logits else 0.0))
        return out

    @torch.no_grad()
    def topk_lists(self, item_seq: Optional[torch.Tensor], candidates: torch.Tensor, k: int, *,
                   exclude_history: bool = True, by: str = "item_id") -> Dict[str, torch.Tensor]:
        """Each user's k best slots of its own list, best first: ``slot`` (index into the user's row of
        ``candidates``), ``index`` (catalogue position), ``item_id``, ``logit``, ``prob``, all [U, k].
        Equal logits go to the smaller slot -- the caller's own order -- and an item listed in two slots
        is two candidates.  Empty slots are never returned; exclude_history as in :meth:`topk`.  With
        fewer than k eligible slots the tail is slot -1, index -1, item_id -1, logit -inf, prob 0."""
        U, C = _check_lists(item_seq, candidates, by, k=k)
        k, dev = int(k), self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            pos = self._lists(candidates, by)
            seq, hist, U, L = self._hist(item_seq, st)
            carry = torch.zeros((U, k), dtype=torch.int64, device=dev)
            out = {n: torch.empty((U, k), dtype=torch.int64, device=dev) for n in ("slot", "index", "item_id")}
            out.update({n: torch.empty((U, k), dtype=torch.float32, device=dev) for n in ("logit", "prob")})
            chunks = list(self._chunks(U, C))
            nws = int(_lib.lib().fbn_rec_topk_workspace_size(U, chunks[0][1], k))
            ws = torch.empty(max(1, (nws + 7) // 8), dtype=torch.int64, device=dev)
            for i, (c0, Cc) in enumerate(chunks):
                a = self._forward_chunk(hist, U, c0, Cc, pos)
                o = out if i == len(chunks) - 1 else {}
                call("fbn_rec_topk_list", ptr(a["logits"]), U, c0, Cc, ptr(pos), C, self.M, ptr(self.cat["item_id"]),
                     ptr(seq), L, int(bool(exclude_history)), k, ptr(carry), ptr(ws), nws, ptr(o.get("slot")),
                     ptr(o.get("index")), ptr(o.get("item_id")), ptr(o.get("logit")), ptr(o.get("prob")),
                     ptr(self.status), st)
        return out

    @torch.no_grad()
    def rank_lists(self, item_seq: Optional[torch.Tensor], candidates: torch.Tensor, target_slot: torch.Tensor, *,
                   exclude_history: bool = True, by: str = "item_id",
                   _status: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The rank of slot ``target_slot[u]`` among the eligible slots of user u's own list, in
        ``topk_lists``' order: ``{"rank": int32 [U], "n_eligible": int32 [U]}``.  A slot is eligible when
        it is not empty and, with exclude_history, passes :meth:`rank`'s id rule (the target's own slot
        stays eligible when the history holds its item).  Rank 0 ("not ranked"): the target slot is
        outside the list, empty, or holds the padding item.  One sweep of the lists into a [U, C] buffer
        of logits, then one ``fbn_rec_rank_list`` call; no host copy and no sync."""
        U, C = _check_lists(item_seq, candidates, by, target_slot=target_slot)
        dev = self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            pos = self._lists(candidates, by)
            tslot = torch.as_tensor(target_slot).to(dev).long().reshape(-1).contiguous()
            seq, hist, U, L = self._hist(item_seq, st)
            buf = self._sweep(hist, U, True, pos)
            out = {"rank": torch.empty(U, dtype=torch.int32, device=dev),
                   "n_eligible": torch.empty(U, dtype=torch.int32, device=dev)}
            call("fbn_rec_rank_list", ptr(buf), C, U, C, ptr(pos), C, self.M, ptr(self.cat["item_id"]), ptr(seq), L,
                 int(bool(exclude_history)), ptr(tslot), ptr(out["rank"]), ptr(out["n_eligible"]),
                 ptr(self.status if _status is None else _status), st)
        return out

    @torch.no_grad()
    def evaluate_sampled(self, pairs, n_neg: int = 99, ks=(5, 10, 20), *, seed: int = 0,
                         exclude_history: bool = True, max_users: Optional[int] = None,
                         users_per_block: int = 1024) -> Dict:
        """HR@K, NDCG@K and MRR@K with sampled negatives: the held-out item of every evaluation user is
        ranked against ``n_neg`` catalogue positions instead of the whole catalogue.  ``pairs`` and the
        selection of the positive rows are :meth:`evaluate`'s.  Per user the list is [target, n_neg
        negatives], target_slot 0.  The negatives are drawn uniformly with replacement from [0, M) by a
        device ``torch.Generator`` seeded with ``seed`` -- one ``torch.randint`` of [users, n_neg] per
        block of at most ``users_per_block`` users, in order, so a result is reproducible for the same
        pairs, seed and blocking.  A draw equal to the target's position becomes an empty slot; padding
        items and (with exclude_history) history items among the draws are not eligible, by
        :meth:`rank_lists`' rule, and a position drawn twice counts twice.  Returns
        ``RankMetrics.compute(ks)`` plus ``"mean_candidates"``: the mean ``n_eligible`` over the ranked
        users (0.0 without any).  Raises as :meth:`evaluate` does."""
        from .rank_metrics import RankMetrics, _check_ks
        ks = _check_ks(ks)
        upb, n_neg = int(users_per_block), int(n_neg)
        if upb < 1:
            raise ValueError("users_per_block must be positive")
        if n_neg < 0:
            raise ValueError("n_neg must not be negative")
        left = None if max_users is None else int(max_users)
        dev = self.device
        metrics = RankMetrics(dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)     # this evaluation's own NaN flag
        n_cand = torch.zeros((), dtype=torch.int64, device=dev)    # sum of n_eligible over the ranked users
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        for batch, labels in pairs:
            if left is not None and left <= 0:
                break
            rows = (labels.to(dev).reshape(-1) == 1).nonzero().reshape(-1)      # the per-batch sync
            if left is not None:
                rows = rows[:left]
                left -= int(rows.numel())
            if rows.numel() == 0:
                continue
            seq, tgt = batch["item_seq"].to(dev)[rows], batch["item_id"].to(dev).reshape(-1)[rows]
            for r0 in range(0, int(rows.numel()), upb):
                tpos = self.positions(tgt[r0:r0 + upb])
                n = int(tpos.numel())
                neg = torch.randint(0, self.M, (n, n_neg), generator=gen, device=dev, dtype=torch.int64)
                neg = torch.where(neg == tpos[:, None], torch.full_like(neg, -1), neg)
                cand = torch.cat([tpos[:, None], neg], dim=1)
                out = self.rank_lists(seq[r0:r0 + upb], cand, torch.zeros(n, dtype=torch.int64, device=dev),
                                      exclude_history=exclude_history, by="index", _status=status)
                metrics.update(out["rank"])
                n_cand += torch.where(out["rank"] > 0, out["n_eligible"], torch.zeros_like(out["n_eligible"])).sum()
        self.status |= status
        if int(status.item()) & 1:
            raise ValueError("Recommender.evaluate_sampled: the logit of a ranked target is NaN")
        result = metrics.compute(ks)
        result["mean_candidates"] = float(n_cand.item()) / result["n"] if result["n"] else 0.0
        self.check_ids()
        return result

    # ------------------------------------------------------------------ retrieval
    def _space(self, space: str, st) -> torch.Tensor:
        """The L2-normalised [M, D] f32 matrix of a space, built on first use and kept (4 M D bytes)."""
        xn = self._knn.get(space)
        if xn is None:
            if space == "content":
                x, row_of = self._x, None
            elif space == "mm":
                x, row_of = self.cache, None
            else:
                x, row_of = self.p["item_emb.weight"], self.cat["item_id"]
            D = int(x.shape[1])
            xn = torch.empty((self.M, D), dtype=torch.float32, device=self.device)
            call("fbn_knn_normalize", ptr(x), D, ptr(row_of), int(x.shape[0]), ptr(xn), self.M, D, ptr(self.err), st)
            self._knn[space] = xn
        return xn

    def _knn_topk(self, xn, Q, k, qn, q_pos, seq, L, st) -> Dict[str, torch.Tensor]:
        """Each query's k most similar catalogue rows through the chunk loop: fbn_knn_scores into
        fbn_rec_topk.  exclude is always on, so padding items never come back; seq [Q, L] (or None)
        names the ids to leave out besides."""
        dev, D = self.device, int(xn.shape[1])
        carry = torch.zeros((Q, k), dtype=torch.int64, device=dev)
        out = {"index": torch.empty((Q, k), dtype=torch.int64, device=dev),
               "item_id": torch.empty((Q, k), dtype=torch.int64, device=dev),
               "score": torch.empty((Q, k), dtype=torch.float32, device=dev)}
        prob = torch.empty((Q, k), dtype=torch.float32, device=dev)     # the sigmoid of a cosine: dropped
        chunks = _knn_chunks(self.M, Q, self.knn_chunk_bytes)
        S = torch.empty(Q * chunks[0][1], dtype=torch.float32, device=dev)
        nws = int(_lib.lib().fbn_rec_topk_workspace_size(Q, chunks[0][1], k))
        ws = torch.empty(max(1, (nws + 7) // 8), dtype=torch.int64, device=dev)
        for i, (m0, Mc) in enumerate(chunks):
            call("fbn_knn_scores", ptr(qn), D, ptr(q_pos), ptr(xn), self.M, Q, m0, Mc, D, ptr(S), st)
            last = i == len(chunks) - 1
            call("fbn_rec_topk", ptr(S), Q, m0, Mc, ptr(self.cat["item_id"]), ptr(seq), L, 1, k, ptr(carry), ptr(ws),
                 nws, ptr(out["index"]) if last else None, ptr(out["item_id"]) if last else None,
                 ptr(out["score"]) if last else None, ptr(prob) if last else None, ptr(self.status), st)
        return out

    @staticmethod
    def _blank(out: Dict[str, torch.Tensor], dead: torch.Tensor) -> None:
        """Rows of queries without a vector become index -1, item_id -1, score -inf (device ops)."""
        dead = dead[:, None]
        out["index"] = torch.where(dead, torch.full_like(out["index"], -1), out["index"])
        out["item_id"] = torch.where(dead, torch.full_like(out["item_id"], -1), out["item_id"])
        out["score"] = torch.where(dead, torch.full_like(out["score"], float("-inf")), out["score"])

    @torch.no_grad()
    def similar_items(self, items: torch.Tensor, k: int, *, space: str = "content", by: str = "item_id",
                      exclude_self: bool = True) -> Dict[str, torch.Tensor]:
        """The k catalogue items most similar to each query item, best first: ``index`` (catalogue
        position), ``item_id``, ``score`` (cosine in ``space``, f32), all [Q, k].  ``items`` [Q] holds
        item ids (``by="item_id"``, mapped by :meth:`positions`) or catalogue positions
        (``by="index"``); the query vector is read out of the catalogue matrix.  Equal scores go to the
        smaller position.  Padding items are never returned; ``exclude_self`` leaves out every catalogue
        row that carries the query's id.  A query that is not in the catalogue gives a row of index -1,
        item_id -1, score -inf, and with fewer than k eligible items the tail is filled the same way.
        Nothing is copied to the host and nothing synchronises."""
        Q = _check_knn(space, k, what="k", by=by, items=items)
        k, dev = int(k), self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            xn = self._space(space, st)
            it = items.to(dev).long()
            pos = (self.positions(it) if by == "item_id" else it).contiguous()
            live = (pos >= 0) & (pos < self.M)
            seq = None
            if exclude_self:                               # fbn_rec_topk's history rule on a one-slot history
                own = self.cat["item_id"][pos.clamp(0, self.M - 1)]
                seq = torch.where(live, own, torch.zeros_like(own)).reshape(Q, 1).contiguous()
            out = self._knn_topk(xn, Q, k, None, pos, seq, 1 if exclude_self else 0, st)
            self._blank(out, ~live)
        return out

    def _queries(self, item_seq: torch.Tensor, xn: torch.Tensor, st):
        """(seq [U, L] on the device, Qn [U, D], n_used [U]) of the users' histories."""
        dev, D = self.device, int(xn.shape[1])
        seq = item_seq.to(dev).long()
        if seq.shape[1] > self.max_len:
            seq = seq[:, seq.shape[1] - self.max_len:]         # the collator keeps the last max_len
        seq = seq.contiguous()
        U, L = int(seq.shape[0]), int(seq.shape[1])
        qn = torch.empty((U, D), dtype=torch.float32, device=dev)
        n_used = torch.empty(U, dtype=torch.int32, device=dev)
        call("fbn_knn_query_pool", ptr(seq) if L else None, U, L, ptr(self._pos), self.V, ptr(xn), self.M, D,
             ptr(qn), ptr(n_used), st)
        return seq, qn, n_used

    @torch.no_grad()
    def retrieve(self, item_seq: torch.Tensor, n: int, *, space: str = "content",
                 exclude_history: bool = True) -> Dict[str, torch.Tensor]:
        """Each user's n nearest catalogue items, best first: ``index``, ``item_id``, ``score`` [U, n]
        and ``n_used`` [U] (int32), the history slots that made the query.  The query is the normalised
        sum of the vectors of the history items the catalogue holds (a repeated id counts each time), so
        ``score`` orders the catalogue as the mean cosine to those items does.  Padding items are never
        returned, nor -- with ``exclude_history`` -- items of the user's own history.  A user with
        ``n_used == 0`` has no query and gets an all-empty row (index -1, item_id -1, score -inf): fall
        back to ``topk(None, k)`` for such users.  ``index`` feeds ``topk_lists(..., by="index")`` as it
        is (-1 is that API's empty slot).  1 <= n <= 256; no host copy and no sync."""
        U = _check_knn(space, n, item_seq=item_seq)
        n, dev = int(n), self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            xn = self._space(space, st)
            seq, qn, n_used = self._queries(item_seq, xn, st)
            L = int(seq.shape[1]) if exclude_history else 0
            out = self._knn_topk(xn, U, n, qn, None, seq if L else None, L, st)
            self._blank(out, n_used == 0)
            out["n_used"] = n_used
        return out

    @torch.no_grad()
    def recommend(self, item_seq: torch.Tensor, k: int, *, n_candidates: int = 200, space: str = "content",
                  exclude_history: bool = True, lam: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """Two stages: :meth:`retrieve` ``n_candidates`` per user, then :meth:`topk_lists` over them
        (``by="index"``).  Returns ``topk_lists``' dict; its logits are the eval forward's for those
        pairs, exactly as ``topk`` gives them.  A user without a usable history gets an all -1 row.
        ``lam`` (a number in [0, 1]): the second stage is :meth:`diversify` over the shortlist instead,
        in the same ``space`` and with its defaults, and its dict is returned."""
        _check_knn(space, n_candidates, what="n_candidates", item_seq=item_seq)
        if not 1 <= int(k) <= K_MAX:
            raise ValueError(f"k must be in 1..{K_MAX}")
        if lam is not None:
            lam = _check_lam(lam)
        cands = self.retrieve(item_seq, n_candidates, space=space, exclude_history=exclude_history)["index"]
        if lam is not None:
            return self.diversify(item_seq, cands, k, lam=lam, space=space, by="index",
                                  exclude_history=exclude_history)
        return self.topk_lists(item_seq, cands, k, exclude_history=exclude_history, by="index")

    @torch.no_grad()
    def evaluate_retrieval(self, pairs, ns=(50, 100, 200), *, space: str = "content", exclude_history: bool = True,
                           max_users: Optional[int] = None, users_per_block: int = 64) -> Dict:
        """Recall of the retrieval stage on held-out interactions: ``pairs`` and the selection of the
        positive rows are :meth:`evaluate`'s; each block's [users, M] similarity rows go to
        ``fbn_rec_rank`` with the held-out item as target, into a :class:`RankMetrics` record.  Returns
        ``RankMetrics.compute(ns)``: ``hr[n]`` is the share of ranked users whose held-out item is among
        ``retrieve(n)``'s -- recall@n.  A user with ``n_used == 0`` has no query: its target becomes -1,
        rank 0, and it is counted in ``n_skipped``.  Ends with ``check_ids()``."""
        from .rank_metrics import RankMetrics, _check_ks
        ns = _check_ks(ns)
        if space not in SPACES:
            raise ValueError(f"space must be one of {SPACES}, not {space!r}")
        upb = int(users_per_block)
        if not 1 <= upb <= Q_MAX:
            raise ValueError(f"users_per_block must be in 1..{Q_MAX}")
        left = None if max_users is None else int(max_users)
        dev = self.device
        metrics = RankMetrics(dev)
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            xn = self._space(space, st)
            D = int(xn.shape[1])
            for batch, labels in pairs:
                if left is not None and left <= 0:
                    break
                rows = (labels.to(dev).reshape(-1) == 1).nonzero().reshape(-1)      # the per-batch sync
                if left is not None:
                    rows = rows[:left]
                    left -= int(rows.numel())
                if rows.numel() == 0:
                    continue
                seqs, tgts = batch["item_seq"].to(dev)[rows], batch["item_id"].to(dev).reshape(-1)[rows]
                for r0 in range(0, int(rows.numel()), upb):
                    seq, qn, n_used = self._queries(seqs[r0:r0 + upb], xn, st)
                    U, L = int(seq.shape[0]), int(seq.shape[1])
                    tpos = self.positions(tgts[r0:r0 + upb])
                    tpos = torch.where(n_used == 0, torch.full_like(tpos, -1), tpos).contiguous()
                    buf = torch.empty((U, self.M), dtype=torch.float32, device=dev)
                    chunks = _knn_chunks(self.M, U, self.knn_chunk_bytes)
                    S = buf if len(chunks) == 1 else torch.empty(U * chunks[0][1], dtype=torch.float32, device=dev)
                    for m0, Mc in chunks:
                        call("fbn_knn_scores", ptr(qn), D, None, ptr(xn), self.M, U, m0, Mc, D, ptr(S), st)
                        if S is not buf:
                            buf[:, m0:m0 + Mc].copy_(S[:U * Mc].view(U, Mc))
                    rank = torch.empty(U, dtype=torch.int32, device=dev)
                    n_el = torch.empty(U, dtype=torch.int32, device=dev)
                    call("fbn_rec_rank", ptr(buf), self.M, U, self.M, ptr(self.cat["item_id"]), ptr(seq) if L else None,
                         L, int(bool(exclude_history)), ptr(tpos), ptr(rank), ptr(n_el), ptr(self.status), st)
                    metrics.update(rank)
        result = metrics.compute(ns)
        self.check_ids()
        return result

    # ------------------------------------------------------------------ diversity
    def _seq(self, item_seq: Optional[torch.Tensor]):
        """(seq [U, L] on the device or None, L) as :meth:`_hist` keeps it, without pooling anything."""
        if item_seq is None:
            return None, 0
        seq = item_seq.to(self.device).long()
        if seq.shape[1] > self.max_len:
            seq = seq[:, seq.shape[1] - self.max_len:]         # the collator keeps the last max_len
        L = int(seq.shape[1])
        return (seq.contiguous(), L) if L else (None, 0)

    def _mmr(self, rel, pos, seq, L, k, lam, xn, exclude_history, st) -> Dict[str, torch.Tensor]:
        """One ``fbn_mmr_select`` call over rel [U, C] f32 and pos [U, C] catalogue positions."""
        dev, (U, C) = self.device, pos.shape
        out = {n: torch.empty((U, k), dtype=torch.int64, device=dev) for n in ("slot", "index", "item_id")}
        out.update({n: torch.empty((U, k), dtype=torch.float32, device=dev) for n in ("relevance", "mmr", "penalty")})
        call("fbn_mmr_select", ptr(rel), int(rel.stride(0)), ptr(pos), C, U, C, ptr(xn), self.M, int(xn.shape[1]),
             ptr(self.cat["item_id"]), ptr(seq), L, int(bool(exclude_history)), lam, k, ptr(out["slot"]),
             ptr(out["index"]), ptr(out["item_id"]), ptr(out["relevance"]), ptr(out["mmr"]), ptr(out["penalty"]),
             ptr(self.status), st)
        return out

    @torch.no_grad()
    def diversify(self, item_seq: Optional[torch.Tensor], candidates: torch.Tensor, k: int, *, lam: float = 0.7,
                  space: str = "content", relevance="prob", by: str = "item_id",
                  exclude_history: bool = True) -> Dict[str, torch.Tensor]:
        """Greedy maximal-marginal-relevance re-ranking of each user's own list (``fbn_mmr_select``,
        DESIGN.md §27): k picks, each the eligible unpicked slot with the largest
        ``lam * relevance - (1 - lam) * max cosine to the slots picked so far`` in ``space``; equal scores
        go to the smaller slot.  ``candidates`` [U, C <= 1024], ``by``, empty slots and ``exclude_history``
        are :meth:`topk_lists`'.  ``relevance``: ``"prob"`` or ``"logit"`` -- the eval forward's numbers
        for the listed pairs, through :meth:`score_lists`' sweep -- or a float32 tensor [U, C] of the
        caller's own scores, in which case nothing is scored.  Returns ``slot``, ``index``, ``item_id``,
        ``relevance``, ``mmr`` (the score when picked) and ``penalty`` (that maximum cosine, 0 for the
        first pick), all [U, k], best first; with fewer than k eligible slots the tail is -1, -1, -1,
        -inf, -inf, 0.  ``lam=1`` is :meth:`topk_lists`' order on the same relevance.  A NaN relevance
        ranks last and sets bit 0 of ``status``.  ``item_seq=None`` with one row is the cold user.
        Nothing is copied to the host and nothing synchronises."""
        U, C, lam = _check_diversify(item_seq, candidates, k, lam, space, relevance, by)
        k, dev = int(k), self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            pos = self._lists(candidates, by)
            if isinstance(relevance, torch.Tensor):
                seq, L = self._seq(item_seq)
                rel = relevance.to(dev)
                if rel.stride(1) != 1:
                    rel = rel.contiguous()
            else:
                seq, hist, U, L = self._hist(item_seq, st)
                rel = self._sweep(hist, U, relevance == "logit", pos)
            return self._mmr(rel, pos, seq, L, k, lam, self._space(space, st), exclude_history, st)

    @torch.no_grad()
    def list_diversity(self, index: torch.Tensor, *, space: str = "content") -> Dict[str, torch.Tensor]:
        """Intra-list diversity of finished lists: ``index`` [U, K <= 256] holds catalogue positions, -1
        (or anything outside the catalogue) an empty slot.  Returns ``{"ild": float64 [U], "n_pairs":
        int32 [U]}``: the mean of ``1 - cosine`` in ``space`` over the pairs of a list's entries, 0 for a
        list with fewer than two.  No host copy and no sync; two calls give equal bits."""
        U, K = _check_positions(index, space)
        dev = self.device
        with torch.cuda.device(dev):
            st = _lib.stream_handle(dev)
            xn = self._space(space, st)
            pos = index.to(dev).long().contiguous()
            out = {"ild": torch.empty(U, dtype=torch.float64, device=dev),
                   "n_pairs": torch.empty(U, dtype=torch.int32, device=dev)}
            call("fbn_list_ild", ptr(pos), K, U, K, ptr(xn), self.M, int(xn.shape[1]), ptr(out["ild"]),
                 ptr(out["n_pairs"]), st)
        return out

    @torch.no_grad()
    def evaluate_diversity(self, pairs, k: int = 10, lams=(1.0, 0.7, 0.5), *, n_candidates: int = 200,
                           space: str = "content", exclude_history: bool = True, max_users: Optional[int] = None,
                           users_per_block: int = 64) -> Dict:
        """What a value of lam costs and buys on held-out interactions.  ``pairs`` and the selection of
        the positive rows are :meth:`evaluate`'s.  Every block of users is retrieved once
        (``n_candidates`` in ``space``) and scored once (probabilities); for each lam the shortlist goes
        through :meth:`diversify` and :meth:`list_diversity`.  Returns ``{lam: {"hr": {k: share of the
        users whose held-out item id is in their list}, "ild": mean ILD over the users whose list has
        two entries or more, "n_ild": their number, "n": the number of users}}``.  The sums stay on the
        device and are read once at the end; selecting a batch's positive rows synchronises once per
        batch.  Ends with ``check_ids()``."""
        if not 1 <= int(k) <= K_MAX:
            raise ValueError(f"k must be in 1..{K_MAX}")
        lams = [_check_lam(x) for x in lams]
        if not lams:
            raise ValueError("lams is empty")
        if space not in SPACES:
            raise ValueError(f"space must be one of {SPACES}, not {space!r}")
        if not 1 <= int(n_candidates) <= K_MAX:
            raise ValueError(f"n_candidates must be in 1..{K_MAX}")
        upb, k = int(users_per_block), int(k)
        if not 1 <= upb <= Q_MAX:
            raise ValueError(f"users_per_block must be in 1..{Q_MAX}")
        left = None if max_users is None else int(max_users)
        dev = self.device
        hits = torch.zeros(len(lams), dtype=torch.int64, device=dev)
        n_ild = torch.zeros(len(lams), dtype=torch.int64, device=dev)
        s_ild = torch.zeros(len(lams), dtype=torch.float64, device=dev)
        n = 0
        for batch, labels in pairs:
            if left is not None and left <= 0:
                break
            rows = (labels.to(dev).reshape(-1) == 1).nonzero().reshape(-1)      # the per-batch sync
            if left is not None:
                rows = rows[:left]
                left -= int(rows.numel())
            if rows.numel() == 0:
                continue
            n += int(rows.numel())
            seqs, tgts = batch["item_seq"].to(dev)[rows], batch["item_id"].to(dev).reshape(-1)[rows].long()
            for r0 in range(0, int(rows.numel()), upb):
                seq, tgt = seqs[r0:r0 + upb], tgts[r0:r0 + upb]
                cands = self.retrieve(seq, n_candidates, space=space, exclude_history=exclude_history)["index"]
                rel = self.score_lists(seq, cands, by="index")
                for i, lam in enumerate(lams):
                    out = self.diversify(seq, cands, k, lam=lam, space=space, relevance=rel, by="index",
                                         exclude_history=exclude_history)
                    hits[i] += ((out["item_id"] == tgt[:, None]) & (out["index"] >= 0)).any(dim=1).sum()
                    d = self.list_diversity(out["index"], space=space)
                    some = d["n_pairs"] > 0
                    n_ild[i] += some.sum()
                    s_ild[i] += torch.where(some, d["ild"], torch.zeros_like(d["ild"])).sum()
        got = torch.stack([hits.double(), n_ild.double(), s_ild]).cpu()          # the one read
        result = {}
        for i, lam in enumerate(lams):
            h, c, s = int(got[0, i]), int(got[1, i]), float(got[2, i])
            result[lam] = {"hr": {k: h / n if n else 0.0}, "ild": s / c if c else 0.0, "n_ild": c, "n": n}
        self.check_ids()
        return result
