"""Logit-bias tables for constrained generation (``Engine.rollout(logit_bias=...)``, include/umgen.h: umgen_rollout_biased).  Host only.

A set of tables is a dict class -> float32 array: "pose" [3, 1024], "map" [1024 codes], "bbox3d" [11, 1028], "image" [codes]; finite entries
shift a token's logit inside the sampler of every decode step, ``-inf`` bans the token.  The builders return such dicts with one class each;
``merge`` adds them up (``-inf`` wins), so a scenario reads

    tables = merge(ban_categories(["pedestrian"]), pose_limits(dx=(0.0, 1.5)))
    tokens, logz = engine.rollout(clip, 10, logit_bias=tables, return_logz=True)

The vocabulary sizes default to UMGen_Large's (config.py); pass ``vocab=`` for another model.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from . import scene_io

CLASSES = ("pose", "map", "bbox3d", "image")
ROWS = {"pose": 3, "map": 1, "bbox3d": 11, "image": 1}           # rows of a class's table: pose component, bbox3d attribute (10: the category token)
DEFAULT_VOCAB = {"pose": 1024, "map": 8192, "bbox3d": 1028, "image": 8192}
CATEGORY_ATTR = 10
CATEGORY_TOKEN0 = 1024                                            # category token = 1024 + index of scene_io.CATEGORIES

Tables = Dict[str, np.ndarray]


def table_shape(mod: str, vocab: int) -> Tuple[int, ...]:
    """the shape of class ``mod``'s table in the C call: [rows, vocab], or [vocab] for the one-row classes"""
    return (ROWS[mod], vocab) if ROWS[mod] > 1 else (vocab,)


def _vocab(mod: str, vocab: Optional[int]) -> int:
    if mod not in ROWS:
        raise ValueError(f"unknown token class {mod!r} (one of {CLASSES})")
    return int(DEFAULT_VOCAB[mod] if vocab is None else vocab)


def _rows(mod: str, attr) -> Sequence[int]:
    """the table rows a builder writes: every row for attr None, else the given row(s)"""
    if attr is None:
        return range(ROWS[mod])
    rows = [int(attr)] if np.isscalar(attr) else [int(a) for a in attr]
    for r in rows:
        if not 0 <= r < ROWS[mod]:
            raise ValueError(f"attr={r} is outside the {ROWS[mod]} rows of class {mod!r}")
    return rows


def _check_rows(mod: str, t: np.ndarray) -> None:
    t2 = t.reshape(ROWS[mod], -1)
    if np.isnan(t2).any() or np.isposinf(t2).any():
        raise ValueError(f"{mod}: bias entries are finite or -inf")
    empty = np.flatnonzero(np.isneginf(t2).all(axis=1))
    if empty.size:
        raise ValueError(f"{mod}: row {int(empty[0])} has no allowed token left")


def bias(mod: str, values, attr=None, vocab: Optional[int] = None) -> Tables:
    """values [vocab] added to the logits of class ``mod`` -- in row(s) ``attr`` (pose component / bbox3d attribute), every row when None"""
    V = _vocab(mod, vocab)
    v = np.asarray(values, dtype=np.float32)
    if v.shape != (V,):
        raise ValueError(f"bias({mod!r}): values have shape {v.shape}, expected {(V,)}")
    t = np.zeros((ROWS[mod], V), np.float32)
    for r in _rows(mod, attr):
        t[r] = v
    _check_rows(mod, t)
    return {mod: t.reshape(table_shape(mod, V))}


def ban(mod: str, tokens: Iterable[int], attr=None, vocab: Optional[int] = None) -> Tables:
    """``tokens`` of class ``mod`` are never drawn (in row(s) ``attr``, every row when None)"""
    V = _vocab(mod, vocab)
    idx = np.asarray(list(tokens), dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= V):
        raise ValueError(f"ban({mod!r}): token outside [0, {V})")
    v = np.zeros(V, np.float32)
    v[idx] = -np.inf
    return bias(mod, v, attr, V)


def allow_only(mod: str, tokens: Iterable[int], attr=None, vocab: Optional[int] = None) -> Tables:
    """only ``tokens`` of class ``mod`` may be drawn (in row(s) ``attr``, every row when None); an empty set raises"""
    V = _vocab(mod, vocab)
    idx = np.asarray(list(tokens), dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= V):
        raise ValueError(f"allow_only({mod!r}): token outside [0, {V})")
    v = np.full(V, -np.inf, np.float32)
    v[idx] = 0.0
    return bias(mod, v, attr, V)


def merge(*tables: Optional[Tables]) -> Tables:
    """the sum of several sets of tables, class by class: finite entries add, -inf wins; a row left without an allowed token raises"""
    out: Tables = {}
    for tb in tables:
        for mod, t in (tb or {}).items():
            if mod not in ROWS:
                raise ValueError(f"unknown token class {mod!r} (one of {CLASSES})")
            t = np.asarray(t, dtype=np.float32)
            if t.ndim == 1 and ROWS[mod] > 1:
                t = np.broadcast_to(t, (ROWS[mod], t.shape[0]))
            if mod in out:
                if out[mod].reshape(ROWS[mod], -1).shape != t.reshape(ROWS[mod], -1).shape:
                    raise ValueError(f"merge: tables of class {mod!r} have shapes {out[mod].shape} and {t.shape}")
                with np.errstate(invalid="ignore"):
                    s = out[mod].reshape(ROWS[mod], -1) + t.reshape(ROWS[mod], -1)
                out[mod] = s.reshape(table_shape(mod, s.shape[1])).astype(np.float32)
            else:
                out[mod] = np.array(t, dtype=np.float32).reshape(table_shape(mod, t.reshape(ROWS[mod], -1).shape[1]))
            _check_rows(mod, out[mod])
    return out


def ban_categories(names: Iterable[str], vocab: Optional[int] = None) -> Tables:
    """no generated agent of these categories (scene_io.CATEGORIES): their category tokens 1024 + index are banned at attribute 10"""
    toks = []
    for n in names:
        if n not in scene_io.CATEGORIES:
            raise ValueError(f"unknown category {n!r} (one of {scene_io.CATEGORIES})")
        toks.append(CATEGORY_TOKEN0 + scene_io.CATEGORIES.index(n))
    return ban("bbox3d", toks, attr=CATEGORY_ATTR, vocab=vocab)


def pose_limits(dx: Optional[Tuple[float, float]] = None, dy: Optional[Tuple[float, float]] = None,
                dheading: Optional[Tuple[float, float]] = None, vocab: Optional[int] = None) -> Tables:
    """Keep the ego step inside an envelope, in the units scene_io.decode_ego returns: per component (lo, hi) or None = free; the pose tokens whose
    decoded value lies outside [lo, hi] are banned.  Derived by decoding every token of every component, so there is no second copy of the bins."""
    V = _vocab("pose", vocab)
    toks = np.repeat(np.arange(V, dtype=np.int64)[:, None], 3, axis=1)
    val = scene_io.decode_ego_numpy(toks).reshape(V, 3)
    t = np.zeros((3, V), np.float32)
    for c, (name, lim) in enumerate((("dx", dx), ("dy", dy), ("dheading", dheading))):
        if lim is None:
            continue
        lo, hi = float(lim[0]), float(lim[1])
        if not lo <= hi:
            raise ValueError(f"pose_limits: {name}=({lo}, {hi}) is empty")
        t[c, (val[:, c] < lo) | (val[:, c] > hi)] = -np.inf
    try:
        _check_rows("pose", t)
    except ValueError:
        raise ValueError("pose_limits: no pose token decodes into the envelope of one component") from None
    return {"pose": t}


BIAS_SETS_MAX = 16      # UMGEN_BIAS_SETS_MAX (include/umgen.h): table sets of one call


class Schedule:
    """Which set of tables a scene / branch draws under in every new frame of ``Engine.rollout(logit_bias=schedule)`` (include/umgen.h:
    umgen_rollout_planned).  ``sets``: the table sets, each a (merged) dict class -> array, ``{}`` for an empty set; ``index``: int array of set numbers,
    -1 = unbiased, with the axes it was given over (``axes``: a subset of ("scene", "branch", "frame") in that order).  Build one with ``schedule`` or
    ``per_frame``."""

    def __init__(self, sets: Sequence[Tables], index: np.ndarray, axes: Tuple[str, ...]):
        self.sets, self.index, self.axes = list(sets), index, tuple(axes)

    def resolve(self, B: int, N: int, new_frames: int) -> np.ndarray:
        """the index of a call over B scenes of N branches and new_frames new frames: int32 [B*N, new_frames]"""
        want = {"scene": B, "branch": N, "frame": new_frames}
        for ax, n in zip(self.axes, self.index.shape):
            if n != want[ax]:
                raise ValueError(f"schedule: the index has {n} entries along its {ax} axis, the call has {want[ax]}")
        shape = tuple(self.index.shape[self.axes.index(ax)] if ax in self.axes else 1 for ax in ("scene", "branch", "frame"))
        full = np.broadcast_to(self.index.reshape(shape), (B, N, new_frames))
        return np.ascontiguousarray(full.reshape(B * N, new_frames), dtype=np.int32)


def schedule(sets: Sequence[Optional[Tables]], index, axis: Optional[str] = None) -> Schedule:
    """A schedule of table sets.  ``sets``: a list of table dicts (``None``: an empty set -- its scenes are unbiased), at most 16.  ``index``: integers in
    [-1, len(sets)), -1 = unbiased, broadcast to [B*N, new_frames] by its SHAPE, never by the sizes that happen to match:

        a scalar                       every scene, branch and frame
        [B]                            per scene (a scene's branches and all frames share it)      -- the default for one dimension
        [new_frames], axis="frame"     per new frame (all scenes and branches share it)
        [B, N]                         per branch
        [B, N, new_frames]             the full index (N = 1 without ``samples``)

    Two dimensions always mean [B, N]: a [B, new_frames] array would be indistinguishable, so per-scene-and-frame indices are given in full, as
    [B, N, new_frames].  Refused: more than three dimensions, ``axis`` with anything but one dimension, an ``axis`` other than "scene" / "frame", entries
    outside [-1, len(sets)), more than 16 sets; a shape that does not fit the call is refused by the call (``Schedule.resolve``)."""
    sets = [merge(t) for t in sets]
    if len(sets) > BIAS_SETS_MAX:
        raise ValueError(f"schedule: {len(sets)} table sets, a call takes at most {BIAS_SETS_MAX}")
    idx = np.asarray(index)
    if idx.dtype.kind not in "iu":
        raise ValueError(f"schedule: the index has dtype {idx.dtype}, expected integers")
    if axis not in (None, "scene", "frame"):
        raise ValueError(f"schedule: axis={axis!r} (one of None, 'scene', 'frame')")
    if axis is not None and idx.ndim != 1:
        raise ValueError(f"schedule: axis={axis!r} names the axis of a one-dimensional index, this one has shape {idx.shape}")
    if idx.ndim > 3:
        raise ValueError(f"schedule: the index has shape {idx.shape}; accepted are a scalar, [B], [new_frames] with axis='frame', [B, N] and [B, N, new_frames]")
    axes = {0: (), 1: ("frame",) if axis == "frame" else ("scene",), 2: ("scene", "branch"), 3: ("scene", "branch", "frame")}[idx.ndim]
    if idx.size and (idx.min() < -1 or idx.max() >= len(sets)):
        raise ValueError(f"schedule: index entries lie in [-1, {len(sets)}), found {int(idx.min())} .. {int(idx.max())}")
    return Schedule(sets, idx.astype(np.int32), axes)


def per_frame(tables_by_frame: Sequence[Optional[Tables]]) -> Schedule:
    """One set of tables per new frame, for every scene and branch: ``tables_by_frame[f]`` applies in new frame f (``None``: unbiased).  Frames that hand over
    the SAME dict object share a set (deduplicated by identity, not by value), so a long rollout that switches between a few constraints fits the call's 16
    sets; more distinct objects are refused."""
    sets, seen, index = [], {}, []
    for t in tables_by_frame:
        if t is None:
            index.append(-1)
            continue
        if id(t) not in seen:
            seen[id(t)] = len(sets)
            sets.append(t)
        index.append(seen[id(t)])
    if len(sets) > BIAS_SETS_MAX:
        raise ValueError(f"per_frame: {len(sets)} distinct table sets over {len(index)} frames, a call takes at most {BIAS_SETS_MAX} (reuse one dict object for "
                         "frames that share their tables)")
    return schedule(sets, np.asarray(index, dtype=np.int32), axis="frame")


def log_importance_weight(tokens: Dict[str, np.ndarray], logz: Dict[str, np.ndarray], tables) -> np.ndarray:
    """The log importance weight of every generated frame of a constrained rollout against the model: the sum over the frame's sampled positions
    of ``logz - r[tok]`` (include/umgen.h), float64 [..., new_frames].

    ``tokens`` and ``logz`` are what ``Engine.rollout(clip, F, logit_bias=tables, return_logz=True)`` returned: mod -> int [..., T, S_mod] whose LAST
    ``F`` frames are the generated ones (only those are read), and mod -> float [..., F, S_mod].  Positions whose logz is NaN (no sampler ran: a
    controlled pose, given tokens) are skipped; a class without a table has r = 0.

    Exact under these conditions only: the rollout drew with an UNTRUNCATED sampler (today: ``sample_method="topp"`` with p = p_map = 1) at temperature
    1, and no token came from a control or pad-avoid resample (``only_ar`` and no control slots) -- then the proposal's density of a drawn token is
    softmax(v + r)[tok] = exp(lp + r[tok] - logz), and model / proposal = exp(logz - r[tok]).  A truncated or tempered sampler renormalises
    differently, and a resampled token was drawn from another head; neither is accounted for here.

    ``tables`` may be the ``Schedule`` of a planned rollout: every position then reads the row of ITS OWN set -- branch i in new frame f the set
    ``schedule.resolve(B, N, F)[i, f]``, r = 0 for -1 and for a class without a table in that set; the leading axes of logz are then [B] or [B, N]."""
    if isinstance(tables, Schedule):
        return _scheduled_weight(tokens, logz, tables)
    tables = merge(tables)
    total = None
    for mod in CLASSES:
        lz = np.asarray(logz[mod], dtype=np.float64)
        F = lz.shape[-2]
        tok = np.asarray(tokens[mod])
        if tok.shape[-1] != lz.shape[-1] or tok.shape[:-2] != lz.shape[:-2] or tok.shape[-2] < F:
            raise ValueError(f"{mod}: tokens {tok.shape} and logz {lz.shape} do not belong together")
        tok = tok[..., tok.shape[-2] - F:, :].astype(np.int64)
        r = np.zeros(lz.shape, np.float64)
        if mod in tables:
            t = tables[mod].reshape(ROWS[mod], -1).astype(np.float64)
            if tok.size and (tok.min() < 0 or tok.max() >= t.shape[1]):
                raise ValueError(f"{mod}: token outside the table's [0, {t.shape[1]})")
            row = np.arange(lz.shape[-1]) % ROWS[mod]      # pose component / bbox3d attribute of the position; 0 for the one-row classes
            r = t[np.broadcast_to(row, tok.shape), tok]
        skip = np.isnan(lz)
        w = np.where(skip, 0.0, lz - np.where(skip, 0.0, r)).sum(axis=-1)
        total = w if total is None else total + w
    return total


def _scheduled_weight(tokens: Dict[str, np.ndarray], logz: Dict[str, np.ndarray], sch: Schedule) -> np.ndarray:
    """log_importance_weight under a Schedule: the per-set weights, picked per (branch, frame) by the resolved index"""
    lead = np.asarray(logz[CLASSES[0]]).shape[:-2]
    F = np.asarray(logz[CLASSES[0]]).shape[-2]
    if len(lead) not in (1, 2):
        raise ValueError(f"logz has leading axes {lead}; a scheduled rollout returns [B, F, S_mod] or [B, N, F, S_mod]")
    B, N = lead[0], (lead[1] if len(lead) == 2 else 1)
    of = sch.resolve(B, N, F).reshape(lead + (F,))
    total = log_importance_weight(tokens, logz, None)      # r = 0: unbiased positions and NaN skipping
    for q, tabs in enumerate(sch.sets):
        if tabs and (of == q).any():
            total = np.where(of == q, log_importance_weight(tokens, logz, tabs), total)
    return total
