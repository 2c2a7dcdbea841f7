"""Python handle of the HIP rollout engine (thin wrapper over the C ABI; numpy in, numpy out)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .config import CONTENT_LEN, MOD_ORDER, SEQ_LEN, RolloutConfig


class UMGenError(RuntimeError):
    pass


def _i64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a), dtype=np.int64)


def _p64(a: Optional[np.ndarray]):
    return a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None


class Engine:
    """One engine = one GPU, one HIP stream.  ``precision``: "bf16" (production), "fp16" (the same kernels with IEEE-half operands:
    the reference's own autocast arithmetic) or "fp32" (exact parity mode)."""

    def __init__(self, cfg: RolloutConfig, precision: str = "bf16", max_batch: int = 1, max_cond_frames: int = 20,
                 device: int = 0, use_graphs: bool = True):
        self.lib = _lib.load_library()
        self.cfg = cfg
        max_cond_frames = min(max_cond_frames, cfg.max_frame_len)
        self.precision = precision
        self.max_batch = max_batch
        self.max_cond_frames = max_cond_frames
        self.last_shared_slots = 0          # of the last rollout(samples=N): window slots of its first frame that ran once per scene
        c = _lib.Config(
            abi_version=4, n_embd=cfg.n_embd, n_head=cfg.n_head, n_ego_tar_layer=cfg.n_ego_tar_layer,
            n_ego_ca_layer=cfg.n_ego_ca_layer, n_map_tar_layer=cfg.n_map_tar_layer, n_box_tar_layer=cfg.n_box_tar_layer,
            n_tar_layer=cfg.n_tar_layer, n_oar_layer=cfg.n_oar_layer, pose_vocab=cfg.pose_vocab_size,
            map_vocab=cfg.map_vocab_size, bbox3d_vocab=cfg.bbox3d_vocab_size, img_vocab=cfg.img_vocab_size,
            aux_vocab=cfg.aux_vocab_size, n_map_embd=cfg.n_map_embd, n_img_embd=cfg.n_img_embd,
            max_frame_len=cfg.max_frame_len, task_num=cfg.task_num, task_id=cfg.task_id,
            precision={"fp32": _lib.PREC_FP32, "bf16": _lib.PREC_BF16, "fp16": _lib.PREC_FP16}[precision], max_batch=max_batch,
            max_cond_frames=max_cond_frames, device=device, use_graphs=int(use_graphs))
        self._h = C.c_void_p()
        rc = self.lib.umgen_create(C.byref(c), C.byref(self._h))
        if rc != 0:
            msg = self.lib.umgen_last_error(self._h).decode() if self._h else "umgen_create failed"
            if self._h:
                self.lib.umgen_destroy(self._h)
                self._h = None
            raise UMGenError(f"umgen_create: {msg} (rc={rc})")

    # -- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.umgen_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc < 0:
            raise UMGenError(f"{what}: {self.lib.umgen_last_error(self._h).decode()} (rc={rc})")
        return rc

    # -- weights -------------------------------------------------------------------------------
    def load_tensor(self, key: str, arr) -> bool:
        """Returns False when the key is not consumed by the rollout (ignored, like strict=False)."""
        a = np.asarray(arr)
        if a.dtype == np.float32:
            dt = _lib.DT_F32
        elif a.dtype == np.float64:
            dt = _lib.DT_F64
        elif a.dtype == np.float16:
            dt = _lib.DT_F16
        elif a.dtype == np.uint16:      # raw bfloat16 bits
            dt = _lib.DT_BF16
        else:
            a = a.astype(np.float32)
            dt = _lib.DT_F32
        a = np.ascontiguousarray(a)
        shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        rc = self._check(self.lib.umgen_load_tensor(self._h, key.encode(), a.ctypes.data_as(C.c_void_p), dt, shape, a.ndim),
                         f"load_tensor({key})")
        return rc == 0

    def load_state_dict(self, items: Iterable[Tuple[str, np.ndarray]]) -> int:
        n = 0
        for k, v in (items.items() if hasattr(items, "items") else items):
            n += bool(self.load_tensor(k, v))
        return n

    def finalize(self):
        self._check(self.lib.umgen_finalize_weights(self._h), "finalize_weights")

    # -- rollout -------------------------------------------------------------------------------
    def _sampling(self, cfg: RolloutConfig, seeds: Sequence[int]):
        s = np.asarray(list(seeds), dtype=np.uint64)
        smp = _lib.Sampling(
            method=0 if cfg.sample_method == "topk" else 1, top_k=cfg.top_k, top_k_map=cfg.top_k_map,
            topk_image=cfg.topk_image, p=cfg.p, p_map=cfg.p_map, temperature=cfg.sfmx_temp,
            rule_constrain=int(cfg.rule_constrain), merge_ar_tar=int(cfg.merage_ar_tar), only_ar=int(cfg.only_ar),
            seeds=s.ctypes.data_as(C.POINTER(C.c_uint64)))
        return smp, s

    @staticmethod
    def _logp_out(lead: Tuple[int, ...], key: str = "logp"):
        """(mod -> float32 [*lead, S_mod] filled with NaN, the umgen_logp_out (key "logp") or umgen_logz_out ("logz") that points at them)"""
        bufs = {m: np.full(tuple(lead) + (CONTENT_LEN[m],), np.nan, np.float32) for m in MOD_ORDER}
        struct = {"logp": _lib.LogpOut, "logz": _lib.LogzOut}[key]
        return bufs, struct(**{f"{key}_{m}": bufs[m].ctypes.data_as(C.POINTER(C.c_float)) for m in MOD_ORDER})

    BIAS_ROWS = {"pose": 3, "map": 1, "bbox3d": 11, "image": 1}

    def _bias_args(self, call: str, logit_bias):
        """logit_bias of a rollout / frame -- class -> float array [vocab] (map, image), [3, vocab] (pose) or [11, vocab] (bbox3d); a [vocab] array for
        pose / bbox3d is every row's -- checked before anything reaches the device: class names, shapes, dtype, NaN / +inf, a row without an allowed
        token.  Returns (the umgen_logit_bias or None, the arrays it points at)."""
        if logit_bias is None:
            return None, None
        if not hasattr(logit_bias, "items"):
            raise UMGenError(f"{call}: logit_bias is a dict class -> array, not {type(logit_bias).__name__}")
        vocab = {"pose": self.cfg.pose_vocab_size, "map": self.cfg.map_vocab_size, "bbox3d": self.cfg.bbox3d_vocab_size, "image": self.cfg.img_vocab_size}
        keep = {}
        for m, t in logit_bias.items():
            if m not in vocab:
                raise UMGenError(f"{call}: logit_bias has no class {m!r} (one of {MOD_ORDER})")
            if t is None:
                continue
            a = np.asarray(t)
            if a.dtype.kind != "f":
                raise UMGenError(f"{call}: logit_bias[{m}] has dtype {a.dtype}, expected a float type")
            rows, V = self.BIAS_ROWS[m], vocab[m]
            if a.shape == (V,) and rows > 1:
                a = np.broadcast_to(a, (rows, V))
            if a.shape != ((rows, V) if rows > 1 else (V,)):
                raise UMGenError(f"{call}: logit_bias[{m}] has shape {np.shape(t)}, expected {(rows, V) if rows > 1 else (V,)}" + (f" or {(V,)}" if rows > 1 else ""))
            a = np.ascontiguousarray(a, dtype=np.float32)
            bad = np.flatnonzero(np.isnan(a.reshape(-1)) | np.isposinf(a.reshape(-1)))
            if bad.size:
                raise UMGenError(f"{call}: logit_bias[{m}] row {int(bad[0]) // V} index {int(bad[0]) % V} is {a.reshape(-1)[bad[0]]} (entries are finite or -inf)")
            empty = np.flatnonzero(np.isneginf(a.reshape(rows, V)).all(axis=1))
            if empty.size:
                raise UMGenError(f"{call}: logit_bias[{m}] row {int(empty[0])} bans every token")
            keep[m] = a
        if not keep:
            return None, None
        return _lib.LogitBias(**{m: a.ctypes.data_as(C.POINTER(C.c_float)) for m, a in keep.items()}), keep

    def _plan_args(self, call: str, sampling, logit_bias, B: int, N: int, new_frames: int, seeds):
        """The umgen_sample_plan of a rollout whose `sampling` is a sequence of RolloutConfig and / or whose `logit_bias` is a constraints.Schedule, checked
        before anything reaches the device with the messages of the C call: -> (the call's umgen_sampling, the plan, whatever both point at).  per-scene
        settings: B entries (a scene's branches share theirs), B*N flat, or [B][N] nested; rule_constrain / merage_ar_tar / only_ar are per call."""
        from .constraints import Schedule
        items = B * N
        keep = []
        cfgs = None
        if isinstance(sampling, RolloutConfig) or sampling is None:
            base = sampling or self.cfg
        else:
            rows = list(sampling)
            if rows and all(not isinstance(r, RolloutConfig) and hasattr(r, "__len__") for r in rows):      # [B][N]
                if len(rows) != B or any(len(r) != N for r in rows):
                    raise UMGenError(f"{call}: sampling has shape [{len(rows)}][{', '.join(str(len(r)) for r in rows)}], expected [{B}][{N}]")
                cfgs = [c for r in rows for c in r]
            elif len(rows) == items:
                cfgs = rows
            elif len(rows) == B:
                cfgs = [c for c in rows for _ in range(N)]
            else:
                raise UMGenError(f"{call}: sampling has {len(rows)} entries, expected {B} (one per scene)" + (f", {items} or [{B}][{N}] (one per branch)" if N > 1 else ""))
            for i, c in enumerate(cfgs):
                if not isinstance(c, RolloutConfig):
                    raise UMGenError(f"{call}: sampling[{i}] is {type(c).__name__}, expected a RolloutConfig")
            base = cfgs[0]
            for i, c in enumerate(cfgs):
                if (bool(c.rule_constrain), bool(c.merage_ar_tar), bool(c.only_ar)) != (bool(base.rule_constrain), bool(base.merage_ar_tar), bool(base.only_ar)):
                    raise UMGenError(f"{call}: sample plan: per_scene[{i}] has rule_constrain / merge_ar_tar / only_ar = {int(c.rule_constrain)} / {int(c.merage_ar_tar)} / "
                                     f"{int(c.only_ar)}, the call's sampling {int(base.rule_constrain)} / {int(base.merage_ar_tar)} / {int(base.only_ar)} (these are per call)")
        smp, skeep = self._sampling(base, seeds)
        keep.append(skeep)
        plan = _lib.SamplePlan()
        if cfgs is not None:
            per = (_lib.Sampling * items)()
            for i, c in enumerate(cfgs):
                per[i] = self._sampling(c, [])[0]
                per[i].seeds = None
            plan.per_scene = C.cast(per, C.POINTER(_lib.Sampling))
            keep.append(per)
        if isinstance(logit_bias, Schedule):
            if len(logit_bias.sets) > _lib.BIAS_SETS_MAX:
                raise UMGenError(f"{call}: sample plan: n_bias_sets={len(logit_bias.sets)} out of range [0,{_lib.BIAS_SETS_MAX}]")
            sets = (_lib.LogitBias * max(1, len(logit_bias.sets)))()
            for q, tabs in enumerate(logit_bias.sets):
                st, k = self._bias_args(f"{call}: sample plan: bias set {q}", tabs or None)
                if st is not None:
                    sets[q] = st
                    keep.append(k)
            try:
                of = logit_bias.resolve(B, N, new_frames)      # int32 [B*N, new_frames]
            except ValueError as err:
                raise UMGenError(f"{call}: {err}") from None
            bad = np.argwhere((of < -1) | (of >= len(logit_bias.sets)))
            if bad.size:
                i, f = (int(x) for x in bad[0])
                raise UMGenError(f"{call}: sample plan: bias_of of scene {i} in new frame {f} is {int(of[i, f])}, outside [-1, {len(logit_bias.sets)})")
            if logit_bias.sets:      # (a schedule without sets constrains nothing: every entry is -1)
                plan.n_bias_sets, plan.bias_sets = len(logit_bias.sets), C.cast(sets, C.POINTER(_lib.LogitBias))
                plan.bias_of = of.ctypes.data_as(C.POINTER(C.c_int32))
                keep += [sets, of]
        else:
            st, k = self._bias_args(call, logit_bias)
            if st is not None:
                one = (_lib.LogitBias * 1)(st)
                plan.n_bias_sets, plan.bias_sets = 1, C.cast(one, C.POINTER(_lib.LogitBias))
                keep += [one, k]
        return smp, plan, keep

    # the diagnostics of score(detail=...) and of rollout / frame (return_detail): key -> (field stem of the C struct, dtype); the "topk_" keys are lists
    _DETAIL_FIELDS = {"rank": ("rank", np.int32), "mass_above": ("mass_above", np.float32), "entropy": ("entropy", np.float32),
                      "topk_tokens": ("topk_tok", np.int32), "topk_logp": ("topk_logp", np.float32)}
    DETAIL_KEYS = tuple(_DETAIL_FIELDS)

    @classmethod
    def _detail_out(cls, struct, keys, lead: Tuple[int, ...], topk: int, fill):
        """(key -> mod -> array [*lead, S_mod] (lists [*lead, S_mod, topk]) filled with fill[dtype], the `struct` -- _lib.ScoreDetailOut or GenDetailOut --
        that points at them)"""
        f = cls._DETAIL_FIELDS
        bufs = {k: {m: np.full(tuple(lead) + (CONTENT_LEN[m],) + ((topk,) if k.startswith("topk_") else ()), fill[f[k][1]], f[k][1]) for m in MOD_ORDER} for k in keys}
        out = struct(**{f"{f[k][0]}_{m}": bufs[k][m].ctypes.data_as(C.POINTER(C.c_int32 if f[k][1] is np.int32 else C.c_float)) for k in keys for m in MOD_ORDER})
        return bufs, out

    @staticmethod
    def _detail_result(bufs, pick=lambda a: a):
        """the buffers as a call returns them: int32 as int64, through pick (a scoring call without the B axis drops it)"""
        return {k: {m: pick(a.astype(np.int64) if a.dtype == np.int32 else a) for m, a in d.items()} for k, d in bufs.items()}

    @classmethod
    def _gen_detail_args(cls, call: str, topk, sampling: RolloutConfig) -> int:
        """topk of a rollout / frame that returns diagnostics, checked before anything reaches the device"""
        if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)) or not 0 <= topk <= _lib.SCORE_TOPK_MAX:
            raise UMGenError(f"{call}: topk={topk!r} is outside [0, {_lib.SCORE_TOPK_MAX}]")
        if not np.isfinite(float(sampling.sfmx_temp)):
            raise UMGenError(f"{call}: diagnostics need a finite sampling temperature, not {sampling.sfmx_temp}")
        return int(topk)

    @classmethod
    def _gen_detail_out(cls, lead: Tuple[int, ...], topk: int):
        """(key -> mod -> array [*lead, S_mod] (lists [*lead, S_mod, topk]) filled with "no head ran": -1 / NaN, the umgen_gen_detail_out that points at them);
        the keys are Engine.score(detail=True)'s, the lists only with topk > 0"""
        keys = [k for k in cls.DETAIL_KEYS if topk > 0 or not k.startswith("topk_")]
        return cls._detail_out(_lib.GenDetailOut, keys, lead, topk, {np.int32: -1, np.float32: np.nan})

    @classmethod
    def _side_out(cls, lead: Tuple[int, ...], logp: bool, logz: bool, detail: bool, topk: int):
        """The optional side outputs of a generation call for a leading shape: (logp buffers, logz buffers, diagnostics buffers, the pointers to their
        umgen_logp_out / umgen_logz_out / umgen_gen_detail_out); None for whatever was not asked for"""
        made = [cls._logp_out(lead) if logp else (None, None), cls._logp_out(lead, "logz") if logz else (None, None),
                cls._gen_detail_out(lead, topk) if detail else (None, None)]
        return tuple(b for b, _ in made) + (tuple(C.byref(s) if s is not None else None for _, s in made),)

    # the two ladders of include/umgen.h, widest rung first: (entry point, what it is the narrowest rung for, how many of the optional arguments it takes) --
    # of (lp, shared_slots, topk, detail, bias | plan, lz) for a rollout, of (lp, topk, detail, bias, lz) for a frame
    _RUNGS = {"rollout": (("umgen_rollout_planned", "plan", 6), ("umgen_rollout_biased", "bias", 6), ("umgen_rollout_detail", "detail", 4),
                          ("umgen_rollout_fan", "fan", 2), ("umgen_rollout_logp", "logp", 1), ("umgen_rollout", None, 0)),
              "frame": (("umgen_frame_biased", "bias", 5), ("umgen_frame_detail", "detail", 3), ("umgen_frame_logp", "logp", 1), ("umgen_frame", None, 0))}

    def _narrowest(self, ladder: str, tail: tuple, **asked):
        """(the narrowest entry point of `ladder` that takes everything asked for, the optional arguments of `tail` it takes)"""
        name, _, n = next(r for r in self._RUNGS[ladder] if r[1] is None or asked.get(r[1]))
        return getattr(self.lib, name), tail[:n]

    @staticmethod
    def _init_token_args(init_tokens: Optional[Dict[str, np.ndarray]], control_test: bool, B: int):
        """init_tokens of a rollout as the arrays of the C call: (T_ctl, control pose, control bbox3d, given map, given bbox3d), int64 [B, T_ctl, S_mod] or
        None.  bbox3d tokens are GIVEN behind a given map without control_test, control tokens otherwise."""
        cp = cb = gm = gb = None
        T_ctl = 0
        if init_tokens is not None:
            # init_tokens["image"] is dropped by the reference before the decode loop ("to avoid image token as init tokens",
            # UMGen.py:1512-1520) but still copied into the output (1640-1651): not a generation path -- refused rather than imitated
            extra = [k for k, v in init_tokens.items() if v is not None and k not in ("pose", "bbox3d", "map")]
            if extra:
                raise UMGenError(f"init_tokens for {extra} are not supported (pose / bbox3d control tokens, given map / map + bbox3d tokens)")
        if init_tokens is not None and init_tokens.get("pose") is not None:
            cp = _i64(init_tokens["pose"])
            if cp.ndim != 3 or cp.shape[0] != B or cp.shape[2] != CONTENT_LEN["pose"]:
                raise UMGenError(f"init_tokens['pose'] has shape {cp.shape}, expected ({B}, T_ctl, {CONTENT_LEN['pose']})")
            T_ctl = cp.shape[1]
        if init_tokens is not None and init_tokens.get("map") is not None:      # the map of every new frame is GIVEN (UMGen.py:1184-1201)
            gm = _i64(init_tokens["map"])
            if gm.ndim != 3 or gm.shape[0] != B or gm.shape[2] != CONTENT_LEN["map"] or (T_ctl and gm.shape[1] != T_ctl):
                raise UMGenError(f"init_tokens['map'] has shape {gm.shape}, expected ({B}, {T_ctl or 'T'}, {CONTENT_LEN['map']})")
            T_ctl = gm.shape[1]
        if init_tokens is not None and init_tokens.get("bbox3d") is not None and not control_test and gm is not None:
            gb = _i64(init_tokens["bbox3d"])                                     # boxes given too (behind a given map)
            if gb.shape != (B, T_ctl, CONTENT_LEN["bbox3d"]):
                raise UMGenError(f"init_tokens['bbox3d'] has shape {gb.shape}, expected {(B, T_ctl, CONTENT_LEN['bbox3d'])}")
        elif init_tokens is not None and init_tokens.get("bbox3d") is not None:   # with or without pose tokens (UMGen.py:1458-1473)
            cb = _i64(init_tokens["bbox3d"])
            if cp is None:
                # (umgen_rollout takes ONE T_ctl for every control / given array: a given map and control boxes must cover the same frames)
                if cb.ndim != 3 or cb.shape[0] != B or cb.shape[2] != CONTENT_LEN["bbox3d"] or (T_ctl and cb.shape[1] != T_ctl):
                    raise UMGenError(f"init_tokens['bbox3d'] has shape {cb.shape}, expected ({B}, {T_ctl or 'T_ctl'}, {CONTENT_LEN['bbox3d']})")
                T_ctl = cb.shape[1]
            elif cb.shape != (B, T_ctl, CONTENT_LEN["bbox3d"]):
                raise UMGenError(f"init_tokens['bbox3d'] has shape {cb.shape}, expected {(B, T_ctl, CONTENT_LEN['bbox3d'])}")
        return T_ctl, cp, cb, gm, gb

    def rollout(self, tokens: Dict[str, np.ndarray], new_frames: int, cond_frames: int = 20,
                input_cond_frames: int = -1, init_tokens: Optional[Dict[str, np.ndarray]] = None,
                control_test: bool = False, seeds: Optional[Sequence[int]] = None,
                sampling=None, return_logp: bool = False, samples: Optional[int] = None,
                return_detail: bool = False, topk: int = 0, logit_bias=None, return_logz: bool = False):
        """tokens: mod -> int64 [B, T, S_mod].  Returns mod -> int64 [B, input_cond_frames + new_frames, S_mod].
        samples=N (umgen_rollout_fan): N sampled futures of every scene off one pass over its history.  seeds: [B, N] or flat B*N (default 0), branch
        (b, s) at b*N + s; init_tokens stay per scene, a scene's branches share them.  Returns mod -> int64 [B, N, input_cond_frames + new_frames, S_mod],
        and with return_logp also mod -> float32 [B, N, new_frames, S_mod]: branch (b, s) has the bits of scene b*N + s of this call on the inputs
        replicated N times.  last_shared_slots records the first frame's window slots that ran once per scene (0: the replicated path).
        samples=None is the plain call.
        return_logp: returns (tokens, mod -> float32 [B, new_frames, S_mod]) -- the log-likelihood of every generated token under the plain AR
        heads at temperature 1 (umgen_rollout_logp, include/umgen.h: Engine.score's measure, taken from the decode steps that sampled the
        token); NaN where no head ran (a controlled pose, given map / bbox3d tokens).  The tokens are the same either way.
        return_detail (with topk <= 16): the result gains, as its last element, the diagnostics of every generated token (umgen_rollout_detail) keyed like
        score(detail=True)'s: "rank" int64, "mass_above" (at the rollout's own temperature), "entropy", and with topk > 0 "topk_tokens" int64 [.., S_mod, topk]
        and "topk_logp"; each mod -> [B, new_frames, S_mod] ([B, N, new_frames, S_mod] with samples).  They are taken from the fp32 row the decode step
        sampled from, for the token logp scores; -1 / NaN where logp is NaN.  Tokens and logp are the same bits with or without them.
        logit_bias (umgen_rollout_biased; umgen_amd.constraints builds the tables): class -> float array, "pose" [3, vocab], "map" [vocab], "bbox3d" [11, vocab]
        (row = attribute, 10 the category token), "image" [vocab]; a [vocab] array for pose / bbox3d is every row's.  Every sampler of every decode step draws from
        logits + bias of its class; -inf bans a token from every draw (not from control / given / forced tokens, nor from the rule constraint's pads).  One set of
        tables per call.  logp and the diagnostics stay on the model's own logits.
        return_logz: the result gains, behind logp, mod -> float32 shaped like logp: lse(logits + bias) - lse(logits) of the AR row per sampled position (+0.0 for
        a class without a table, NaN where logp is NaN); for bans the log of the model's mass on the allowed tokens.
        Sampling plans (umgen_rollout_planned): sampling may be a sequence of RolloutConfig -- B entries (one per scene; a scene's branches share it), or with
        samples=N also B*N flat / [B][N] nested (one per branch) -- and logit_bias a constraints.Schedule (constraints.schedule / per_frame: which set of tables
        scene / branch i draws under in new frame f, -1 = none).  Branch i in frame f returns the bits of the unplanned call that applies its settings and its set
        to everyone; seeds stay per branch; rule_constrain / merage_ar_tar / only_ar must agree across the entries."""
        from .constraints import Schedule
        planned = isinstance(logit_bias, Schedule) or not (sampling is None or isinstance(sampling, RolloutConfig))
        bias_struct, bias_keep = (None, None) if planned else self._bias_args("rollout", logit_bias)
        if return_detail or topk:
            one = sampling is None or isinstance(sampling, RolloutConfig)
            for c in ([sampling or self.cfg] if one else [c for r in sampling for c in ([r] if isinstance(r, RolloutConfig) else r)]):      # (every entry of a plan)
                topk = self._gen_detail_args("rollout", topk, c)
            return_detail = True
        if new_frames < 0:
            raise UMGenError(f"new_frames={new_frames}")
        if input_cond_frames == -1:
            input_cond_frames = cond_frames
        arrs = {m: _i64(tokens[m])[:, :input_cond_frames] for m in MOD_ORDER}
        arrs = {m: np.ascontiguousarray(a) for m, a in arrs.items()}
        B, T_in = arrs["pose"].shape[:2]
        for m in MOD_ORDER:
            if arrs[m].shape != (B, T_in, CONTENT_LEN[m]):
                raise UMGenError(f"tokens[{m}] has shape {arrs[m].shape}, expected {(B, T_in, CONTENT_LEN[m])}")
        lead = (B,)
        if samples is not None:
            if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
                raise UMGenError(f"rollout: samples={samples!r} must be an integer >= 1")
            samples = int(samples)
            lead = (B, samples)
            sd = np.zeros(B * samples, np.uint64) if seeds is None else np.asarray(seeds)
            if sd.shape not in ((B, samples), (B * samples,)):
                raise UMGenError(f"rollout: seeds has shape {sd.shape}, expected {(B, samples)} or {(B * samples,)}")
            if sd.dtype.kind not in "iu":
                raise UMGenError(f"rollout: seeds has dtype {sd.dtype}, expected an integer type")
            seeds = sd.reshape(-1)
        outs = {m: np.empty(lead + (T_in + new_frames, CONTENT_LEN[m]), dtype=np.int64) for m in MOD_ORDER}
        T_ctl, cp, cb, gm, gb = self._init_token_args(init_tokens, control_test, B)
        if planned:
            smp, plan_struct, keep = self._plan_args("rollout", sampling, logit_bias, B, samples or 1, new_frames, seeds if seeds is not None else [0] * B)
        else:
            smp, keep = self._sampling(sampling or self.cfg, seeds if seeds is not None else [0] * B)
        args = (self._h, B, T_in, new_frames, cond_frames, _p64(arrs["pose"]), _p64(arrs["map"]), _p64(arrs["bbox3d"]),
                _p64(arrs["image"]), T_ctl, _p64(cp), _p64(cb), int(control_test), _p64(gm), _p64(gb), C.byref(smp),
                _p64(outs["pose"]), _p64(outs["map"]), _p64(outs["bbox3d"]), _p64(outs["image"]))
        # the optional structs once, then the narrowest entry point that takes what was asked for
        logp, logz, dbufs, (lp, lz, det) = self._side_out(lead + (new_frames,), return_logp, return_logz, return_detail, topk)
        shared = C.c_int32(-1)
        last = C.byref(plan_struct) if planned else C.byref(bias_struct) if bias_struct is not None else None
        fn, tail = self._narrowest("rollout", (lp, C.byref(shared), topk, det, last, lz), plan=planned, bias=bias_struct is not None or return_logz,
                                   detail=return_detail, fan=samples is not None, logp=return_logp)
        rc = fn(*(args if len(tail) < 2 else (self._h, B, samples or 1) + args[2:]), *tail)      # (from umgen_rollout_fan on: B, N)
        self._check(rc, "rollout")
        del keep, bias_keep
        if samples is not None or planned:
            self.last_shared_slots = int(shared.value)
        res = (outs,) + tuple(x for x in (logp, logz, self._detail_result(dbufs) if return_detail else None) if x is not None)
        return res if len(res) > 1 else outs

    def frame(self, window: Dict[str, np.ndarray], frame_idx: int = 0, ctrl: Optional[Dict[str, np.ndarray]] = None,
              control_test: bool = False, seed: int = 0, sampling: Optional[RolloutConfig] = None,
              forced: Optional[Dict[str, np.ndarray]] = None, trace: bool = False, given: Optional[Dict[str, np.ndarray]] = None,
              logp: bool = False, detail: bool = False, topk: int = 0, logit_bias: Optional[Dict[str, np.ndarray]] = None, logz: bool = False):
        """One frame of one scene.  window: mod -> [T, S_mod].  Returns (tokens dict, trace dict or None).
        given: {"map": [1024]} or {"map": ..., "bbox3d": [660]}: the frame's GIVEN tokens (init_tokens of `rollout` for one frame).
        logp: the trace dict (created if need be) gains "logp": mod -> float32 [S_mod], `rollout(return_logp=True)` for this frame; under
        `forced` the values are those of the forced tokens: a step-by-step `score`.
        detail (with topk <= 16): the trace dict gains "detail", `rollout(return_detail=True, topk=topk)` for this frame: key -> mod -> [S_mod] (lists
        [S_mod, topk]).
        logit_bias / logz: `rollout(logit_bias=..., return_logz=True)` for this frame (umgen_frame_biased); the trace dict gains "logz": mod -> float32 [S_mod]."""
        cfg = self.cfg
        bias_struct, bias_keep = self._bias_args("frame", logit_bias)
        if detail or topk:
            topk = self._gen_detail_args("frame", topk, sampling or cfg)
            detail = True
        w = {m: _i64(window[m]) for m in MOD_ORDER}
        T = w["pose"].shape[0]
        outs = {m: np.empty((CONTENT_LEN[m],), dtype=np.int64) for m in MOD_ORDER}
        cp = _i64(ctrl["pose"]) if ctrl is not None and ctrl.get("pose") is not None else None
        cb = _i64(ctrl["bbox3d"]) if ctrl is not None and ctrl.get("bbox3d") is not None else None
        smp, keep = self._sampling(sampling or cfg, [seed])
        tr = None
        tbuf = None
        fz = None
        gz = None
        if trace or forced is not None or given is not None:
            tr = _lib.Trace()
            if given is not None:
                gz = {m: _i64(given[m]).reshape(-1) for m in given}
                tr.given_map = _p64(gz["map"]) if "map" in gz else None
                tr.given_bbox3d = _p64(gz["bbox3d"]) if "bbox3d" in gz else None
            counters = np.zeros(8, np.int32)
            tr.counters = counters.ctypes.data_as(C.POINTER(C.c_int32))
            fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
            if trace:
                tbuf = {"cond": np.zeros((SEQ_LEN, cfg.n_embd), np.float32),
                        "ego_logits": np.zeros((3, cfg.pose_vocab_size), np.float32),
                        "logits_map": np.zeros((1024, cfg.map_vocab_size), np.float32),
                        "logits_bbox3d": np.zeros((660, cfg.bbox3d_vocab_size), np.float32),
                        "logits_image": np.zeros((512, cfg.img_vocab_size), np.float32)}
                tr.cond, tr.ego_logits = fp(tbuf["cond"]), fp(tbuf["ego_logits"])
                tr.logits_map, tr.logits_bbox3d, tr.logits_image = fp(tbuf["logits_map"]), fp(tbuf["logits_bbox3d"]), fp(tbuf["logits_image"])
            if forced is not None:
                fz = {m: _i64(forced[m]).reshape(-1) for m in MOD_ORDER}
                tr.forced_pose, tr.forced_map = _p64(fz["pose"]), _p64(fz["map"])
                tr.forced_bbox3d, tr.forced_image = _p64(fz["bbox3d"]), _p64(fz["image"])
        args = (self._h, T, _p64(w["pose"]), _p64(w["map"]), _p64(w["bbox3d"]), _p64(w["image"]), _p64(cp), _p64(cb),
                int(control_test), C.byref(smp), frame_idx, C.byref(tr) if tr is not None else None,
                _p64(outs["pose"]), _p64(outs["map"]), _p64(outs["bbox3d"]), _p64(outs["image"]))
        lpv, lzv, dbufs, (lp, lz, det) = self._side_out((), logp, logz, detail, topk)
        fn, tail = self._narrowest("frame", (lp, topk, det, C.byref(bias_struct) if bias_struct is not None else None, lz),
                                   bias=bias_struct is not None or logz, detail=detail, logp=logp)
        rc = fn(*args, *tail)
        self._check(rc, "frame")
        del bias_keep
        del keep, fz, gz
        if tr is not None:
            tbuf = tbuf if tbuf is not None else {}
            tbuf["counters"] = dict(zip(("pad_avoid", "control_resample", "rule_checked", "rule_collision", "rule_blanked",
                                         "sampled_ne_forced"), counters[:6].tolist()))
        for key, val in (("logp", lpv), ("logz", lzv), ("detail", self._detail_result(dbufs) if dbufs is not None else None)):
            if val is not None:
                tbuf = tbuf if tbuf is not None else {}
                tbuf[key] = val
        return outs, tbuf

    # -- scoring -------------------------------------------------------------------------------
    @staticmethod
    def _window_lead(pose):
        """(batched, (B, T)) of a window or clip argument, read off its pose array: [B, T, 3], or [T, 3] for one scene"""
        shape = tuple(np.shape(pose))
        batched = len(shape) == 3
        return batched, (shape + (0, 0))[:2] if batched else (1,) + (shape + (0,))[:1]

    def _token_arrays(self, call: str, name: str, arrs: Dict[str, np.ndarray], lead: Tuple[int, ...], batched: bool, int_dtype: bool):
        """One argument of a scoring call, checked before anything reaches the device: arrs[mod] has shape lead + (S_mod,) (without lead's first axis
        when the call is not batched), every token lies inside its vocabulary and, with int_dtype, the arrays are of an integer dtype -- tokens are
        indices: a float array is a caller's mistake, not something to truncate.  Returns mod -> int64 [*lead, S_mod]."""
        vocab = {"pose": self.cfg.pose_vocab_size, "map": self.cfg.map_vocab_size, "bbox3d": self.cfg.bbox3d_vocab_size, "image": self.cfg.img_vocab_size}
        out = {}
        for m in MOD_ORDER:
            if int_dtype and np.asarray(arrs[m]).dtype.kind not in "iu":
                raise UMGenError(f"{call}: {name}[{m}] has dtype {np.asarray(arrs[m]).dtype}, expected an integer type")
            a = _i64(arrs[m])
            want = tuple(lead if batched else lead[1:]) + (CONTENT_LEN[m],)
            if a.shape != want:
                raise UMGenError(f"{call}: {name}[{m}] has shape {a.shape}, expected {want}")
            bad = np.flatnonzero((a.reshape(-1) < 0) | (a.reshape(-1) >= vocab[m]))
            if bad.size:
                raise UMGenError(f"{call}: {name}[{m}] token {int(a.reshape(-1)[bad[0]])} at flat index {int(bad[0])} is outside [0, {vocab[m]})")
            out[m] = a if batched else a[None]
        return out

    @staticmethod
    def _score_out(lead: Tuple[int, ...]):
        """(logp: mod -> float32 [*lead, S_mod] of NaN, argmax: mod -> int32 of -1, the umgen_score_out that points at them)"""
        logp = {m: np.full(tuple(lead) + (CONTENT_LEN[m],), np.nan, np.float32) for m in MOD_ORDER}
        arg = {m: np.full(tuple(lead) + (CONTENT_LEN[m],), -1, np.int32) for m in MOD_ORDER}
        return logp, arg, _lib.ScoreOut(**{f"logp_{m}": logp[m].ctypes.data_as(C.POINTER(C.c_float)) for m in MOD_ORDER},
                                        **{f"argmax_{m}": arg[m].ctypes.data_as(C.POINTER(C.c_int32)) for m in MOD_ORDER})

    @classmethod
    def _score_result(cls, logp, arg, batched: bool, total: bool = False, **extra) -> dict:
        """What a scoring call returns: "logp", "argmax" (int64), with total the ranking key "total", and the call's own entries; without the B
        axis for un-batched inputs."""
        pick = (lambda a: a) if batched else (lambda a: a[0])
        res = {"logp": {m: pick(logp[m]) for m in MOD_ORDER}, "argmax": {m: pick(arg[m].astype(np.int64)) for m in MOD_ORDER}}
        if total:
            res["total"] = pick(cls._candidate_total(logp))
        res.update(extra)
        return res

    def _score_args(self, window: Dict[str, np.ndarray], next_frame: Dict[str, np.ndarray]):
        """Shapes and token ranges of a score call.  Returns (w [B, T, S], nx [B, S], batched).  (Unlike the two calls below, score does not
        refuse float token arrays.)"""
        batched, (B, T) = self._window_lead(window["pose"])
        w = self._token_arrays("score", "window", window, (B, T), batched, False)
        nx = self._token_arrays("score", "next_frame", next_frame, (B,), batched, False)
        if T < 1:
            raise UMGenError("score: the window has no history frame")
        return w, nx, batched

    def _candidate_args(self, window: Dict[str, np.ndarray], candidates: Dict[str, np.ndarray]):
        """Shapes, dtypes and token ranges of a score_candidates call.  Returns (w [B, T, S], cd [B, C, S], batched)."""
        batched, (B, T) = self._window_lead(window["pose"])
        Cn = (tuple(np.shape(candidates["pose"])) + (0, 0))[1 if batched else 0]
        w = self._token_arrays("score_candidates", "window", window, (B, T), batched, True)
        cd = self._token_arrays("score_candidates", "candidates", candidates, (B, Cn), batched, True)
        if T < 1:
            raise UMGenError("score_candidates: the window has no history frame")
        if Cn < 1:
            raise UMGenError("score_candidates: no candidate frame")
        return w, cd, batched

    def _clip_args(self, clip: Dict[str, np.ndarray], input_frames, cond_frames):
        """Shapes, dtypes, token ranges and frame counts of a score_clip call.  Returns (c [B, L, S], cond_frames, batched)."""
        batched, (B, L) = self._window_lead(clip["pose"])
        c = self._token_arrays("score_clip", "clip", clip, (B, L), batched, True)
        if isinstance(input_frames, bool) or not isinstance(input_frames, (int, np.integer)) or not 1 <= input_frames < L:
            raise UMGenError(f"score_clip: input_frames={input_frames!r} must be an integer in [1, {L}) for a clip of {L} frames")
        if cond_frames is None:
            cond_frames = min(self.max_cond_frames, L - 1)
        if isinstance(cond_frames, bool) or not isinstance(cond_frames, (int, np.integer)) or not 1 <= cond_frames <= self.max_cond_frames:
            raise UMGenError(f"score_clip: cond_frames={cond_frames!r} must be an integer in [1, {self.max_cond_frames}] (max_cond_frames)")
        if B < 1 or B > self.max_batch:
            raise UMGenError(f"score_clip: {B} clips, the engine holds max_batch={self.max_batch}")
        return c, int(cond_frames), batched

    @classmethod
    def _detail_args(cls, detail, topk, temperature):
        """What a score call asks for beyond the scores, checked before anything reaches the device.  Returns (keys or None, topk, temperature)."""
        if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)) or not 0 <= topk <= _lib.SCORE_TOPK_MAX:
            raise UMGenError(f"score: topk={topk!r} is outside [0, {_lib.SCORE_TOPK_MAX}]")
        temperature = float(temperature)
        if not (np.isfinite(temperature) and temperature > 0):
            raise UMGenError(f"score: temperature={temperature} must be positive and finite")
        if isinstance(detail, (bool, np.bool_)) or detail is None:
            keys = cls.DETAIL_KEYS if detail or topk > 0 else None
            if keys and topk == 0:
                keys = keys[:3]
        else:
            keys = tuple(detail)
            unknown = [k for k in keys if k not in cls.DETAIL_KEYS]
            if unknown:
                raise UMGenError(f"score: unknown detail outputs {unknown}; known: {cls.DETAIL_KEYS}")
            if topk == 0 and any(k.startswith("topk_") for k in keys):
                raise UMGenError("score: topk_tokens / topk_logp requested with topk=0")
        return keys, int(topk), temperature

    def score(self, window: Dict[str, np.ndarray], next_frame: Dict[str, np.ndarray], detail=False, topk: int = 0,
              temperature: float = 1.0) -> Dict[str, Dict[str, np.ndarray]]:
        """Per-token log-likelihood of a given next frame (umgen_score: one forward pass, no sampling).
        window: mod -> [B, T, S_mod] (or [T, S_mod]); next_frame: mod -> [B, S_mod] (or [S_mod]).
        Returns {"logp": {mod: float32 [B, S_mod]}, "argmax": {mod: int64 [B, S_mod]}} (without the B axis for un-batched inputs):
        logp[mod][b, k] = log softmax(AR head logits at that position)[next_frame[mod][b, k]], the teacher-forced trace of `frame` in closed form.
        With ``detail`` (True, or the names wanted among DETAIL_KEYS) or ``topk > 0`` the dict gains, per position (umgen_score_detail):
        "rank" int64 (logits strictly above the target's: rank < k means inside a top-k sampler's support), "mass_above" (their share of
        softmax(logits / temperature): <= p means kept by a nucleus sampler), "entropy" (nats, temperature 1), "topk_tokens" int64 [.., S_mod, topk]
        and "topk_logp" (the topk <= 16 most likely tokens, best first, with their log-probabilities)."""
        keys, topk, temperature = self._detail_args(detail, topk, temperature)
        w, nx, batched = self._score_args(window, next_frame)
        B, T = w["pose"].shape[:2]
        logp, arg, out = self._score_out((B,))
        tokens = [_p64(w[m]) for m in MOD_ORDER] + [_p64(nx[m]) for m in MOD_ORDER]
        pick = (lambda a: a) if batched else (lambda a: a[0])
        res = {}
        if keys is None:
            self._check(self.lib.umgen_score(self._h, B, T, *tokens, C.byref(out)), "score")
        else:
            bufs, det = self._detail_out(_lib.ScoreDetailOut, keys, (B,), topk, {np.int32: 0, np.float32: 0.0})
            self._check(self.lib.umgen_score_detail(self._h, B, T, *tokens, topk, temperature, C.byref(out), C.byref(det)), "score_detail")
            res = self._detail_result(bufs, pick)
        res.update(self._score_result(logp, arg, batched))
        return res

    @staticmethod
    def _candidate_total(logp: Dict[str, np.ndarray]) -> np.ndarray:
        """The ranking key: float64 sum of logp over all content positions of every candidate, [..]."""
        return sum(np.asarray(logp[m]).astype(np.float64).sum(axis=-1) for m in MOD_ORDER)

    def score_candidates(self, window: Dict[str, np.ndarray], candidates: Dict[str, np.ndarray]) -> dict:
        """Per-token log-likelihoods of C candidate next frames per scene against one history (umgen_score_candidates: the history slots run once
        per scene, every candidate only its last slot, the BlockOAR pass and the heads).
        window: mod -> [B, T, S_mod] (or [T, S_mod]); candidates: mod -> [B, C, S_mod] (or [C, S_mod]).
        Returns {"logp": {mod: float32 [B, C, S_mod]}, "argmax": {mod: int64 [B, C, S_mod]}, "total": float64 [B, C], "shared_slots": int} (without
        the B axis for un-batched inputs).  Entry (b, c) has the bits of score(window[b], candidates[b, c]); "total" is the sum of logp over the 2199
        content positions, the ranking key; "shared_slots" is T - 1 when the history was evaluated once per scene, 0 when every candidate ran the
        whole window (T == 1, slot caches that do not fit, UMGEN_SCORE_SHARE=0)."""
        w, cd, batched = self._candidate_args(window, candidates)
        B, T = w["pose"].shape[:2]
        Cn = cd["pose"].shape[1]
        logp, arg, out = self._score_out((B, Cn))
        tokens = [_p64(w[m]) for m in MOD_ORDER] + [_p64(cd[m]) for m in MOD_ORDER]
        shared = C.c_int32(-1)
        self._check(self.lib.umgen_score_candidates(self._h, B, T, Cn, *tokens, C.byref(out), C.byref(shared)), "score_candidates")
        return self._score_result(logp, arg, batched, total=True, shared_slots=int(shared.value))

    @staticmethod
    def future_windows(T: int, K: int, cond_frames: int):
        """The window rule of score_futures, stated once: [(k, start, n, shared), ...] for the future frames k in [0, K) of a candidate.  Over the
        concatenated sequence history ++ future, frame T + k is scored against its n = min(T + k, cond_frames) frames seq[start : start + n],
        start = T + k - n (clip_windows' rule).  h = max(0, n - k) of them are history frames, and shared = max(0, h - 1) is the number of window
        slots of the map / bbox3d / TAR stacks that every candidate of a scene has in common (slot h - 1 carries the pose of future frame 0): what
        "shared_slots" reports for a frame on the shared path."""
        out = []
        for k in range(K):
            n = min(T + k, cond_frames)
            out.append((k, T + k - n, n, max(0, max(0, n - k) - 1)))
        return out

    def _future_args(self, window: Dict[str, np.ndarray], futures: Dict[str, np.ndarray], cond_frames):
        """Shapes, dtypes, token ranges and counts of a score_futures call.  Returns (w [B, T, S], fu [B, C, K, S], cond_frames, batched)."""
        batched, (B, T) = self._window_lead(window["pose"])
        Cn, Kn = (tuple(np.shape(futures["pose"])) + (0, 0, 0))[1 if batched else 0:][:2]
        w = self._token_arrays("score_futures", "window", window, (B, T), batched, True)
        fu = self._token_arrays("score_futures", "futures", futures, (B, Cn, Kn), batched, True)
        if T < 1:
            raise UMGenError("score_futures: the window has no history frame")
        if Cn < 1:
            raise UMGenError("score_futures: no candidate future")
        if Kn < 1:
            raise UMGenError("score_futures: no future frame")
        if cond_frames is None:
            cond_frames = self.max_cond_frames
        if isinstance(cond_frames, bool) or not isinstance(cond_frames, (int, np.integer)) or not 1 <= cond_frames <= self.max_cond_frames:
            raise UMGenError(f"score_futures: cond_frames={cond_frames!r} must be an integer in [1, {self.max_cond_frames}] (max_cond_frames)")
        if B < 1 or B > self.max_batch:
            raise UMGenError(f"score_futures: {B} scenes, the engine holds max_batch={self.max_batch}")
        return w, fu, int(cond_frames), batched

    def score_futures(self, window: Dict[str, np.ndarray], futures: Dict[str, np.ndarray], cond_frames=None) -> dict:
        """Per-token log-likelihoods of C candidate futures of K frames per scene against one history (umgen_score_futures: the history slots a
        scene's candidates share run once per scene, every candidate only its own tail of slots, the BlockOAR pass and the heads).
        window: mod -> [B, T, S_mod] (or [T, S_mod]); futures: mod -> [B, C, K, S_mod] (or [C, K, S_mod]), integer dtypes; cond_frames (default
        max_cond_frames) caps every frame's window as a rollout's does (future_windows).
        Returns {"logp": {mod: float32 [B, C, K, S_mod]}, "argmax": {mod: int64 [B, C, K, S_mod]}, "total": float64 [B, C, K], "cum_total": float64
        [B, C], "shared_slots": int64 [K]} (without the B axis for un-batched inputs).  Entry (b, c, k) has the bits of score on the window
        future_windows names inside window[b] ++ futures[b, c] and frame futures[b, c, k]; "total" is the sum of logp over the 2199 content
        positions of a frame, "cum_total" its sum over the K frames, the trajectory's ranking key; "shared_slots"[k] is the number of history
        slots evaluated once per scene at frame k, 0 when that frame ran every candidate's whole window (no shared slot left, a tail longer than
        the kernel holds, slot caches that do not fit, UMGEN_SCORE_FUTURES_SHARE=0)."""
        w, fu, cond_frames, batched = self._future_args(window, futures, cond_frames)
        B, T = w["pose"].shape[:2]
        Cn, Kn = fu["pose"].shape[1:3]
        logp, arg, out = self._score_out((B, Cn, Kn))
        tokens = [_p64(w[m]) for m in MOD_ORDER] + [_p64(fu[m]) for m in MOD_ORDER]
        shared = np.full(Kn, -1, np.int32)
        self._check(self.lib.umgen_score_futures(self._h, B, T, Cn, Kn, cond_frames, *tokens, C.byref(out), shared.ctypes.data_as(C.POINTER(C.c_int32))),
                    "score_futures")
        res = self._score_result(logp, arg, batched, total=True, shared_slots=shared.astype(np.int64))
        res["cum_total"] = res["total"].sum(axis=-1)
        return res

    @staticmethod
    def clip_windows(L: int, input_frames: int, cond_frames: int):
        """The window rule of score_clip (and of a rollout, UMGen.py:1597-1603), stated once: [(f, start, n), ...] for every scored frame f in
        [input_frames, L) -- frame f is scored against the n = min(f, cond_frames) frames clip[start : start + n], start = f - n."""
        return [(f, f - min(f, cond_frames), min(f, cond_frames)) for f in range(input_frames, L)]

    def score_clip(self, clip: Dict[str, np.ndarray], input_frames: int, cond_frames=None) -> dict:
        """Per-token log-likelihoods of every frame of a recorded clip, each against the frames before it under the rollout's window rule
        (umgen_score_clip: the teacher-forced counterpart of a rollout; the frames whose window starts at frame 0 are read off one pass).
        clip: mod -> [B, L, S_mod] (or [L, S_mod]), an integer dtype; frames input_frames .. L - 1 are scored, frame f against the
        min(f, cond_frames) frames before it (clip_windows); cond_frames defaults to min(max_cond_frames, L - 1).
        Returns {"logp": {mod: float32 [B, F, S_mod]}, "argmax": {mod: int64 [B, F, S_mod]}, "total": float64 [B, F], "frames": int64 [F],
        "shared_frames": int} with F = L - input_frames (without the B axis for un-batched inputs).  Entry (b, i) has the bits of
        score(clip[b, start : f], clip[b, f]) for f = frames[i]; "total" is the sum of logp over the 2199 content positions of the frame;
        "shared_frames" is the number of frames per clip that shared one pass, 0 when every frame ran its own (fewer than two growing windows,
        no room for the clip buffers, UMGEN_SCORE_CLIP_SHARE=0)."""
        c, cond_frames, batched = self._clip_args(clip, input_frames, cond_frames)
        B, L = c["pose"].shape[:2]
        F = L - int(input_frames)
        logp, arg, out = self._score_out((B, F))
        shared = C.c_int32(-1)
        self._check(self.lib.umgen_score_clip(self._h, B, L, int(input_frames), cond_frames, *[_p64(c[m]) for m in MOD_ORDER], C.byref(out), C.byref(shared)),
                    "score_clip")
        return self._score_result(logp, arg, batched, total=True, frames=np.arange(int(input_frames), L, dtype=np.int64), shared_frames=int(shared.value))

    def dbg_oar_step(self, x: np.ndarray, L: int, use_engine, unmasked: bool = True, return_frag: bool = False):
        """Test hook: one decode step through the BlockOAR layers for x [B, n_embd] at KV length L (appends K/V row L).
        use_engine goes through int() as it is: 0 / False five launches per layer, 1 / True the XCD-resident engine, 2 the batched decode
        layer, 3 the chip-wide engine.  A path that a decode step of B scenes would not take on this engine is refused (UMGenError), never
        replaced by another: 2 runs exactly at the batch sizes the batched layer takes (UMGEN_DECODE_BATCHED), 0 / 1 / 3 at the others.
        return_frag (use_engine 2 only): -> (x out, the fragment-major copy of x behind the step -- the buffer the head's launch would stream --
        as rows [B, n_embd])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        if return_frag:
            frag = np.empty_like(x)
            self._check(self.lib.umgen_dbg_oar_step_frag(self._h, x.shape[0], L, fp(x), fp(out), fp(frag), int(use_engine), int(unmasked)), "dbg_oar_step")
            return out, frag
        self._check(self.lib.umgen_dbg_oar_step(self._h, x.shape[0], L, fp(x), fp(out), int(use_engine), int(unmasked)), "dbg_oar_step")
        return out

    def dbg_oar_cache_get(self, layer: int, scene: int, row0: int, n_rows: int) -> np.ndarray:
        """Test hook: rows [row0, row0 + n_rows) of one (layer, scene) block of the decode K/V cache as uint16 bits [2, n_head, n_rows, 48]."""
        out = np.empty((2, self.cfg.n_head, n_rows, 48), np.uint16)
        self._check(self.lib.umgen_dbg_oar_cache(self._h, layer, scene, row0, n_rows, out.ctypes.data_as(C.c_void_p), 0), "dbg_oar_cache")
        return out

    def dbg_oar_cache_put(self, layer: int, scene: int, row0: int, rows: np.ndarray):
        """Test hook: writes uint16 bits [2, n_head, n_rows, 48] over rows [row0, row0 + n_rows) of one (layer, scene) block of the decode K/V cache."""
        rows = np.ascontiguousarray(rows)
        if rows.dtype != np.uint16 or rows.ndim != 4 or rows.shape[:2] != (2, self.cfg.n_head) or rows.shape[3] != 48:
            raise UMGenError(f"dbg_oar_cache_put: rows {rows.dtype} {rows.shape}, expected uint16 (2, {self.cfg.n_head}, n_rows, 48)")
        self._check(self.lib.umgen_dbg_oar_cache(self._h, layer, scene, row0, rows.shape[2], rows.ctypes.data_as(C.c_void_p), 1), "dbg_oar_cache")

    def dbg_oar_epoch(self, epoch: int):
        """Test hook: moves the decode engines' hand-off tag epoch forward (towards its wrap at 0xE0000000); a smaller value is refused."""
        self._check(self.lib.umgen_dbg_oar_epoch(self._h, int(epoch)), "dbg_oar_epoch")

    # -- test hooks on the background pass of the decode engine's workers (csrc/debug_bg.hip) ---
    STACK_LEN = (SEQ_LEN, 1031, 1693, SEQ_LEN)        # rows per slot of the ego, map, box and TAR stacks (csrc/frame.h stack_len)
    BG_WORKERS = 128

    def dbg_bg_begin(self, window: Dict[str, np.ndarray], ego, cond_cap: int, foreground: bool, chunk: int = 0, margin_ticks: int = -1) -> np.ndarray:
        """Test hook: the next frame's pass over the known slots, as launch_prefix runs it behind a frame with this window (mod -> [T, S_mod]; ego: the
        new frame's 3 pose tokens).  foreground: as stand-alone kernels, synchronised.  Otherwise recorded and uploaded for the workers, nothing runs yet;
        chunk > 0 / margin_ticks >= 0 override every op's chunk / the margin.  Returns the recorded BgOpHead words int32 [n_ops, 8]
        (kind, mode, n_units, chunk, i0..i3); empty for a foreground pass."""
        w = {m: np.ascontiguousarray(np.asarray(window[m]), dtype=np.int32) for m in MOD_ORDER}
        T = w["pose"].shape[0]
        for m in MOD_ORDER:
            if w[m].shape != (T, CONTENT_LEN[m]):
                raise UMGenError(f"dbg_bg_begin: window[{m}] has shape {w[m].shape}, expected {(T, CONTENT_LEN[m])}")
        ego = np.ascontiguousarray(np.asarray(ego).reshape(3), dtype=np.int32)
        heads = np.zeros((4096, 8), np.int32)
        n = C.c_int32(0)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        self._check(self.lib.umgen_dbg_bg_begin(self._h, T, cond_cap, ip(w["pose"]), ip(w["map"]), ip(w["bbox3d"]), ip(w["image"]), ip(ego), int(foreground),
                                                int(chunk), int(margin_ticks), C.byref(n), ip(heads), heads.shape[0]), "dbg_bg_begin")
        return heads[:n.value].copy()

    def dbg_bg_est(self, value: int):
        """Test hook: every unit-time estimate of the queue = value ticks; 0 restores the host's guesses."""
        self._check(self.lib.umgen_dbg_bg_est(self._h, int(value)), "dbg_bg_est")

    def dbg_bg_state(self, n_ops: int):
        """Test hook: (state uint32 [128, 4] -- op, units done | arrived << 31, batch start, - --, ops_done, arrive uint32 [n_ops]) behind a stream sync."""
        state = np.zeros((self.BG_WORKERS, 4), np.uint32)
        arrive = np.zeros(max(n_ops, 1), np.uint32)
        done = C.c_uint32(0)
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        self._check(self.lib.umgen_dbg_bg_state(self._h, up(state), C.byref(done), up(arrive), n_ops), "dbg_bg_state")
        return state, int(done.value), arrive[:n_ops]

    def dbg_bg_steps(self, n: int, est: int = 0, until_done: bool = True, states: bool = False):
        """Test hook: up to n decode launches on the pending pass, est != 0 written over every estimate before each; until_done: stops once ops_done
        is the op count and every worker stands at the end of the list.  Returns (ops_done behind every launch
        uint32 [n_run], the workers' states behind every launch uint32 [n_run, 128, 4] or None)."""
        done = np.zeros(max(n, 1), np.uint32)
        st = np.zeros((max(n, 1), self.BG_WORKERS, 4), np.uint32) if states else None
        n_run = C.c_int32(0)
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)) if a is not None else None  # noqa: E731
        self._check(self.lib.umgen_dbg_bg_steps(self._h, n, int(est), int(until_done), up(st), up(done), C.byref(n_run)), "dbg_bg_steps")
        return done[:n_run.value], (st[:n_run.value] if states else None)

    def dbg_bg_drain(self):
        """Test hook: the launch without an engine part that runs the pending pass to its end, synchronised."""
        self._check(self.lib.umgen_dbg_bg_drain(self._h), "dbg_bg_drain")

    def dbg_bg_end(self):
        """Test hook: empties the queue and forgets the pass: the handle serves ordinary rollouts again."""
        self._check(self.lib.umgen_dbg_bg_end(self._h), "dbg_bg_end")

    def _tcache_shape(self, stack: int):
        if not 0 <= stack < 4:
            raise UMGenError(f"dbg_tcache: stack={stack} (0 ego, 1 map, 2 box, 3 TAR)")
        return (self.max_batch, self.max_cond_frames, self.STACK_LEN[stack], 2 * self.cfg.n_embd)

    def dbg_tcache_get(self, stack: int, block: int) -> np.ndarray:
        """Test hook: the slot cache of one (stack, block) as uint16 bits [max_batch, max_cond_frames, S_stack, 2 n_embd]."""
        out = np.empty(self._tcache_shape(stack), np.uint16)
        self._check(self.lib.umgen_dbg_tcache(self._h, stack, block, out.ctypes.data_as(C.c_void_p), 0), "dbg_tcache")
        return out

    def dbg_tcache_put(self, stack: int, block: int, bits: np.ndarray):
        """Test hook: writes uint16 bits [max_batch, max_cond_frames, S_stack, 2 n_embd] over the slot cache of one (stack, block)."""
        bits = np.ascontiguousarray(bits)
        if bits.dtype != np.uint16 or bits.shape != self._tcache_shape(stack):
            raise UMGenError(f"dbg_tcache_put: bits {bits.dtype} {bits.shape}, expected uint16 {self._tcache_shape(stack)}")
        self._check(self.lib.umgen_dbg_tcache(self._h, stack, block, bits.ctypes.data_as(C.c_void_p), 1), "dbg_tcache")

    # -- measurement ---------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._check(self.lib.umgen_set_profiling(self._h, int(on)), "set_profiling")

    def timings(self) -> dict:
        t = _lib.Timings()
        self._check(self.lib.umgen_get_timings(self._h, C.byref(t)), "get_timings")
        return {n: getattr(t, n) for n, _ in _lib.Timings._fields_}
