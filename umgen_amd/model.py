"""Drop-in ``UMGen`` model class for the reference's callers (evaluate.py:193-220, model_pl.py:173-175, 237-239).

Same surface as projects/models/UMGen.py: ``UMGen(config)`` with the reference's argparse.Namespace config, an
``nn.Module`` (so Lightning can own/move it), ``load_state_dict(sd, strict=False)`` with the reference's key names,
``eval()``, ``.cpu()/.to()``, and ``inference(**kwargs) -> Dict[str, np.ndarray int64 [1, T_out, S_mod]]``.
Internally nothing is a torch op: tokens go to the HIP engine through the C ABI (include/umgen.h).  There is no CPU
fallback -- constructing the engine without a GPU / without libumgen_hip.so raises.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from .config import MOD_ORDER, RolloutConfig
from .engine import Engine, UMGenError
from .registry import MODELS
from .weights import OPTIONAL_KEYS, expected_keys, is_matrix_weight


@MODELS.register_module()
class UMGen(nn.Module):
    def __init__(self, config, precision: str = "bf16", max_batch: int = 1, device: Optional[int] = None):
        super().__init__()
        self.config = config
        self.rcfg = config if isinstance(config, RolloutConfig) else RolloutConfig.from_namespace(config)
        self.precision = precision
        self._engine: Optional[Engine] = None
        # one process per GPU: the harness (Lightning / torchrun) tells the rank its device through LOCAL_RANK and .to(device)
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self._engine_args = dict(precision=precision, max_batch=max_batch, device=int(device))
        self._state: Optional[Dict[str, np.ndarray]] = None      # host copy of the weights: lets the engine move / grow
        self._loaded = False
        self.frame_idx = 0
        self.seed = 0

    # -- engine lifetime -------------------------------------------------------------------------
    @property
    def engine(self) -> Engine:
        if self._engine is None:
            self._engine = Engine(self.rcfg, max_cond_frames=min(20, self.rcfg.max_frame_len), **self._engine_args)
            if self._state is not None:      # re-created on another device / with a larger batch: reload the weights
                for k, arr in self._state.items():
                    if not self._engine.load_tensor(k, arr) and k not in OPTIONAL_KEYS:
                        raise UMGenError(f"re-created engine refused state-dict entry {k!r}")
                if self._loaded:             # (a partial load_state_dict was never finalized: nothing to finalize now either)
                    self._engine.finalize()
        return self._engine

    def _host_copy(self, key: str, arr: np.ndarray) -> np.ndarray:
        """Host copy kept so that the engine can move to another GPU / grow its scene batch: nn.Linear weights in the engine's own
        16-bit storage type (what umgen_load_tensor rounds them to anyway: half the host memory), everything else as given."""
        if arr.dtype == np.float32 and is_matrix_weight(key):
            if self.precision == "bf16":
                return torch.from_numpy(arr).bfloat16().view(torch.int16).numpy().view(np.uint16)
            if self.precision == "fp16":
                return arr.astype(np.float16)
        return arr

    def _recreate(self, **changes):
        """The weights live in the engine's HBM: a new device or a larger scene batch means a new engine."""
        new = dict(self._engine_args, **changes)
        if new == self._engine_args:
            return
        if self._engine is not None:
            warnings.warn(f"umgen_amd.UMGen: engine re-created ({self._engine_args} -> {new}); the weights are uploaded again", stacklevel=3)
            self._engine.close()
            self._engine = None
        self._engine_args = new

    def load_state_dict(self, state_dict, strict: bool = False):
        """infer_fun.load_model_paramter (infer_fun.py:43-50) calls this with ckpt["module"], strict=False."""
        want = expected_keys(self.rcfg)
        eng = self.engine
        missing, unexpected = [], []
        for k in want:
            if k not in state_dict:
                missing.append(k)
        kept: Dict[str, np.ndarray] = {}
        for k, v in state_dict.items():
            t = v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if t.dtype == torch.bfloat16:
                arr = t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
            else:
                arr = t.cpu().float().contiguous().numpy()
            if not eng.load_tensor(k, arr) and k not in OPTIONAL_KEYS:
                unexpected.append(k)
            elif k in want or k in OPTIONAL_KEYS:
                kept[k] = self._host_copy(k, arr)
        self._state = kept
        if strict and (missing or unexpected):
            raise RuntimeError(f"missing keys {missing[:5]}..., unexpected keys {unexpected[:5]}...")
        if not missing:
            eng.finalize()
            self._loaded = True
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    # The parameters live in the engine's HBM, not in nn.Parameters.  `.to(device)` / `.cuda(i)` (model_pl.py:366-368, Lightning's
    # device placement) select the engine's GPU; `.cpu()` (model_pl.py:445-447, around the VAE decode) keeps it where it is.
    @staticmethod
    def _device_index(dev) -> Optional[int]:
        if dev is None:
            return None
        if isinstance(dev, int):
            return dev
        d = torch.device(dev) if not isinstance(dev, torch.device) else dev
        if d.type != "cuda":
            return None
        return d.index if d.index is not None else int(os.environ.get("LOCAL_RANK", "0"))

    def to(self, *args, **kwargs):
        dev = kwargs.get("device")
        for a in args:
            if isinstance(a, (str, torch.device, int)) and not isinstance(a, bool):
                dev = a
        idx = self._device_index(dev)
        if idx is not None:
            self._recreate(device=idx)
        return self

    def cpu(self):
        return self

    def cuda(self, device=None):
        idx = self._device_index(device if device is not None else "cuda")
        if idx is not None:
            self._recreate(device=idx)
        return self

    # -- the hot path ----------------------------------------------------------------------------
    @torch.no_grad()
    def inference(self, new_frames: int, cond_frames: int = 1, input_cond_frames: int = -1, pred_task: str = "image",
                  input_cond_tokens: Optional[Dict[str, torch.Tensor]] = None,
                  init_tokens: Optional[Dict[str, torch.Tensor]] = None, cond_on_tar: bool = False,
                  test_map_affine: bool = False, max_objects=100, control_test=False, return_logp: bool = False,
                  num_samples: Optional[int] = None, return_detail: bool = False, topk: int = 0, logit_bias=None, return_logz: bool = False, **kwargs):
        """UMGen.inference (UMGen.py:1542-1671).  ``cond_on_par`` / ``infer_from_gt`` are swallowed like the reference.
        return_logp (extension): returns (tokens, mod -> torch.float32 [B, new_frames, S_mod]), the log-likelihood of every generated token
        (Engine.rollout's return_logp; NaN on controlled / given positions), beside the tokens it returns today.
        num_samples=N (extension): N sampled futures of every scene off one pass over its history (Engine.rollout's samples).  Returns mod -> torch.int64
        [B, N, T, S_mod]; with return_logp (tokens, logp) where logp holds mod -> torch.float32 [B, N, new_frames, S_mod] and "total", torch.float64
        [B, N, new_frames]: the host sum over a frame's finite entries, the ranking key for best-of-N.  seeds: [B, N] or flat B*N (default seed + i).
        return_detail=True, topk=K (extension): the result gains, as its last element, Engine.rollout's detail dict -- rank, mass_above, entropy and the K most
        likely tokens of every generated token, from the decode step that sampled it -- as key -> mod -> torch tensor; combines with return_logp and num_samples.
        logit_bias=tables, return_logz=True (extension): constrained generation (Engine.rollout's logit_bias / return_logz; umgen_amd.constraints builds the tables,
        arrays or torch tensors).  logz follows logp in the result, mod -> torch.float32 shaped like logp; combines with return_logp, num_samples and return_detail.
        Sampling plans (extension): logit_bias may be a constraints.Schedule and sampling= a sequence of RolloutConfig, as Engine.rollout takes them."""
        return_detail = bool(return_detail) or bool(topk)
        extra = {}      # (only what the call asks for reaches Engine.rollout: the plain calls stay the plain calls)
        from .constraints import Schedule
        if isinstance(logit_bias, Schedule):      # a sampling plan's table sets (constraints.schedule / per_frame), handed on as it is
            extra["logit_bias"] = logit_bias
        elif logit_bias is not None:
            if not hasattr(logit_bias, "items"):
                raise UMGenError(f"logit_bias is a dict class -> array or a constraints.Schedule, not {type(logit_bias).__name__}")
            extra["logit_bias"] = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in logit_bias.items()}
        if kwargs.get("sampling") is not None:    # one RolloutConfig, or a sequence of them: per-scene / per-branch settings (Engine.rollout)
            extra["sampling"] = kwargs["sampling"]
        if return_logz:
            extra["return_logz"] = True
        as_torch = lambda d: {k: {m: torch.from_numpy(v) for m, v in per.items()} for k, per in d.items()}      # noqa: E731
        if pred_task != "pose_map_bbox3d_image":
            raise UMGenError(f"pred_task={pred_task!r}: only 'pose_map_bbox3d_image' (the evaluation task) is implemented")
        if not self._loaded:
            raise UMGenError("load_state_dict() has not provided every tensor the rollout reads")
        assert isinstance(input_cond_tokens, dict)
        toks = {m: (input_cond_tokens[m].detach().cpu().numpy() if isinstance(input_cond_tokens[m], torch.Tensor)
                    else np.asarray(input_cond_tokens[m])) for m in MOD_ORDER}
        init = None
        if init_tokens is not None:
            init = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
                    for k, v in init_tokens.items() if v is not None}      # (pose / bbox3d control, given map / map + bbox3d; the engine rejects anything else)
        B = toks["pose"].shape[0]
        if num_samples is not None:
            if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 1:
                raise UMGenError(f"num_samples={num_samples!r} must be an integer >= 1")
            N = int(num_samples)
            if B * N > self._engine_args["max_batch"]:
                self._recreate(max_batch=B * N)
            seeds = kwargs.get("seeds", [self.seed + i for i in range(B * N)])
            out = self.engine.rollout(toks, new_frames, cond_frames=cond_frames, input_cond_frames=input_cond_frames, init_tokens=init,
                                      control_test=bool(control_test), seeds=seeds, return_logp=bool(return_logp), samples=N,
                                      return_detail=return_detail, topk=topk, **extra)
            if not return_logp and not return_detail and not return_logz:
                return {m: torch.from_numpy(v) for m, v in out.items()}
            res = [{m: torch.from_numpy(v) for m, v in out[0].items()}]
            if return_logp:
                lp = {m: torch.from_numpy(v) for m, v in out[1].items()}
                lp["total"] = torch.from_numpy(sum(np.where(np.isfinite(v), v, 0).astype(np.float64).sum(axis=-1) for v in out[1].values()))
                res.append(lp)
            if return_logz:
                res.append({m: torch.from_numpy(v) for m, v in out[2 if return_logp else 1].items()})
            if return_detail:
                res.append(as_torch(out[-1]))
            return tuple(res)
        if B > self._engine_args["max_batch"]:      # extension over the reference (B = 1): several scenes per call
            self._recreate(max_batch=B)
        seeds = kwargs.get("seeds", [self.seed + i for i in range(B)])
        out = self.engine.rollout(toks, new_frames, cond_frames=cond_frames, input_cond_frames=input_cond_frames,
                                  init_tokens=init, control_test=bool(control_test), seeds=seeds, return_logp=bool(return_logp),
                                  return_detail=return_detail, topk=topk, **extra)
        if not return_logp and not return_detail and not return_logz:
            return out
        res = [out[0]]
        if return_logp:
            res.append({m: torch.from_numpy(v) for m, v in out[1].items()})
        if return_logz:
            res.append({m: torch.from_numpy(v) for m, v in out[2 if return_logp else 1].items()})
        if return_detail:
            res.append(as_torch(out[-1]))
        return tuple(res)

    @staticmethod
    def _score_window(cond: Dict[str, np.ndarray], tgt: Dict[str, np.ndarray], input_cond_frames: int, t: Optional[int], cap: int):
        """What `score` hands the engine: (window mod -> [B, n, S], frame mod -> [B, S]).  Pure numpy, raises UMGenError on bad shapes."""
        for m in MOD_ORDER:
            if cond[m].ndim != 3 or tgt[m].ndim not in (2, 3) or cond[m].shape[0] != tgt[m].shape[0] or tgt[m].ndim != tgt["pose"].ndim:
                raise UMGenError(f"score: input_cond_tokens[{m}] {cond[m].shape} / target_tokens[{m}] {tgt[m].shape}: expected [B, T, S] and [B, S] or [B, T_all, S]")
        have = cond["pose"].shape[1]
        if tgt["pose"].ndim == 2:      # one frame: scored against the last frames of the conditioning clip
            if t is not None:
                raise UMGenError("score: t selects a frame of 3-D target_tokens")
            end, frame = have, tgt
        else:                          # a clip: frame t against the frames before it (t counts in both clips)
            T_all = tgt["pose"].shape[1]
            t = min(have, T_all - 1) if t is None else t
            if not 0 < t < T_all or t > have:
                raise UMGenError(f"score: t={t} needs 1 <= t < {T_all} target frames and at least t of the {have} conditioning frames")
            end, frame = t, {m: tgt[m][:, t] for m in MOD_ORDER}
        n = min(end, cap) if input_cond_frames == -1 else input_cond_frames
        if n < 1 or n > end or n > cap:
            raise UMGenError(f"score: input_cond_frames={input_cond_frames} with {end} frames before the scored one (window cap {cap})")
        return {m: np.ascontiguousarray(cond[m][:, end - n:end]) for m in MOD_ORDER}, frame

    @staticmethod
    def _candidate_window(cond: Dict[str, np.ndarray], cand: Dict[str, np.ndarray], input_cond_frames: int, cap: int):
        """What `score_candidates` hands the engine: the last frames of the conditioning clip, mod -> [B, n, S].  Pure numpy, raises UMGenError on bad shapes."""
        for m in MOD_ORDER:
            if cond[m].ndim != 3 or cand[m].ndim != 3 or cond[m].shape[0] != cand[m].shape[0]:
                raise UMGenError(f"score_candidates: input_cond_tokens[{m}] {cond[m].shape} / candidate_tokens[{m}] {cand[m].shape}: expected [B, T, S] and [B, C, S]")
        have = cond["pose"].shape[1]
        n = min(have, cap) if input_cond_frames == -1 else input_cond_frames
        if n < 1 or n > have or n > cap:
            raise UMGenError(f"score_candidates: input_cond_frames={input_cond_frames} with {have} conditioning frames (window cap {cap})")
        return {m: np.ascontiguousarray(cond[m][:, have - n:have]) for m in MOD_ORDER}

    @staticmethod
    def _topk_acc(rank: Dict[str, np.ndarray]) -> Dict[str, Dict[int, float]]:
        """mod -> {k: share of positions whose target is among the k most likely tokens (rank < k)} for k in (1, 5, 16)"""
        return {m: {k: float((np.asarray(rank[m]) < k).mean()) for k in (1, 5, 16)} for m in MOD_ORDER}

    @torch.no_grad()
    def score(self, input_cond_tokens: Dict[str, torch.Tensor], target_tokens: Dict[str, torch.Tensor], input_cond_frames: int = -1,
              t: Optional[int] = None, detail=False, topk: int = 0, temperature: Optional[float] = None) -> Dict[str, dict]:
        """Per-token log-likelihood of a recorded frame under the model: the reference's loss terms (get_targets, d_loss, F.cross_entropy per
        modality, UMGen.py:539-582) without the sampler.  Scores ``target_tokens[m][:, t]`` ([B, T_all, S_mod]; default: the frame behind the
        conditioning clip) -- or ``target_tokens[m]`` itself when it is one frame [B, S_mod] -- against the ``input_cond_frames`` frames of
        ``input_cond_tokens`` before it (-1: as many as there are, at most the engine's window of 20).
        Returns Engine.score's dict plus "nll": mod -> float64 [B], the mean negative log-likelihood per scene.
        ``detail`` / ``topk`` / ``temperature`` are Engine.score's (rank, mass_above, entropy, the topk most likely tokens per position); a
        temperature of None means the model's sfmx_temp, the one its sampler divides by.  With them the dict also carries "topk_acc":
        mod -> {k: share of positions with rank < k} for k in (1, 5, 16)."""
        Engine._detail_args(detail, topk, 1.0 if temperature is None else temperature)
        if not self._loaded:
            raise UMGenError("load_state_dict() has not provided every tensor the model reads")
        np_ = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
        window, frame = self._score_window({m: np_(input_cond_tokens[m]) for m in MOD_ORDER}, {m: np_(target_tokens[m]) for m in MOD_ORDER},
                                           input_cond_frames, t, min(20, self.rcfg.max_frame_len))
        B = window["pose"].shape[0]
        if B > self._engine_args["max_batch"]:
            self._recreate(max_batch=B)
        res = self.engine.score(window, frame, detail=detail, topk=topk, temperature=self.rcfg.sfmx_temp if temperature is None else temperature)
        if "rank" in res:
            res["topk_acc"] = self._topk_acc(res["rank"])
        res["nll"] = {m: -res["logp"][m].astype(np.float64).mean(axis=1) for m in MOD_ORDER}
        return res

    @torch.no_grad()
    def score_candidates(self, input_cond_tokens: Dict[str, torch.Tensor], candidate_tokens: Dict[str, torch.Tensor],
                         input_cond_frames: int = -1) -> Dict[str, dict]:
        """Ranks C candidate next frames per scene: ``candidate_tokens[m]`` [B, C, S_mod] against the last ``input_cond_frames`` frames of
        ``input_cond_tokens`` [B, T, S_mod] (-1: as many as there are, at most the engine's window of 20).  The history is evaluated once per
        scene (Engine.score_candidates); every entry (b, c) has the bits of `score` on scene b with candidate (b, c) as its one target frame.
        Returns Engine.score_candidates' dict -- "logp", "argmax", "total" (float64 [B, C], the sum of logp: the ranking key), "shared_slots" --
        plus "nll": mod -> float64 [B, C], the mean negative log-likelihood, and "best": int64 [B], the candidate with the highest total."""
        if not self._loaded:
            raise UMGenError("load_state_dict() has not provided every tensor the model reads")
        np_ = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
        cand = {m: np_(candidate_tokens[m]) for m in MOD_ORDER}
        window = self._candidate_window({m: np_(input_cond_tokens[m]) for m in MOD_ORDER}, cand, input_cond_frames, min(20, self.rcfg.max_frame_len))
        B = window["pose"].shape[0]
        if B > self._engine_args["max_batch"]:
            self._recreate(max_batch=B)
        res = self.engine.score_candidates(window, cand)
        res["nll"] = {m: -res["logp"][m].astype(np.float64).mean(axis=-1) for m in MOD_ORDER}
        res["best"] = np.argmax(res["total"], axis=-1).astype(np.int64)
        return res

    @staticmethod
    def _future_split(cond: Dict[str, np.ndarray], fut: Dict[str, np.ndarray], includes_history: Optional[bool]):
        """What `score_futures` hands the engine as futures, mod -> [B, C, K, S]: ``fut`` itself, or -- for the output of
        ``inference(num_samples=N)``, [B, N, T_in + K, S] with every branch's first T_in frames the conditioning clip -- the branches' new frames.
        includes_history None decides by looking: more frames than the clip, and every modality's leading frames equal to it.  Pure numpy, raises
        UMGenError on bad shapes."""
        for m in MOD_ORDER:
            if cond[m].ndim != 3 or fut[m].ndim != 4 or cond[m].shape[0] != fut[m].shape[0] or fut[m].shape[:3] != fut["pose"].shape[:3]:
                raise UMGenError(f"score_futures: input_cond_tokens[{m}] {cond[m].shape} / futures[{m}] {fut[m].shape}: expected [B, T, S] and [B, C, K, S] "
                                 "(or [B, N, T + K, S], an inference(num_samples=N) output)")
        T, L = cond["pose"].shape[1], fut["pose"].shape[2]
        same = L > T and all(fut[m].shape[3:] == cond[m].shape[2:] and np.array_equal(fut[m][:, :, :T], np.broadcast_to(cond[m][:, None], fut[m][:, :, :T].shape))
                             for m in MOD_ORDER)
        if includes_history is None:
            includes_history = same
        elif includes_history and not same:
            raise UMGenError(f"score_futures: includes_history=True, but the first {T} frames of every branch are not the conditioning clip")
        return {m: np.ascontiguousarray(fut[m][:, :, T:]) for m in MOD_ORDER} if includes_history else fut

    @torch.no_grad()
    def score_futures(self, input_cond_tokens: Dict[str, torch.Tensor], futures: Dict[str, torch.Tensor], cond_frames: int = -1,
                      includes_history: Optional[bool] = None) -> Dict[str, dict]:
        """Ranks C candidate futures of K frames per scene: ``futures[m]`` [B, C, K, S_mod] behind the history ``input_cond_tokens[m]`` [B, T, S_mod],
        every future frame scored against the frames before it, at most ``cond_frames`` of them (-1: the engine's window of 20) -- `inference`'s
        window rule with the given frames in place of generated ones (Engine.score_futures: what a scene's candidates share of the history runs
        once per scene).  The output of ``inference(num_samples=N)``, [B, N, T + K, S_mod], is accepted as it is: the history is its first T
        frames, the futures are the branches' new frames (``includes_history``: None looks, True insists, False takes every frame as future).
        Returns Engine.score_futures' dict -- "logp", "argmax", "total" (float64 [B, C, K]), "cum_total" (float64 [B, C], the ranking key),
        "shared_slots" -- plus "nll": mod -> float64 [B, C, K], the mean negative log-likelihood per frame, and "best": int64 [B], the candidate
        with the highest cum_total."""
        if not self._loaded:
            raise UMGenError("load_state_dict() has not provided every tensor the model reads")
        np_ = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
        cond = {m: np_(input_cond_tokens[m]) for m in MOD_ORDER}
        fut = self._future_split(cond, {m: np_(futures[m]) for m in MOD_ORDER}, includes_history)
        cap = min(20, self.rcfg.max_frame_len)
        if isinstance(cond_frames, bool) or not isinstance(cond_frames, (int, np.integer)) or not (cond_frames == -1 or 1 <= cond_frames <= cap):
            raise UMGenError(f"score_futures: cond_frames={cond_frames!r} must be -1 or an integer in [1, {cap}] (window cap)")
        B = cond["pose"].shape[0]
        if B > self._engine_args["max_batch"]:
            self._recreate(max_batch=B)
        res = self.engine.score_futures(cond, fut, cap if cond_frames == -1 else int(cond_frames))
        res["nll"] = {m: -res["logp"][m].astype(np.float64).mean(axis=-1) for m in MOD_ORDER}
        res["best"] = np.argmax(res["cum_total"], axis=-1).astype(np.int64)
        return res

    @torch.no_grad()
    def score_clip(self, tokens: Dict[str, torch.Tensor], input_cond_frames: int = 1, cond_frames: int = 20) -> Dict[str, dict]:
        """The validation loss of the model over a recorded clip: ``tokens[m]`` [B, L, S_mod] (torch or numpy); every frame from
        ``input_cond_frames`` on is scored against the frames before it, at most ``cond_frames`` of them -- `inference`'s window rule with the
        recorded frames in place of generated ones (Engine.score_clip: the frames whose window starts at frame 0 share one pass).
        Returns Engine.score_clip's dict -- "logp", "argmax", "total" (float64 [B, F]), "frames" (int64 [F]), "shared_frames" -- plus "nll":
        mod -> float64 [B, F], the mean negative log-likelihood per frame."""
        if not self._loaded:
            raise UMGenError("load_state_dict() has not provided every tensor the model reads")
        np_ = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
        clip = {m: np_(tokens[m]) for m in MOD_ORDER}
        if clip["pose"].ndim == 3 and clip["pose"].shape[0] > self._engine_args["max_batch"]:
            self._recreate(max_batch=clip["pose"].shape[0])
        res = self.engine.score_clip(clip, input_cond_frames, min(int(cond_frames), 20, self.rcfg.max_frame_len))      # (the engine's window cap)
        res["nll"] = {m: -res["logp"][m].astype(np.float64).mean(axis=-1) for m in MOD_ORDER}
        return res
