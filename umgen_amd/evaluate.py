"""Build-owned counterpart of projects/tools/evaluate.py + the token-saving half of projects/tools/model_pl.py.

    python -m umgen_amd.evaluate --infer_task video --set_num_new_frames 30 --ckpt_dir data/weights/UMGen_Large.pt \
        --data_test_root data/tokenized_scenes --output_path output/UMGen/

Flags and resolution follow evaluate.py:28-133 and infer_fun.py:56-159 (set_inference_setting / set_model_config):
``video`` -> input_cond_frames 20, new frames = --set_num_new_frames; ``control`` -> input_cond_frames 13, 30 frames
(infer_fun.py:64-71); ``--model_scale larger`` -> 36 TAR layers; sampler "topk", k = 5 / 5 / 16.  The artefact is the
one parity is judged on: ``<output_path>/saved_token/<name>_tokens.pkl`` = pickle of dict mod -> np.int64
[1, T_out, S_mod] (model_pl.py:350-355), skipped when it already exists (model_pl.py:215-216).
VAE decoding / video rendering (model_pl.py:254ff) stay on the reference side.

Scenes are read from ``*.pkl`` clips in the reference's raw ``tokenized_origin_scenes`` schema (tokenised on the fly exactly as
``NuPlanTokenDataset`` + ``transforms_val`` do, see scene_io.py), from ``*.npz`` / ``*.pkl`` files that already hold the token
dict handed to ``inference`` (pose [T,3] / map [T,1024] / bbox3d [T,660] / image [T,512], optional control_pose /
control_bbox3d), or generated with ``--synthetic N``.  Under ``torchrun`` the scenes are sharded over ranks (umgen_amd/shard.py).
"""
from __future__ import annotations

import argparse
import dataclasses
import glob
import os
import pickle
import sys

import numpy as np

from .config import MOD_ORDER, large_config, tiny_config
from .scene_io import is_raw_scene, save_tokens, scene_tokens
from .synth import synthetic_control, synthetic_scene
from .weights import expected_keys, synth_tensor


def str2bool(v):   # evaluate.py declares these flags with type=bool (True for ANY non-empty string); keep it parseable
    return str(v).lower() not in ("0", "false", "no", "")


def positive_int(v):
    k = int(v)
    if k < 1:
        raise argparse.ArgumentTypeError(f"{v!r} is not a positive integer")
    return k


def temperature_list(v):
    try:
        ts = [float(x) for x in str(v).split(",") if x.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"{v!r} is not a comma-separated list of temperatures") from None
    if not ts or any(not (t > 0 and np.isfinite(t)) for t in ts):
        raise argparse.ArgumentTypeError(f"{v!r}: temperatures are finite and > 0")
    return ts


def build_parser():
    p = argparse.ArgumentParser("umgen_amd.evaluate")
    p.add_argument("--pred_task", type=str, default="pose_map_bbox3d_image")
    p.add_argument("--ckpt_dir", type=str, default="data/weights/UMGen_Large.pt")
    p.add_argument("--model_scale", type=str, default="larger", choices=["larger", "stander", "debug"])
    p.add_argument("--infer_task", type=str, default="control")
    p.add_argument("--rule_constrain", type=str2bool, default=True)
    p.add_argument("--set_num_new_frames", type=int, default=10)
    p.add_argument("--debug", type=str2bool, default=False, help="skip the checkpoint and use random-init weights")
    p.add_argument("--output_path", default="output/UMGen/")
    p.add_argument("--launcher", type=str, default=None)
    # sampler (config.py:442-463 infer_task_config)
    p.add_argument("--top_k", type=positive_int, default=5, help="top-k of the pose and bbox3d heads (the engine takes 1 .. 16)")
    p.add_argument("--top_k_map", type=positive_int, default=5, help="top-k of the map head")
    p.add_argument("--topk_image", type=positive_int, default=16, help="top-k of the image head")
    p.add_argument("--top_p", type=float, default=0.4)
    p.add_argument("--sample_method", type=str, default="topk")
    # build-side additions
    p.add_argument("--data_test_root", type=str, default=None, help="directory of token-dict scenes (*.npz / *.pkl)")
    p.add_argument("--synthetic", type=int, default=0, help="generate N synthetic scenes instead of reading files")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"],
                   help="bf16: production; fp16: the reference's own autocast arithmetic; fp32: exact parity mode")
    p.add_argument("--batch", type=int, default=1, help="scenes rolled out together per GPU")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--ban_category", action="append", default=[], metavar="NAME",
                   help="constrained generation: no generated agent of this category (vehicle / bicycle / pedestrian); repeatable")
    p.add_argument("--ban_from_frame", type=int, default=0, metavar="F",
                   help="the tables of --ban_category apply from generated frame F on (0: every generated frame); a per-frame schedule inside ONE rollout call")
    p.add_argument("--num_samples", type=positive_int, default=1, help="sampled futures per scene (saved as <scene>_s<k>)")
    p.add_argument("--temperatures", type=temperature_list, default=None, metavar="T1,T2,...",
                   help="sampling temperature per future: sample s draws at temperatures[s %% len]; one call for all of them")
    return p


def plan_kwargs(args, cfg, n_scenes, new_frames):
    """What --num_samples / --temperatures / --ban_category / --ban_from_frame add to Engine.rollout for a batch of n_scenes scenes: samples, per-branch sampling
    (a sampling plan only when the temperatures differ), and the tables -- one set for the call, or a per-frame schedule when they start at a later frame"""
    kw = {}
    N = args.num_samples
    if N > 1:
        kw["samples"] = N
    if args.temperatures:
        temps = [args.temperatures[s % len(args.temperatures)] for s in range(N)]
        per = [dataclasses.replace(cfg, sfmx_temp=t) for t in temps]
        kw["sampling"] = per[0] if len(set(temps)) == 1 else [list(per) for _ in range(n_scenes)]
    if args.ban_from_frame < 0:
        raise ValueError(f"--ban_from_frame {args.ban_from_frame}: a generated frame index >= 0")
    if args.ban_category:
        from .constraints import ban_categories, per_frame
        tables = ban_categories(args.ban_category, vocab=cfg.bbox3d_vocab_size)
        F = min(args.ban_from_frame, new_frames)
        kw["logit_bias"] = tables if F == 0 else per_frame([None] * F + [tables] * (new_frames - F))
    return kw


def resolve(args):
    """infer_fun.set_inference_setting / set_model_config value resolution."""
    if args.infer_task == "video":
        new_frames, input_cond = args.set_num_new_frames, 20
    elif "control" in args.infer_task:
        new_frames, input_cond = 30, 13
    else:
        new_frames, input_cond = -1, 20
    if args.model_scale == "debug":
        cfg = tiny_config()
    else:
        cfg = large_config(n_tar_layer=36 if args.model_scale == "larger" else 24)
    cfg.top_k, cfg.p, cfg.sample_method, cfg.rule_constrain = args.top_k, args.top_p, args.sample_method, bool(args.rule_constrain)
    cfg.top_k_map, cfg.topk_image = args.top_k_map, args.topk_image
    return cfg, new_frames, input_cond


def load_scene(path, block_size=42, sampling_gap=4, start_index=10):
    d = dict(np.load(path)) if path.endswith(".npz") else pickle.load(open(path, "rb"))
    if is_raw_scene(d):        # a tokenized_origin_scenes clip: what NuPlanTokenDataset + transforms_val turn it into (scene_io.py)
        d = scene_tokens(d, block_size, sampling_gap, start_index)
    if "dataset_token" in d:   # control pickle layout (model_pl.py:137-171)
        ctl = d.get("control_dict", {})
        d = dict(d["dataset_token"], **{f"control_{k}": v for k, v in ctl.items()})
    sc = {m: np.asarray(d[m]).reshape(1, -1, np.asarray(d[m]).shape[-1]).astype(np.int64) for m in MOD_ORDER}
    ctl = {k[8:]: np.asarray(v).reshape(1, -1, np.asarray(v).shape[-1]).astype(np.int64) for k, v in d.items() if k.startswith("control_")}
    return sc, (ctl or None)


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    import torch.distributed as dist

    from .engine import Engine
    from .shard import scene_partition, sharded_rollout

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if world > 1:   # one process per GPU: bind the device BEFORE the RCCL communicator exists
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    cfg, new_frames, input_cond = resolve(args)
    control = "control" in args.infer_task
    T_hist = min(20, cfg.max_frame_len - 1)
    if args.synthetic:
        scenes = [(f"synthetic_{i:04d}", synthetic_scene(i, n_frames=min(input_cond, T_hist)),
                   synthetic_control(i, n_frames=new_frames) if control else None) for i in range(args.synthetic)]
    else:
        files = sorted(glob.glob(os.path.join(args.data_test_root or "", "*.npz")) + glob.glob(os.path.join(args.data_test_root or "", "*.pkl")))
        if not files:
            sys.exit("no scenes: pass --data_test_root <dir with *.npz|*.pkl token dicts> or --synthetic N")
        # dataset_block_size = set_num_new_frames + cond_frames (infer_fun.py:176-186), sampling_gap 4, start_index 10 (evaluate.py:157)
        block = (args.set_num_new_frames if args.infer_task == "video" else max(new_frames, 0)) + 20
        scenes = [(os.path.basename(f)[:-4],) + load_scene(f, block_size=block) for f in files]
    save_dir = os.path.join(args.output_path, "saved_token")
    os.makedirs(save_dir, exist_ok=True)
    # skip-if-exists stays per scene (model_pl.py:215-216); every rank takes the same decision before anybody writes
    todo = []
    for sid, (name, _, _) in enumerate(scenes):
        if os.path.exists(os.path.join(save_dir, (name if args.num_samples == 1 else f"{name}_s{args.num_samples - 1}") + "_tokens.pkl")):
            if rank == 0:
                print(name, " has been processed")
        else:
            todo.append(sid)
    if world > 1:
        dist.barrier()
    if not todo:
        if world > 1:
            dist.destroy_process_group()
        return
    eng = Engine(cfg, precision=args.precision, max_batch=args.batch * args.num_samples, max_cond_frames=T_hist, device=local_rank)
    if args.debug:
        for key, shape in expected_keys(cfg).items():
            eng.load_tensor(key, synth_tensor(key, shape, seed=0))
    else:
        ckpt = torch.load(args.ckpt_dir, map_location="cpu")
        sd = ckpt["model_state"] if "model_state" in ckpt else ckpt          # infer_fun.py:43-50
        for k, v in sd["module"].items():
            eng.load_tensor(k, v.float().numpy() if v.dtype != torch.bfloat16 else v.view(torch.int16).numpy().view(np.uint16))
    eng.finalize()
    # Scenes that can share a batch: same history length, same number of new frames, same kind of control tokens.  Each group goes
    # through umgen_amd.shard.sharded_rollout -- THE multi-scene / multi-GPU implementation (scene i -> rank i mod P, `--batch`
    # scenes per engine call, one all-gather of the sampled tokens at the end) that bench.py and the tests use too.
    groups = {}
    for sid in todo:
        _, toks, ctl = scenes[sid]
        icf = min(input_cond, toks["pose"].shape[1])
        nf = new_frames if new_frames >= 0 else toks["pose"].shape[1] - icf
        key = (icf, nf, tuple(sorted((k, v.shape[1:]) for k, v in ctl.items())) if ctl else None)
        groups.setdefault(key, []).append(sid)
    N = args.num_samples
    for (icf, nf, _), sids in groups.items():
        def rollout_fn(toks, seeds, scene_ids):
            ctls = [scenes[s][2] for s in scene_ids]
            init = {k: np.concatenate([c[k] for c in ctls]) for k in ctls[0]} if ctls[0] else None
            if N > 1:      # a seed per future; the futures of a scene travel through the gather as one [N * T] sequence
                seeds = np.array([[(int(sd) + 0x9E3779B97F4A7C15 * k) % 2 ** 64 for k in range(N)] for sd in seeds], dtype=np.uint64)
            out = eng.rollout(toks, nf, cond_frames=T_hist, input_cond_frames=icf, init_tokens=init,
                              control_test=control and init is not None and "bbox3d" in init, seeds=seeds, **plan_kwargs(args, cfg, len(scene_ids), nf))
            return {m: out[m].reshape(out[m].shape[0], -1, out[m].shape[-1]) for m in MOD_ORDER} if N > 1 else out
        out = sharded_rollout(rollout_fn, [scenes[s][1] for s in sids], base_seed=args.seed, batch=args.batch,
                              device="cuda" if world > 1 else "cpu", scene_ids=sids, pass_ids=True)
        for pos in scene_partition(len(sids), world, rank):                   # every rank writes the scenes it rolled out
            name = scenes[sids[pos]][0]
            for k in range(N):
                T = out["pose"].shape[1] // N
                one = {m: out[m][pos:pos + 1, k * T:(k + 1) * T] for m in MOD_ORDER}
                print("saved", save_tokens(one, args.output_path, name if N == 1 else f"{name}_s{k}"))
    eng.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
