"""What the ten generation entry points refuse (umgen_rollout .. umgen_rollout_planned, umgen_frame .. umgen_frame_biased), through raw ctypes calls on
the tiny fp32 engine with max_batch 4, two scenes and two new frames: the return code, the whole umgen_last_error text and that nothing was written to
the caller's arrays.  The codes, texts and order are the contract of include/umgen.h ("refused before anything reaches the device, the message
naming ..."); tests/host/gen_call_test.cpp holds the same checks (csrc/gen_call.h) to every refusal without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_rollout_bias import NEG, random_tables, scenes_of
from tests.test_gpu_rollout_logp import close_engines, engine, sampled  # noqa: F401
from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER
from umgen_amd.engine import Engine

pytestmark = pytest.mark.gpu
INVALID, STATE, UNSUPPORTED = -1, -2, -5
B, N, T_IN, NF, COND = 2, 2, 2, 2, 4
TOK_FILL, F_FILL = -7, np.float32(7.5)
ROLLOUTS = ("umgen_rollout", "umgen_rollout_logp", "umgen_rollout_fan", "umgen_rollout_detail", "umgen_rollout_biased", "umgen_rollout_planned")
FRAMES = ("umgen_frame", "umgen_frame_logp", "umgen_frame_detail", "umgen_frame_biased")
NOT_FINALIZED = "umgen_finalize_weights has not been called"
NAN_TABLE = "logit bias: class bbox3d row 4 index 9 is NaN (entries are finite or -inf)"
DETAIL_KEYS = ("rank", "mass_above", "entropy", "topk_tok", "topk_logp")


def p64(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def side_structs(lead, topk):
    """logp, logz and diagnostics buffers of a call with their fill values, and the three structs that point at them"""
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == np.float32 else C.c_int32))      # noqa: E731
    bufs = {}
    for key in ("logp", "logz") + DETAIL_KEYS:
        dt = np.int32 if key in ("rank", "topk_tok") else np.float32
        for m in MOD_ORDER:
            shape = tuple(lead) + (CONTENT_LEN[m],) + ((max(topk, 1),) if key.startswith("topk_") else ())
            bufs[f"{key}_{m}"] = np.full(shape, TOK_FILL if dt is np.int32 else F_FILL, dt)
    pick = lambda keys: {k: fp(a) for k, a in bufs.items() if k.rsplit("_", 1)[0] in keys}      # noqa: E731
    return bufs, _lib.LogpOut(**pick(("logp",))), _lib.LogzOut(**pick(("logz",))), _lib.GenDetailOut(**pick(DETAIL_KEYS))


def bias_struct(tabs, hold):
    arrs = {m: np.ascontiguousarray(t, np.float32) for m, t in tabs.items()}
    hold.append(arrs)
    return _lib.LogitBias(**{m: a.ctypes.data_as(C.POINTER(C.c_float)) for m, a in arrs.items()})


def refused(e, name, rc_want, msg_want, **over):
    """One raw call through entry point `name` with the valid arguments of its form and `over` on top; asserts the refusal and that every output array keeps
    its fill value.  over: any of a's keys below; tokens = {mod: array} replaces input arrays; null = names of token buffers passed as NULL; smp = fields
    of the umgen_sampling (or None for a NULL pointer); given = {"map" / "bbox3d": array} (a frame call takes them through its trace)"""
    hold = []
    frame = name in FRAMES
    fan = name in ROLLOUTS[2:]
    sc = scenes_of(B)
    a = dict(B=B, N=N, T_in=T_IN, new_frames=NF, cond_frames=COND, T_ctl=0, ctrl_pose=None, ctrl_bbox3d=None, control_test=0, topk=0, bias=None, plan=None)
    unknown = set(over) - set(a) - {"tokens", "null", "smp", "given"}
    assert not unknown, unknown
    a.update({k: v for k, v in over.items() if k in a})
    ins = {m: np.ascontiguousarray(sc[m][0] if frame else sc[m], dtype=np.int64) for m in MOD_ORDER}
    ins.update({m: np.ascontiguousarray(t, dtype=np.int64) for m, t in over.get("tokens", {}).items()})
    lead = () if frame else (B * max(a["N"], 1),) if fan else (max(a["B"], 1),)
    outs = {m: np.full(lead + (() if frame else (T_IN + NF,)) + (CONTENT_LEN[m],), TOK_FILL, np.int64) for m in MOD_ORDER}
    null = over.get("null", ())
    in_p = [None if m in null else p64(ins[m]) for m in MOD_ORDER]
    out_p = [None if f"out_{m}" in null else p64(outs[m]) for m in MOD_ORDER]
    smp = None
    if over.get("smp", {}) is not None:
        smp, keep = e._sampling(sampled(e.cfg), list(range(1, 1 + B * N)))
        hold.append(keep)
        for k, v in over.get("smp", {}).items():
            setattr(smp, k, v)
    smp_p = C.byref(smp) if smp is not None else None
    given = {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in over.get("given", {}).items()}
    side, lp, lz, det = side_structs(lead + (() if frame else (NF,)), a["topk"])
    cp, cb = (None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.int64) for k in ("ctrl_pose", "ctrl_bbox3d"))
    shared = C.c_int32(-1)
    bias = None if a["bias"] is None else C.byref(bias_struct(a["bias"], hold))
    if frame:
        tr = None
        if given:
            tr = _lib.Trace()
            tr.given_map, tr.given_bbox3d = p64(given.get("map")), p64(given.get("bbox3d"))
        args = [e._h, a["T_in"], *in_p, p64(cp), p64(cb), a["control_test"], smp_p, 0, C.byref(tr) if tr is not None else None, *out_p]
        tail = {"umgen_frame": [], "umgen_frame_logp": [C.byref(lp)], "umgen_frame_detail": [C.byref(lp), a["topk"], C.byref(det)],
                "umgen_frame_biased": [C.byref(lp), a["topk"], C.byref(det), bias, C.byref(lz)]}[name]
    else:
        args = [e._h, a["B"]] + ([a["N"]] if fan else []) + [a["T_in"], a["new_frames"], a["cond_frames"], *in_p, a["T_ctl"], p64(cp), p64(cb), a["control_test"],
                                                             p64(given.get("map")), p64(given.get("bbox3d")), smp_p, *out_p]
        last = bias if name == "umgen_rollout_biased" else None if a["plan"] is None else C.byref(a["plan"])
        tail = {"umgen_rollout": [], "umgen_rollout_logp": [C.byref(lp)], "umgen_rollout_fan": [C.byref(lp), C.byref(shared)],
                "umgen_rollout_detail": [C.byref(lp), C.byref(shared), a["topk"], C.byref(det)]}.get(name, [C.byref(lp), C.byref(shared), a["topk"], C.byref(det), last, C.byref(lz)])
    rc = getattr(e.lib, name)(*args, *tail)
    msg = e.lib.umgen_last_error(e._h).decode()
    assert (rc, msg) == (rc_want, msg_want), (name, rc, msg)
    assert all((o == TOK_FILL).all() for o in outs.values()), f"{name}: a refused call wrote tokens"
    assert all((b == (TOK_FILL if b.dtype == np.int32 else F_FILL)).all() for b in side.values()), f"{name}: a refused call wrote side outputs"
    if fan:
        assert shared.value == 0, "shared_slots of a refused fan-out call"
    del hold


def fp32_engine():
    return engine("tiny", "fp32", max_batch=4)


def test_engine_state():
    e = Engine(fp32_engine().cfg, precision="fp32", max_batch=4, max_cond_frames=4)      # weights never finalized
    try:
        for name in ROLLOUTS + FRAMES:
            refused(e, name, STATE, NOT_FINALIZED)
        refused(e, "umgen_rollout_fan", STATE, NOT_FINALIZED, B=0)      # (the engine's state comes before the counts)
        refused(e, "umgen_frame", STATE, NOT_FINALIZED, T_in=9)
    finally:
        e.close()


def test_counts():
    e = fp32_engine()
    refused(e, "umgen_rollout", INVALID, "B=5 out of range [1,4]", B=5)
    refused(e, "umgen_rollout_logp", INVALID, "B=0 out of range [1,4]", B=0)
    refused(e, "umgen_rollout_fan", INVALID, "B=0: at least one scene", B=0, N=0)
    refused(e, "umgen_rollout_detail", INVALID, "N=0: at least one sample per scene", N=0)
    refused(e, "umgen_rollout_biased", INVALID, "B*N=6 (B=2, N=3) exceeds max_batch=4", N=3)
    refused(e, "umgen_rollout_planned", INVALID, "T_in=2 new_frames=2 cond_frames=5 (max 4)", cond_frames=5)
    refused(e, "umgen_rollout", INVALID, "T_in=0 new_frames=-1 cond_frames=4 (max 4)", T_in=0, new_frames=-1)
    for name in FRAMES:
        refused(e, name, INVALID, "T=5 out of range [1,4]", T_in=5)
    refused(e, "umgen_frame", INVALID, "T=0 out of range [1,4]", T_in=0, smp=None)      # (the count comes before the sampling)


def test_sampling():
    e = fp32_engine()
    refused(e, "umgen_rollout", INVALID, "sampling is null", smp=None)
    refused(e, "umgen_frame_biased", INVALID, "sampling is null", smp=None)
    refused(e, "umgen_rollout_fan", INVALID, "sample method 2", smp=dict(method=2))
    refused(e, "umgen_frame_logp", INVALID, "top-k values must be in [1, 16] (reference: 5 / 5 / 16)", smp=dict(top_k=17))
    refused(e, "umgen_rollout_planned", INVALID, "top-p mass must be > 0", smp=dict(method=1, p_map=0.0))
    refused(e, "umgen_rollout_logp", INVALID, "temperature must be > 0", smp=dict(temperature=0.0), null=("map",))      # (before the buffers)


def test_side_request():
    e = fp32_engine()
    refused(e, "umgen_rollout_detail", INVALID, "topk=17 out of range [0,16]", topk=17)
    refused(e, "umgen_frame_detail", INVALID, "topk=-1 out of range [0,16]", topk=-1)
    refused(e, "umgen_frame_detail", INVALID, "top-K outputs requested with topk = 0")
    refused(e, "umgen_rollout_biased", INVALID, "top-K outputs requested with topk = 0", null=("out_pose",))      # (before the buffers)
    refused(e, "umgen_rollout_planned", INVALID, "temperature must be > 0 and finite", topk=4, smp=dict(temperature=np.inf))
    refused(e, "umgen_frame_biased", INVALID, "temperature must be > 0 and finite", topk=4, smp=dict(temperature=np.inf))


def test_null_buffers():
    e = fp32_engine()
    refused(e, "umgen_rollout_logp", INVALID, "null token buffer", null=("map",))
    refused(e, "umgen_rollout_fan", INVALID, "null token buffer", null=("out_bbox3d",))
    refused(e, "umgen_frame", INVALID, "null token buffer", null=("out_image",))
    refused(e, "umgen_frame_logp", INVALID, "null token buffer", null=("pose",))


def test_history_tokens():
    e = fp32_engine()
    sc = scenes_of(B)
    bad_map = sc["map"].copy()
    bad_map[1, 1, 5] = 8192      # scene 1 of the caller's [B][T_in][1024]: N = 2 branches do not move the index
    refused(e, "umgen_rollout_fan", INVALID, "map token 8192 at flat index 3077 is outside [0, 8192)", tokens={"map": bad_map}, topk=4)
    refused(e, "umgen_rollout", INVALID, "map token 8192 at flat index 3077 is outside [0, 8192)", tokens={"map": bad_map})
    bad_pose, bad_img = sc["pose"][0].copy(), sc["image"][0].copy()
    bad_pose[0, 0], bad_img[1, 511] = -1, 1 << 40
    refused(e, "umgen_frame", INVALID, "pose token -1 at flat index 0 is outside [0, 1024)", tokens={"pose": bad_pose, "image": bad_img})
    refused(e, "umgen_frame_detail", INVALID, f"image token {1 << 40} at flat index 1023 is outside [0, 8192)", tokens={"image": bad_img}, topk=4)


def test_control_tokens():
    e = fp32_engine()
    free = np.full((B, 1, CONTENT_LEN["bbox3d"]), -1, np.int64)
    bad = free.copy()
    bad[1, 0, 7] = 1028
    refused(e, "umgen_rollout_biased", INVALID, "control bbox3d token 1028 at flat index 667 is outside [0, 1028) (and is not -1 = free)",
            T_ctl=1, ctrl_bbox3d=bad, control_test=1, topk=4)
    refused(e, "umgen_rollout_detail", INVALID, "control tokens given with T_ctl=0", ctrl_bbox3d=free, control_test=1, topk=4)
    pose = np.zeros((B, 1, 3), np.int64)
    pose[1, 0, 2] = 1024
    refused(e, "umgen_rollout_logp", INVALID, "control pose token 1024 at flat index 5 is outside [0, 1024)", T_ctl=1, ctrl_pose=pose, ctrl_bbox3d=bad)
    refused(e, "umgen_frame_logp", INVALID, "control pose token 1024 at flat index 2 is outside [0, 1024)", ctrl_pose=pose[1, 0], ctrl_bbox3d=bad[1, 0])
    refused(e, "umgen_frame_biased", INVALID, "control bbox3d token 1028 at flat index 7 is outside [0, 1028) (and is not -1 = free)", ctrl_bbox3d=bad[1, 0], topk=4)
    refused(e, "umgen_frame_biased", UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path", ctrl_bbox3d=free[0, 0], topk=4)


def test_given_tokens():
    e = fp32_engine()
    sc = scenes_of(B)
    gm, gb = sc["map"][:, -1:].copy(), sc["bbox3d"][:, -1:].copy()
    bad = gm.copy()
    bad[1, 0, 3] = -1
    refused(e, "umgen_rollout_detail", INVALID, "given map token -1 at flat index 1027 is outside [0, 8192)", T_ctl=1, given={"map": bad}, topk=4)
    refused(e, "umgen_frame", INVALID, "given map token -1 at flat index 3 is outside [0, 8192)", given={"map": bad[1, 0]})
    refused(e, "umgen_rollout_planned", INVALID, "given tokens with T_ctl=0", given={"map": gm}, topk=4)
    refused(e, "umgen_rollout", UNSUPPORTED, "init_tokens['bbox3d'] without init_tokens['map'] (and without control_test): the reference concatenates the given "
            "modalities back to back behind the pose, so the boxes would sit on the map's positions -- not a meaningful path", T_ctl=1, given={"bbox3d": gb})
    refused(e, "umgen_frame_detail", UNSUPPORTED, "given bbox3d tokens without a given map: the reference would put them on the map's positions (UMGen.py:1190-1201)",
            given={"bbox3d": gb[0, 0]}, topk=4)
    refused(e, "umgen_rollout_fan", INVALID, "given bbox3d tokens and bbox3d control exclude each other", T_ctl=1, given={"map": gm, "bbox3d": gb}, control_test=1)
    refused(e, "umgen_frame_logp", UNSUPPORTED, "given tokens and control_test exclude each other", given={"map": gm[0, 0]}, control_test=1)
    gb[0, 0, 659] = 1028
    refused(e, "umgen_rollout_biased", INVALID, "given bbox3d token 1028 at flat index 659 is outside [0, 1028)", T_ctl=1, given={"map": gm, "bbox3d": gb}, topk=4)
    refused(e, "umgen_frame_biased", INVALID, "given bbox3d token 1028 at flat index 659 is outside [0, 1028)", given={"map": gm[0, 0], "bbox3d": gb[0, 0]}, topk=4)


def test_bias_tables():
    e = fp32_engine()
    good = random_tables(e.cfg, 3)
    bad = {m: t.copy() for m, t in good.items()}
    bad["bbox3d"][4, 9] = np.nan
    # one set without a name: the frame call and the rollout call word it alike, without a "bias set" prefix
    refused(e, "umgen_frame_biased", INVALID, NAN_TABLE, bias=bad, topk=4)
    refused(e, "umgen_rollout_biased", INVALID, NAN_TABLE, bias=bad, topk=4)
    last = {"bbox3d": np.full((11, e.cfg.bbox3d_vocab_size), NEG, np.float32)}
    last["bbox3d"][:, -1] = 0.0
    ctl = np.full((B, 1, CONTENT_LEN["bbox3d"]), -1, np.int64)
    only_last = "logit bias: class bbox3d row 0 allows only index 1027, which the control resample of a controlled slot masks"
    refused(e, "umgen_frame_biased", INVALID, only_last, bias=last, ctrl_bbox3d=ctl[0, 0], control_test=1, topk=4)
    refused(e, "umgen_rollout_biased", INVALID, only_last, bias=last, T_ctl=1, ctrl_bbox3d=ctl, control_test=1, topk=4)
    hold = []
    banned = {m: t.copy() for m, t in good.items()}
    banned["map"][:] = NEG
    sets = (_lib.LogitBias * 2)(bias_struct(good, hold), bias_struct(banned, hold))
    plan = _lib.SamplePlan(None, 2, C.cast(sets, C.POINTER(_lib.LogitBias)), None)
    refused(e, "umgen_rollout_planned", INVALID, "sample plan: bias set 1: logit bias: class map row 0 bans every token (index 0 .. 8191 are all -inf)", plan=plan, topk=4)
    plan.n_bias_sets = 17
    refused(e, "umgen_rollout_planned", INVALID, "sample plan: n_bias_sets=17 out of range [0,16]", plan=plan, topk=4)
