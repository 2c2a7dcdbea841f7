"""The Python side of sampling plans without a GPU: constraints.schedule's broadcasting rule and refusals, constraints.per_frame's identity
deduplication and the 16-set limit, log_importance_weight under a Schedule against a numpy restatement, the new flags of umgen_amd.evaluate and its main loop with
--num_samples (a recording engine in the device engine's place), and what Engine.rollout / UMGen.inference hand to umgen_rollout_planned."""
import numpy as np
import pytest

from umgen_amd import constraints, evaluate
from umgen_amd.config import CONTENT_LEN, tiny_config
from umgen_amd.constraints import CLASSES, ROWS

VOCAB = {"pose": 12, "map": 9, "bbox3d": 1028, "image": 7}


def tables(seed, classes=CLASSES):
    rng = np.random.default_rng(seed)
    out = {}
    for m in classes:
        t = rng.uniform(-3, 3, (ROWS[m], VOCAB[m])).astype(np.float32)
        t[rng.random(t.shape) < 0.3] = -np.inf
        t[:, 0] = 0.0
        out[m] = t.reshape(constraints.table_shape(m, VOCAB[m]))
    return out


# ---- constraints.schedule ---------------------------------------------------------------------------------------------------------------------
def test_schedule_broadcasts_by_shape():
    A, Bt = tables(1), tables(2)
    B, N, F = 3, 2, 4
    want = np.empty((B, N, F), np.int32)
    s = constraints.schedule([A, Bt], 1)                                            # a scalar
    want[:] = 1
    np.testing.assert_array_equal(s.resolve(B, N, F), want.reshape(B * N, F))
    s = constraints.schedule([A, Bt], [0, -1, 1])                                   # [B]
    want[:] = np.array([0, -1, 1])[:, None, None]
    np.testing.assert_array_equal(s.resolve(B, N, F), want.reshape(B * N, F))
    s = constraints.schedule([A, Bt], [0, 0, 1, -1], axis="frame")                  # [new_frames]
    want[:] = np.array([0, 0, 1, -1])[None, None, :]
    np.testing.assert_array_equal(s.resolve(B, N, F), want.reshape(B * N, F))
    bn = np.array([[0, 1], [1, -1], [-1, 0]])                                       # [B, N]
    s = constraints.schedule([A, Bt], bn)
    want[:] = bn[:, :, None]
    np.testing.assert_array_equal(s.resolve(B, N, F), want.reshape(B * N, F))
    full = np.random.default_rng(0).integers(-1, 2, (B, N, F))                      # [B, N, new_frames]
    s = constraints.schedule([A, Bt], full)
    got = s.resolve(B, N, F)
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"]
    for b in range(B):
        for n in range(N):
            for f in range(F):
                assert got[b * N + n, f] == full[b, n, f]
    s = constraints.schedule([A, None], [0, 1, 1])                                  # None: an empty set
    assert s.sets[1] == {} and s.resolve(3, 1, 2).shape == (3, 2)


def test_schedule_refusals():
    A = tables(1)
    with pytest.raises(ValueError, match="axis"):
        constraints.schedule([A], np.zeros((3, 4), np.int64), axis="frame")         # [B, new_frames] would be indistinguishable from [B, N]
    with pytest.raises(ValueError, match="axis"):
        constraints.schedule([A], [0, 0], axis="branch")
    with pytest.raises(ValueError, match="shape"):
        constraints.schedule([A], np.zeros((2, 2, 2, 2), np.int64))
    with pytest.raises(ValueError, match="integers"):
        constraints.schedule([A], [0.0, 1.0])
    with pytest.raises(ValueError, match=r"\[-1, 1\)"):
        constraints.schedule([A], [0, 1])
    with pytest.raises(ValueError, match=r"\[-1, 1\)"):
        constraints.schedule([A], [0, -2])
    with pytest.raises(ValueError, match="at most 16"):
        constraints.schedule([A] * 17, 0)
    assert len(constraints.schedule([A] * 16, 15).sets) == 16
    # a shape that does not fit the call: refused when the call's sizes are known
    with pytest.raises(ValueError, match="scene axis"):
        constraints.schedule([A], [0, 0, 0]).resolve(2, 1, 3)                       # (3 entries are NOT taken for the 3 frames)
    with pytest.raises(ValueError, match="frame axis"):
        constraints.schedule([A], [0, 0], axis="frame").resolve(2, 1, 3)
    with pytest.raises(ValueError, match="branch axis"):
        constraints.schedule([A], np.zeros((2, 3), np.int64)).resolve(2, 1, 3)
    with pytest.raises(ValueError):
        constraints.schedule([{"map": np.full(9, -np.inf, np.float32)}], 0)         # a set is checked like merge checks it


def test_per_frame_deduplicates_by_identity():
    A, Bt = tables(1), tables(2)
    s = constraints.per_frame([A, A, None, Bt, A, Bt])
    assert len(s.sets) == 2 and s.axes == ("frame",)
    np.testing.assert_array_equal(s.index, [0, 0, -1, 1, 0, 1])
    np.testing.assert_array_equal(s.resolve(2, 3, 6), np.tile([0, 0, -1, 1, 0, 1], (6, 1)))
    same_values = [tables(1) for _ in range(3)]                                      # equal values, distinct objects: three sets
    assert len(constraints.per_frame(same_values).sets) == 3
    many = [tables(i) for i in range(17)]
    assert len(constraints.per_frame(many[:16] * 2).sets) == 16
    with pytest.raises(ValueError, match="17 distinct table sets"):
        constraints.per_frame(many)
    assert constraints.per_frame([None, None]).sets == [] and constraints.per_frame([None, None]).resolve(1, 1, 2).tolist() == [[-1, -1]]


# ---- log_importance_weight under a schedule ------------------------------------------------------------------------------------------------
def test_log_importance_weight_reads_each_positions_own_set():
    rng = np.random.default_rng(3)
    B, N, T, F = 2, 3, 5, 3
    sets = [tables(1), tables(2, ("bbox3d", "pose")), None]
    of = rng.integers(-1, 3, (B, N, F))
    sch = constraints.schedule(sets, of)
    tokens, logz = {}, {}
    for m in CLASSES:
        S = CONTENT_LEN[m]
        tokens[m] = np.zeros((B, N, T, S), np.int64)
        logz[m] = rng.standard_normal((B, N, F, S)).astype(np.float32)
        logz[m][rng.random(logz[m].shape) < 0.05] = np.nan
        for b in range(B):
            for n in range(N):
                for f in range(F):
                    tabs = {} if of[b, n, f] < 0 else (sets[of[b, n, f]] or {})
                    for k in range(S):                                              # an allowed token of the position's own row
                        row = tabs[m].reshape(ROWS[m], -1)[k % ROWS[m]] if m in tabs else np.zeros(VOCAB[m])
                        tokens[m][b, n, T - F + f, k] = rng.choice(np.flatnonzero(~np.isneginf(row)))
    got = constraints.log_importance_weight(tokens, logz, sch)
    want = np.zeros((B, N, F))
    for b in range(B):
        for n in range(N):
            for f in range(F):
                tabs = {} if of[b, n, f] < 0 else (sets[of[b, n, f]] or {})
                for m in CLASSES:
                    for k in range(CONTENT_LEN[m]):
                        z = float(logz[m][b, n, f, k])
                        if np.isnan(z):
                            continue
                        r = float(tabs[m].reshape(ROWS[m], -1)[k % ROWS[m], tokens[m][b, n, T - F + f, k]]) if m in tabs else 0.0
                        want[b, n, f] += z - r
    assert got.shape == (B, N, F) and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max() + 1e-9)
    # one set everywhere is the unscheduled value; leading axes [B] work too
    flat_t = {m: tokens[m][:, 0] for m in CLASSES}
    flat_z = {m: logz[m][:, 0] for m in CLASSES}
    one = constraints.schedule([sets[0]], 0)
    np.testing.assert_array_equal(constraints.log_importance_weight(flat_t, flat_z, one), constraints.log_importance_weight(flat_t, flat_z, sets[0]))


# ---- umgen_amd.evaluate ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_flags():
    p = evaluate.build_parser()
    d = p.parse_args([])
    assert d.temperatures is None and d.ban_from_frame == 0 and d.num_samples == 1
    cfg = tiny_config()
    assert evaluate.plan_kwargs(d, cfg, 2, 5) == {}                                  # the defaults add nothing to the call
    a = p.parse_args(["--num_samples", "4", "--temperatures", "0.7,1.0,1.3", "--ban_category", "pedestrian", "--ban_from_frame", "2"])
    assert a.temperatures == [0.7, 1.0, 1.3] and a.ban_from_frame == 2 and a.num_samples == 4
    kw = evaluate.plan_kwargs(a, cfg, 2, 5)
    assert kw["samples"] == 4 and len(kw["sampling"]) == 2 and [c.sfmx_temp for c in kw["sampling"][1]] == [0.7, 1.0, 1.3, 0.7]      # branch s: temperatures[s % len]
    assert all(c.top_k == cfg.top_k and c.rule_constrain == cfg.rule_constrain for c in kw["sampling"][0])
    sch = kw["logit_bias"]
    assert isinstance(sch, constraints.Schedule) and len(sch.sets) == 1 and sch.index.tolist() == [-1, -1, 0, 0, 0]
    ped = constraints.CATEGORY_TOKEN0 + constraints.scene_io.CATEGORIES.index("pedestrian")
    assert np.isneginf(sch.sets[0]["bbox3d"][constraints.CATEGORY_ATTR, ped])
    # frame 0: today's one-set call; a start behind the last frame: no frame is constrained
    kw0 = evaluate.plan_kwargs(p.parse_args(["--ban_category", "pedestrian"]), cfg, 1, 5)
    assert set(kw0) == {"logit_bias"} and isinstance(kw0["logit_bias"], dict)
    late = evaluate.plan_kwargs(p.parse_args(["--ban_category", "pedestrian", "--ban_from_frame", "9"]), cfg, 1, 5)["logit_bias"]
    assert late.sets == [] and late.index.tolist() == [-1] * 5
    # one temperature for every sample: a plain RolloutConfig, no plan
    one = evaluate.plan_kwargs(p.parse_args(["--num_samples", "2", "--temperatures", "0.5"]), cfg, 3, 5)
    assert one["samples"] == 2 and one["sampling"].sfmx_temp == 0.5
    for bad in ("0.5,,x", "0", "-1,2", "inf", ""):
        with pytest.raises(SystemExit):
            p.parse_args(["--temperatures", bad])
    with pytest.raises(SystemExit):
        p.parse_args(["--num_samples", "0"])
    with pytest.raises(ValueError):
        evaluate.plan_kwargs(p.parse_args(["--ban_from_frame", "-1"]), cfg, 1, 5)


# ---- Engine.rollout / UMGen.inference: what reaches umgen_rollout_planned (no engine exists here; any other device call is an assertion failure) ----
class PlannedRecorder:
    """stands where the C library stands: reads the plan of a umgen_rollout_planned call while the call's arrays are alive"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name != "umgen_rollout_planned":
            raise AssertionError(f"device call {name} reached")

        def call(*args):
            B, N, nf, smp, plan = args[1], args[2], args[4], args[16]._obj, args[25]._obj
            items = B * N
            rec = {"B": B, "N": N, "temperature": smp.temperature, "seeds": [smp.seeds[i] for i in range(items)], "n_sets": plan.n_bias_sets,
                   "per_scene": [(plan.per_scene[i].method, plan.per_scene[i].top_k, round(plan.per_scene[i].temperature, 6)) for i in range(items)] if plan.per_scene else None,
                   "bias_of": np.ctypeslib.as_array(plan.bias_of, shape=(items, nf)).copy() if plan.bias_of else None,
                   "classes": [[bool(getattr(plan.bias_sets[q], m)) for m in CLASSES] for q in range(plan.n_bias_sets)]}
            if plan.n_bias_sets:
                rec["map0"] = np.ctypeslib.as_array(plan.bias_sets[0].map, shape=(tiny_config().map_vocab_size,)).copy() if plan.bias_sets[0].map else None
            self.calls.append(rec)
            return 0
        return call


def full_tables(seed):
    rng = np.random.default_rng(seed)
    cfg = tiny_config()
    return {"map": rng.uniform(-1, 1, cfg.map_vocab_size).astype(np.float32), "bbox3d": rng.uniform(-1, 1, (11, cfg.bbox3d_vocab_size)).astype(np.float32)}


def test_rollout_and_inference_hand_the_plan_to_the_planned_entry_point():
    import dataclasses

    import torch

    from tests.test_rollout_fan_host import _engine_without_device, _scene
    from umgen_amd.engine import UMGenError
    from umgen_amd.model import UMGen
    rec = PlannedRecorder()
    e = _engine_without_device(rec)
    cfg = e.cfg
    sc = _scene(B=2)
    A, Bt = full_tables(1), {"bbox3d": full_tables(2)["bbox3d"]}
    cfgs = [dataclasses.replace(cfg, sfmx_temp=0.5), dataclasses.replace(cfg, sample_method="top_p", top_k=3, sfmx_temp=1.5)]
    sch = constraints.schedule([A, Bt], [[0, 1, -1], [1, 1, 0]])                      # [B, N]
    e.rollout(sc, 2, cond_frames=2, sampling=cfgs, samples=3, seeds=np.arange(6).reshape(2, 3), logit_bias=sch, return_logz=True)
    c = rec.calls[-1]
    assert (c["B"], c["N"], c["n_sets"], c["seeds"]) == (2, 3, 2, [0, 1, 2, 3, 4, 5])
    assert c["per_scene"] == [(0, cfg.top_k, 0.5)] * 3 + [(1, 3, 1.5)] * 3           # B entries: a scene's branches share theirs
    np.testing.assert_array_equal(c["bias_of"], np.repeat(np.array([0, 1, -1, 1, 1, 0])[:, None], 2, axis=1))
    assert c["classes"] == [[False, True, True, False], [False, False, True, False]]
    np.testing.assert_array_equal(c["map0"], A["map"])
    # per-branch settings flat and nested; one set of tables beside them: no index array
    six = [dataclasses.replace(cfg, sfmx_temp=0.5 + 0.1 * i) for i in range(6)]
    for form in (six, [six[:3], six[3:]]):
        e.rollout(sc, 1, cond_frames=2, sampling=form, samples=3, logit_bias=A)
        c = rec.calls[-1]
        assert [t for _, _, t in c["per_scene"]] == [round(0.5 + 0.1 * i, 6) for i in range(6)] and c["n_sets"] == 1 and c["bias_of"] is None
    # a schedule alone: the call's sampling, no per-scene entries
    e.rollout(sc, 3, cond_frames=2, logit_bias=constraints.per_frame([A, None, A]))
    c = rec.calls[-1]
    assert c["per_scene"] is None and c["n_sets"] == 1 and c["bias_of"].tolist() == [[0, -1, 0]] * 2
    e.rollout(sc, 2, cond_frames=2, logit_bias=constraints.per_frame([None, None]))      # nothing constrained: no sets, no index
    assert rec.calls[-1]["n_sets"] == 0 and rec.calls[-1]["bias_of"] is None
    with pytest.raises(UMGenError, match="sampling has 5 entries"):
        e.rollout(sc, 1, cond_frames=2, sampling=six[:5], samples=3)
    with pytest.raises(UMGenError, match="per call"):
        e.rollout(sc, 1, cond_frames=2, sampling=[cfg, dataclasses.replace(cfg, only_ar=not cfg.only_ar)])
    with pytest.raises(UMGenError, match="bias set 1"):
        e.rollout(sc, 1, cond_frames=2, logit_bias=constraints.Schedule([A, {"map": np.full(cfg.map_vocab_size, np.nan, np.float32)}], np.zeros(2, np.int32), ("scene",)))
    # UMGen.inference forwards both, as Engine.rollout takes them
    m = UMGen(tiny_config())
    m._engine, m._loaded = _engine_without_device(rec), True
    m._engine_args = dict(getattr(m, "_engine_args", {}) or {}, max_batch=8)
    tsc = {k: torch.from_numpy(v) for k, v in sc.items()}
    n = len(rec.calls)
    m.inference(2, cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=tsc, num_samples=3, sampling=cfgs, logit_bias=sch, return_logz=True,
                seeds=list(range(6)))
    assert len(rec.calls) == n + 1
    a, b = rec.calls[0], rec.calls[-1]
    assert a["per_scene"] == b["per_scene"] and a["seeds"] == b["seeds"] and a["classes"] == b["classes"] and (a["bias_of"] == b["bias_of"]).all()
    m.inference(2, cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=tsc, sampling=cfgs)      # without num_samples: B entries, N = 1
    assert rec.calls[-1]["per_scene"] == [(0, cfg.top_k, 0.5), (1, 3, 1.5)] and rec.calls[-1]["N"] == 1


# ---- umgen_amd.evaluate's main loop with --num_samples, an engine of recorded calls in the device engine's place ------------------------------------
def test_evaluate_main_loop_with_samples(tmp_path, monkeypatch):
    import pickle

    import umgen_amd.engine as engine_mod
    from umgen_amd.config import MOD_ORDER
    from umgen_amd.shard import scene_seed
    made, calls = [], []

    class FakeEngine:
        def __init__(self, cfg, precision="bf16", max_batch=1, max_cond_frames=20, device=0):
            made.append(dict(max_batch=max_batch))

        def load_tensor(self, key, arr):
            return True

        def finalize(self):
            pass

        def close(self):
            pass

        def rollout(self, toks, nf, seeds=None, samples=None, **kw):
            calls.append(dict(kw, nf=nf, seeds=np.asarray(seeds), samples=samples, B=toks["pose"].shape[0]))
            B, T = toks["pose"].shape[:2]
            sd = np.asarray(seeds).reshape(B, samples or 1)
            out = {}
            for m in MOD_ORDER:      # history, then new frames that carry the branch's seed (mod 1000) so that a future can be told from its siblings
                a = np.zeros((B, samples or 1, T + nf, CONTENT_LEN[m]), np.int64)
                a[:, :, :T] = toks[m][:, None]
                a[:, :, T:] = (sd % 1000).astype(np.int64)[:, :, None, None]
                out[m] = a if samples else a[:, 0]
            return out
    monkeypatch.setattr(engine_mod, "Engine", FakeEngine)
    argv = ["--model_scale", "debug", "--debug", "1", "--synthetic", "3", "--infer_task", "video", "--set_num_new_frames", "2", "--batch", "2", "--seed", "5",
            "--num_samples", "3", "--temperatures", "0.7,1.2", "--ban_category", "pedestrian", "--ban_from_frame", "1", "--output_path", str(tmp_path)]
    evaluate.main(argv)
    assert made == [dict(max_batch=6)]                                               # batch x samples branches per call
    assert [c["B"] for c in calls] == [2, 1] and all(c["samples"] == 3 and c["nf"] == 2 for c in calls)
    seeds = np.concatenate([c["seeds"] for c in calls])
    assert seeds.dtype == np.uint64 and seeds.shape == (3, 3) and len(set(seeds.reshape(-1).tolist())) == 9
    assert seeds[:, 0].tolist() == [scene_seed(5, i) for i in range(3)]              # future 0 keeps the scene's seed
    c = calls[0]
    assert [[s.sfmx_temp for s in row] for row in c["sampling"]] == [[0.7, 1.2, 0.7]] * 2
    assert isinstance(c["logit_bias"], constraints.Schedule) and c["logit_bias"].index.tolist() == [-1, 0]
    for i in range(3):
        for k in range(3):
            d = pickle.load(open(tmp_path / "saved_token" / f"synthetic_{i:04d}_s{k}_tokens.pkl", "rb"))
            T = d["pose"].shape[1]
            assert d["map"].shape == (1, T, CONTENT_LEN["map"]) and T == c["input_cond_frames"] + 2
            assert (d["image"][0, -2:] == int(seeds[i, k] % 1000)).all(), "future k of scene i is not the one saved under _s<k>"
    n = len(calls)
    evaluate.main(argv)                                                              # everything is there: nothing is rolled out again
    assert len(calls) == n
    (tmp_path / "saved_token" / "synthetic_0001_s2_tokens.pkl").unlink()             # the last future of a scene missing: that scene runs again
    evaluate.main(argv)
    assert len(calls) == n + 1 and calls[-1]["B"] == 1 and calls[-1]["seeds"][0, 0] == scene_seed(5, 1)
    # without --num_samples the loop is the old one: one file per scene, no samples keyword
    out1 = tmp_path / "single"
    evaluate.main(["--model_scale", "debug", "--debug", "1", "--synthetic", "1", "--infer_task", "video", "--set_num_new_frames", "2", "--output_path", str(out1)])
    assert calls[-1]["samples"] is None and "sampling" not in calls[-1] and (out1 / "saved_token" / "synthetic_0000_tokens.pkl").exists()
