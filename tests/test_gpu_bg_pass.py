"""The next frame's ego / TAR pass as the decode engine's background workers run it (umgen_amd/csrc/bg_worker.h: the engine workgroups of the four idle
XCDs execute an op list recorded from the stand-alone launchers, bg_queue.h, engine_stacks.hip launch_prefix) against the same pass as stand-alone
launches, BIT FOR BIT on every slot cache, under stop / resume schedules that the test forces.  Every test needs a GPU except the last.

What is held to what: the slot caches ([max_batch][max_cond_frames][S_stack][2E] per stack and block: the k | v rows of every temporal sub-block, all
that the pass leaves behind for the next frame) after the workers' pass must equal, byte for byte, the slot caches after the foreground pass --
umgen_dbg_bg_begin with foreground = 1 runs the very run_stack calls of launch_prefix as stand-alone kernels.  Equality and not a tolerance: the
stand-alone kernels have their own fp64 tests (test_gpu_kernels.py, test_gpu_stack_forms.py, test_gpu_attn_patterns.py, test_gpu_frame_kernels.py) and
the foreground path is tied to the oracle by test_gpu_parity.py; what is under test here is the design's claim that the workers produce the same bits
whatever the schedule is.  Every cache starts as POISON (0x7fa5: a NaN in bf16 and in fp16): the reference must leave slots >= P untouched and no
poison in slots < P, so a unit that a resume skipped shows as poison and a unit that ran twice on a residual shows as different bits.

Behind every schedule the queue is read back: ops_done == n_ops, every worker's op index == n_ops and arrive[k] == 128 for EVERY op -- a worker that
arrives twice after a deadline, or never, shows here even when the data happens to be right.  A schedule without a drain runs decode launches until
the workers' states say so too (the host's own criterion, check_frame_results): ops_done moves first -- a worker that arrived on the last op and met its
deadline before the last arrival keeps op index n_ops - 1 until its next launch, where it must move on WITHOUT arriving again.  Seen with the 40 us
margin: ops_done 99 of 99 behind 103 launches with workers 0 .. 7 still at op 98; the first version of this file stopped at ops_done and failed there.

Handle: the `one` handle of test_gpu_engine_step.py (E = 768, H = 16 -- the narrowest the 256-tile GEMM body takes --, one block per stack, 12 BlockOAR
layers, max_batch 1, max_cond_frames 4), bf16 and fp16.  Windows from synthetic_scene, the next pose tokens from the scene's next frame:
  P3     T = 3 growing to 4: the general case
  P1     T = 1 growing to 2: ops with fewer units than workers, empty GEMM tile lists; the foreground GEMMs fall under UMGEN_GEMM256_MIN_TILES, so this is
         the small-tile kernel against the 256-tile body, bit for bit
  slide  T = 4 under a cap of 4: the window slides (slots 1 .. 3 and the new frame), P = 3
Schedules (the workers are steered through host-written memory alone -- est[], chunk, margin_ticks; bg_worker.h and oar_engine.hip are as shipped):
  S-drain     one drain launch with the recorded chunks, then with every op's chunk = 1, 3, 5 (a drain batch is exactly min(mine - done, chunk) units: 5
              drives bg_ln through one four-unit group and a remainder from offsets 5, 10, ..; 3 gives GEMM ranges that start in the middle of a list);
              a second drain launch on the finished queue changes neither the state nor the caches
  S-one-unit  est[] = 0x40000000 before every decode launch: nothing fits, the progress rule runs exactly one unit per worker per launch; no drain.  The
              dealing of units is restated here from the op heads (mine_of), sum over the workers == n_units for every op; launches are capped at
              2 x (sum over the ops of the largest share + n_ops).  Read back behind every launch: for every op kind with a share >= 2 a worker is seen
              with 0 < done < mine, and a worker is seen arrived on an op that is not complete.  At P = 3 all six kinds have a share >= 2 (asserted from the
              op heads), so none of these checks moved to another window; at P = 1 the kinds that have one are checked.
  S-natural   the host's estimates and the default margin: decode launches until the pass completes (n_full, capped at NATURAL_CAP), then again
              n_full // 3 launches -- the premise 0 < ops_done < n_ops is asserted and printed -- and a drain
  margin      S-natural at P3 (bf16) with margin_ticks 4000 instead of 1000: the same pass cut at other units
  long        one bf16 handle with max_cond_frames 22, max_frame_len 32 at P = 21: the 32-slot temporal body, S-natural only
Clean exit: a pass abandoned in the middle by umgen_dbg_bg_end, then a two-frame greedy rollout on that handle == the rollout on a fresh handle, one
overlapped frame.  Refusals: no workers (UMGEN_BG_ENGINE=0), max_batch 2, a window whose pass would not fit; the reason through umgen_last_error.

Measured on an MI355X (bf16 | fp16) -- op count; S-one-unit launches / cap; n_full and ops_done of n_ops behind n_full // 3 launches:
(n_full is a measured quantity: the range over four runs is given where they differed)
  P3     99 ops | 99;  532 launches of at most 1260 | 532 of 1260;  n_full 87 .. 88 | 90 .. 93;  behind n_full // 3 = 29 | 30 .. 31 launches ops_done 27 | 27 .. 29
  P1     99 ops | 99;  376 launches of at most 948 | 376 of 948;    n_full 53 .. 54 | 55 .. 57;  behind 17 .. 18 | 18 .. 19 launches ops_done 29 .. 32 | 28 .. 33
  slide  99 ops | 99;  532 launches of at most 1260 | 532 of 1260;  n_full 88 | 90 .. 91;        behind 29 | 30 launches ops_done 27 | 27 .. 29
  margin 99 ops;  n_full 103;  behind 34 launches ops_done 30 of 99  (bf16 only)
  long   99 ops;  n_full 400 .. 414;  behind 133 .. 138 launches ops_done 29 of 99  (bf16 only)
Every schedule left every byte of every slot cache equal to the foreground pass's and 128 arrivals on every op: nothing was found in bg_worker.h, the
bodies or the recorders.  The premise of S-natural has room: a third of the launches leaves 27 .. 33 of the 99 ops complete.
"""
import functools

import numpy as np
import pytest

from tests.test_gpu_engine_step import PRECS, PREC_NAME, create, handles_fixture
from umgen_amd.config import MOD_ORDER

POISON = 0x7FA5                                        # exponent all ones, mantissa not zero in both 16-bit types
STACKS = ("ego", "map", "box", "tar")
N_WORKERS, GROUP = 128, 32                             # 4 XCDs x 32 workgroups (bg_queue.h kBgMaxWorkers, oar_common.h kEngGroup)
BG_GEMM, BG_LN, BG_ATTN_S, BG_ATTN_T, BG_EMBED, BG_WARP = 1, 2, 3, 4, 5, 6
KIND_NAME = {BG_GEMM: "gemm", BG_LN: "ln", BG_ATTN_S: "attn_s", BG_ATTN_T: "attn_t", BG_EMBED: "embed", BG_WARP: "warp"}
EST_NEVER_FITS = 0x40000000
NATURAL_CAP = 20000                                    # decode launches; the production pass (many blocks per stack) takes ~1800
WINDOWS = {"P3": (3, 4, 11), "P1": (1, 2, 12), "slide": (4, 4, 13)}      # name -> (T, cond_cap, scene id)

one = handles_fixture("one")


@pytest.fixture(scope="module")
def long_handle():
    e = create("one", 1, max_cond_frames=22, max_frame_len=32)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------
# windows, caches, the reference
# ---------------------------------------------------------------------------------------------------------------------------
def window(T, scene_id):
    """(mod -> [T, S_mod], the next frame's pose tokens)"""
    from umgen_amd.synth import synthetic_scene
    sc = synthetic_scene(scene_id, n_frames=T + 1)
    return {m: sc[m][0, :T] for m in MOD_ORDER}, sc["pose"][0, T]


def known_slots(T, cap):
    return min(T + 1, cap) - 1


@functools.lru_cache(maxsize=None)
def poison_bits(shape):
    return np.full(shape, POISON, np.uint16)


def poison(e):
    for s in range(4):
        e.dbg_tcache_put(s, 0, poison_bits(e._tcache_shape(s)))


def caches(e):
    return [e.dbg_tcache_get(s, 0) for s in range(4)]


def begin(e, T, cap, scene_id, **kw):
    w, ego = window(T, scene_id)
    return e.dbg_bg_begin(w, ego, cap, **kw)


_REF = {}


def reference(e, key, T, cap, scene_id):
    """the slot caches behind the foreground pass over poisoned caches, once per (handle, window)"""
    if key not in _REF:
        P = known_slots(T, cap)
        poison(e)
        assert begin(e, T, cap, scene_id, foreground=True).shape[0] == 0
        ref = caches(e)
        for name, c in zip(STACKS, ref):
            assert (c[:, P:] == POISON).all(), f"{name} stack: the foreground pass wrote a slot >= {P}"
            assert not (c[:, :P] == POISON).any(), f"{name} stack: poison left in a slot < {P} (a k | v row the pass did not write, or a NaN)"
        _REF[key] = ref
    return _REF[key]


def same_caches(got, ref, what):
    for s, (g, r) in enumerate(zip(got, ref)):
        if not np.array_equal(g, r):
            b, t, row = (int(i[0]) for i in np.nonzero((g != r).any(axis=3)))
            n = int((g != r).any(axis=3).sum())
            raise AssertionError(f"{what}: {STACKS[s]} stack, block 0, slot {t}, first differing row {row} ({n} rows differ in all): "
                                 f"{g[b, t, row][g[b, t, row] != r[b, t, row]][:4]} against {r[b, t, row][g[b, t, row] != r[b, t, row]][:4]}")


def complete(e, n_ops, what):
    state, ops_done, arrive = e.dbg_bg_state(n_ops)
    assert ops_done == n_ops, f"{what}: ops_done {ops_done} of {n_ops}; workers' ops {sorted(set(state[:, 0].tolist()))}"
    assert (state[:, 0] == n_ops).all(), f"{what}: workers not at the end of the list: {np.flatnonzero(state[:, 0] != n_ops)[:8]} at ops {state[state[:, 0] != n_ops, 0][:8]}"
    bad = np.flatnonzero(arrive != N_WORKERS)
    assert bad.size == 0, f"{what}: arrivals != {N_WORKERS} on ops {bad[:8]}: {arrive[bad[:8]]}"
    return state, arrive


# ---------------------------------------------------------------------------------------------------------------------------
# the dealing of units, restated (bg_worker.h bg_worker / gemm256_list_count)
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_list_count(nI, nJ, splitI, nx, xcd):
    gJ = nx // splitI
    hI, qJ = -(-nI // splitI), -(-nJ // gJ)
    i0, j0 = (xcd % splitI) * hI, (xcd // splitI) * qJ
    return max(0, min(nI, i0 + hI) - i0) * max(0, min(nJ, j0 + qJ) - j0)


def mine_of(head):
    """units of every worker [128] of the op with these BgOpHead words"""
    kind, _, n_units, _, i0, i1, i2, _ = (int(v) for v in head)
    out = np.zeros(N_WORKERS, np.int64)
    for w in range(N_WORKERS):
        if kind == BG_GEMM:
            cnt, lb = gemm_list_count(i0, i1, i2, N_WORKERS // GROUP, w // GROUP), w % GROUP
            out[w] = -(-(cnt - lb) // GROUP) if lb < cnt else 0
        else:
            out[w] = -(-(n_units - w) // N_WORKERS) if w < n_units else 0
    return out


def shares(heads):
    m = np.stack([mine_of(h) for h in heads])
    for k, h in enumerate(heads):
        assert m[k].sum() == h[2], f"op {k} ({KIND_NAME.get(int(h[0]), h[0])}): the workers' shares add up to {m[k].sum()}, not its {h[2]} units"
    return m


def kinds_with_a_share_of_two(heads, m):
    return {int(h[0]) for k, h in enumerate(heads) if m[k].max() >= 2}


# ---------------------------------------------------------------------------------------------------------------------------
# the schedules
# ---------------------------------------------------------------------------------------------------------------------------
def drain_schedule(e, key, T, cap, scene_id):
    ref = reference(e, key, T, cap, scene_id)
    for chunk in (0, 1, 3, 5):
        poison(e)
        heads = begin(e, T, cap, scene_id, foreground=False, chunk=chunk)
        n_ops = heads.shape[0]
        assert n_ops > 0 and (chunk == 0 or (heads[:, 3] == chunk).all())
        shares(heads)
        e.dbg_bg_drain()
        what = f"{key} drain, chunk {chunk or 'as recorded'}"
        same_caches(caches(e), ref, what)
        state, arrive = complete(e, n_ops, what)
        e.dbg_bg_drain()                                             # a finished queue: nothing left to do, nothing done
        state2, arrive2 = complete(e, n_ops, what + ", second drain")
        np.testing.assert_array_equal(state2, state, err_msg=what + ": a drain launch on the finished queue changed a worker's state")
        same_caches(caches(e), ref, what + ", second drain")
    e.dbg_bg_end()
    print(f"BGPASS {key}: {n_ops} ops")


def one_unit_schedule(e, key, T, cap, scene_id, all_kinds):
    ref = reference(e, key, T, cap, scene_id)
    poison(e)
    heads = begin(e, T, cap, scene_id, foreground=False)
    n_ops = heads.shape[0]
    m = shares(heads)
    need = kinds_with_a_share_of_two(heads, m)
    if all_kinds:
        assert need == set(KIND_NAME), f"kinds without an op of >= 2 units for some worker: {[KIND_NAME[k] for k in set(KIND_NAME) - need]}"
    limit = 2 * (int(m.max(axis=1).sum()) + n_ops)
    done, states = e.dbg_bg_steps(limit, est=EST_NEVER_FITS, until_done=True, states=True)
    if done[-1] != n_ops:
        state, ops_done, arrive = e.dbg_bg_state(n_ops)
        raise AssertionError(f"{key} one unit per launch: {ops_done} of {n_ops} ops after {limit} launches; workers (op, done | arrived):\n{state[:, :2]}")
    print(f"BGPASS {key}: {n_ops} ops, one unit per launch: {len(done)} launches (cap {limit})")
    # what the launch boundaries looked like: a worker in the middle of its share for every kind that has one, an arrival on an incomplete op
    op, word = states[:, :, 0].astype(np.int64), states[:, :, 1]
    live = op < n_ops
    opc = np.minimum(op, n_ops - 1)
    units, arrived = (word & 0x7FFFFFFF).astype(np.int64), (word >> 31) != 0
    share = m[opc, np.arange(N_WORKERS)[None, :]]
    assert (units[live] <= share[live]).all(), "a worker with more units done than its share"
    kind = heads[opc, 0]
    mid = live & (units > 0) & (units < share)
    seen = {int(k) for k in np.unique(kind[mid])}
    assert need <= seen, f"{key}: no worker seen inside its share of a {[KIND_NAME[k] for k in need - seen]} op at a launch boundary"
    assert (live & arrived & (op >= done[:, None].astype(np.int64))).any(), f"{key}: no worker seen arrived on an op that was not complete"
    # one unit per worker and launch: behind a launch no worker is more than one unit further into the SAME op than before it
    same_op = (op[1:] == op[:-1]) & live[1:]
    assert (units[1:][same_op] - units[:-1][same_op] <= 1).all(), f"{key}: a worker ran more than one unit of an op in one launch"
    what = f"{key} one unit per launch"
    same_caches(caches(e), ref, what)
    complete(e, n_ops, what)
    e.dbg_bg_end()


def natural_schedule(e, key, T, cap, scene_id, compare_full=True, note="", **kw):
    ref = reference(e, key, T, cap, scene_id)
    key += note
    if compare_full:
        poison(e)
    heads = begin(e, T, cap, scene_id, foreground=False, **kw)
    n_ops = heads.shape[0]
    done, _ = e.dbg_bg_steps(NATURAL_CAP, until_done=True)
    n_full = len(done)
    assert done[-1] == n_ops, f"{key}: {done[-1]} of {n_ops} ops after {n_full} decode launches"
    what = f"{key} natural schedule, {n_full} launches"
    if compare_full:
        same_caches(caches(e), ref, what)
    complete(e, n_ops, what)
    poison(e)
    assert begin(e, T, cap, scene_id, foreground=False, **kw).shape[0] == n_ops
    part, _ = e.dbg_bg_steps(n_full // 3, until_done=False)
    _, ops_done, _ = e.dbg_bg_state(n_ops)
    print(f"BGPASS {key}: {n_ops} ops, n_full {n_full}; behind {len(part)} launches ops_done {ops_done} of {n_ops}")
    assert len(part) == n_full // 3 and 0 < ops_done < n_ops, f"{key}: behind {len(part)} of {n_full} launches ops_done is {ops_done} of {n_ops}: the drain has nothing to resume"
    e.dbg_bg_drain()
    what = f"{key} {len(part)} launches, then the drain"
    same_caches(caches(e), ref, what)
    complete(e, n_ops, what)
    e.dbg_bg_end()


@pytest.mark.gpu
@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("prec", PRECS)
def test_drain_launches_equal_the_foreground_pass(one, prec, win):
    drain_schedule(one(prec), f"{PREC_NAME[prec]} {win}", *WINDOWS[win])


@pytest.mark.gpu
@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("prec", PRECS)
def test_one_unit_per_launch_equals_the_foreground_pass(one, prec, win):
    T, cap, _ = WINDOWS[win]
    one_unit_schedule(one(prec), f"{PREC_NAME[prec]} {win}", *WINDOWS[win], all_kinds=known_slots(T, cap) == 3)


@pytest.mark.gpu
@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("prec", PRECS)
def test_decode_launches_then_drain_equal_the_foreground_pass(one, prec, win):
    natural_schedule(one(prec), f"{PREC_NAME[prec]} {win}", *WINDOWS[win])


@pytest.mark.gpu
def test_wider_margin_stops_the_workers_elsewhere(one):
    """margin_ticks 4000 instead of 1000: the workers leave every launch 40 us before its expected end, so the same pass is cut at other units"""
    natural_schedule(one(1), "bf16 P3", *WINDOWS["P3"], note=", margin 40 us", margin_ticks=4000)


@pytest.mark.gpu
def test_long_window_decode_launches_then_drain(long_handle):
    """P = 21: more than 20 slots, the 32-slot instantiation of the temporal body (bg_attn_t<TT, 32>)"""
    e = long_handle
    heads = begin(e, 21, 22, 14, foreground=False)
    e.dbg_bg_end()
    assert {int(h[1]) for h in heads if h[0] == BG_ATTN_T} == {32}
    natural_schedule(e, "bf16 long", 21, 22, 14, compare_full=False)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_handle_serves_rollouts_after_an_abandoned_pass(one, prec):
    """begin, a few decode launches, end in the middle of the pass; then two greedy frames: the second one runs on the slot caches of ITS OWN background pass"""
    from umgen_amd.synth import synthetic_scene
    e = one(prec)
    poison(e)
    heads = begin(e, *WINDOWS["P3"], foreground=False)
    done, _ = e.dbg_bg_steps(8, until_done=False)
    assert 0 < done[-1] < heads.shape[0], f"ops_done {done[-1]} of {heads.shape[0]} behind 8 launches"
    e.dbg_bg_end()
    scene = synthetic_scene(15, n_frames=2)
    before = e.timings()["overlapped_frames"]
    out = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    assert e.timings()["overlapped_frames"] - before == 1
    fresh = create("one", prec)
    try:
        want = fresh.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
        assert fresh.timings()["overlapped_frames"] == 1
    finally:
        fresh.close()
    for m in MOD_ORDER:
        np.testing.assert_array_equal(out[m], want[m], err_msg=m)


@pytest.mark.gpu
def test_hooks_refuse_what_the_workers_do_not_serve(one):
    from umgen_amd.engine import UMGenError
    w, ego = window(3, 11)
    for kw, reason in ((dict(which="many", max_batch=1), "no background workers"), (dict(which="one", max_batch=2), "no background workers")):
        e = create(kw["which"], 1, max_batch=kw["max_batch"])
        try:
            for call in (lambda: e.dbg_bg_begin(w, ego, 4, foreground=True), lambda: e.dbg_bg_est(7), lambda: e.dbg_bg_state(1), lambda: e.dbg_bg_steps(1),
                         e.dbg_bg_drain, e.dbg_bg_end, lambda: e.dbg_tcache_get(0, 0)):
                with pytest.raises(UMGenError, match=reason) as err:
                    call()
                assert "rc=-5" in str(err.value)                    # UMGEN_E_UNSUPPORTED
        finally:
            e.close()
    e = one(1)
    for T in (0, 4, 5):                                             # growing windows: the pass covers 1 .. max_cond_frames - 1 = 3 slots
        wt, _ = window(max(T, 1), 11)
        with pytest.raises(UMGenError, match=f"a window of {T} slots"):
            e.dbg_bg_begin({m: wt[m][:T] for m in MOD_ORDER}, ego, T + 1, foreground=True)
    with pytest.raises(UMGenError, match="no background pass is pending"):
        e.dbg_bg_drain()
    with pytest.raises(UMGenError, match="outside its vocabulary"):
        e.dbg_bg_begin(w, ego + 5000, 4, foreground=True)
    with pytest.raises(UMGenError, match="stack=4"):
        e.dbg_tcache_get(4, 0)
    with pytest.raises(UMGenError, match="block=1"):
        e.dbg_tcache_get(3, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the restated dealing of units
# ---------------------------------------------------------------------------------------------------------------------------
def test_restated_shares_cover_every_unit_once():
    """mine_of over all workers == n_units: for the GEMM partition (4 lists with and without the feature split, fewer tiles than lists) and the strided kinds"""
    for nI, nJ, splitI in ((3, 9, 1), (12, 26, 2), (6, 1, 2), (3, 1, 1), (1, 1, 1), (24, 26, 2)):
        m = mine_of((BG_GEMM, 0, nI * nJ, 64, nI, nJ, splitI, 0))
        assert m.sum() == nI * nJ and m.reshape(4, GROUP).sum(axis=1).tolist() == [gemm_list_count(nI, nJ, splitI, 4, x) for x in range(4)]
        assert (np.diff(m.reshape(4, GROUP), axis=1) <= 0).all() and (m.reshape(4, GROUP).max(axis=1) - m.reshape(4, GROUP).min(axis=1) <= 1).all()
    for n in (1, 127, 128, 129, 828, 8828):
        m = mine_of((BG_LN, 0, n, 256, 768, 0, 0, 0))
        assert m.sum() == n and m.max() == -(-n // N_WORKERS) and (np.diff(m) <= 0).all()
