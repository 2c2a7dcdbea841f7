"""The side outputs of generated tokens -- logp, the diagnostics, logz -- travel one path from the samplers to the caller (TokenSide / FrameSide /
GenSide); what one of them is must not depend on which others the call asked for.  One tiny-config rollout -- 2 scenes x 2 samples, so the first frame
takes the fan ego path and the second the plain one, with scene offsets in both; 2 history frames, 2 new frames, logit-bias tables with a few bans on
pose and bbox3d -- is run under every subset of {return_logp, return_detail (topk 5), return_logz}: the tokens are byte-equal across all eight calls,
and every output is byte-equal (NaN positions as bits) to the same output of the call that asked for it alone.  One pair under top-p: all three
against none.  The references are the engine's own narrower calls, each held to its own oracle by the tests of its pull request."""
import numpy as np
import pytest

from tests.test_gpu_rollout_bias import scenes_of, vocab_of
from tests.test_gpu_rollout_logp import close_engines, engine, sampled  # noqa: F401
from umgen_amd.config import MOD_ORDER

pytestmark = pytest.mark.gpu
B, N, NEW, TOPK = 2, 2, 2, 5
ASK = ("logp", "logz", "detail")      # in the order rollout returns them
SUBSETS = [tuple(k for i, k in enumerate(ASK) if mask >> i & 1) for mask in range(8)]
_calls = {}


def tables(cfg):
    """finite bias on pose and bbox3d, a few tokens of every row banned"""
    rng = np.random.default_rng(11)
    V = vocab_of(cfg)
    out = {"pose": rng.uniform(-2, 2, (3, V["pose"])).astype(np.float32), "bbox3d": rng.uniform(-2, 2, (11, V["bbox3d"])).astype(np.float32)}
    for t in out.values():
        for row in t:
            row[rng.choice(np.arange(1, row.size), 7, replace=False)] = -np.inf
    return out


def call(method, asked):
    """the rollout with the outputs `asked` -> {"tokens": ..., and every output asked for}; one call per (method, asked) and module"""
    key = (method, asked)
    if key not in _calls:
        e = engine("tiny", "fp32", max_batch=B * N)
        smp = sampled(e.cfg, sample_method=method, p=0.6, p_map=0.3)
        res = e.rollout(scenes_of(B), NEW, cond_frames=3, input_cond_frames=2, seeds=list(range(41, 41 + B * N)), sampling=smp, samples=N,
                        logit_bias=tables(e.cfg), return_logp="logp" in asked, return_logz="logz" in asked, return_detail="detail" in asked,
                        topk=TOPK if "detail" in asked else 0)
        assert e.last_shared_slots == 1, "the first frame did not take the fan path"
        res = res if isinstance(res, tuple) else (res,)
        assert len(res) == 1 + len(asked)
        _calls[key] = dict(zip(("tokens",) + tuple(k for k in ASK if k in asked), res))
    return _calls[key]


def bits(x):
    """an output as bytes per (key,) modality: NaN positions compare as bits"""
    if all(m in x for m in MOD_ORDER):
        return {m: np.ascontiguousarray(x[m]).tobytes() for m in MOD_ORDER}
    return {(k, m): np.ascontiguousarray(x[k][m]).tobytes() for k in x for m in MOD_ORDER}


@pytest.fixture(scope="module", autouse=True)
def forget_calls():
    yield
    _calls.clear()


@pytest.mark.parametrize("asked", SUBSETS, ids=lambda a: "+".join(a) or "none")
def test_an_output_does_not_depend_on_what_else_was_asked(asked):
    got = call("topk", asked)
    assert bits(got["tokens"]) == bits(call("topk", ())["tokens"]), f"tokens of the call that asked for {asked}"
    for k in asked:
        alone = call("topk", (k,))[k]
        same = bits(got[k]) == bits(alone)
        assert same, f"{k} of the call that asked for {asked} differs from the call that asked for it alone"


def test_the_outputs_are_what_the_call_describes():
    """shapes, and that the run exercised what it is meant to: every head ran (no NaN), the biased classes have a logz, the others +0.0, lists of 5"""
    got = call("topk", ASK)
    for m in MOD_ORDER:
        lead = got["tokens"][m].shape[:2] + (NEW,)
        assert lead == (B, N, NEW) and got["logp"][m].shape[:3] == lead and got["logz"][m].shape == got["logp"][m].shape
        assert np.isfinite(got["logp"][m]).all() and np.isfinite(got["logz"][m]).all()
        assert got["detail"]["rank"][m].shape == got["logp"][m].shape and (got["detail"]["rank"][m] >= 0).all()
        assert got["detail"]["topk_tokens"][m].shape == got["logp"][m].shape + (TOPK,)
        assert got["logz"][m].view(np.uint32).any() == (m in ("pose", "bbox3d")), f"logz of {m}"
    assert len({got["tokens"]["map"][b, s, 2:].tobytes() for b in range(B) for s in range(N)}) == B * N, "the branches drew the same maps"


def test_top_p_all_three_against_none():
    got, none = call("top_p", ASK), call("top_p", ())
    assert bits(got["tokens"]) == bits(none["tokens"])
    assert bits(got["tokens"]) != bits(call("topk", ())["tokens"]), "top-p drew the top-k run's tokens: the pair checks nothing new"
