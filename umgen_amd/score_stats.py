"""Host-side reading of the score diagnostics (Engine.score(..., detail=True): umgen_score_detail)."""
from __future__ import annotations

import numpy as np


def in_sampler_support(rank, mass_above, method: str = "topk", top_k: int = 5, p: float = 0.9) -> np.ndarray:
    """Whether the scored token could have been drawn by the rollout's truncated sampler, per position (bool array).
    "topk": rank < top_k -- the sampler masks logits below the k-th value and keeps ties, rank counts the logits strictly above the token's.
    "topp": mass_above <= p -- the reference removes a token when the mass sorted in front of it exceeds p ((cumsum - p_sorted) > p);
    mass_above must have been computed at the sampler's temperature.
    The detail dict of a rollout (Engine.rollout(return_detail=True)) is accepted unchanged -- the same keys with the same meanings, and there the answer is exact
    for a token of the main draw: it is the row the sampler drew from.  A bbox3d token resampled from the TAR head (control / pad-avoid) is ranked on the AR row
    and may lie outside; positions where no head ran carry rank -1 / NaN mass and come back True / False."""
    if method == "topk":
        return np.asarray(rank) < top_k
    if method == "topp":
        return np.asarray(mass_above) <= p
    raise ValueError(f"in_sampler_support: method {method!r} is neither 'topk' nor 'topp'")
