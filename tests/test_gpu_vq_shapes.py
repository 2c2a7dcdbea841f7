"""-m gpu: the VQ decoder and encoder handles (csrc/vqdec.hip, csrc/vqenc.hip through umgen_amd/vq.py) at the configurations the
recorded goldens never reach, against the float64 restatement of tests/vq_ref.py computed at test time (one run per configuration and
session; tests/test_vq_ref.py pins the restatement on the CPU, against the goldens and the reference itself).

The six configurations (vq_ref.CONFIGS) reach: one level without any resampling; attention over 1, 4, 6, 15, 24, 35, 96 and 99 positions
(not multiples of 4, below and above one wave's 64 lanes, odd K in the P.V product), of 32 / 64 / 96 / 192 channels; attention at every
level, so that the finest level sizes the attention workspace; widths that shrink towards the coarse end and go down and up again
(nin_shortcut in both directions, the finest level sizing `act` and `col`); 1, 2, 5 and 7 input channels; 3 res blocks; embed_dim 4, 16,
32 and 64 with codebooks that end in a partial quantiser tile; one code; an empty batch.

Bars, all from the restatement (never from the GPU run): outputs and rows within 10 x err32, err32 = max |restatement(float32) -
restatement(float64)| on the same inputs (test_gpu_vq_encode.py's Z_BAR rule); codes by test_codes_match_reference's rule with the
restatement's margin.

Measured on an MI355X, max |gpu - float64| (its bar, 10 x err32 as measured on that machine's CPU):
  configuration      decoder output         encoder rows
  one_level          6.1e-7  (1.20e-5)      5.7e-7  (3.64e-6)
  wide_groups        5.7e-6  (4.88e-5)      1.0e-6  (4.42e-6)
  attn_everywhere    4.7e-6  (4.61e-5)      5.6e-7  (4.19e-6)
  shrinking_widths   1.5e-6  (2.16e-5)      4.4e-7  (2.92e-6)
  single_token       3.5e-6  (5.89e-5)      2.7e-7  (3.17e-4)
  ninety_nine        1.7e-6  (1.65e-5)      1.1e-6  (6.59e-6)
and every code equal to the restatement's in all six (no position under the margin threshold in any of them).

What these configurations found (read in the code before the first run; the unfixed code writes out of bounds at these shapes and was not run on
them): attn_block stored its score rows n floats apart through the GEMM epilogue that writes 4 floats at a time, so for n not a multiple of 4
the last store of a row ran into the next row -- wrong scores wherever the neighbour's own store came earlier, e.g. rows 4, 8, 12 of a 15-position
attention: one_level (15), wide_groups (35), attn_everywhere (6), ninety_nine (99) -- and, behind the last row, past the buffer (those four, and
shrinking_widths (2) and single_token (1), whose values were right).  Fixed in csrc/vq_common.h (rows attn_ld(n) floats apart) and csrc/gemm.hip
(epilogue_tail); tests/test_gpu_vq_blocks.py::test_score_gemm_with_a_row_count_that_is_no_multiple_of_4 holds the GEMM form itself.  No
workspace of either create function was undersized.
"""
import numpy as np
import pytest

from tests import vq_ref
from tests.test_gpu_vq_encode import host_argmin
from umgen_amd.vq import VQDecoder, VQEncoder, decoder_keys, encoder_keys, synth_vq_tensor

pytestmark = pytest.mark.gpu
NAMES = list(vq_ref.CONFIGS)

_handles = {}
_runs = {}


def handles(name):
    """one decoder and one encoder per configuration and session"""
    if name not in _handles:
        cfg = vq_ref.CONFIGS[name]
        d = VQDecoder(cfg)
        missing, _ = d.load_state_dict(vq_ref.weights(cfg, decoder_keys))
        assert not missing
        e = VQEncoder(cfg)
        missing, _ = e.load_state_dict(vq_ref.weights(cfg, encoder_keys))
        assert not missing
        _handles[name] = (d, e)
    return _handles[name]


def run(name):
    """One decode and one encode per configuration and session: (restatement, out, codes, z)."""
    if name not in _runs:
        r = vq_ref.restated(name)
        d, e = handles(name)
        out = d.decode_code(r["codes_in"])
        codes, z = e.encode(r["x"], return_z=True)
        assert out.shape == r["out64"].shape and out.dtype == np.float32
        assert codes.shape == r["codes64"].shape and codes.dtype == np.int64 and z.shape == r["z64"].shape and z.dtype == np.float32
        _runs[name] = (r, out, codes, z)
    return _runs[name]


@pytest.mark.parametrize("name", NAMES)
def test_decoder_output(name):
    r, out, _, _ = run(name)
    err = float(np.abs(out.astype(np.float64) - r["out64"]).max())
    print(f"{name}: max |out_gpu - out64| = {err:.3e}, bar = {10.0 * r['err32_out']:.3e}, restatement fp32 vs float64 = {r['err32_out']:.3e}")
    assert np.isfinite(out).all()
    assert err <= 10.0 * r["err32_out"]


@pytest.mark.parametrize("name", NAMES)
def test_encoder_rows(name):
    r, _, _, z = run(name)
    err = float(np.abs(z.astype(np.float64) - r["z64"]).max())
    print(f"{name}: max |z_gpu - z64| = {err:.3e}, bar = {10.0 * r['err32_z']:.3e}, restatement fp32 vs float64 = {r['err32_z']:.3e}")
    assert np.isfinite(z).all()
    assert err <= 10.0 * r["err32_z"]


@pytest.mark.parametrize("name", NAMES)
def test_codes(name):
    """test_codes_match_reference's rule with the restatement's margin: equal wherever the margin is at least 4 x (4 x 10 x err32_z) + 1e-6, the
    best or the second best below it, and at most 2 % of the positions below it (none in a case of fewer than 50 positions)."""
    r, _, codes, _ = run(name)
    thr = vq_ref.code_threshold(r["err32_z"])
    close = r["margin"] < thr
    diff = codes != r["codes64"]
    print(f"{name}: threshold {thr:.3e}, {int(close.sum())} of {close.size} positions under it, {int(diff.sum())} codes differ from the restatement "
          f"({int((diff & ~close).sum())} of them at or above the threshold)")
    assert close.mean() <= 0.02 and (close.size >= 50 or not close.any())
    assert not (diff & ~close).any()
    assert np.all((codes == r["codes64"]) | (codes == r["second64"]))
    assert codes.min() >= 0 and codes.max() < vq_ref.CONFIGS[name]["n_embed"]


@pytest.mark.parametrize("name", NAMES)
def test_quantiser_is_the_exact_argmin_of_its_own_rows(name):
    """As in test_gpu_vq_encode.py, on the GPU's own rows; for embed_dim != 16 with the derived threshold (8 D + 24) 2^-24 of
    test_gpu_vq_quantize.py in place of that file's 1e-6."""
    cfg = vq_ref.CONFIGS[name]
    _, _, codes, z = run(name)
    D = cfg["embed_dim"]
    thr = 1e-6 if D == 16 else (8 * D + 24) * 2.0 ** -24
    np.testing.assert_allclose(np.linalg.norm(z.astype(np.float64), axis=-1), 1.0, atol=1e-6)
    cb = synth_vq_tensor("quantize.embedding.weight", (cfg["n_embed"], D), vq_ref.WEIGHT_SEED)
    if cfg["n_embed"] == 1:
        assert not codes.any()
        return
    best, margin = host_argmin(z, cb)
    clear = margin > thr
    print(f"{name}: {int((~clear).sum())} of {clear.size} positions within {thr:.2e}, {int((codes.reshape(-1) != best).sum())} codes differ from the float64 arg-min")
    assert (~clear).mean() < 0.005
    np.testing.assert_array_equal(codes.reshape(-1)[clear], best[clear])


@pytest.mark.parametrize("name", NAMES)
def test_frames_are_independent(name):
    """byte for byte: the batch of 2 equals the two singles, on both handles"""
    r, out, codes, z = run(name)
    d, e = handles(name)
    for i in range(vq_ref.N_FRAMES):
        assert d.decode_code(r["codes_in"][i:i + 1]).tobytes() == out[i:i + 1].tobytes()
        ci, zi = e.encode(r["x"][i:i + 1], return_z=True)
        assert ci.tobytes() == codes[i:i + 1].tobytes() and zi.tobytes() == z[i:i + 1].tobytes()


def test_empty_batch():
    """n = 0 returns empty arrays of the right shape and leaves both handles usable"""
    name = "single_token"
    cfg = vq_ref.CONFIGS[name]
    r, out, codes, z = run(name)
    d, e = handles(name)
    o0 = d.decode_code(np.zeros((0,) + tuple(cfg["token_hw"]), np.int64))
    assert o0.shape == (0,) + out.shape[1:] and o0.dtype == np.float32
    c0, z0 = e.encode(np.zeros((0,) + r["x"].shape[1:], np.float32), return_z=True)
    assert c0.shape == (0,) + codes.shape[1:] and c0.dtype == np.int64 and z0.shape == (0,) + z.shape[1:]
    assert e.encode(np.zeros((0,) + r["x"].shape[1:], np.float32)).shape == (0,) + codes.shape[1:]
    assert d.decode_code(r["codes_in"]).tobytes() == out.tobytes()
    c1, z1 = e.encode(r["x"], return_z=True)
    assert c1.tobytes() == codes.tobytes() and z1.tobytes() == z.tobytes()
