"""Helpers shared by the -m gpu tests (ctypes calls into libumgen_hip.so's kernel-level hooks)."""
import ctypes as C

import numpy as np
import torch

from umgen_amd import _lib


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 ndarray -> raw bfloat16 bits (uint16), round-to-nearest-even like torch."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


def bf16_round(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def from_bits(b: np.ndarray) -> np.ndarray:
    return torch.from_numpy(b.view(np.int16)).view(torch.bfloat16).float().numpy()


# precision codes of the umgen_dbg_* hooks: 0 = fp32, 1 = bf16 (raw bits), 2 = fp16 (IEEE half bits)
def bits16(a: np.ndarray, code: int) -> np.ndarray:
    return bf16_bits(a) if code == 1 else np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def round16(a: np.ndarray, code: int) -> np.ndarray:
    return bf16_round(a) if code == 1 else np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def from_bits16(b: np.ndarray, code: int) -> np.ndarray:
    return from_bits(b) if code == 1 else b.view(np.float16).astype(np.float32)


NAN32 = 0x7FC00000
NAN16 = {1: 0x7FC0, 2: 0x7E00}
SCALE_QK = float(np.float32(1.0 / np.sqrt(48.0)))


def ulp16(v, prec):
    """spacing of the 16-bit type at |v| (the subnormal spacing below its normal range)"""
    mant, emin = (7, -126) if prec == 1 else (10, -14)
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** emin))) - mant)


def attn_bound(ref, A, prec, S, vmax):
    """Componentwise bar of an S-key softmax attention output against its fp64 reference `ref` on the operands as handed over, with
    A = sum_j p_j |v_j| / sum_j p_j from that reference: u (A + |ref|) + 2e-5 max(1, A), u = 2^-8 (bf16) | 2^-11 (fp16) | 0 (fp32).  u A is
    the worst case of rounding every p to the operand type while l sums the unrounded p, u |ref| the output rounding, 2e-5 the project's bar
    for what is computed in fp32.  fp16 adds S 2^-25 max|v| (`vmax`, broadcastable): a p below fp16's subnormal range is lost."""
    u = {0: 0.0, 1: 2.0 ** -8, 2: 2.0 ** -11}[prec]
    b = u * (A + np.abs(ref)) + 2e-5 * np.maximum(1.0, A)
    return b + S * 2.0 ** -25 * vmax if prec == 2 else b


def ln_input(rng, M, K):
    """rows fed to LayerNorm: per-row means in [-4, 4] and standard deviations in [0.05, 3] (both ends present)"""
    mu = rng.uniform(-4, 4, (M, 1))
    sd = rng.uniform(0.05, 3, (M, 1))
    mu[0], sd[0] = 4.0, 0.05
    mu[-1], sd[-1] = -4.0, 3.0
    return (mu + sd * rng.standard_normal((M, K))).astype(np.float32)


def ref_ln(x, w):
    x = x.astype(np.float64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * w.astype(np.float64)


def gelu64(v):
    return torch.nn.functional.gelu(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))).numpy()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def check(rc):
    assert rc == 0, f"libumgen_hip debug hook failed rc={rc}"


def lib():
    return _lib.load_library()
