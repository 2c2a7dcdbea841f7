"""VQ decoders and encoders on the GPU: the rollout's map / image tokens back to rasters, and
map / image rasters to the tokens the rollout conditions on.

Mirrors, on the C ABI of include/umgen.h (``umgen_vq_*``, csrc/vqdec.hip):
  * ``NormVQModel.decode_code`` / ``indices_to_quant`` + ``decode``    projects/tokenizer/vq_model.py:88-103, 126-150
  * the two model configurations                                       vq_model.py:153-202 (image: dim16 res512 f16, map: dim16 res256 f8)
  * ``Mapdecoder.decode_maps`` / ``Imagedecoder.decode_images``        projects/tools/decode_map.py:110-183
State-dict keys are the reference checkpoint's (``decoder.*``, ``post_quant_conv.*``, ``quantize.embedding.weight``); encoder and
EMA entries are ignored like ``strict=False``.  fp32 throughout (the reference decodes outside autocast).  No CPU fallback.

The encode side (``umgen_vqenc_*``, csrc/vqenc.hip) mirrors
  * ``NormVQModelTokenizer.encode`` / ``NormVQModel.encode``            projects/tokenizer/vq_tokenizer.py:25-47, vq_model.py:80-85
  * ``Encoder.forward`` -> ``quant_conv`` -> ``NormEMAVectorQuantizer``  vq_modules.py:179-290, quantize.py:414-479
with the keys ``encoder.*``, ``quant_conv.*`` and ``quantize.embedding.weight``; ``cfg`` may carry ``in_channels`` (default ``out_ch``).
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, Iterable, Tuple

import numpy as np

from . import _lib

# vq_model.py:153-202
IMAGE_VQ = dict(n_embed=8192, embed_dim=16, z_channels=256, resolution=512, out_ch=3, ch=128, ch_mult=(1, 1, 2, 2, 4), num_res_blocks=2,
                attn_resolutions=(32,), post_quant_ks=3, post_quant_pad=1, token_hw=(16, 32))
MAP_VQ = dict(n_embed=8192, embed_dim=16, z_channels=16, resolution=256, out_ch=5, ch=128, ch_mult=(1, 2, 2, 4), num_res_blocks=2,
              attn_resolutions=(16,), post_quant_ks=1, post_quant_pad=0, token_hw=(32, 32))


class VQError(RuntimeError):
    pass


def decoder_keys(cfg: dict) -> "OrderedDict[str, Tuple[int, ...]]":
    """Every state-dict entry the decode path reads, with its shape (Decoder.__init__, vq_modules.py:294-383; VQModel / NormVQModel
    __init__, vq_model.py:22-59, 126-150)."""
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    L = len(cfg["ch_mult"])
    ch, z = cfg["ch"], cfg["z_channels"]

    def conv(k, cin, cout, ks):
        out[k + ".weight"] = (cout, cin, ks, ks)
        out[k + ".bias"] = (cout,)

    def norm(k, c):
        out[k + ".weight"] = (c,)
        out[k + ".bias"] = (c,)

    def res(k, cin, cout):
        norm(k + ".norm1", cin)
        conv(k + ".conv1", cin, cout, 3)
        norm(k + ".norm2", cout)
        conv(k + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(k + ".nin_shortcut", cin, cout, 1)

    def attn(k, c):
        norm(k + ".norm", c)
        for n in ("q", "k", "v", "proj_out"):
            conv(f"{k}.{n}", c, c, 1)

    out["quantize.embedding.weight"] = (cfg["n_embed"], cfg["embed_dim"])
    conv("post_quant_conv", cfg["embed_dim"], z, cfg["post_quant_ks"])
    block_in = ch * cfg["ch_mult"][L - 1]
    curr_res = cfg["resolution"] // 2 ** (L - 1)
    conv("decoder.conv_in", z, block_in, 3)
    res("decoder.mid.block_1", block_in, block_in)
    attn("decoder.mid.attn_1", block_in)
    res("decoder.mid.block_2", block_in, block_in)
    for lv in reversed(range(L)):
        block_out = ch * cfg["ch_mult"][lv]
        for b in range(cfg["num_res_blocks"] + 1):
            res(f"decoder.up.{lv}.block.{b}", block_in, block_out)
            block_in = block_out
            if curr_res in cfg["attn_resolutions"]:
                attn(f"decoder.up.{lv}.attn.{b}", block_in)
        if lv != 0:
            conv(f"decoder.up.{lv}.upsample.conv", block_in, block_in, 3)
            curr_res *= 2
    norm("decoder.norm_out", block_in)
    conv("decoder.conv_out", block_in, cfg["out_ch"], 3)
    return out


def synth_vq_tensor(key: str, shape: Tuple[int, ...], seed: int) -> np.ndarray:
    """Deterministic PyTorch-default-like initialisation per key (no checkpoint offline): the golden generator loads the same
    tensors into the reference's NormVQModel."""
    import zlib
    rng = np.random.Generator(np.random.PCG64([seed & 0xFFFFFFFF, zlib.crc32(key.encode())]))
    if key.endswith("embedding.weight"):
        w = rng.standard_normal(shape).astype(np.float32)
        return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(np.float32)       # l2-normalised codes (NormEMAVectorQuantizer)
    if ".norm" in key:
        return (1.0 + 0.1 * (rng.random(shape, dtype=np.float32) * 2 - 1)).astype(np.float32) if key.endswith("weight") else \
            (0.1 * (rng.random(shape, dtype=np.float32) * 2 - 1)).astype(np.float32)
    fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
    bound = 1.0 / math.sqrt(max(fan_in, 1))
    return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(bound)).astype(np.float32)


def encoder_keys(cfg: dict) -> "OrderedDict[str, Tuple[int, ...]]":
    """Every state-dict entry the encode path reads, with its shape, in the order of the reference's ``state_dict()``
    (Encoder.__init__, vq_modules.py:180-261, then the codebook and quant_conv, vq_model.py:43-50, 130-136)."""
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    L = len(cfg["ch_mult"])
    ch = cfg["ch"]

    def conv(k, cin, cout, ks):
        out[k + ".weight"] = (cout, cin, ks, ks)
        out[k + ".bias"] = (cout,)

    def norm(k, c):
        out[k + ".weight"] = (c,)
        out[k + ".bias"] = (c,)

    def res(k, cin, cout):
        norm(k + ".norm1", cin)
        conv(k + ".conv1", cin, cout, 3)
        norm(k + ".norm2", cout)
        conv(k + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(k + ".nin_shortcut", cin, cout, 1)

    def attn(k, c):
        norm(k + ".norm", c)
        for n in ("q", "k", "v", "proj_out"):
            conv(f"{k}.{n}", c, c, 1)

    conv("encoder.conv_in", cfg.get("in_channels", cfg["out_ch"]), ch, 3)
    block_in = ch
    curr_res = cfg["resolution"]
    for lv in range(L):
        block_out = ch * cfg["ch_mult"][lv]
        widths = []
        for b in range(cfg["num_res_blocks"]):
            res(f"encoder.down.{lv}.block.{b}", block_in, block_out)
            block_in = block_out
            widths.append(block_in)
        if curr_res in cfg["attn_resolutions"]:         # (down.block is registered before down.attn)
            for b, c in enumerate(widths):
                attn(f"encoder.down.{lv}.attn.{b}", c)
        if lv != L - 1:
            conv(f"encoder.down.{lv}.downsample.conv", block_in, block_in, 3)
            curr_res //= 2
    res("encoder.mid.block_1", block_in, block_in)
    attn("encoder.mid.attn_1", block_in)
    res("encoder.mid.block_2", block_in, block_in)
    norm("encoder.norm_out", block_in)
    conv("encoder.conv_out", block_in, cfg["z_channels"], 3)
    out["quantize.embedding.weight"] = (cfg["n_embed"], cfg["embed_dim"])
    conv("quant_conv", cfg["z_channels"], cfg["embed_dim"], 1)
    return out


def synth_vq_raster(cfg: dict, n: int, seed: int) -> np.ndarray:
    """Deterministic numpy-only test rasters [n, in_channels, H, W] in [-1, 1] on the uint8 grid: coarse noise in 8 x 8 blocks plus
    0.3 x fine noise through tanh (the golden generator and the GPU tests build identical inputs from the seed)."""
    L = len(cfg["ch_mult"])
    H, W = cfg["token_hw"][0] << (L - 1), cfg["token_hw"][1] << (L - 1)
    c = cfg.get("in_channels", cfg["out_ch"])
    rng = np.random.Generator(np.random.PCG64(seed))
    coarse = rng.standard_normal((n, c, (H + 7) // 8, (W + 7) // 8))
    fine = rng.standard_normal((n, c, H, W))
    v = np.tanh(np.kron(coarse, np.ones((8, 8)))[:, :, :H, :W] + 0.3 * fine)
    return (np.round((v + 1.0) * 127.5) / 127.5 - 1.0).astype(np.float32)


def quantized(codes, z, codebook):
    """What the reference's ``QuantizedToken`` carries besides the indices (vq_model.py:80-85, quantize.py:431, 467-474): the codebook
    rows ``z_q`` [n, embed_dim, h, w] of ``codes`` [n, h, w] and ``loss = beta * mean((z_q - z) ** 2)`` with NormVQModel's
    ``beta = 1.0`` (vq_model.py:130-136), for the normalised rows ``z`` [n, h, w, embed_dim] that ``VQEncoder.encode(return_z=True)``
    returns and the ``quantize.embedding.weight`` array ``codebook``.  On the host, in numpy.  The reference's eval-mode side effect
    (the ``cluster_size`` usage EMA, quantize.py:435-439) is statistics only and is not reproduced."""
    codes = np.asarray(codes)
    z = np.asarray(z, dtype=np.float32)
    z_q = np.asarray(codebook, dtype=np.float32)[codes]
    loss = np.float32(1.0) * np.mean((z_q - z) ** 2, dtype=np.float32)
    return np.ascontiguousarray(np.moveaxis(z_q, -1, 1)), loss


class VQDecoder:
    """One decoder = one GPU.  ``cfg``: IMAGE_VQ / MAP_VQ or a dict with the same keys (the reference's ddconfig)."""

    def __init__(self, cfg: dict, device: int = 0):
        self.lib = _lib.load_library()
        self.cfg = dict(cfg)
        L = len(cfg["ch_mult"])
        c = _lib.VQConfig(n_embed=cfg["n_embed"], embed_dim=cfg["embed_dim"], z_channels=cfg["z_channels"], ch=cfg["ch"], out_ch=cfg["out_ch"],
                          n_levels=L, num_res_blocks=cfg["num_res_blocks"], n_attn_res=len(cfg["attn_resolutions"]),
                          resolution=cfg["resolution"], post_quant_ks=cfg["post_quant_ks"], post_quant_pad=cfg["post_quant_pad"],
                          token_h=cfg["token_hw"][0], token_w=cfg["token_hw"][1], device=device)
        for i, m in enumerate(cfg["ch_mult"]):
            c.ch_mult[i] = m
        for i, r in enumerate(cfg["attn_resolutions"]):
            c.attn_resolutions[i] = r
        self._h = C.c_void_p()
        rc = self.lib.umgen_vq_create(C.byref(c), C.byref(self._h))
        if rc != 0:
            msg = self.lib.umgen_vq_last_error(self._h).decode() if self._h else "umgen_vq_create failed"
            if self._h:
                self.lib.umgen_vq_destroy(self._h)
                self._h = None
            raise VQError(f"umgen_vq_create: {msg} (rc={rc})")
        self.out_hw = (cfg["token_hw"][0] << (L - 1), cfg["token_hw"][1] << (L - 1))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.umgen_vq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise VQError(f"{what}: {self.lib.umgen_vq_last_error(self._h).decode()} (rc={rc})")
        return rc

    def load_state_dict(self, sd: Iterable, strict: bool = False):
        """``sd``: the VQ checkpoint's ``state_dict`` (torch tensors or arrays).  Returns (missing, unexpected) like torch."""
        items = sd.items() if hasattr(sd, "items") else sd
        want = decoder_keys(self.cfg)
        seen, unexpected = set(), []
        for k, v in items:
            a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v), dtype=np.float32)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            rc = self._check(self.lib.umgen_vq_load_tensor(self._h, k.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), shape, a.ndim), f"load_tensor({k})")
            (seen.add(k) if rc == 0 else unexpected.append(k))
        missing = [k for k in want if k not in seen]
        if strict and (missing or unexpected):
            raise VQError(f"missing {missing[:4]}, unexpected {unexpected[:4]}")
        if not missing:
            self._check(self.lib.umgen_vq_finalize(self._h), "finalize")
        return missing, unexpected

    def decode_code(self, code_b) -> np.ndarray:
        """NormVQModel.decode_code (vq_model.py:93-97): codes [n, h, w] -> float32 [n, out_ch, H, W]."""
        codes = np.ascontiguousarray(np.asarray(code_b), dtype=np.int64)
        th, tw = self.cfg["token_hw"]
        if codes.ndim != 3 or codes.shape[1:] != (th, tw):
            raise VQError(f"codes have shape {codes.shape}, expected (n, {th}, {tw})")
        out = np.empty((codes.shape[0], self.cfg["out_ch"]) + self.out_hw, dtype=np.float32)
        self._check(self.lib.umgen_vq_decode(self._h, codes.shape[0], codes.ctypes.data_as(C.POINTER(C.c_int64)),
                                             out.ctypes.data_as(C.POINTER(C.c_float))), "decode")
        return out


class Mapdecoder:
    """decode_map.py:110-148: map tokens [1, T, 1024] (or [T, 1024]) -> reconstructions [T, 5, 256, 256] (``decode_maps`` of the
    reference additionally projects them to RGB with a seeded random 1x1 conv for visualisation: ``to_rgb`` below)."""

    def __init__(self, ckpt=None, device: int = 0, cfg: dict = MAP_VQ):
        self.dec = VQDecoder(cfg, device=device)
        sd = _state_dict_of(ckpt)
        if sd is not None:
            missing, _ = self.dec.load_state_dict(sd)
            if missing:
                raise VQError(f"map VQ checkpoint lacks {len(missing)} decoder tensors, e.g. {missing[:3]}")

    def decode_maps(self, map_tokens, H: int = 32, W: int = 32, rgb: bool = True) -> np.ndarray:
        t = np.asarray(map_tokens)
        t = t.reshape(-1, t.shape[-1]).reshape(-1, H, W)
        rec = np.concatenate([self.dec.decode_code(t[i:i + 20]) for i in range(0, t.shape[0], 20)])   # 20 frames per call like the reference
        if not rgb:
            return rec
        return np.concatenate([to_rgb(rec[i:i + 20]) for i in range(0, rec.shape[0], 20)])


class Imagedecoder:
    """decode_map.py:151-183: image tokens [1, T, 512] -> images [T, 3, 256, 512] in [-1, 1]."""

    def __init__(self, ckpt=None, device: int = 0, cfg: dict = IMAGE_VQ):
        self.dec = VQDecoder(cfg, device=device)
        sd = _state_dict_of(ckpt)
        if sd is not None:
            missing, _ = self.dec.load_state_dict(sd)
            if missing:
                raise VQError(f"image VQ checkpoint lacks {len(missing)} decoder tensors, e.g. {missing[:3]}")

    def decode_images(self, image_tokens, H: int = 16, W: int = 32) -> np.ndarray:
        t = np.asarray(image_tokens)
        if t.ndim == 1:
            t = t[None]
        t = t.reshape(-1, t.shape[-1]).reshape(-1, H, W)
        return np.concatenate([self.dec.decode_code(t[i:i + 20]) for i in range(0, t.shape[0], 20)])


class VQEncoder:
    """One encoder = one GPU.  ``cfg``: IMAGE_VQ / MAP_VQ or a dict with the same keys (``in_channels`` optional, default ``out_ch``)."""

    def __init__(self, cfg: dict, device: int = 0):
        try:
            self.lib = _lib.load_library()
        except (RuntimeError, OSError) as ex:
            raise VQError(str(ex)) from ex
        self.cfg = dict(cfg)
        L = len(cfg["ch_mult"])
        self.in_channels = int(cfg.get("in_channels", cfg["out_ch"]))
        c = _lib.VQConfig(n_embed=cfg["n_embed"], embed_dim=cfg["embed_dim"], z_channels=cfg["z_channels"], ch=cfg["ch"], out_ch=cfg["out_ch"],
                          n_levels=L, num_res_blocks=cfg["num_res_blocks"], n_attn_res=len(cfg["attn_resolutions"]),
                          resolution=cfg["resolution"], post_quant_ks=cfg.get("post_quant_ks", 1), post_quant_pad=cfg.get("post_quant_pad", 0),
                          token_h=cfg["token_hw"][0], token_w=cfg["token_hw"][1], device=device)
        for i, m in enumerate(cfg["ch_mult"]):
            c.ch_mult[i] = m
        for i, r in enumerate(cfg["attn_resolutions"]):
            c.attn_resolutions[i] = r
        self._h = C.c_void_p()
        rc = self.lib.umgen_vqenc_create(C.byref(c), self.in_channels, C.byref(self._h))
        if rc != 0:
            msg = self.lib.umgen_vqenc_last_error(self._h).decode() if self._h else "umgen_vqenc_create failed"
            if self._h:
                self.lib.umgen_vqenc_destroy(self._h)
                self._h = None
            raise VQError(f"umgen_vqenc_create: {msg} (rc={rc})")
        self.in_hw = (cfg["token_hw"][0] << (L - 1), cfg["token_hw"][1] << (L - 1))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.umgen_vqenc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise VQError(f"{what}: {self.lib.umgen_vqenc_last_error(self._h).decode()} (rc={rc})")
        return rc

    def load_state_dict(self, sd: Iterable, strict: bool = False):
        """``sd``: the VQ checkpoint's ``state_dict`` (torch tensors or arrays).  Returns (missing, unexpected) like torch."""
        items = sd.items() if hasattr(sd, "items") else sd
        want = encoder_keys(self.cfg)
        seen, unexpected = set(), []
        for k, v in items:
            a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v), dtype=np.float32)
            if k == "quantize.embedding.weight":
                self.codebook = a.copy()                      # host copy for quantized()
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            rc = self._check(self.lib.umgen_vqenc_load_tensor(self._h, k.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), shape, a.ndim), f"load_tensor({k})")
            (seen.add(k) if rc == 0 else unexpected.append(k))
        missing = [k for k in want if k not in seen]
        if strict and (missing or unexpected):
            raise VQError(f"missing {missing[:4]}, unexpected {unexpected[:4]}")
        if not missing:
            self._check(self.lib.umgen_vqenc_finalize(self._h), "finalize")
        return missing, unexpected

    def encode(self, x, return_z: bool = False):
        """NormVQModel.encode (vq_model.py:80-85): rasters [n, in_channels, H, W] in [-1, 1] -> int64 codes [n, token_h, token_w]
        (and, with ``return_z``, the l2-normalised rows [n, token_h, token_w, embed_dim] the nearest-code search ran on)."""
        x = np.ascontiguousarray(np.asarray(x), dtype=np.float32)
        th, tw = self.cfg["token_hw"]
        if x.ndim != 4 or x.shape[1:] != (self.in_channels,) + self.in_hw:
            raise VQError(f"rasters have shape {x.shape}, expected (n, {self.in_channels}, {self.in_hw[0]}, {self.in_hw[1]})")
        n = x.shape[0]
        codes = np.empty((n, th, tw), dtype=np.int64)
        z = np.empty((n, th, tw, self.cfg["embed_dim"]), dtype=np.float32) if return_z else None
        self._check(self.lib.umgen_vqenc_encode(self._h, n, x.ctypes.data_as(C.POINTER(C.c_float)), codes.ctypes.data_as(C.POINTER(C.c_int64)),
                                                z.ctypes.data_as(C.POINTER(C.c_float)) if return_z else None), "encode")
        return (codes, z) if return_z else codes

    def quantized(self, codes, z):
        """``quantized(codes, z, codebook)`` with the codebook this encoder was loaded with."""
        if getattr(self, "codebook", None) is None:
            raise VQError("no codebook loaded")
        return quantized(codes, z, self.codebook)


def _loaded_encoder(ckpt, device, cfg, what):
    enc = VQEncoder(cfg, device=device)
    sd = _state_dict_of(ckpt)
    if sd is not None:
        missing, _ = enc.load_state_dict(sd)
        if missing:
            raise VQError(f"{what} VQ checkpoint lacks {len(missing)} encoder tensors, e.g. {missing[:3]}")
    return enc


class Maptokenizer:
    """The inverse layout of ``Mapdecoder.decode_maps``: map rasters [T, 5, 256, 256] in [-1, 1] -> map tokens [T, 1024]."""

    def __init__(self, ckpt=None, device: int = 0, cfg: dict = MAP_VQ):
        self.enc = _loaded_encoder(ckpt, device, cfg, "map")

    def encode_maps(self, maps) -> np.ndarray:
        m = np.asarray(maps)
        if m.ndim == 3:
            m = m[None]
        codes = [self.enc.encode(m[i:i + 20]) for i in range(0, m.shape[0], 20)]       # 20 frames per call like the decoders
        return np.concatenate(codes).reshape(m.shape[0], -1) if codes else np.zeros((0, int(np.prod(self.enc.cfg["token_hw"]))), np.int64)


class Imagetokenizer:
    """The inverse layout of ``Imagedecoder.decode_images``: images [T, 3, 256, 512] in [-1, 1], or uint8 [T, 256, 512, 3] (mapped
    with ``x / 127.5 - 1``), -> image tokens [T, 512]."""

    def __init__(self, ckpt=None, device: int = 0, cfg: dict = IMAGE_VQ):
        self.enc = _loaded_encoder(ckpt, device, cfg, "image")

    def encode_images(self, images) -> np.ndarray:
        m = np.asarray(images)
        if m.dtype == np.uint8:
            if m.ndim == 3:
                m = m[None]
            m = (np.moveaxis(m, -1, 1).astype(np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)
        elif m.ndim == 3:
            m = m[None]
        codes = [self.enc.encode(m[i:i + 20]) for i in range(0, m.shape[0], 20)]
        return np.concatenate(codes).reshape(m.shape[0], -1) if codes else np.zeros((0, int(np.prod(self.enc.cfg["token_hw"]))), np.int64)


def _state_dict_of(ckpt):
    """``ckpt``: a path (VQModel.init_from_ckpt, vq_model.py:65-73: ``torch.load(path)["state_dict"]``), a loaded checkpoint dict
    holding ``state_dict``, or the state dict itself."""
    if ckpt is None:
        return None
    if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, "__fspath__"):
        import torch
        ckpt = torch.load(ckpt, map_location="cpu")
    if hasattr(ckpt, "keys") and "state_dict" in ckpt and not any(str(k).startswith("decoder.") for k in ckpt.keys()):
        ckpt = ckpt["state_dict"]
    return ckpt


def to_rgb(x: np.ndarray, seed: int = 0) -> np.ndarray:
    """decode_map.py:25-30 (visualisation only: a seeded random 1x1 convolution to 3 channels, min-max scaled to [-1, 1]; torch's
    generator is part of its definition, so it runs through torch on the host)."""
    import torch
    import torch.nn.functional as F
    torch.manual_seed(seed)
    xt = torch.from_numpy(np.ascontiguousarray(x))
    w = torch.randn(3, xt.shape[1], 1, 1).to(xt)
    y = F.conv2d(xt, weight=w)
    y = 2.0 * (y - y.min()) / (y.max() - y.min()) - 1.0
    return y.numpy()
