"""Synthetic inputs for the BASELINE.json configs.

The reference's default scene (rs = 10, sphere 500, observer (25, 0, 1),
camera (PI, 0), fov PI/2, FrozenFall with E = 1: renderer.rs:83-85,
lib.rs:72, observer.rs:70-81) is scale-invariant in rs (the RK4 step is an
angle), so the configs use it divided by 10: rs = 1, sphere 50, observer
(2.5, 0, 0.1).  The sky textures of the reference (.MISSING_LARGE_BLOBS) are
absent; configs 2-5 use a synthetic equirect checkerboard with xorshift noise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np


@dataclass(frozen=True)
class SceneConfig:
    name: str
    width: int
    height: int
    max_steps: int
    rs: float = 1.0
    sphere_r: float = 50.0
    position: tuple = (2.5, 0.0, 0.1)
    camera: tuple = (math.pi, 0.0)
    fov: float = math.pi / 2
    energy: float = 1.0
    state: int = 1  # GEO_OBSERVER_FROZEN_FALL
    step: float = math.pi / 100.0
    sky: str = "equirect"  # or "flat"
    sky_size: tuple = (4096, 2048)
    mode: str = "direct"  # "direct" (per-pixel fixed RK4), "fan" (reference-exact), "adaptive" (RK5(4))
    tol: float = 0.0      # adaptive mode: local error tolerance in u (0 = 1e-6)
    extra: dict = field(default_factory=dict)


CONFIGS = {
    "cfg1_256_cpu": SceneConfig("cfg1_256_cpu", 256, 256, 128, sky="flat", sky_size=(1, 1)),
    "cfg2_1080p": SceneConfig("cfg2_1080p", 1920, 1080, 512),
    "cfg3_4k": SceneConfig("cfg3_4k", 3840, 2160, 2048),
    "cfg4_4k_8gpu": SceneConfig("cfg4_4k_8gpu", 3840, 2160, 2048),
    # config 5 (a build extension): 8K, error-controlled Dormand-Prince RK5(4)
    # steps (tol 1e-6 in u, budget 2048 attempts), observer off-axis at
    # r = 1.3 rs (inside the photon sphere; (1.2, 0.5, 0) has |pos| = 1.3
    # exactly), camera (PI + 0.6, 0.3)
    "cfg5_8k_adaptive": SceneConfig("cfg5_8k_adaptive", 7680, 4320, 2048, position=(1.2, 0.5, 0.0),
                                    camera=(math.pi + 0.6, 0.3), mode="adaptive", tol=1e-6),
}

FLAT_COLOUR = (64, 128, 255, 255)


def xorshift32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32, copy=True)
    x ^= (x << np.uint32(13))
    x ^= (x >> np.uint32(17))
    x ^= (x << np.uint32(5))
    return x


def make_sky(kind: str = "equirect", size=(4096, 2048), seed: int = 0x5C4A) -> np.ndarray:
    """(h, w, 4) uint8.  'flat' = one colour; 'equirect' = 8 deg x 8 deg
    lat/long checkerboard plus per-texel xorshift noise (seed 0x5C4A)."""
    w, h = size
    if kind == "flat":
        sky = np.empty((h, w, 4), dtype=np.uint8)
        sky[:] = np.array(FLAT_COLOUR, dtype=np.uint8)
        return sky
    lon = (np.arange(w, dtype=np.float64) + 0.5) / w * 360.0
    lat = (np.arange(h, dtype=np.float64) + 0.5) / h * 180.0
    cell = ((np.floor(lat / 8.0)[:, None] + np.floor(lon / 8.0)[None, :]) % 2).astype(np.int32)
    idx = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    noise = xorshift32(xorshift32(idx ^ np.uint32(seed)) + np.uint32(0x9E3779B9))
    n = (noise & np.uint32(63)).astype(np.int32) - 32
    base_a = np.array([200, 170, 90], dtype=np.int32)
    base_b = np.array([30, 60, 140], dtype=np.int32)
    rgb = np.where(cell[..., None] == 1, base_a, base_b) + n[..., None]
    sky = np.empty((h, w, 4), dtype=np.uint8)
    sky[..., :3] = np.clip(rgb, 0, 255).astype(np.uint8)
    sky[..., 3] = 255
    return sky


def make_disk_texture(size=(512, 64)) -> np.ndarray:
    """(h, w, 4) uint8 disk texture for Context.set_disk: U (columns) is the
    azimuth, V (rows) the radius from r_in to r_out.  A radial gradient (hot
    white-yellow inside to dull red outside) with 16 azimuthal stripes; alpha
    rises from 0 at both rims to 255 (a smooth window), so the rims fade out."""
    w, h = size
    u = (np.arange(w, dtype=np.float64) + 0.5) / w
    v = (np.arange(h, dtype=np.float64) + 0.5) / h
    stripe = 0.75 + 0.25 * np.cos(2.0 * math.pi * 16.0 * u)[None, :]
    t = v[:, None]
    rgb = np.stack([255.0 * (1.0 - 0.25 * t) * stripe, 230.0 * (1.0 - 0.7 * t) * stripe,
                    160.0 * (1.0 - t) ** 2 * stripe], axis=-1)
    tr = (np.arange(h, dtype=np.float64) / max(h - 1, 1))[:, None]  # 0 and 1 on the rim rows (V clamps to them)
    alpha = np.clip(np.minimum(tr, 1.0 - tr) * 8.0, 0.0, 1.0) * np.ones((1, w))
    tex = np.empty((h, w, 4), dtype=np.uint8)
    tex[..., :3] = np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
    tex[..., 3] = np.clip(np.rint(255.0 * alpha), 0, 255).astype(np.uint8)
    return tex


def _lobe(lam: np.ndarray, mu: float, s1: float, s2: float) -> np.ndarray:
    t = (lam - mu) / np.where(lam < mu, s1, s2)
    return np.exp(-0.5 * t * t)


def blackbody_xyz(temps) -> np.ndarray:
    """(..., 3) f64 CIE 1931 XYZ (arbitrary common scale) of Planckian radiators
    at `temps` kelvin: Planck's law over 360..830 nm in 1 nm steps, weighted by
    the multi-lobe Gaussian fit to the CIE 1931 standard observer."""
    T = np.asarray(temps, dtype=np.float64)[..., None]
    lam = np.arange(360.0, 831.0, 1.0)
    xb = 1.056 * _lobe(lam, 599.8, 37.9, 31.0) + 0.362 * _lobe(lam, 442.0, 16.0, 26.7) \
        - 0.065 * _lobe(lam, 501.1, 20.4, 26.2)
    yb = 0.821 * _lobe(lam, 568.8, 46.9, 40.5) + 0.286 * _lobe(lam, 530.9, 16.3, 31.1)
    zb = 1.217 * _lobe(lam, 437.0, 11.8, 36.0) + 0.681 * _lobe(lam, 459.0, 26.0, 13.8)
    c2 = 1.438776877e7  # h c / k_B in nm K
    # (the spectral radiance up to a constant factor; the ramp is normalised)
    planck = (lam / 560.0) ** -5 / np.expm1(c2 / (lam * T))
    return np.stack([(planck * xb).sum(axis=-1), (planck * yb).sum(axis=-1), (planck * zb).sum(axis=-1)], axis=-1)


def blackbody_ramp(n: int, t_lo: float, t_hi: float) -> np.ndarray:
    """(n, 4) uint8 colour ramp for Context.set_disk_emission: entry i is the
    colour of a Planckian radiator at 1/T = 1/t_lo - i/(n-1) (1/t_lo - 1/t_hi)
    (evenly spaced in 1/T), its XYZ (blackbody_xyz) taken to linear sRGB,
    negatives clipped, divided by its largest channel (the brightness comes from
    the renderer's T^4 factor) and encoded with the sRGB transfer curve; alpha 255."""
    if not (2 <= n <= 1024) or not (0.0 < t_lo < t_hi) or not math.isfinite(t_hi):
        raise ValueError("blackbody_ramp needs 2 <= n <= 1024 and 0 < t_lo < t_hi")
    inv = 1.0 / t_lo - np.arange(n, dtype=np.float64) / (n - 1) * (1.0 / t_lo - 1.0 / t_hi)
    xyz = blackbody_xyz(1.0 / inv)
    m = np.array([[3.2406, -1.5372, -0.4986], [-0.9689, 1.8758, 0.0415], [0.0557, -0.2040, 1.0570]])
    rgb = np.clip(xyz @ m.T, 0.0, None)
    rgb = rgb / rgb.max(axis=-1, keepdims=True)
    enc = np.where(rgb <= 0.0031308, 12.92 * rgb, 1.055 * np.power(rgb, 1.0 / 2.4) - 0.055)
    ramp = np.empty((n, 4), dtype=np.uint8)
    ramp[:, :3] = np.clip(np.rint(255.0 * enc), 0, 255).astype(np.uint8)
    ramp[:, 3] = 255
    return ramp
