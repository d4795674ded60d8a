"""Shared cases of the frame-sequence tests (test_sequence_cpu.py, test_gpu_sequence.py,
gpu_sequence_worker.py): the frames, the parent emitter, and the direction batch."""
import numpy as np

from helpers import hemisphere_wo, sun_cone_wo

# five frames: elevations 2, 20, 45, 89.9 degrees and one 5 degrees below the horizon, each
# with its own azimuth, turbidity and weight (non-uniform, one 0)
ELEVATIONS = [2.0, 20.0, 45.0, 89.9, -5.0]
AZIMUTHS = [10.0, 100.0, 200.0, 300.0, 40.0]
TURBIDITY = [1.0, 2.5, 6.0, 10.0, 3.0]
WEIGHTS = [0.5, 2.0, 0.0, 1.25, 3.0]
LAMBDAS = [400.0, 550.0, 700.0, 720.0, 300.0]   # 300 nm is outside the model: plane of zeros
SEED = 20
# one day's hourly suns (night hours included), non-uniform weights with one 0
DAY_TIMES = [(2010, 7, 10, float(h)) for h in range(24)]
DAY_TURBIDITY = [1.0 + 9.0 * ((7 * h) % 24) / 23.0 for h in range(24)]
DAY_WEIGHTS = [0.0 if h == 13 else 0.25 + 0.125 * ((5 * h) % 24) for h in range(24)]


def rotation(axis=(0.3, -0.5, 0.8), angle=0.7):
    """4x4 rotation about `axis` (Rodrigues)."""
    k = np.asarray(axis, np.float64)
    k /= np.linalg.norm(k)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    r = np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * (kx @ kx)
    m = np.eye(4)
    m[:3, :3] = r
    return m.astype(np.float32)


def to_world_dirs(local, to_world):
    """Rows of `local` (n, 3) through the linear part of to_world, fp32."""
    if to_world is None:
        return np.asarray(local, np.float32)
    return (np.asarray(local, np.float64) @ np.asarray(to_world, np.float64)[:3, :3].T).astype(np.float32)


def frame_dirs(to_world=None):
    """World-space frame directions whose LOCAL elevations are ELEVATIONS (to_world applied)."""
    e, a = np.deg2rad(ELEVATIONS), np.deg2rad(AZIMUTHS)
    return to_world_dirs(np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], 1), to_world)


def base_dict(**kw):
    d = {"type": "sunsky", "turbidity": 4.0, "albedo": 0.25, "sky_scale": 0.8, "sun_scale": 1.1,
         "sun_direction": [0.0, 0.6, 0.8]}
    d.update(kw)
    return d


def frame_dict(base, sun_dir, turbidity):
    """The single emitter a frame stands for: the parent with that sun direction and turbidity."""
    return dict(base, sun_direction=[float(x) for x in sun_dir], turbidity=float(turbidity))


def batch_wo(local_suns, half_aperture, seed=SEED, n_sky=8192 + 37):
    """Local-frame directions of the GPU checks, in a fixed shuffled order (so every prefix holds
    all three kinds): n_sky uniform over the upper hemisphere, per frame 64 strictly inside
    that frame's disc (0.9 of the half aperture), 16 below the horizon.  n is odd, n % 4 != 0."""
    parts = [hemisphere_wo(n_sky, seed)]
    for k, s in enumerate(local_suns):
        parts.append(sun_cone_wo(64, s, half_aperture, seed=seed + 1 + k, scale=0.9))
    low = hemisphere_wo(16, seed + 1000)
    low[:, 2] = -np.maximum(low[:, 2], 1e-3)
    parts.append(low)
    wo = np.concatenate(parts).astype(np.float32)
    n = wo.shape[0]
    assert n % 2 == 1 and n % 4 != 0, n
    return wo[np.random.default_rng(seed + 2000).permutation(n)]
