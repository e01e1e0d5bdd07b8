"""Synthetic spinning-LiDAR scans over synth.make_scene's rectangles: test data for the feature extraction (glio_features_*).

N lasers fire per azimuth step, column-major as Velodyne drivers emit them, over one full clockwise turn (the reference's orientation
-atan2(y, x) grows) from an arbitrary start azimuth; ~1 cm range noise; misses as NaN; a few returns inside 3 m; an optional yaw of the
sensor during the sweep (so that qIMU matters); records of 16 or 32 bytes or any multiple of 4.

Elevation tables: `centred` puts every laser in the middle of the reference formula's ring bin (parity data); `hdl32` is the nominal
HDL-32E table (-30.67 deg upwards in 4/3 deg steps), which sits ON the 32-line formula's bin edges (Preprocessing.cpp:443).
"""
import numpy as np

from . import synth


def elevations(n_scans, table="centred"):
    """laser elevation angles in degrees, in firing order"""
    if table == "hdl32":
        assert n_scans == 32
        return -30.67 + np.arange(32) * (4.0 / 3.0)
    if n_scans == 16:                                   # scanID = int((angle + 15) / 2 + 0.5)
        return -15.0 + 2.0 * np.arange(16)
    if n_scans == 32:                                   # scanID = int((angle + 92/3) * 3/4)
        return (np.arange(32) + 0.5) * (4.0 / 3.0) - 92.0 / 3.0
    if n_scans == 64:                                   # 0..32: int((2 - angle) * 3 + 0.5); 33..50: 32 + int((-8.83 - angle) * 2 + 0.5); > 50 rejected
        up = 2.0 - np.arange(33) / 3.0
        low = -8.83 - (np.arange(33, 51) - 32) / 2.0
        rejected = -24.9 - 0.5 * np.arange(13)
        return np.concatenate([up, low, rejected])
    raise ValueError(n_scans)


def _cast(scene, o, d):
    """ranges of rays o + t d (d unit, [m][3]) against the scene's rectangles; inf where nothing is hit"""
    n = np.cross(scene.u, scene.v)                                        # [P][3]
    den = d @ n.T                                                         # [m][P]
    num = ((scene.c - o) * n).sum(1)                                      # [P]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = num[None, :] / den
    t[~np.isfinite(t) | (t <= 1e-6)] = np.inf
    best = np.full(len(d), np.inf)
    for p in range(len(scene.c)):
        tp = t[:, p]
        ok = np.isfinite(tp)
        if not ok.any():
            continue
        h = o + tp[ok, None] * d[ok]
        rel = h - scene.c[p]
        a = rel @ scene.u[p] / (scene.u[p] @ scene.u[p])
        b = rel @ scene.v[p] / (scene.v[p] @ scene.v[p])
        inside = (np.abs(a) <= 1.0) & (np.abs(b) <= 1.0)
        idx = np.nonzero(ok)[0][inside]
        best[idx] = np.minimum(best[idx], tp[idx])
    return best


def make_scan(n_scans=32, n_az=1800, table="centred", origin=(60.0, 1.0, 1.8), start_az=0.7, sweep_yaw=0.0, noise=0.01,
              close_frac=0.002, scene=None, seed=3, max_range=120.0):
    """One turn.  Returns [n_az * lasers][4] float32 (x y z intensity) in the sensor frame at the firing time of each point, column-major.
    sweep_yaw: the sensor's yaw over the turn (rad), the turn's start being the sensor frame of the scan."""
    rng = np.random.default_rng(seed)
    scene = scene if scene is not None else synth.make_scene(seed=synth.SEED_BASE)
    el = np.radians(elevations(n_scans, table))
    L = len(el)
    k = np.repeat(np.arange(n_az), L)
    az = start_az - 2.0 * np.pi * k / n_az                               # clockwise: -atan2(y, x) grows
    e = np.tile(el, n_az)
    ds = np.stack([np.cos(e) * np.cos(az), np.cos(e) * np.sin(az), np.sin(e)], 1)      # sensor-frame directions
    yaw = sweep_yaw * k / n_az
    c, s = np.cos(yaw), np.sin(yaw)
    dw = np.stack([c * ds[:, 0] - s * ds[:, 1], s * ds[:, 0] + c * ds[:, 1], ds[:, 2]], 1)
    r = _cast(scene, np.asarray(origin, float), dw)
    r = r + noise * rng.standard_normal(len(r))
    close = rng.random(len(r)) < close_frac
    r[close] = rng.uniform(0.5, 2.9, close.sum())
    miss = ~np.isfinite(r) | (r > max_range)
    pts = (ds * r[:, None]).astype(np.float32)
    pts[miss] = np.nan
    out = np.zeros((len(r), 4), np.float32)
    out[:, :3] = pts
    out[:, 3] = rng.uniform(0, 255, len(r)).astype(np.float32)          # reflectivity (the extraction ignores it)
    return out


def to_records(xyzi, stride=16, ioff=12, seed=7):
    """[n][4] float32 -> records of `stride` bytes (x y z floats at 0, intensity at ioff; padding filled with garbage on purpose)"""
    xyzi = np.asarray(xyzi, np.float32)
    if stride == 16 and ioff == 12:
        return np.ascontiguousarray(xyzi)
    assert stride % 4 == 0 and stride >= 16 and ioff % 4 == 0 and 12 <= ioff <= stride - 4
    dt = np.dtype({"names": ["x", "y", "z", "intensity"], "formats": ["<f4"] * 4, "offsets": [0, 4, 8, ioff], "itemsize": stride})
    out = np.frombuffer(np.random.default_rng(seed).integers(0, 255, len(xyzi) * stride, dtype=np.uint8).tobytes(), dtype=dt).copy()
    out["x"], out["y"], out["z"], out["intensity"] = xyzi[:, 0], xyzi[:, 1], xyzi[:, 2], xyzi[:, 3]
    return out


def drive(n_frames=8, n_scans=16, n_az=900, step=(0.6, 0.05, 0.0), yaw_step=0.01, seed=11, **kw):
    """A short drive down the corridor: scan k from origin0 + k * step with a yaw of k * yaw_step (the scan rotated into the sensor frame)."""
    scene = synth.make_scene(seed=synth.SEED_BASE)
    out = []
    for f in range(n_frames):
        o = np.array([40.0, 0.5, 1.8]) + f * np.asarray(step)
        out.append(make_scan(n_scans, n_az, origin=o, start_az=0.3 + f * yaw_step, scene=scene, seed=seed + f, **kw))
    return out
