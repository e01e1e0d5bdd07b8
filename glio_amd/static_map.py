"""The static map: the device object (glio_static_*, include/glio_static.h, csrc/static_kernels.hip: range images of the resident frames, the visibility
votes of every point against its views, the frames without the points that were seen through) and the host's share -- which frames view which
(static_views).  mapping.GlobalMap(static) is the map of rows k / p over the static store.  `glio::StaticClouds` and `glio::staticViews`
(host/glio_static_backend.hpp) are the C++ twins: the same scalar arithmetic in the same order.  There is no CPU fallback for the classification."""
import ctypes as C

import numpy as np

from . import capi
from . import ctypes_types as T

MAX_VIEWS = T.STATIC_MAX_VIEWS
PATH_AUTO, PATH_GLOBAL = T.STATIC_PATH_AUTO, T.STATIC_PATH_GLOBAL
MIN_BASELINE = 0.5                      # m: a stationary vehicle gives no parallax

default_opts = capi.static_opts


def static_views(poses, half_window, min_baseline=MIN_BASELINE):
    """The usual choice of views: for frame f of poses [n][7] (t, q) the nearest frames in list order on both sides -- up to half_window earlier ones (nearest
    first), then up to half_window later ones (nearest first) -- whose position differs from f's by at least min_baseline (squared distances compared in
    double).  Returns (view_offsets [n + 1] int32, views int32) as StaticClouds.classify takes them."""
    p = np.asarray(poses, np.float64).reshape(-1, 7)
    n, hw, b2 = len(p), int(half_window), float(min_baseline) * float(min_baseline)
    off, views = [0], []
    for f in range(n):
        for step in (-1, 1):
            taken, j = 0, f + step
            while 0 <= j < n and taken < hw:
                dx, dy, dz = float(p[j, 0]) - float(p[f, 0]), float(p[j, 1]) - float(p[f, 1]), float(p[j, 2]) - float(p[f, 2])
                if (dx * dx + dy * dy) + dz * dz >= b2:
                    views.append(j)
                    taken += 1
                j += step
        off.append(len(views))
    return np.array(off, np.int32), np.array(views, np.int32)


class StaticInfo:
    def __init__(self, r):
        self.n_points, self.n_tested, self.n_dynamic, self.n_frames, self.lds_path = int(r.n_points), int(r.n_tested), int(r.n_dynamic), int(r.n_frames), bool(r.lds_path)

    def as_dict(self):
        return dict(n_points=self.n_points, n_tested=self.n_tested, n_dynamic=self.n_dynamic, n_frames=self.n_frames, lds_path=self.lds_path)


class StaticClouds:
    """One glio_static on a batch.BatchAssociation or a mapping.DenseClouds (which owns the resident clouds and must outlive this object).  Static frame k is
    the owner's frame k without its dynamic points."""

    def __init__(self, owner, opts=None, **kw):
        from .mapping import DenseClouds
        lib = capi.load()
        self.opts = default_opts(**kw) if opts is None else opts
        self.rows, self.cols = int(self.opts.rows), 4 * int(self.opts.cols_per_quadrant)
        self._owner = owner
        self._h = C.c_void_p()
        create = lib.glio_static_create_on_dense if isinstance(owner, DenseClouds) else lib.glio_static_create
        capi._check(create(owner._h, C.byref(self.opts), C.byref(self._h)))

    def close(self):
        if self._h:
            capi.load().glio_static_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def classify(self, frames, poses, view_offsets, views):
        """rules 1 - 6 of glio_static.h for the owner's frames `frames` at poses [n][7] (t, q) with the ragged view list; returns StaticInfo.  A refusal
        (GlioError) leaves the store, the counts and the votes exactly as they were."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        off, views = np.ascontiguousarray(view_offsets, np.int32).reshape(-1), np.ascontiguousarray(views, np.int32).reshape(-1)
        assert len(poses) == len(frames) and len(off) == len(frames) + 1
        info = T.GlioStaticInfo()
        n = len(frames)
        capi._check(capi.load().glio_static_classify(self._h, n, T.iptr(frames) if n else None, T.dptr(poses) if n else None, T.iptr(off),
                                                     T.iptr(views) if len(views) else None, C.byref(info)))
        return StaticInfo(info)

    def frame_count(self, k):
        n = C.c_int(0)
        capi._check(capi.load().glio_static_frame_count(self._h, int(k), C.byref(n)))
        return n.value

    def read_frame(self, k):
        """static frame k: [n][4] float32"""
        n = self.frame_count(k)
        out = np.zeros((max(n, 1), 4), np.float32)
        m = C.c_int(0)
        capi._check(capi.load().glio_static_read_frame(self._h, int(k), T.fptr(out), n, C.byref(m)))
        return out[:m.value].copy()

    def read_votes(self, k):
        """(through, tested) uint8 per point of the owner's frame k as its last classification saw it"""
        n = C.c_int(0)
        capi._check(capi.load().glio_static_read_votes(self._h, int(k), None, None, 0, C.byref(n)))
        th, te = np.zeros(max(n.value, 1), np.uint8), np.zeros(max(n.value, 1), np.uint8)
        capi._check(capi.load().glio_static_read_votes(self._h, int(k), th.ctypes.data_as(T.c_uint8_p), te.ctypes.data_as(T.c_uint8_p), n.value, C.byref(n)))
        return th[:n.value].copy(), te[:n.value].copy()

    def read_image(self, view):
        """(raw, floor) [rows][cols] float32 of the last call's call-local frame `view`"""
        raw, fl = np.zeros((self.rows, self.cols), np.float32), np.zeros((self.rows, self.cols), np.float32)
        capi._check(capi.load().glio_static_read_image(self._h, int(view), T.fptr(raw), T.fptr(fl)))
        return raw, fl

    def last_device_ms(self):
        """images, floor, votes, compaction of the last call, ms"""
        ms = np.zeros(4, np.float32)
        capi._check(capi.load().glio_static_last_device_ms(self._h, T.fptr(ms)))
        return [float(x) for x in ms]
