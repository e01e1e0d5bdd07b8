"""The global map: the device object (glio_gmap_*, csrc/globalmap_kernels.hip: the live part of mapVisualizationThread, Estimator.cpp:5315-5350, and the same
computation of publishCompleteMap, :5275-5313 -- every mapping_interval-th keyframe's surf cloud moved to the world at its final pose, the concatenation through ONE
pcl::VoxelGrid at 0.2 m) and the host's share: which keyframes enter the map (:5339).  The poses are loop.frame_poses (:5287-5288).  `glio::GlobalMap` and
`glio::globalMapFrames` (host/glio_map_backend.hpp) are the C++ twins.  Writing the .pcd stays with the caller.  There is no CPU fallback.

DenseClouds is the store of full_clouds_ds (glio_dense_*, csrc/dense_cloud_kernels.hip, include/glio_dense.h): per keyframe the FULL cloud, de-skewed and filtered
at 0.4 m; GlobalMap(dense) is publishCompleteMap over it -- the dense map.  `glio::DenseClouds` is the C++ twin."""
import ctypes as C

import numpy as np

from . import capi
from . import ctypes_types as T


def default_opts(**kw):
    """glio_gmap_opts: leaf 0.2 (Estimator.cpp:856) and the default capacities; keyword arguments override fields"""
    lib = capi.load()
    lib.glio_gmap_opts_default.restype = None
    o = T.GlioGmapOpts()
    lib.glio_gmap_opts_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def global_map_frames(n_keyframes, mapping_interval):
    """Estimator.cpp:5339: for (i = 0; i < n; i += mapping_interval)"""
    return list(range(0, int(n_keyframes), int(mapping_interval)))


class MapInfo:
    def __init__(self, r):
        self.n_points_total, self.n_voxels, self.radix_passes, self.pcl_index_overflow = int(r.n_points_total), int(r.n_voxels), int(r.radix_passes), bool(r.pcl_index_overflow)

    def as_dict(self):
        return dict(n_points_total=self.n_points_total, n_voxels=self.n_voxels, radix_passes=self.radix_passes, pcl_index_overflow=self.pcl_index_overflow)


class DenseClouds:
    """One glio_dense: K frames of up to max_points_per_frame points, each pcl::VoxelGrid(leaf) of undistortion(cloud, trans, quat) -- the bytes
    capi.Context.set_scan_filtered puts into a window slot -- on a stream of its own."""

    def __init__(self, K, max_points_per_frame, max_input_points, device=0):
        lib = capi.load()
        self.K, self.cap, self.max_in = int(K), int(max_points_per_frame), int(max_input_points)
        self._h = C.c_void_p()
        capi._check(lib.glio_dense_create(int(device), self.K, self.cap, self.max_in, C.byref(self._h)))

    def close(self):
        if self._h:
            capi.load().glio_dense_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_frame(self, k, points, leaf, deskew_trans=None, deskew_quat=None, ioff=None):
        """points: [n][4] float32 (x y z intensity), or records of any stride with the intensity float at byte `ioff`.  Returns the frame's point count; a refusal
        (GlioError with .code and .n_out) leaves the frame as it was."""
        n = C.c_int(0)
        t, q, tp, qp = capi.Context._motion(deskew_trans, deskew_quat)
        pts = np.ascontiguousarray(points)
        if ioff is None:
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
            stride, ioff = 16, 12
        else:
            stride = pts.dtype.itemsize if pts.ndim == 1 else pts.dtype.itemsize * pts.shape[1]
        ptr = pts.ctypes.data_as(C.c_void_p) if len(pts) else None
        rc = capi.load().glio_dense_set_frame_strided(self._h, int(k), ptr, len(pts), stride, int(ioff), float(leaf), tp, qp, C.byref(n))
        return capi.Context._check_count(rc, n)

    def set_frame_from_features(self, k, frontend, leaf, deskew_trans=None, deskew_quat=None):
        """the same from the CUT cloud of `frontend`'s (a capi.Context) last features_extract, read where it lies on the device"""
        n = C.c_int(0)
        t, q, tp, qp = capi.Context._motion(deskew_trans, deskew_quat)
        rc = capi.load().glio_dense_set_frame_from_features(self._h, int(k), frontend._h, float(leaf), tp, qp, C.byref(n))
        return capi.Context._check_count(rc, n)

    def frame_count(self, k):
        n = C.c_int(0)
        capi._check(capi.load().glio_dense_frame_count(self._h, int(k), C.byref(n)))
        return n.value

    def read_frame(self, k):
        """frame k: [n][4] float32"""
        n = self.frame_count(k)
        out = np.zeros((max(n, 1), 4), np.float32)
        m = C.c_int(0)
        capi._check(capi.load().glio_dense_read_frame(self._h, int(k), T.fptr(out), n, C.byref(m)))
        return out[:m.value].copy()

    def world_cloud(self, pose):
        """pub_full_cloud_map: the last set_frame*'s de-skewed, unfiltered cloud moved by transformCloud at pose = t[3], q[4] (w first): [n][4] float32"""
        pose = np.ascontiguousarray(pose, np.float64).reshape(7)
        n = C.c_int(0)
        capi._check(capi.load().glio_dense_world_cloud(self._h, T.dptr(pose), None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        capi._check(capi.load().glio_dense_world_cloud(self._h, T.dptr(pose), T.fptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def last_device_ms(self):
        """device ms of the last non-empty set_frame*: (de-skew + box, VoxelGrid, copy into the store); needs GLIO_DENSE_TIMING=1 at creation"""
        ms = np.zeros(3, np.float32)
        capi._check(capi.load().glio_dense_last_device_ms(self._h, T.fptr(ms)))
        return [float(x) for x in ms]


class GlobalMap:
    """One glio_gmap on a batch.BatchAssociation (which owns the resident keyframe clouds), or on a DenseClouds (whose frames it then reads: the dense map), or on a
    static_map.StaticClouds (the frames without the points that were seen through: the static map)."""

    def __init__(self, assoc, opts=None):
        lib = capi.load()
        lib.glio_gmap_destroy.restype = None
        self.opts = default_opts() if opts is None else opts
        self._assoc = assoc             # (the association / dense store must outlive the map object)
        self._h = C.c_void_p()
        from .static_map import StaticClouds
        if isinstance(assoc, StaticClouds):
            capi._check(lib.glio_gmap_create_on_static(assoc._h, C.byref(self.opts), C.byref(self._h)))
        elif isinstance(assoc, DenseClouds):
            capi._check(lib.glio_gmap_create_on_dense(assoc._h, C.byref(self.opts), C.byref(self._h)))
        else:
            capi._check(lib.glio_gmap_create(assoc._h, C.byref(self.opts), C.byref(self._h)))

    def close(self):
        if self._h:
            capi.load().glio_gmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, frames, poses):
        """frames: resident keyframe indices in list order (repeats allowed); poses [n][7] = t, q (loop.frame_poses).  The clouds go behind everything added
        since the last clear; returns MapInfo.  A refusal (GlioError, code -1) leaves the map exactly as it was."""
        frames = np.ascontiguousarray(frames, np.int32)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        assert len(poses) == len(frames)
        info = T.GlioGmapInfo()
        capi._check(capi.load().glio_gmap_add_frames(self._h, len(frames), T.iptr(frames) if len(frames) else None, T.dptr(poses) if len(frames) else None, C.byref(info)))
        return MapInfo(info)

    def clear(self):
        capi._check(capi.load().glio_gmap_clear(self._h))

    def size(self):
        n = C.c_int(0)
        capi._check(capi.load().glio_gmap_size(self._h, C.byref(n)))
        return n.value

    def read(self, first=0, n=None):
        """voxels [first, first + n) of the map (all of it by default), [n][4] float32"""
        n = self.size() - int(first) if n is None else int(n)
        out = np.zeros((max(n, 0), 4), np.float32)
        capi._check(capi.load().glio_gmap_read(self._h, int(first), n, T.fptr(out) if n > 0 else None))
        return out

    def points_dev(self):
        """(device address of the map's [n][4] float32 array, n): valid until the next successful add"""
        p, n = C.c_void_p(), C.c_int(0)
        capi._check(capi.load().glio_gmap_points_dev(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def last_device_ms(self):
        ms = C.c_float(0)
        capi._check(capi.load().glio_gmap_last_device_ms(self._h, C.byref(ms)))
        return ms.value

    def last_stage_ms(self):
        """transform, sort, runs + sums, merge of the last add"""
        ms = (C.c_float * 4)()
        capi._check(capi.load().glio_gmap_last_stage_ms(self._h, ms))
        return [float(x) for x in ms]
