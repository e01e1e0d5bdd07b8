"""The global map: the device object (glio_gmap_*, csrc/globalmap_kernels.hip: the live part of mapVisualizationThread, Estimator.cpp:5315-5350, and the same
computation of publishCompleteMap, :5275-5313 -- every mapping_interval-th keyframe's surf cloud moved to the world at its final pose, the concatenation through ONE
pcl::VoxelGrid at 0.2 m) and the host's share: which keyframes enter the map (:5339).  The poses are loop.frame_poses (:5287-5288).  `glio::GlobalMap` and
`glio::globalMapFrames` (host/glio_map_backend.hpp) are the C++ twins.  Writing the .pcd stays with the caller.  There is no CPU fallback."""
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


class GlobalMap:
    """One glio_gmap on a batch.BatchAssociation (which owns the resident keyframe clouds)."""

    def __init__(self, assoc, opts=None):
        lib = capi.load()
        lib.glio_gmap_destroy.restype = None
        self.opts = default_opts() if opts is None else opts
        self._assoc = assoc             # (the association must outlive the map object)
        self._h = C.c_void_p()
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
