"""ctypes binding of libglio_hip.so (include/glio_hip.h) and the host-side mirror of the reference's
sliding-window call sequence.  There is no CPU fallback: if the library or a HIP device is missing,
construction raises."""
import ctypes as C
import os

import numpy as np

from . import ctypes_types as T
from . import synth

_LIB = None
LIB_PATH = os.environ.get("GLIO_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libglio_hip.so")

(KERNEL_LIDAR_LINEARIZE, KERNEL_FULL_LINEARIZE, KERNEL_TR_STEP, KERNEL_ASSOCIATE, KERNEL_MAP_BUILD, KERNEL_MARGINALIZE, KERNEL_STREAM_READ,
 KERNEL_LINEARIZE_ALL, KERNEL_TR_STEP_STEADY) = range(9)
LIDAR_F64, LIDAR_F32_MFMA = 0, 1


class GlioError(RuntimeError):
    """code: the GLIO_E_* value where the raiser knows it; n_out: the output count a refused keyframe-cloud call still reports"""
    code = None
    n_out = None


E_ARG, E_HIP, E_STATE = -1, -2, -3
E_NUMERIC = -4


class GlioCovInfo(C.Structure):
    """glio_cov_info (include/glio_cov.h)"""
    _fields_ = [("n", C.c_int32), ("n_free", C.c_int32), ("n_free_asked", C.c_int32), ("bad_pivot", C.c_int32),
                ("min_pivot", C.c_double), ("max_pivot", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GlioError(f"{LIB_PATH} is missing: build it with `python -m glio_amd.build` (hipcc, gfx950). "
                            "There is no CPU fallback for the GLIO hot path.")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 under the same SONAME as /opt/rocm's.
        # Whichever is loaded first serves both; torch cannot start on the system one ("No HIP GPUs are available"), so
        # when torch is installed it goes first.  (A C++ caller without torch simply uses /opt/rocm's.)
        if os.environ.get("GLIO_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = C.CDLL(LIB_PATH)
        lib.glio_last_error.restype = C.c_char_p
        lib.glio_destroy.restype = None
        lib.glio_opts_default.restype = None
        T.apply_prototypes(lib)
        _LIB = lib
    return _LIB


def _check(rc):
    if rc != 0:
        raise GlioError(f"libglio_hip error {rc}: {load().glio_last_error().decode()}")


def align_opts(**kw):
    """glio_align_opts_default with fields replaced; `thresholds` (a sequence) also sets n_rounds"""
    o = T.GlioAlignOpts()
    load().glio_align_opts_default(C.byref(o))
    th = kw.pop("thresholds", None)
    if th is not None:
        th = [float(x) for x in th]
        o.n_rounds = len(th)
        for k in range(min(len(th), T.ALIGN_MAX_ROUNDS)):
            o.thresholds[k] = th[k]
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def place_opts(**kw):
    """glio_place_opts_default with fields replaced"""
    o = T.GlioPlaceOpts()
    load().glio_place_opts_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def place_tables(max_radius):
    """glio_place_tables: (rb2 [21], dir [60][2]) float32; needs no device"""
    rb2, dirs = np.zeros(T.PLACE_RINGS + 1, np.float32), np.zeros((T.PLACE_SECTORS, 2), np.float32)
    _check(load().glio_place_tables(float(max_radius), T.fptr(rb2), T.fptr(dirs)))
    return rb2, dirs


def static_opts(**kw):
    """glio_static_opts_default with fields replaced"""
    o = T.GlioStaticOpts()
    load().glio_static_opts_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def static_tables(opts):
    """glio_static_tables: (s2 [rows + 1], dir [4 cols_per_quadrant][2]) float32; needs no device"""
    s2, dirs = np.zeros(max(opts.rows, 0) + 1, np.float32), np.zeros((4 * max(opts.cols_per_quadrant, 1), 2), np.float32)
    _check(load().glio_static_tables(C.byref(opts), T.fptr(s2), T.fptr(dirs)))
    return s2, dirs


def static_relative_pose(pose_v, pose_f):
    """glio_static_relative_pose: T(v, f) = pose_v^-1 o pose_f as a float32 [3][4]; poses are t[3], q[4] (w first); needs no device"""
    pv, pf = np.ascontiguousarray(pose_v, np.float64).reshape(7), np.ascontiguousarray(pose_f, np.float64).reshape(7)
    out = np.zeros((3, 4), np.float32)
    _check(load().glio_static_relative_pose(T.dptr(pv), T.dptr(pf), T.fptr(out)))
    return out


def device_count():
    return load().glio_device_count()


def switches():
    """The library's environment switches (csrc/glio_switches.h; INTEGRATION.md, "Environment switches") as a list of dicts: name, default, scope
    ("PROCESS": the process's snapshot, taken by the first query; "CREATE": read when an object is created), value (what the library works with now), doc."""
    lib, out = load(), []
    name, doc, dflt, scope, value = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
    while lib.glio_debug_switch_row(len(out), C.byref(name), C.byref(dflt), C.byref(scope), C.byref(doc)) == 0:
        _check(lib.glio_debug_switch_value(name.value, C.byref(value)))
        out.append({"name": name.value.decode(), "default": dflt.value, "scope": ("PROCESS", "CREATE")[scope.value], "value": value.value, "doc": doc.value.decode()})
    return out


# pcl::PointXYZI as numpy sees it (GLIO/include/utils/common.h: PointType): 32-byte records, x y z at 0, intensity at byte 16
PCL_XYZI = np.dtype({"names": ["x", "y", "z", "intensity"], "formats": ["<f4", "<f4", "<f4", "<f4"], "offsets": [0, 4, 8, 16], "itemsize": 32})
PCL_XYZI_INTENSITY_OFFSET = 16


def to_pcl_xyzi(xyzi):
    """[n][4] float32 -> the 32-byte records a pcl::PointCloud<pcl::PointXYZI> holds (padding filled with garbage on purpose: it must not matter)"""
    xyzi = np.asarray(xyzi, np.float32)
    out = np.frombuffer(np.random.default_rng(7).integers(0, 255, len(xyzi) * 32, dtype=np.uint8).tobytes(), dtype=PCL_XYZI).copy()
    out["x"], out["y"], out["z"], out["intensity"] = xyzi[:, 0], xyzi[:, 1], xyzi[:, 2], xyzi[:, 3]
    return out


class Context:
    """One glio_ctx = the device-resident state of one sliding window (one HIP stream)."""

    def __init__(self, opts, device=0):
        lib = load()
        if lib.glio_device_count() < 1:
            raise GlioError("no HIP device visible: libglio_hip has no CPU fallback")
        self.opts = opts
        self.W = opts.window
        self._h = C.c_void_p()
        _check(lib.glio_create(device, C.byref(opts), C.byref(self._h)))
        self._keep = []

    def close(self):
        if self._h:
            load().glio_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- uploads
    def set_map(self, map_pts):
        _check(load().glio_set_map(self._h, T.fptr(map_pts), len(map_pts)))

    # ---- LiDAR features from the raw scan (Preprocessing::cloudHandler on the device; glio_features_*)
    def features_config(self, opts=None):
        if opts is None:
            from . import features
            opts = features.default_opts()
        _check(load().glio_features_config(self._h, C.byref(opts)))
        self.feat_opts = opts

    def features_extract(self, raw, q_imu, ioff=12):
        """raw: [n][4] float32 (x y z intensity) or records of any stride (x y z floats at 0, the intensity float at ioff).  Returns glio_feat_counts."""
        pts, ptr, n, stride = self._raw(raw)
        if pts.dtype == np.float32 and pts.ndim == 2:
            stride = 4 * pts.shape[1]
        q = np.ascontiguousarray(q_imu, np.float64)
        cnt = T.GlioFeatCounts()
        _check(load().glio_features_extract_strided(self._h, ptr if n else None, n, stride, ioff, T.dptr(q), C.byref(cnt)))
        return cnt

    def features_read(self, which):
        n = C.c_int(0)
        _check(load().glio_features_read(self._h, int(which), None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        _check(load().glio_features_read(self._h, int(which), T.fptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def features_to_scan(self, slot, leaf):
        n = C.c_int(0)
        _check(load().glio_features_to_scan(self._h, int(slot), C.c_float(leaf), C.byref(n)))
        return n.value

    def features_last_device_ms(self):
        ms = C.c_float(0)
        _check(load().glio_features_last_device_ms(self._h, C.byref(ms)))
        return ms.value

    # ---- strided point input: clouds as records of `stride` bytes (x y z floats at 0, intensity float at `ioff`); pcl::PointXYZI = PCL_XYZI
    @staticmethod
    def _raw(points):
        pts = np.ascontiguousarray(points)
        return pts, pts.ctypes.data_as(C.c_void_p), len(pts), pts.dtype.itemsize

    def set_map_strided(self, points, ioff):
        pts, ptr, n, stride = self._raw(points)
        _check(load().glio_set_map_strided(self._h, ptr, n, stride, ioff))

    def set_scan_strided(self, slot, points, ioff):
        pts, ptr, n, stride = self._raw(points)
        _check(load().glio_set_scan_strided(self._h, slot, ptr, n, stride, ioff))

    def localmap_push_strided(self, points, ioff, q, t):
        pts, ptr, n, stride = self._raw(points)
        q = np.ascontiguousarray(q, float); t = np.ascontiguousarray(t, float)
        _check(load().glio_localmap_push_strided(self._h, ptr if n else None, n, stride, ioff, T.dptr(q), T.dptr(t)))

    # ---- device-resident local map
    def localmap_config(self, width, leaf, max_points_per_keyframe):
        _check(load().glio_localmap_config(self._h, width, C.c_float(leaf), max_points_per_keyframe))

    def localmap_push(self, cloud, q, t):
        cloud = np.ascontiguousarray(cloud, np.float32)
        q = np.ascontiguousarray(q, float); t = np.ascontiguousarray(t, float)
        _check(load().glio_localmap_push(self._h, T.fptr(cloud) if len(cloud) else None, len(cloud), T.dptr(q), T.dptr(t)))

    def localmap_push_scan(self, scan_slot, lidar_offset, q, t):
        """push the scan that set_scan put into window slot `scan_slot` (no second upload): body point = scan point - lidar_offset (float)"""
        off = np.ascontiguousarray(lidar_offset, np.float32); q = np.ascontiguousarray(q, np.float64); t = np.ascontiguousarray(t, np.float64)
        _check(load().glio_localmap_push_scan(self._h, int(scan_slot), T.fptr(off), T.dptr(q), T.dptr(t)))

    def localmap_set_accumulation(self, mode):
        """0: exact fixed-point voxel sums (default); 1: pcl::VoxelGrid's float sums in concatenation order (bit-identical to the oracle's map)"""
        _check(load().glio_localmap_set_accumulation(self._h, int(mode)))

    def localmap_stats(self):
        """test hook (glio_debug_localmap_stats): [table_cap, nkeys_seen, table rebuilds from the ring, ordered-output path of the last build (0 empty, 1 bitmap
        rank, 2 radix sort), its radix passes, its voxels, builds that wiped the whole bitmap, 0] -- host fields, no synchronisation"""
        out = np.zeros(8, np.int32)
        _check(load().glio_debug_localmap_stats(self._h, T.iptr(out)))
        return [int(x) for x in out]

    def localmap_build(self):
        n = C.c_int()
        _check(load().glio_localmap_build(self._h, C.byref(n)))
        return n.value

    def localmap_rebuild_from_frames(self, assoc, frames, poses):
        """the ring rebuilt from the resident keyframe clouds `frames` (oldest first) of a batch.BatchAssociation at poses [n][7] = t, q (loop.frame_poses):
        buildLocalMapWithLandMark's rebuild branch (Estimator.cpp:3545-3579) + the build; returns the map size"""
        frames = np.ascontiguousarray(frames, np.int32)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        assert len(poses) == len(frames)
        n = C.c_int()
        _check(load().glio_localmap_rebuild_from_frames(self._h, assoc._h, len(frames), T.iptr(frames) if len(frames) else None,
                                                        T.dptr(poses) if len(frames) else None, C.byref(n)))
        return n.value

    def localmap_last_rebuild_device_ms(self):
        """device ms of the last rebuild's own two launches; needs GLIO_LM_REBUILD_TIMING=1 in the environment when the ring is first rebuilt"""
        ms = C.c_float(0)
        _check(load().glio_localmap_last_rebuild_device_ms(self._h, C.byref(ms)))
        return ms.value

    def localmap_read(self):
        n = C.c_int()
        _check(load().glio_localmap_read(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        _check(load().glio_localmap_read(self._h, T.fptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def set_scan(self, slot, scan):
        _check(load().glio_set_scan(self._h, slot, T.fptr(scan), len(scan)))

    def localmap_push_scan_ahead_and_build(self, lidar_offset, q, t):
        """behind set_scan_ahead: the next call's local map (the cloud just sent, at the new keyframe's pose) on the upload stream; returns the map size"""
        off = np.ascontiguousarray(lidar_offset, np.float32); q = np.ascontiguousarray(q, float); t = np.ascontiguousarray(t, float)
        n = C.c_int()
        _check(load().glio_localmap_push_scan_ahead_and_build(self._h, T.fptr(off), T.dptr(q), T.dptr(t), C.byref(n)))
        return n.value

    # ---- the keyframe cloud: de-skew + pcl::VoxelGrid + set_scan on the device (glio_scan_filter_config, glio_set_scan_filtered*, glio_set_scan_from_features*)
    def scan_filter_config(self, max_input_points):
        _check(load().glio_scan_filter_config(self._h, int(max_input_points)))

    @staticmethod
    def _motion(deskew_trans, deskew_quat):
        t = None if deskew_trans is None else np.ascontiguousarray(deskew_trans, np.float64).reshape(3)
        q = None if deskew_quat is None else np.ascontiguousarray(deskew_quat, np.float64).reshape(4)
        return t, q, (None if t is None else T.dptr(t)), (None if q is None else T.dptr(q))

    @staticmethod
    def _check_count(rc, n):
        if rc != 0:
            e = GlioError(f"libglio_hip error {rc}: {load().glio_last_error().decode()}")
            e.code, e.n_out = rc, n.value
            raise e
        return n.value

    def set_scan_filtered(self, slot, points, leaf, deskew_trans=None, deskew_quat=None, ioff=None, ahead=False):
        """points: [n][4] float32 (x y z intensity), or records of any stride with the intensity float at byte `ioff` (capi.PCL_XYZI: 16).  The cloud
        de-skewed by (deskew_trans, deskew_quat) -- None: no de-skew / the identity -- and voxel-filtered at `leaf` becomes window slot `slot`
        (ahead=True: slot W - 1 after the next slide_window(); `slot` is not used).  Returns the slot's point count."""
        n = C.c_int(0)
        t, q, tp, qp = self._motion(deskew_trans, deskew_quat)
        pts = np.ascontiguousarray(points)
        if ioff is None:
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
            stride, ioff = 16, 12
        else:
            stride = pts.dtype.itemsize if pts.ndim == 1 else pts.dtype.itemsize * pts.shape[1]
        ptr = pts.ctypes.data_as(C.c_void_p) if len(pts) else None
        if ahead:
            rc = load().glio_set_scan_filtered_ahead_strided(self._h, ptr, len(pts), stride, int(ioff), float(leaf), tp, qp, C.byref(n))
        else:
            rc = load().glio_set_scan_filtered_strided(self._h, int(slot), ptr, len(pts), stride, int(ioff), float(leaf), tp, qp, C.byref(n))
        return self._check_count(rc, n)

    def set_scan_from_features(self, frontend, slot, leaf, deskew_trans=None, deskew_quat=None, ahead=False):
        """the same from the surf features of `frontend`'s (a Context, possibly this one) last features_extract, read where they lie on the device"""
        n = C.c_int(0)
        t, q, tp, qp = self._motion(deskew_trans, deskew_quat)
        if ahead:
            rc = load().glio_set_scan_from_features_ahead(self._h, frontend._h, float(leaf), tp, qp, C.byref(n))
        else:
            rc = load().glio_set_scan_from_features(self._h, int(slot), frontend._h, float(leaf), tp, qp, C.byref(n))
        return self._check_count(rc, n)

    def get_scan(self, slot):
        """what window slot `slot` holds, in the caller's order: [n][4] float32"""
        n = C.c_int(0)
        _check(load().glio_get_scan(self._h, int(slot), None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        _check(load().glio_get_scan(self._h, int(slot), T.fptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def scan_filter_last_device_ms(self):
        """device ms of the last non-empty keyframe-cloud call: (de-skew + box, VoxelGrid + copy, presort); needs GLIO_KFCLOUD_TIMING=1 at scan_filter_config"""
        ms = np.zeros(3, np.float32)
        _check(load().glio_scan_filter_last_device_ms(self._h, T.fptr(ms)))
        return [float(x) for x in ms]

    def set_scan_ahead(self, scan):
        """the NEXT keyframe's scan into the ring row that is slot W - 1 after the next slide_window() (the current slot 0's scan is gone afterwards)"""
        _check(load().glio_set_scan_ahead(self._h, T.fptr(scan), len(scan)))

    def associate(self, slot, scan, q, t):
        cnt = C.c_int()
        q = np.ascontiguousarray(q, float); t = np.ascontiguousarray(t, float)
        _check(load().glio_associate(self._h, slot, T.fptr(scan), len(scan), T.dptr(q), T.dptr(t), C.byref(cnt)))
        return cnt.value

    def associate_resident(self, slot, q, t):
        cnt = C.c_int()
        q = np.ascontiguousarray(q, float); t = np.ascontiguousarray(t, float)
        _check(load().glio_associate_resident(self._h, slot, T.dptr(q), T.dptr(t), C.byref(cnt)))
        return cnt.value

    def select_correspondences_window(self, per_slot):
        """per_slot[s]: None (slot untouched) or the indices slot s keeps, in order -- featureSelection of the whole window in one call"""
        W = self.W
        offs = np.zeros(W + 1, np.int32); changed = np.zeros(W, np.uint8); parts = []
        for s in range(W):
            if per_slot[s] is not None:
                changed[s] = 1; parts.append(np.ascontiguousarray(per_slot[s], np.int32))
            offs[s + 1] = offs[s] + (len(per_slot[s]) if per_slot[s] is not None else 0)
        idx = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
        _check(load().glio_select_correspondences_window(self._h, T.iptr(offs), T.iptr(idx) if len(idx) else None, changed.ctypes.data_as(C.POINTER(C.c_uint8))))

    def select_correspondences(self, slot, indices):
        idx = np.ascontiguousarray(indices, np.int32)
        _check(load().glio_select_correspondences(self._h, slot, T.iptr(idx) if len(idx) else None, len(idx)))

    def slide_window(self):
        _check(load().glio_slide_window(self._h))

    def associate_window_async(self, quats, trans):
        """enqueue the association of all W slots and return at once (counts: associate_window_counts, or implicitly at the next solve)"""
        q = np.ascontiguousarray(quats, np.float64); t = np.ascontiguousarray(trans, np.float64)
        _check(load().glio_associate_window_async(self._h, T.dptr(q), T.dptr(t)))

    def associate_window_counts(self):
        out = np.zeros(self.W, np.int32)
        _check(load().glio_associate_window_counts(self._h, T.iptr(out)))
        return out

    def associate_window(self, quats, trans):
        quats = np.ascontiguousarray(quats, float); trans = np.ascontiguousarray(trans, float)
        cnt = np.zeros(self.W, np.int32)
        _check(load().glio_associate_window(self._h, T.dptr(quats), T.dptr(trans), T.iptr(cnt)))
        return cnt

    def set_correspondences(self, slot, pts, planes, scores):
        pts = np.ascontiguousarray(pts, np.float32); planes = np.ascontiguousarray(planes, np.float32)
        scores = np.ascontiguousarray(scores, np.float64)
        n = len(scores)
        if n == 0:
            pts = np.zeros((1, 4), np.float32); planes = np.zeros((1, 4), np.float32); scores = np.zeros(1)
        _check(load().glio_set_correspondences(self._h, slot, T.fptr(pts), T.fptr(planes), T.dptr(scores), n))

    def get_correspondences(self, slot):
        cap = self.opts.max_points_per_scan
        pts = np.zeros((cap, 4), np.float32); planes = np.zeros((cap, 4), np.float32); scores = np.zeros(cap)
        cnt = C.c_int()
        _check(load().glio_get_correspondences(self._h, slot, T.fptr(pts), T.fptr(planes), T.dptr(scores), cap, C.byref(cnt)))
        n = cnt.value
        return pts[:n].copy(), planes[:n].copy(), scores[:n].copy()

    @staticmethod
    def marshal_imu(preints, slots=None):
        """The C arrays glio_set_imu takes (a C++ caller owns these natively; Python pays ~0.5 ms to build them)."""
        n = len(preints)
        arr = T.preint_array(n)
        for k, p in enumerate(preints):
            synth.fill_preint(arr[k], p)
        slots = np.arange(max(n, 1), dtype=np.int32) if slots is None else np.ascontiguousarray(slots, np.int32)
        return n, arr, slots

    @staticmethod
    def marshal_gnss(frame, dd, dop):
        return frame, len(dd), (T.GlioDdPsr * max(len(dd), 1))(*dd), len(dop), (T.GlioDoppler * max(len(dop), 1))(*dop)

    def set_imu_marshalled(self, m):
        n, arr, slots = m
        _check(load().glio_set_imu(self._h, n, arr, T.iptr(slots)))

    def set_gnss_marshalled(self, m):
        frame, ndd, dd_arr, ndop, dop_arr = m
        _check(load().glio_set_gnss(self._h, C.byref(frame) if frame is not None else None, ndd, dd_arr, ndop, dop_arr))

    def set_imu(self, preints, slots=None):
        self.set_imu_marshalled(self.marshal_imu(preints, slots))

    def set_imu_from_store(self, store, edges, slots=None):
        """glio_set_imu with the edges taken from an imu.ImuStore on the same device: edges[k] links slots slots[k], slots[k] + 1 (default k)"""
        edges = np.ascontiguousarray(edges, np.int32)
        n = len(edges)
        slots = np.arange(max(n, 1), dtype=np.int32) if slots is None else np.ascontiguousarray(slots, np.int32)
        _check(load().glio_set_imu_from_store(self._h, store._h, n, T.iptr(edges) if n else None, T.iptr(slots) if n else None))

    def set_prior(self, prior):
        ps = synth.prior_struct(prior)
        self._keep = [prior]          # glio_set_prior copies synchronously; only the latest is held (for the caller's convenience)
        _check(load().glio_set_prior(self._h, C.byref(ps)))

    def set_speed_bias_priors(self, targets):
        """The speed-bias priors of the window after a loop closure on slots 0 .. len(targets) - 1 (at most W - 1); None or an empty list removes them."""
        t = np.ascontiguousarray(np.zeros((0, 9)) if targets is None else targets, np.float64).reshape(-1, 9)
        _check(load().glio_set_speed_bias_priors(self._h, len(t), T.dptr(t) if len(t) else None))

    def marginalize_size(self):
        """(n, n_blocks) the next marginalize() will return"""
        n, nb = C.c_int32(), C.c_int32()
        _check(load().glio_marginalize_size(self._h, C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def set_gnss(self, frame, dd, dop):
        self.set_gnss_marshalled(self.marshal_gnss(frame, dd, dop))

    def load_window(self, win, corr=None, use_gnss=True, use_prior=True, use_imu=True):
        """Upload a synth.Window: correspondences (pre-made, parity hook) + all small factors."""
        if corr is not None:
            for s in range(win.W):
                self.set_correspondences(s, *corr[s])
        self.set_imu(win.preints if use_imu else [])
        self.set_prior(win.prior if use_prior else None)
        if use_gnss and win.frame is not None:
            self.set_gnss(win.frame, win.dd, win.dop)
        else:
            self.set_gnss(None, [], [])

    # ---- compute
    def linearize(self, state, want_H=True):
        n = 15 * self.W + state.n_ddt
        H = np.zeros((n, n)) if want_H else None
        g = np.zeros(n) if want_H else None
        cost = C.c_double()
        cs = state.c()
        _check(load().glio_linearize(self._h, C.byref(cs), T.dptr(H) if want_H else None, T.dptr(g) if want_H else None, C.byref(cost)))
        return H, g, cost.value

    def covariance(self, state, slots=None, columns=None):
        """Rows and columns of H^-1 at `state`, H the matrix linearize() returns (include/glio_cov.h: the coordinates, the free columns, the bits).
        slots: the 15 columns of every listed keyframe, in list order; columns: any list of columns; neither: the newest keyframe.
        Returns (cov [m][m], GlioCovInfo).  A matrix that is not positive definite raises GlioError with code E_NUMERIC and the record in .info."""
        if slots is not None and columns is not None:
            raise ValueError("covariance: slots or columns, not both")
        if columns is None:
            slots = [self.W - 1] if slots is None else slots
        lst = np.ascontiguousarray(np.asarray(slots if columns is None else columns, np.int64).ravel().astype(np.int32))
        m = len(lst) * (15 if columns is None else 1)
        out = np.full((m, m), np.nan)
        info = GlioCovInfo()
        cs = state.c()
        fn = load().glio_covariance_slots if columns is None else load().glio_covariance_columns
        rc = fn(self._h, C.byref(cs), len(lst), T.iptr(lst), T.dptr(out), C.byref(info))
        return self._cov_result(rc, out, info)

    def covariance_of(self, H, columns):
        """the same kernels on a caller's matrix (glio_debug_covariance_of: tests and timing); only the lower triangle of H is read"""
        H = np.ascontiguousarray(H, np.float64)
        lst = np.ascontiguousarray(np.asarray(columns, np.int64).ravel().astype(np.int32))
        out = np.full((len(lst), len(lst)), np.nan)
        info = GlioCovInfo()
        rc = load().glio_debug_covariance_of(self._h, len(H), T.dptr(H), len(lst), T.iptr(lst), T.dptr(out), C.byref(info))
        return self._cov_result(rc, out, info)

    @staticmethod
    def _cov_result(rc, out, info):
        if rc != 0:
            e = GlioError(f"libglio_hip error {rc}: {load().glio_last_error().decode()}")
            e.code, e.info, e.out = rc, info, out
            raise e
        return out, info

    def covariance_last_device_ms(self):
        ms = C.c_float()
        _check(load().glio_covariance_last_device_ms(self._h, C.byref(ms)))
        return ms.value

    def solve(self, state):
        s = state.copy()
        cs = s.c()
        summ = T.GlioSummary()
        _check(load().glio_solve(self._h, C.byref(cs), C.byref(summ)))
        return s, summ

    def marginalize(self, state):
        """Marginalize slot 0 at `state` (Estimator.cpp:2462-2607): returns the glio_prior fields of the next window."""
        n, nb = self.marginalize_size()
        out = dict(n=n, lin_jac=np.zeros((n, n)), lin_res=np.zeros(n), blk_slot=np.zeros(nb, np.int32),
                   blk_kind=np.zeros(nb, np.int32), blk_idx=np.zeros(nb, np.int32), blk_x0=np.zeros((nb, 9)))
        cs = state.c()
        on, onb = C.c_int32(), C.c_int32()
        _check(load().glio_marginalize(self._h, C.byref(cs), T.dptr(out["lin_jac"]), T.dptr(out["lin_res"]), T.iptr(out["blk_slot"]),
                                       T.iptr(out["blk_kind"]), T.iptr(out["blk_idx"]), T.dptr(out["blk_x0"]), C.byref(on), C.byref(onb)))
        assert on.value == n and onb.value == nb
        return out

    def marginalize_keep(self, state):
        cs = state.c()
        _check(load().glio_marginalize_keep(self._h, C.byref(cs)))

    def marginalize_keep_async(self, state):
        """enqueue the marginalization and return; marginalize_keep_finish() (or the next entry point that reads the prior) waits"""
        cs = state.c()
        _check(load().glio_marginalize_keep_async(self._h, C.byref(cs)))

    def marginalize_keep_finish(self):
        _check(load().glio_marginalize_keep_finish(self._h))

    def time_kernel(self, which, reps=20):
        ms = C.c_float()
        _check(load().glio_time_kernel(self._h, which, reps, C.byref(ms)))
        return ms.value

    def time_solve(self, state, reps=5):
        ms = C.c_float()
        summ = T.GlioSummary()
        cs = state.c()
        _check(load().glio_time_solve(self._h, C.byref(cs), reps, C.byref(ms), C.byref(summ)))
        return ms.value, summ

    def set_stream(self, stream_ptr):
        _check(load().glio_set_stream(self._h, C.c_void_p(stream_ptr)))

    # ---- single-factor evaluators (Ceres Evaluate convention)
    def eval_lidar_plane(self, cp, plane, score, t, q):
        cp = np.ascontiguousarray(cp, np.float32); plane = np.ascontiguousarray(plane, np.float32)
        r = np.zeros(1); Jt = np.zeros(3); Jq = np.zeros(4)
        params = [np.ascontiguousarray(t, float), np.ascontiguousarray(q, float)]
        P = (T.c_double_p * 2)(T.dptr(params[0]), T.dptr(params[1]))
        J = (T.c_double_p * 2)(T.dptr(Jt), T.dptr(Jq))
        _check(load().glio_eval_lidar_plane(self._h, T.fptr(cp), T.fptr(plane), C.c_double(score), P, T.dptr(r), J))
        return r[0], Jt, Jq

    def eval_imu(self, pre, params):
        ps = T.GlioPreint()
        synth.fill_preint(ps, pre)
        params = [np.ascontiguousarray(p, float) for p in params]
        P = (T.c_double_p * 6)(*[T.dptr(p) for p in params])
        r = np.zeros(15)
        Js = [np.zeros((15, s)) for s in (3, 4, 9, 3, 4, 9)]
        J = (T.c_double_p * 6)(*[T.dptr(j) for j in Js])
        _check(load().glio_eval_imu(self._h, C.byref(ps), P, T.dptr(r), J))
        return r, Js


def _ptrs(arrs):
    return (T.c_double_p * len(arrs))(*[T.dptr(a) if a is not None else None for a in arrs])


def _ctx_eval_methods():
    def eval_dd_psr(self, f, Pi, Pj, yaw, anc):
        params = [np.ascontiguousarray(Pi, float), np.ascontiguousarray(Pj, float), np.array([yaw], float), np.ascontiguousarray(anc, float)]
        r = np.zeros(19); Js = [np.zeros((19, 3)), np.zeros((19, 3)), None, None]
        _check(load().glio_eval_dd_psr(self._h, C.byref(f), _ptrs(params), T.dptr(r), _ptrs(Js)))
        return r, Js[:2]

    def eval_doppler(self, f, Pi, SBi, Pj, SBj, ddt, yaw, anc):
        params = [np.ascontiguousarray(a, float) for a in (Pi, SBi, Pj, SBj, ddt)] + [np.array([yaw], float), np.ascontiguousarray(anc, float)]
        r = np.zeros(1); Js = [np.zeros(3), np.zeros(9), np.zeros(3), np.zeros(9), np.zeros(1), None, None]
        _check(load().glio_eval_doppler(self._h, C.byref(f), _ptrs(params), T.dptr(r), _ptrs(Js)))
        return r[0], Js[:5]

    def eval_marginalization(self, prior, params):
        ps = synth.prior_struct(prior)
        n = prior["n"]
        sizes = [3 if k == 0 else (4 if k == 1 else 9) for k in prior["blk_kind"]]
        params = [np.ascontiguousarray(p, float) for p in params]
        r = np.zeros(n); Js = [np.zeros((n, s)) for s in sizes]
        _check(load().glio_eval_marginalization(self._h, C.byref(ps), _ptrs(params), T.dptr(r), _ptrs(Js)))
        return r, Js

    def eval_binary_plane(self, cp, pnc, score, t1, q1, t2, q2):
        cp = np.ascontiguousarray(cp, np.float32); pnc = np.ascontiguousarray(pnc, float)
        params = [np.ascontiguousarray(a, float) for a in (t1, q1, t2, q2)]
        r = np.zeros(1); Js = [np.zeros(3), np.zeros(4), np.zeros(3), np.zeros(4)]
        _check(load().glio_eval_binary_plane(self._h, T.fptr(cp), T.dptr(pnc), C.c_double(score), _ptrs(params), T.dptr(r), _ptrs(Js)))
        return r[0], Js
    for fn in (eval_dd_psr, eval_doppler, eval_marginalization, eval_binary_plane):
        setattr(Context, fn.__name__, fn)


_ctx_eval_methods()


def lidar_pose(opts, q, t):
    """Q2 = Q * q_lb^-1, T2 = T - Q2 * t_lb: the LiDAR pose handed to findCorrespondingSurfFeatures
    (reference GLIO/src/Estimator.cpp:2216-2217)."""
    qlb = np.array(opts.q_lb)
    q2 = synth.qmul(np.asarray(q, float), synth.qconj(qlb) / (qlb @ qlb))
    t2 = np.asarray(t, float) - synth.q2R(q2 / np.linalg.norm(q2)) @ np.array(opts.t_lb)
    return q2, t2
