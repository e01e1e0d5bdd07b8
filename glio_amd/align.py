"""The GNSS frame estimate: yaw_enu_local and anc_ecef of a GlioGnssFrame from a local trajectory and the DD pseudorange factors along it (glio_align_*,
csrc/align_kernels.hip, include/glio_align.h).  It replaces what the reference reads from the yaml and from the data set's ground-truth heading
(Estimator.cpp:1434-1448); the result goes into Context.set_gnss / BatchStage.set_small_factors unchanged.  `glio::GnssAlignment`
(host/glio_align_backend.hpp) is the C++ twin.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import capi
from . import ctypes_types as T

OK, WEAK, UNOBSERVABLE = T.ALIGN_OK, T.ALIGN_WEAK, T.ALIGN_UNOBSERVABLE


class AlignResult:
    def __init__(self, frame, info):
        self.frame, self.info = frame, info

    @property
    def status(self):
        return self.info["status"]

    @property
    def delivered(self):
        return self.info["status"] != UNOBSERVABLE

    @property
    def yaw(self):
        return float(self.frame.yaw_enu_local)

    @property
    def anchor(self):
        return np.array(self.frame.anc_ecef[:], float)


def frame_of(yaw, anchor):
    f = T.GlioGnssFrame()
    f.yaw_enu_local = float(yaw)
    f.anc_ecef[:] = [float(x) for x in anchor]
    return f


class GnssAlignment:
    def __init__(self, max_factors, max_positions, device=0, opts=None):
        lib = capi.load()
        if lib.glio_device_count() < 1:
            raise capi.GlioError("no HIP device visible: the alignment has no CPU fallback")
        self._h = C.c_void_p()
        capi._check(lib.glio_align_create(device, int(max_factors), int(max_positions), C.byref(self._h)))
        self.n_hypotheses = capi.align_opts().n_hypotheses
        if opts is not None:
            self.set_opts(opts)

    def close(self):
        if self._h:
            capi.load().glio_align_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_opts(self, opts=None, **kw):
        """a GlioAlignOpts, or the defaults with fields replaced (capi.align_opts)"""
        o = opts if opts is not None else capi.align_opts(**kw)
        capi._check(capi.load().glio_align_set_opts(self._h, C.byref(o)))
        self.n_hypotheses = int(o.n_hypotheses)

    def set_factors(self, dd):
        """a list of GlioDdPsr (or a ctypes array of them); slot_i / slot_j index the position table"""
        arr = dd if isinstance(dd, C.Array) else (T.GlioDdPsr * max(len(dd), 1))(*dd)
        capi._check(capi.load().glio_align_set_factors(self._h, len(dd), arr))

    def set_positions(self, table):
        """[n][3] positions, or an [n][7] pose table as it lies (t first)"""
        t = np.asarray(table, np.float64)
        if t.ndim != 2 or t.shape[1] < 3 or t.strides[1] != 8 or t.strides[0] % 8 or t.strides[0] < 24:
            t = np.ascontiguousarray(np.asarray(table, np.float64).reshape(len(table), -1))
        self._pos = t
        capi._check(capi.load().glio_align_set_positions(self._h, len(t), t.ctypes.data_as(T.c_double_p), t.strides[0] // 8 if len(t) else 3))

    def solve(self, start):
        """start: a GlioGnssFrame (any anchor within the drive's neighbourhood).  Returns an AlignResult; UNOBSERVABLE returns the start frame."""
        out, info = T.GlioGnssFrame(), T.GlioAlignInfo()
        capi._check(capi.load().glio_align_solve(self._h, C.byref(start), C.byref(out), C.byref(info)))
        return AlignResult(out, info.as_dict())

    def cost(self, frame, threshold):
        """(the reference's DD cost at `frame`, the number of down-weighted rows)"""
        c, n = C.c_double(), C.c_int32()
        capi._check(capi.load().glio_align_cost(self._h, C.byref(frame), C.c_double(threshold), C.byref(c), C.byref(n)))
        return c.value, n.value

    def read_coarse(self):
        """the reduced costs of the last solve's hypotheses"""
        n = C.c_int32()
        capi._check(capi.load().glio_align_read_coarse(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value)
        capi._check(capi.load().glio_align_read_coarse(self._h, T.dptr(out), n.value, None))
        return out

    def last_device_ms(self):
        ms = C.c_float()
        capi._check(capi.load().glio_align_last_device_ms(self._h, C.byref(ms)))
        return ms.value
