"""Streaming driver: the per-keyframe call sequence of `Estimator::optimizeSlidingWindowWithLandMark`
(reference GLIO/src/Estimator.cpp:2046-2736) over a stream of keyframes, written against a backend with the
methods of `capi.Context` (set_map / associate / set_imu / set_prior / set_gnss / solve / marginalize).

Per window: local map -> (:2056), state arrays (:2100-2127), prior (:2153-2158), IMU edges (:2182-2192),
correspondences per slot from the pre-solve poses (:2198-2248, once per solve: quirk Q3), solve (:2424-2433),
quaternion sign unification (:2439-2457), marginalization of slot 0 with the kept blocks renamed s -> s-1
(:2462-2607).  The window then slides by one keyframe; the newest slot starts from the caller's prediction
(the reference takes it from IMU propagation, outside this path).
"""
import numpy as np

from . import capi
from . import ctypes_types as T


def unify_quaternions(state):
    """Estimator.cpp:2439-2457: q and -q are the same rotation; the reference keeps w >= 0."""
    flip = state.quat[:, 0] < 0
    state.quat[flip] *= -1.0
    return state


def pose3_covariance(cov6, q):
    """The 6 x 6 pose block of Context.covariance (columns 15 s .. 15 s + 5 of slot s: translation, then the quaternion's tangent) at the slot's
    quaternion q = (w, x, y, z), in GTSAM's Pose3 order and chart: rotation first, body-frame rotation vector in radians, translation increment R v.
      The window moves a pose by  t' = t + dt,  q' = (cos |d|, sin |d| d / |d|) * q  (Ceres' QuaternionParameterization: d multiplies on the LEFT and is HALF
      a rotation vector), i.e. R' = Exp(2 d) R with R = R(q).  Pose3's chart moves it by  R' = R Exp(omega),  t' = t + R v.
      Exp(2 d) R = R Exp(R^T 2 d) exactly, so omega = 2 R^T d; and t + dt = t + R v gives v = R^T dt.  Both are linear in (dt, d): to first order (and for the
      rotation at any size) (omega, v) = A (dt, d) with the constant
          A = [ 0     2 R^T ]
              [ R^T   0     ]
      and the covariance maps as A Sigma A^T.  glio::pose3Covariance (glio_backend.hpp) is the C++ twin."""
    q = np.asarray(q, np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    A = np.zeros((6, 6))
    A[0:3, 3:6] = 2.0 * R.T
    A[3:6, 0:3] = R.T
    out = A @ np.asarray(cov6, np.float64).reshape(6, 6) @ A.T
    return 0.5 * (out + out.T)


def feature_selection_draws(count, feature_res_num, rng, random_select=True):
    """The index sequence `featureSelection` (Estimator.cpp:3894-3992) keeps, for `count` correspondences: nothing
    changes when count - 1 < feature_res_num (early return :3906-3909, quirk Q9); otherwise feature_res_num draws, each
    uniform over the first size - 1 of the `size` records still left: the reference shuffles geneRandArrayNoRepeat(0,
    size - 1, rand_set_num) = the indices 0 .. size - 2 (random_generator.hpp:79-93), takes element rand_set_num - 1
    (:3948-3957) and erases that record (:3964-3978), so the last record still left is never drawn.  With
    random_select == false the set is emptied (:3945,3981-3987).  At count = feature_res_num + 1 the reference clamps
    rand_set_num to 0 (:3914-3916) and reads record -1; this port draws there as for any other count, and claims parity
    for count > feature_res_num + 1 only (glio::featureSelectionDraws decides the same).
    Returns None for "keep all", else the kept original indices in draw order."""
    if count < 1 or count - 1 < feature_res_num:
        return None
    if not random_select:
        return np.zeros(0, np.int32)
    # the d-th draw picks the k-th record STILL LEFT, k uniform below count - d - 1; its original index is k advanced past every removed index <= it
    # (the same as popping from the list of remaining records, without building a list of `count` entries per slot; glio::featureSelectionDraws
    # in glio_backend.hpp is this loop in C++: same generator in, same indices out)
    gone, out = [], []
    for d in range(feature_res_num):
        v = int(rng.integers(0, int(count) - d - 1))
        pos = 0
        while pos < len(gone) and gone[pos] <= v:
            v += 1; pos += 1
        gone.insert(pos, v)
        out.append(v)
    return np.asarray(out, np.int32)


class TableRng:
    """A generator that both hosts can share: integers(lo, hi) = lo + table[k++] mod (hi - lo) over a table of 63-bit numbers (written to a file for
    host_demo_stream's `draws=`).  Not a statistical generator -- the means by which a test makes the C++ and the Python host draw the same records."""

    def __init__(self, table):
        self.table, self.k = np.ascontiguousarray(table, np.uint64), 0

    def integers(self, lo, hi):
        v = int(self.table[self.k % len(self.table)]); self.k += 1
        lo, hi = int(lo), int(hi)
        return lo + v % (hi - lo)


def feature_selection(backend, slot, count, feature_res_num, rng, random_select=True):
    sel = feature_selection_draws(count, feature_res_num, rng, random_select)
    if sel is None:
        return count
    backend.select_correspondences(slot, sel)
    return len(sel)


def feature_selection_window(backend, counts, feature_res_num, rng, random_select=True):
    """featureSelection for every slot of the window, the draws in slot order (as W calls of feature_selection would make them), ONE device call.
    Returns the residual counts."""
    sels = [feature_selection_draws(int(c), feature_res_num, rng, random_select) for c in counts]
    if any(sel is not None for sel in sels):
        backend.select_correspondences_window(sels)
    return [int(c) if sel is None else len(sel) for c, sel in zip(counts, sels)]


MIN_MAP_POINTS = 50        # `if (surf_local_map_ds->points.size() > 50)` guards the correspondence search, Estimator.cpp:2221,2244


def set_imu_edges(backend, preints):
    """The window's IMU edges (Estimator.cpp:2182-2192): a list of pre-integrations (host path, glio_set_imu), or a pair
    (imu.ImuStore, edge indices) -- edge_indices[s] is the store's edge between slots s and s + 1 -- taken on the device (glio_set_imu_from_store)."""
    if isinstance(preints, tuple) and len(preints) == 2 and hasattr(preints[0], "integrate_raw"):
        backend.set_imu_from_store(preints[0], preints[1])
    else:
        backend.set_imu(preints)


FILTER_MAX_INPUT_POINTS = 1 << 17        # glio_scan_filter_config of a driver with filter=LEAF, unless the caller gives filter_max_points


def _scan_filter_config(ctx, scans, filter_max_points):
    ctx.scan_filter_config(filter_max_points or max(FILTER_MAX_INPUT_POINTS, max(len(s) for s in scans)))


class SlidingWindowDriver:
    def __init__(self, backend, opts, lidar_pose=capi.lidar_pose, filter=None, filter_max_points=None, covariance=False):
        """filter=LEAF (opt-in, capi.Context only): step() takes the keyframes' UNFILTERED surf clouds and downSampleCloud's ds_filter_surf
        (Estimator.cpp:3628-3630, surfDSRange) runs on the device with the upload (glio_set_scan_filtered); the default takes filtered clouds.
        covariance=True (opt-in, capi.Context only): step() asks for the newest keyframe's 15 x 15 marginal covariance at the solved state, after the solve
        and before the marginalization (glio_covariance_slots), and returns it as a fourth value; last_covariance_info holds the call's record."""
        self.covariance, self.last_covariance, self.last_covariance_info = covariance, None, None
        self.be, self.opts, self.W = backend, opts, opts.window
        self.lidar_pose = lidar_pose
        self.filter, self.filter_max_points, self._filter_ready = filter, filter_max_points, False
        self.prior = None
        self.state = None
        self.first = 0                   # index (into the keyframe stream) of slot 0
        self.history = []
        self.speed_bias_priors_armed = False

    def arm_speed_bias_priors(self):
        """correctPoses' `marg = false` (Estimator.cpp:4785; dropping the prior as the loop thread does, :5264-5267, is the caller's `self.prior = None`): the
        next step() installs SpeedBiasPriorFactorAutoDiff on the speed/bias of slots 0 .. W-2 as they stand before its solve (:2164-2176); its marginalization
        re-creates them at the solved state, keeps the blocks of slots 1 .. W-2 in the new prior and disarms (`marg = true`, :2517).  Opt-in.
        glio::SlidingWindowBackend::armSpeedBiasPriors is the C++ twin."""
        self.speed_bias_priors_armed = True

    def start(self, init_states):
        """init_states: WindowState of the first full window."""
        self.state = init_states.copy()
        self.state.n_ddt = 0
        self.first = 0

    def step(self, map_pts, scans, preints):
        """One optimizeSlidingWindowWithLandMark() call.  scans[s] / preints[s] are those of window slot s
        (preints[s] links slots s and s+1; or preints = (imu.ImuStore, edge indices), see set_imu_edges).  Returns (solved state, summary,
        correspondence counts)."""
        be, W = self.be, self.W
        be.set_map(map_pts)
        counts = []
        for s in range(W):
            if len(map_pts) <= MIN_MAP_POINTS:          # Estimator.cpp:2221: "Not enough feature points from the map" -- no LiDAR factors
                be.set_correspondences(s, np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), np.zeros(0))
                counts.append(0)
                continue
            q2, t2 = self.lidar_pose(self.opts, self.state.quat[s], self.state.trans[s])
            if self.filter is None:
                counts.append(be.associate(s, scans[s], q2, t2))
            else:
                if not self._filter_ready:
                    _scan_filter_config(be, scans, self.filter_max_points)
                    self._filter_ready = True
                be.set_scan_filtered(s, scans[s], self.filter)
                counts.append(be.associate_resident(s, q2, t2))
        set_imu_edges(be, preints)
        be.set_prior(self.prior)
        be.set_gnss(None, [], [])
        if self.speed_bias_priors_armed:
            be.set_speed_bias_priors(self.state.speed_bias[:W - 1])
        sol, summ = be.solve(self.state)
        unify_quaternions(sol)
        if self.covariance:
            self.last_covariance, self.last_covariance_info = be.covariance(sol, slots=[W - 1])
        self.prior = be.marginalize(sol)
        if self.speed_bias_priors_armed:             # (marginalize leaves the backend as it found it)
            be.set_speed_bias_priors(None)
            self.speed_bias_priors_armed = False
        self.state = sol
        self.history.append((self.first, sol.copy(), summ, counts))
        if self.covariance:
            return sol, summ, counts, self.last_covariance
        return sol, summ, counts

    def slide(self, new_trans, new_quat, new_speed_bias):
        """Drop slot 0, shift the rest down, append the prediction of the new keyframe."""
        st = self.state
        st.trans[:-1] = st.trans[1:].copy(); st.quat[:-1] = st.quat[1:].copy(); st.speed_bias[:-1] = st.speed_bias[1:].copy()
        st.trans[-1], st.quat[-1], st.speed_bias[-1] = new_trans, new_quat, new_speed_bias
        self.first += 1


# ------------------------------------------------------------------ the local map's schedule (scalar bookkeeping, mirrored by glio::localMapPlan)
MAP_NOTHING, MAP_PUSH, MAP_REBUILD = 0, 1, 2


def local_map_plan(recent_size, n_keyframes, width, latest_frame_idx):
    """buildLocalMapWithLandMark's bookkeeping (Estimator.cpp:3545-3610) without the clouds: what the call does to recent_surf_keyframes when the deque holds
    `recent_size` clouds, pose_keyframe `n_keyframes` poses, local_map_width = `width`.  Returns (action, frames, recent_size', latest_frame_idx'):
      MAP_REBUILD  the deque is thrown away and refilled with the keyframes `frames` (oldest first) at their CURRENT poses (:3545-3579) -- taken whenever
                   recent_size < width.  With n_keyframes > width the loop's guard `i <= size - local_map_width` (:3550) ends it after width - 1 frames, so
                   the deque never reaches `width` again and EVERY later call rebuilds (quirk Q17: the permanent state after the first loop closure, whose
                   correctPoses clears the deque, :4660); with n_keyframes <= width it takes them all.  latest_frame_idx is not touched here.
      MAP_PUSH     the deque is full: the oldest cloud leaves, keyframe n_keyframes - 1 (= frames[0]) enters at the pose it has now (:3582-3609)
      MAP_NOTHING  full and no new keyframe since the last push (:3582), or no keyframe yet (:3531-3543: the initial map is the caller's).
    (Keyframes whose pose_keyframe intensity is negative, :3549, do not occur: every keyframe of this port has a cloud.)"""
    recent_size, n, width, latest = int(recent_size), int(n_keyframes), int(width), int(latest_frame_idx)
    if n < 1:
        return MAP_NOTHING, [], recent_size, latest
    if recent_size < width:
        frames = []
        i = n - 1
        while i >= 0:
            if n > width and i <= n - width:
                break
            frames.insert(0, i)
            if len(frames) >= width:
                break
            i -= 1
        return MAP_REBUILD, frames, len(frames), latest
    if latest != n - 1:
        return MAP_PUSH, [n - 1], recent_size, n - 1
    return MAP_NOTHING, [], recent_size, latest


class ReferenceMapSchedule:
    """The local map kept the way the reference keeps it (opt-in; the drivers above push each keyframe once and never re-pose it): every keyframe call asks
    local_map_plan and either rebuilds the ring from the keyframe clouds resident in a batch.BatchAssociation at the poses pose_info_keyframe holds NOW
    (glio_localmap_rebuild_from_frames) or pushes the newest keyframe's resident scan (glio_localmap_push_scan + glio_localmap_build).  loop_closed() is
    correctPoses' recent_surf_keyframes.clear() (Estimator.cpp:4660).  glio::ReferenceMapSchedule (glio_backend.hpp) is the C++ twin."""

    def __init__(self, ctx, assoc, width, q_bl=(1.0, 0.0, 0.0, 0.0), t_bl=(0.0, 0.0, 0.0)):
        self.ctx, self.assoc, self.width = ctx, assoc, int(width)
        self.q_bl, self.t_bl = q_bl, t_bl
        self.recent_size, self.latest_frame_idx = 0, -1
        self.last_action, self.last_frames = MAP_NOTHING, []

    def loop_closed(self):
        self.recent_size = 0

    def will_rebuild(self, n_keyframes):
        """a call whose plan says "rebuild" does not use a map built ahead: ask before glio_localmap_push_scan_ahead_and_build"""
        return local_map_plan(self.recent_size, n_keyframes, self.width, self.latest_frame_idx)[0] == MAP_REBUILD

    def update(self, n_keyframes, pose_info, scan_slot, lidar_offset):
        """pose_info [>= n_keyframes][7] = t_po, q_po of every keyframe; the newest keyframe's scan is resident in window slot `scan_slot` and its own-frame
        cloud in the association (set_frame_from_scan).  Returns the map size (None when the plan says nothing)."""
        from . import loop
        action, frames, self.recent_size, self.latest_frame_idx = local_map_plan(self.recent_size, n_keyframes, self.width, self.latest_frame_idx)
        self.last_action, self.last_frames = action, frames
        if action == MAP_NOTHING:
            return None
        pose_info = np.asarray(pose_info, np.float64).reshape(-1, 7)
        poses = loop.frame_poses(pose_info[frames], self.q_bl, self.t_bl)
        if action == MAP_REBUILD:
            return self.ctx.localmap_rebuild_from_frames(self.assoc, frames, poses)
        self.ctx.localmap_push_scan(scan_slot, lidar_offset, poses[0, 3:], poses[0, :3])
        return self.ctx.localmap_build()


class ResidentSlidingWindow:
    """The same per-keyframe sequence with everything kept on the device between keyframes (capi.Context only):
    scans slide with `glio_slide_window`, only the NEW keyframe's scan is uploaded, all slots are associated in one call,
    and the marginalization result stays resident as the next prior (`glio_marginalize_keep`)."""

    def __init__(self, ctx, opts, lidar_pose=capi.lidar_pose, filter=None, filter_max_points=None, covariance=False):
        """filter=LEAF (opt-in): as SlidingWindowDriver -- the new keyframe's unfiltered surf cloud is filtered on the device on its way into slot W - 1.
        covariance=True (opt-in): as SlidingWindowDriver -- the newest keyframe's 15 x 15 block, asked between solve and marginalize_keep, a fourth value."""
        self.covariance, self.last_covariance, self.last_covariance_info = covariance, None, None
        self.ctx, self.opts, self.W = ctx, opts, opts.window
        self.lidar_pose = lidar_pose
        self.filter, self.filter_max_points = filter, filter_max_points
        self.state = None
        self.first = 0
        self._have_scans = False
        self.speed_bias_priors_armed = False

    def arm_speed_bias_priors(self):
        """As SlidingWindowDriver.arm_speed_bias_priors; here marginalize_keep removes the factors from the context itself.  (The loop thread's deletion of the
        prior is the caller's ctx.set_prior(None).)"""
        self.speed_bias_priors_armed = True

    def start(self, init_states):
        self.state = init_states.copy()
        self.state.n_ddt = 0
        self.ctx.set_prior(None)
        self.ctx.set_gnss(None, [], [])

    def step(self, map_pts, scans, preints):
        ctx, W = self.ctx, self.W
        ctx.set_map(map_pts)
        if self.filter is None:
            put = ctx.set_scan
        else:
            if not self._have_scans:
                _scan_filter_config(ctx, scans, self.filter_max_points)
            put = lambda slot, cloud: ctx.set_scan_filtered(slot, cloud, self.filter)
        if not self._have_scans:
            for s in range(W):
                put(s, scans[s])
            self._have_scans = True
        else:
            ctx.slide_window()
            put(W - 1, scans[W - 1])
        poses = [self.lidar_pose(self.opts, self.state.quat[s], self.state.trans[s]) for s in range(W)]
        if len(map_pts) <= MIN_MAP_POINTS:              # Estimator.cpp:2221
            for s in range(W):
                ctx.set_correspondences(s, np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), np.zeros(0))
            counts = [0] * W
        else:
            counts = ctx.associate_window(np.array([p[0] for p in poses]), np.array([p[1] for p in poses]))
        set_imu_edges(ctx, preints)
        if self.speed_bias_priors_armed:
            ctx.set_speed_bias_priors(self.state.speed_bias[:W - 1])
        sol, summ = ctx.solve(self.state)
        unify_quaternions(sol)
        if self.covariance:
            self.last_covariance, self.last_covariance_info = ctx.covariance(sol, slots=[W - 1])
        ctx.marginalize_keep(sol)
        self.speed_bias_priors_armed = False
        self.state = sol
        if self.covariance:
            return sol, summ, [int(c) for c in counts], self.last_covariance
        return sol, summ, [int(c) for c in counts]

    def slide(self, new_trans, new_quat, new_speed_bias):
        st = self.state
        st.trans[:-1] = st.trans[1:].copy(); st.quat[:-1] = st.quat[1:].copy(); st.speed_bias[:-1] = st.speed_bias[1:].copy()
        st.trans[-1], st.quat[-1], st.speed_bias[-1] = new_trans, new_quat, new_speed_bias
        self.first += 1


class KeyframeBatchAssociation:
    """batchFeatureAssociation() (Estimator.cpp:3413-3432), the call that ends every optimizeSlidingWindowWithLandMark (:2733): once the stream holds
    2 search_range keyframes, the keyframe idx = size - search_range - 1 is matched against its 2 search_range neighbours at the CURRENT poses
    (findGlobalCorrespondingSurfFeaturesAdd_Batch :3808-3892: 12 hash builds + 12 pair searches on the device) and -- with a generator --
    globalFeatureSelectionAdd_Batch (:4057-4116) keeps batch_feature_res_num records per pair.  The records accumulate in `ba` (a batch.BatchAssociation
    sized for the stream), pair major, exactly what BatchAssociation.run over the same pairs and poses gives; `pairs` / `counts` list them in call order."""

    def __init__(self, ba, search_range=6, feature_res_num=None, rng=None, device_draws=False):
        """device_draws: the selection's raw draws (res_num uint64 per pair, from `rng`) travel with the enqueue and the selection runs on the association's stream
        behind the searches (glio_bassoc_select_tail_draws_async) instead of after a host round trip at finish()."""
        self.ba, self.sr, self.res_num, self.rng = ba, search_range, feature_res_num, rng
        self.device_draws = bool(device_draws) and feature_res_num is not None and rng is not None and 1 <= feature_res_num <= 64
        self._on_stream = False
        self.pair_ci, self.pair_cj, self.counts = [], [], []
        self._enq = None

    @staticmethod
    def pairs_of(size, search_range):
        """(idx, [j ...]) of the call made when the stream holds `size` keyframes, or None (Estimator.cpp:3414-3416)."""
        idx = size - search_range - 1
        if size < 2 * search_range or idx < search_range:
            return None
        return idx, [j for j in range(idx - search_range, idx + search_range + 1) if j != idx]

    def prepare(self, size):
        """Optional, before the poses exist (before the solve of the same keyframe call): the pairs follow from the keyframe count alone; their search frames'
        build descriptors go to the device and their hash tables are cleared now (glio_bassoc_prepare_async), enqueue() then starts with the clouds' transform."""
        pr = self.pairs_of(size, self.sr)
        if pr is not None:
            idx, js = pr
            self.ba.prepare(np.full(len(js), idx, np.int32), np.asarray(js, np.int32))

    def enqueue(self, size, poses):
        """poses [K][7] = t, q of every keyframe slot of `ba`.  Enqueues the searches on the association's own stream and returns."""
        pr = self.pairs_of(size, self.sr)
        if pr is None:
            self._enq = None
            return 0
        idx, js = pr
        ci, cj = np.full(len(js), idx, np.int32), np.asarray(js, np.int32)
        self._first = self.ba.total
        self.ba.run_append(poses, ci, cj, wait=False)
        self._enq = (ci, cj)
        self._on_stream = False
        if self.device_draws:
            raws = np.array([int(self.rng.integers(0, 2 ** 62)) for _ in range(len(js) * self.res_num)], np.uint64)
            self.ba.select_tail_draws(self.res_num, raws)
            self._on_stream = True
        return len(js)

    def finish(self):
        """Waits for the enqueued call, applies the selection, books the pairs (`counts`: what was kept).  Returns the per-pair counts FOUND."""
        if self._enq is None:
            return np.zeros(0, np.int64)
        ci, cj = self._enq
        self._enq = None
        cnt, total = self.ba.finish()
        found = cnt.copy()
        if self._on_stream:            # the device applied the rule: everything of a pair with at most res_num records, else res_num (never the last record)
            cnt = np.array([c if c <= self.res_num else min(self.res_num, c - 1) for c in found.tolist()], np.int64)
        elif self.res_num is not None and self.rng is not None:
            from .batch import batch_selection_draws
            offs = self._first + np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
            keep, kept = [], cnt.copy()
            for p in range(len(cnt)):
                d = batch_selection_draws(int(cnt[p]), self.res_num, self.rng)
                sel = np.arange(int(cnt[p]), dtype=np.int64) if d is None else d
                keep.append(offs[p] + sel); kept[p] = len(sel)
            src = np.concatenate(keep) if keep else np.zeros(0, np.int64)
            if len(src) != total - self._first:
                self.ba.select_range(self._first, src, total)
            cnt = kept
        self.pair_ci += ci.tolist(); self.pair_cj += cj.tolist(); self.counts += [int(c) for c in cnt]
        return found

    def step(self, size, poses):
        self.enqueue(size, poses)
        return self.finish()
