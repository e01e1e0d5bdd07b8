"""Flat binary window file for glio_amd/host/host_demo (the C++ call sequence of the hot path)."""
import ctypes as C
import os
import subprocess

import numpy as np

from .. import ctypes_types as T
from .. import synth

HERE = os.path.dirname(os.path.abspath(__file__))
DEMO = os.path.join(HERE, "host_demo")
_ABI_HEADERS = [os.path.join(HERE, "..", "..", "include", h) for h in ("glio_hip.h", "glio_types.h", "glio_pgraph_lm.h", "glio_cov.h", "glio_dense.h")] + \
    [os.path.join(HERE, "..", "csrc", "tr_math.h")]      # a changed struct must rebuild the demos


def build_demo(force=False):
    src = [os.path.join(HERE, "host_demo.cpp"), os.path.join(HERE, "glio_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO) or any(os.path.getmtime(s) > os.path.getmtime(DEMO) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO])
    return DEMO


def write_window(path, win):
    """opts | n_map n_imu 0 0 | map | trans quat speed_bias | preints | per slot: n, scan"""
    with open(path, "wb") as f:
        f.write(bytes(win.opts))
        f.write(np.array([len(win.map_pts), len(win.preints), 0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(win.map_pts, np.float32).tobytes())
        f.write(win.init.trans.tobytes()); f.write(win.init.quat.tobytes()); f.write(win.init.speed_bias.tobytes())
        arr = T.preint_array(len(win.preints))
        for k, p in enumerate(win.preints):
            synth.fill_preint(arr[k], p)
        if win.preints:
            f.write(bytes(arr)[:C.sizeof(T.GlioPreint) * len(win.preints)])
        for s in range(win.W):
            f.write(np.array([len(win.scans[s])], np.int32).tobytes())
            f.write(np.ascontiguousarray(win.scans[s], np.float32).tobytes())


def run_demo(path, arm=False):
    """arm: the window is the first after a loop closure (host_demo's `arm`): info gains "rearmed" and "next" """
    out = subprocess.run([build_demo(), path] + (["arm"] if arm else []), capture_output=True, text=True, check=True).stdout.splitlines()
    head = out[0].split()
    info = dict(kept=int(head[1]), iterations=int(head[3]), termination=int(head[5]), initial_cost=float(head[7]), final_cost=float(head[9]))
    rows = np.array([[float(x) for x in ln.split()[2:]] for ln in out[1:] if ln.startswith("kf ")])
    for ln in out[1:]:
        if ln.startswith("prior "):
            p = ln.split()
            info["prior"] = dict(n=int(p[1]), n_blocks=int(p[2]), jac_fro2=float(p[3]), res2=float(p[4]))
        if ln.startswith("resident "):
            p = ln.split()
            info["resident"] = dict(kept=int(p[1]), iterations=int(p[2]), final_cost=float(p[3]))
        if ln.startswith("rearmed "):
            p = ln.split()
            info["rearmed"] = dict(iterations=int(p[1]), final_cost=float(p[2]))
        if ln.startswith("next "):
            p = ln.split()
            info["next"] = dict(n=int(p[1]), n_blocks=int(p[2]), armed=int(p[3]))
    return info, rows[:, :3], rows[:, 3:]


DEMO_BATCH = os.path.join(HERE, "host_demo_batch")


def build_demo_batch(force=False):
    """The C++ sharded batch stage (links librccl: ncclAllReduce between linearise and step)."""
    src = [os.path.join(HERE, "host_demo_batch.cpp"), os.path.join(HERE, "glio_batch_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_BATCH) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_BATCH) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-I/opt/rocm/include", "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-L/opt/rocm/lib", "-lrccl", "-lamdhip64", "-lpthread",
                               "-Wl,-rpath,$ORIGIN/../lib", "-Wl,-rpath,/opt/rocm/lib", "-o", DEMO_BATCH])
    return DEMO_BATCH


def write_batch_problem(path, K, band, iterations, poses, ci, cj, cp, nc, score, full=None):
    """full = (odo [K][7], search_range, frame, dd list): appends the data of the full pose problem (see host_demo_batch.cpp)."""
    with open(path, "wb") as f:
        f.write(np.array([K, band, iterations, 1 if full else 0], np.int32).tobytes())
        f.write(np.array([len(ci)], np.int64).tobytes())
        f.write(np.ascontiguousarray(poses, np.float64).tobytes())
        f.write(np.ascontiguousarray(ci, np.int32).tobytes()); f.write(np.ascontiguousarray(cj, np.int32).tobytes())
        f.write(np.ascontiguousarray(cp, np.float32).tobytes()); f.write(np.ascontiguousarray(nc, np.float64).tobytes())
        f.write(np.ascontiguousarray(score, np.float64).tobytes())
        if full:
            odo, search_range, frame, dd = full
            f.write(np.ascontiguousarray(odo, np.float64).tobytes())
            f.write(np.array([search_range, len(dd)], np.int32).tobytes())
            f.write(bytes(frame))
            for d in dd:
                f.write(bytes(d))


def write_batch_assoc_problem(path, K, band, iterations, poses, odo, search_range, frame, dd, clouds, max_points):
    """The association mode of host_demo_batch.cpp (header word 3 = 2): no constraints, the keyframe clouds instead."""
    with open(path, "wb") as f:
        f.write(np.array([K, band, iterations, 2], np.int32).tobytes())
        f.write(np.array([0], np.int64).tobytes())
        f.write(np.ascontiguousarray(poses, np.float64).tobytes())
        f.write(np.ascontiguousarray(odo, np.float64).tobytes())
        f.write(np.array([search_range, len(dd), max_points, 0], np.int32).tobytes())
        f.write(bytes(frame))
        for d in dd:
            f.write(bytes(d))
        for c in clouds:
            c = np.ascontiguousarray(c, np.float32)
            f.write(np.array([len(c)], np.int32).tobytes()); f.write(c.tobytes())


def run_demo_batch(path, iterations=None, env=None):
    cmd = [build_demo_batch(), path] + ([str(iterations)] if iterations is not None else [])
    out = subprocess.run(cmd, capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    # (RCCL prints its own version banner on stdout: pick our lines by their first word)
    head = next(ln for ln in out if ln.startswith("batch ")).split()
    info = {head[i]: head[i + 1] for i in range(1, len(head) - 1, 2)}
    hist = [float(x) for x in next(ln for ln in out if ln.split()[:1] == ["cost"]).split()[1:]]
    rows = np.array([[float(x) for x in ln.split()[2:]] for ln in out if ln.startswith("kf ")])
    info["raw"] = [ln for ln in out if not ln.startswith("kf ")]
    for ln in out:
        if ln.startswith("assoc "):
            w = ln.split()
            info["assoc"] = {w[i]: float(w[i + 1]) for i in range(1, len(w) - 1, 2)}
    info["rounds"] = []
    for ln in out:
        if ln.startswith("round "):
            w = ln.split()
            info["rounds"].append({w[i]: float(w[i + 1]) for i in range(1, len(w) - 1, 2)})
    return info, hist, rows


DEMO_STREAM = os.path.join(HERE, "host_demo_stream")


def build_demo_stream(force=False):
    """The C++ moving-stream keyframe cycle (host_demo_stream.cpp): what bench.py times as keyframe_pipeline_cpp."""
    src = [os.path.join(HERE, "host_demo_stream.cpp"), os.path.join(HERE, "glio_backend.hpp"), os.path.join(HERE, "glio_batch_backend.hpp"),
           os.path.join(HERE, "glio_trajectory_backend.hpp"), os.path.join(HERE, "..", "..", "include", "glio_traj.h")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_STREAM) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_STREAM) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_STREAM])
    return DEMO_STREAM


def write_stream(path, long, wins, W, n_keyframes, pts, lm_width=50, leaf=0.4, batch_res_num=0):
    """The moving stream of bench.py's keyframe_stream as a flat file: opts | n_keyframes pts lm_width 0 | leaf tlb[3] | the W + n_keyframes scans |
    ground-truth q [.][4], t [.][3] (the poses the local map is pushed with) | per window j = 0..n_keyframes: n_ddt n_preint n_dd n_dop, init trans quat
    speed_bias rcv_ddt, preints, GNSS frame, DD factors, Doppler factors."""
    opts = wins[0].opts
    with open(path, "wb") as f:
        f.write(bytes(opts))
        f.write(np.array([n_keyframes, pts, lm_width, batch_res_num], np.int32).tobytes())      # (batch_feature_res_num of the per-keyframe batch association; 0 = the yaml's 25)
        f.write(np.array([leaf] + list(opts.t_lb), np.float32).tobytes())
        for j in range(W + n_keyframes):
            f.write(np.ascontiguousarray(long.scans[j], np.float32).tobytes())
        f.write(np.ascontiguousarray(long.gt.quat[:W + n_keyframes], np.float64).tobytes())
        f.write(np.ascontiguousarray(long.gt.trans[:W + n_keyframes], np.float64).tobytes())
        for win in wins:
            st = win.init
            f.write(np.array([st.n_ddt, len(win.preints), len(win.dd), len(win.dop)], np.int32).tobytes())
            f.write(np.ascontiguousarray(st.trans, np.float64).tobytes()); f.write(np.ascontiguousarray(st.quat, np.float64).tobytes())
            f.write(np.ascontiguousarray(st.speed_bias, np.float64).tobytes()); f.write(np.ascontiguousarray(np.asarray(st.rcv_ddt)[:st.n_ddt], np.float64).tobytes())
            arr = T.preint_array(len(win.preints))
            for k, p in enumerate(win.preints):
                synth.fill_preint(arr[k], p)
            if win.preints:
                f.write(bytes(arr)[:C.sizeof(T.GlioPreint) * len(win.preints)])
            f.write(bytes(win.frame) if win.frame is not None else bytes(C.sizeof(T.GlioGnssFrame)))
            for d in win.dd:
                f.write(bytes(d))
            for d in win.dop:
                f.write(bytes(d))


def run_demo_stream(path, device=0, env=None, search_range=6, defer=False, feature_res_num=0, draws=None, timed=None, per_slot=False, sleep_ms=0, sleep_at=0, stream_draws=True, prepare_early=True, ahead=False, map_ahead=False, map_rebuild=False, filter=None, traj=False, cov=False):
    """cov: the newest keyframe's marginal covariance is asked for after every solve (opt-in; covariance_newest_trace, one per keyframe call, the first included);
    traj: a gap of the every-frame trajectory is pushed per keyframe call (opt-in); filter=LEAF: the stream's clouds are filtered on the device on their way into the window (setScanFiltered*; opt-in);
    feature_res_num > 0: featureSelection behind every slot's search (Estimator.cpp:2223); draws: file of uint64 both hosts draw from (sliding.TableRng);
    timed: only the last `timed` keyframes enter the time averages"""
    import json
    cmd = [build_demo_stream(), path, str(device), str(search_range), str(int(defer))]
    if feature_res_num:
        cmd.append(f"res={int(feature_res_num)}")
    if draws:
        cmd.append(f"draws={draws}")
    if timed:
        cmd.append(f"timed={int(timed)}")
    if per_slot:
        cmd.append("per_slot=1")
    if sleep_ms:
        cmd += [f"sleep_ms={int(sleep_ms)}", f"sleep_at={int(sleep_at)}"]
    cmd.append("stream_draws=%d" % (1 if stream_draws else 0))
    if not prepare_early:
        cmd.append("prepare_early=0")
    if ahead:
        cmd.append("ahead=1")
    if map_ahead:
        cmd.append("map_ahead=1")
    if map_rebuild:
        cmd.append("map_rebuild=1")
    if filter:
        cmd.append(f"filter={float(filter)!r}")
    if traj:
        cmd.append("traj=1")
    if cov:
        cmd.append("cov=1")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_stream failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("{")))


DEMO_ODOMETRY = os.path.join(HERE, "host_demo_odometry")


def build_demo_odometry(force=False):
    """The C++ front end (host_demo_odometry.cpp over glio::ScanToMapOdometry)."""
    src = [os.path.join(HERE, "host_demo_odometry.cpp"), os.path.join(HERE, "glio_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_ODOMETRY) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_ODOMETRY) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_ODOMETRY])
    return DEMO_ODOMETRY


def write_odometry_stream(path, opts, scans, scan_match_cnt=1):
    """opts | n_scans scan_match_cnt 0 0 | per scan: n, points xyzi (the downsampled surf cloud of each LiDAR frame, body frame)"""
    with open(path, "wb") as f:
        f.write(bytes(opts))
        f.write(np.array([len(scans), scan_match_cnt, 0, 0], np.int32).tobytes())
        for sc in scans:
            sc = np.ascontiguousarray(sc, np.float32)
            f.write(np.array([len(sc)], np.int32).tobytes()); f.write(sc.tobytes())


def run_demo_odometry(path, device=0, env=None):
    """-> (poses [n][7] q then t, per-scan dicts, {"ms_per_scan": ...})"""
    import json
    r = subprocess.run([build_demo_odometry(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_odometry failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    poses, rows = [], []
    for ln in r.stdout.splitlines():
        if ln.startswith("pose "):
            w = ln.split()
            poses.append([float(x) for x in w[2:9]])
            rows.append({"rounds": int(w[9]), "kept": int(w[10]), "iterations": int(w[11]), "final_cost": float(w[12]), "map_points": int(w[13])})
    info = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("{")))
    return np.array(poses), rows, info


DEMO_FRONTEND_RAW = os.path.join(HERE, "host_demo_frontend_raw")


def build_demo_frontend_raw(force=False):
    """The C++ front end from raw scans (host_demo_frontend_raw.cpp over glio::ScanToMapOdometry::runRaw); built on demand by its test."""
    src = [os.path.join(HERE, "host_demo_frontend_raw.cpp"), os.path.join(HERE, "glio_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_FRONTEND_RAW) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_FRONTEND_RAW) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_FRONTEND_RAW])
    return DEMO_FRONTEND_RAW


def write_frontend_raw_stream(path, opts, feat_opts, scans, q_imus, scan_match_cnt=1, ioff=12):
    """opts | feat_opts | n_scans scan_match_cnt stride ioff | per scan: n, q_imu[4], raw records (all scans of one stride)"""
    recs = [np.ascontiguousarray(s) for s in scans]
    stride = 4 * recs[0].shape[1] if recs[0].dtype == np.float32 and recs[0].ndim == 2 else recs[0].dtype.itemsize
    with open(path, "wb") as f:
        f.write(bytes(opts)); f.write(bytes(feat_opts))
        f.write(np.array([len(recs), scan_match_cnt, stride, ioff], np.int32).tobytes())
        for r, q in zip(recs, q_imus):
            f.write(np.array([len(r)], np.int32).tobytes()); f.write(np.ascontiguousarray(q, np.float64).tobytes()); f.write(r.tobytes())


def run_demo_frontend_raw(path, device=0, env=None):
    """-> (poses [n][7] q then t, per-scan dicts, {"ms_per_scan": ...})"""
    import json
    r = subprocess.run([build_demo_frontend_raw(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_frontend_raw failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    poses, rows = [], []
    for ln in r.stdout.splitlines():
        if ln.startswith("pose "):
            w = ln.split()
            poses.append([float(x) for x in w[2:9]])
            rows.append({"rounds": int(w[9]), "kept": int(w[10]), "iterations": int(w[11]), "final_cost": float(w[12]), "map_points": int(w[13]), "surf": int(w[14])})
    info = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("{")))
    return np.array(poses), rows, info


DEMO_KEYFRAME_CLOUD = os.path.join(HERE, "host_demo_keyframe_cloud")


def build_demo_keyframe_cloud(force=False):
    """The C++ hand-over of the keyframes' surf clouds (host_demo_keyframe_cloud.cpp: runRaw -> glio::KeyframeGate -> setScanFromFrontEnd / setScanFiltered)."""
    src = [os.path.join(HERE, "host_demo_keyframe_cloud.cpp"), os.path.join(HERE, "glio_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_KEYFRAME_CLOUD) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_KEYFRAME_CLOUD) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_KEYFRAME_CLOUD])
    return DEMO_KEYFRAME_CLOUD


def run_demo_keyframe_cloud(path, device=0, leaf=0.9, deskew=True, window=3, env=None):
    """the stream file of write_frontend_raw_stream -> (per-scan dicts {kf, surf}, per-keyframe dicts {scan, slot, n_resident, hash_resident, n_host, hash_host}, info)"""
    import json
    r = subprocess.run([build_demo_keyframe_cloud(), path, str(device), f"leaf={leaf!r}", f"deskew={int(bool(deskew))}", f"window={int(window)}"],
                       capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"host_demo_keyframe_cloud failed: {r.stderr}")
    scans, kfs, info = [], [], None
    for line in r.stdout.strip().splitlines():
        v = line.split()
        if v[0] == "scan":
            scans.append({"kf": int(v[2]), "surf": int(v[3])})
        elif v[0] == "kf":
            kfs.append({"scan": int(v[1]), "slot": int(v[2]), "n_resident": int(v[3]), "hash_resident": int(v[4]), "n_host": int(v[5]), "hash_host": int(v[6])})
        else:
            info = json.loads(line)
    return scans, kfs, info


DEMO_DENSE_MAP = os.path.join(HERE, "host_demo_dense_map")


def build_demo_dense_map(force=False):
    """The C++ dense map (host_demo_dense_map.cpp: runRaw -> glio::KeyframeGate -> glio::DenseClouds::setFrameFromFeatures -> glio::GlobalMap on the store)."""
    src = [os.path.join(HERE, "host_demo_dense_map.cpp"), os.path.join(HERE, "glio_backend.hpp"), os.path.join(HERE, "glio_loop_backend.hpp"),
           os.path.join(HERE, "glio_map_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_DENSE_MAP) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_DENSE_MAP) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_DENSE_MAP])
    return DEMO_DENSE_MAP


def run_demo_dense_map(path, device=0, leaf=0.4, map_leaf=0.2, chunk=2, deskew=True, env=None):
    """the stream file of write_frontend_raw_stream -> (per-scan dicts {kf, cut}, per-keyframe dicts {scan, frame, n, hash}, the map {n_voxels, hash, n_points,
    frames}, info)"""
    import json
    r = subprocess.run([build_demo_dense_map(), path, str(device), f"leaf={leaf!r}", f"map_leaf={map_leaf!r}", f"chunk={int(chunk)}", f"deskew={int(bool(deskew))}"],
                       capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"host_demo_dense_map failed: {r.stderr}")
    scans, kfs, gmap, info = [], [], None, None
    for line in r.stdout.strip().splitlines():
        v = line.split()
        if v[0] == "scan":
            scans.append({"kf": int(v[2]), "cut": int(v[3])})
        elif v[0] == "kf":
            kfs.append({"scan": int(v[1]), "frame": int(v[2]), "n": int(v[3]), "hash": int(v[4])})
        elif v[0] == "map":
            gmap = {"n_voxels": int(v[1]), "hash": int(v[2]), "n_points": int(v[3]), "frames": int(v[4])}
        else:
            info = json.loads(line)
    return scans, kfs, gmap, info


DEMO_LOOP = os.path.join(HERE, "host_demo_loop")


def build_demo_loop(force=False):
    """The C++ loop-closure sequence (host_demo_loop.cpp over glio::LoopClosure and the host mirrors of glio_loop_backend.hpp)."""
    src = [os.path.join(HERE, "host_demo_loop.cpp"), os.path.join(HERE, "glio_loop_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_LOOP) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_LOOP) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_LOOP])
    return DEMO_LOOP


def write_loop_case(path, opts, cap, clouds, src_frames, src_pose_info, tgt_frames, tgt_pose_info, q_bl, t_bl, icp_thres, src_points=None, tgt_points=None):
    """K cap n_src_frames n_tgt_frames n_src_points n_tgt_points 0 0 | glio_loop_opts | icp_thres | K x (n, cloud) | src frames, pose_info | tgt frames, pose_info
    | q_bl t_bl | ready submaps (used when a frame list is empty)"""
    sp = np.zeros((0, 4), np.float32) if src_points is None else np.ascontiguousarray(src_points, np.float32).reshape(-1, 4)
    tp = np.zeros((0, 4), np.float32) if tgt_points is None else np.ascontiguousarray(tgt_points, np.float32).reshape(-1, 4)
    with open(path, "wb") as f:
        f.write(np.array([len(clouds), cap, len(src_frames), len(tgt_frames), len(sp), len(tp), 0, 0], np.int32).tobytes())
        f.write(bytes(opts)); f.write(np.array([icp_thres], np.float64).tobytes())
        for c in clouds:
            c = np.ascontiguousarray(c, np.float32).reshape(-1, 4)
            f.write(np.array([len(c)], np.int32).tobytes()); f.write(c.tobytes())
        f.write(np.ascontiguousarray(src_frames, np.int32).tobytes()); f.write(np.ascontiguousarray(src_pose_info, np.float64).tobytes())
        f.write(np.ascontiguousarray(tgt_frames, np.int32).tobytes()); f.write(np.ascontiguousarray(tgt_pose_info, np.float64).tobytes())
        f.write(np.ascontiguousarray(q_bl, np.float64).tobytes()); f.write(np.ascontiguousarray(t_bl, np.float64).tobytes())
        f.write(sp.tobytes()); f.write(tp.tobytes())


def loop_checksum(cloud):
    """FNV-1a over the 32-bit words of a float cloud, as host_demo_loop prints it"""
    h = 1469598103934665603
    for u in np.ascontiguousarray(cloud, np.float32).view(np.uint32).ravel().tolist():
        h = ((h ^ u) * 1099511628211) & 0xffffffffffffffff
    return h


def run_demo_loop(path, device=0, env=None):
    """-> dict(n_src, src_sum, n_tgt, tgt_sum, converged, state, iterations, last_n_corr, rank_deficient, fitness, last_mse, transform (float32 [4][4]),
    constraint (None or (relative [7], variance)), align_device_ms)"""
    import json
    r = subprocess.run([build_demo_loop(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_loop failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "submap":
            out.update(n_src=int(w[1]), src_sum=int(w[2], 16), n_tgt=int(w[3]), tgt_sum=int(w[4], 16))
        elif w[0] == "result":
            out.update(converged=bool(int(w[1])), state=int(w[2]), iterations=int(w[3]), last_n_corr=int(w[4]), rank_deficient=bool(int(w[5])),
                       fitness=float.fromhex(w[6]), last_mse=float.fromhex(w[7]))
        elif w[0] == "transform":
            out["transform"] = np.array([int(x, 16) for x in w[1:]], np.uint32).view(np.float32).reshape(4, 4)
        elif w[0] == "constraint":
            out["constraint"] = None if w[1] == "none" else (np.array([float.fromhex(x) for x in w[1:8]]), float.fromhex(w[8]))
        elif ln.startswith("{"):
            out.update(json.loads(ln))
    return out


DEMO_MAP_SCHEDULE = os.path.join(HERE, "host_demo_map_schedule")


def build_demo_map_schedule(force=False):
    """The C++ reference map schedule (host_demo_map_schedule.cpp over glio::SlidingWindowBackend); built on demand by its test."""
    src = [os.path.join(HERE, "host_demo_map_schedule.cpp"), os.path.join(HERE, "glio_backend.hpp"), os.path.join(HERE, "glio_batch_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_MAP_SCHEDULE) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_MAP_SCHEDULE) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_MAP_SCHEDULE])
    return DEMO_MAP_SCHEDULE


def write_map_schedule(path, opts, cap, width, leaf, scans, pose_info, loop_after=-1, accumulation=0, q_bl=(1.0, 0.0, 0.0, 0.0), t_bl=(0.0, 0.0, 0.0)):
    """opts | n_keyframes cap width loop_after accumulation 0 0 0 | leaf tlb[3] | q_bl[4] t_bl[3] | per keyframe: n, scan | pose_info [call][keyframe][7] = t_po, q_po
    (pose_info_keyframe as call j finds it; rows of keyframes that do not exist yet are ignored)"""
    nk = len(scans)
    pose_info = np.ascontiguousarray(pose_info, np.float64)
    assert pose_info.shape == (nk, nk, 7)
    with open(path, "wb") as f:
        f.write(bytes(opts))
        f.write(np.array([nk, cap, width, loop_after, accumulation, 0, 0, 0], np.int32).tobytes())
        f.write(np.array([leaf] + list(opts.t_lb), np.float32).tobytes())
        f.write(np.ascontiguousarray(q_bl, np.float64).tobytes()); f.write(np.ascontiguousarray(t_bl, np.float64).tobytes())
        for sc in scans:
            sc = np.ascontiguousarray(sc, np.float32)
            f.write(np.array([len(sc)], np.int32).tobytes()); f.write(sc.tobytes())
        f.write(pose_info.tobytes())


def run_demo_map_schedule(path, out_path, device=0, env=None, arm=False):
    """-> per keyframe call (action, map size reported, map [n][4]); arm: the loop closure arms the speed-bias priors, and every row gains whether they are armed"""
    r = subprocess.run([build_demo_map_schedule(), path, out_path, str(device)] + (["arm"] if arm else []), capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_map_schedule failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    raw = open(out_path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        action, reported, n, armed = np.frombuffer(raw, np.int32, 4, o); o += 16
        out.append((int(action), int(reported), np.frombuffer(raw, np.float32, 4 * int(n), o).reshape(-1, 4).copy()) + ((int(armed),) if arm else ())); o += 16 * int(n)
    return out


DEMO_MAP = os.path.join(HERE, "host_demo_map")


def build_demo_map(force=False):
    """The C++ global-map sequence (host_demo_map.cpp over glio::GlobalMap, glio_map_backend.hpp)."""
    src = [os.path.join(HERE, "host_demo_map.cpp"), os.path.join(HERE, "glio_map_backend.hpp"), os.path.join(HERE, "glio_loop_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_MAP) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_MAP) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_MAP])
    return DEMO_MAP


def write_map_case(path, opts, cap, clouds, pose_info, q_bl, t_bl, mapping_interval, chunk_frames):
    """K cap mapping_interval chunk_frames 0 0 0 0 | glio_gmap_opts | K x (n, cloud) | pose_info [K][7] = t_po, q_po | q_bl t_bl"""
    pose_info = np.ascontiguousarray(pose_info, np.float64)
    assert pose_info.shape == (len(clouds), 7)
    with open(path, "wb") as f:
        f.write(np.array([len(clouds), cap, mapping_interval, chunk_frames, 0, 0, 0, 0], np.int32).tobytes())
        f.write(bytes(opts))
        for c in clouds:
            c = np.ascontiguousarray(c, np.float32).reshape(-1, 4)
            f.write(np.array([len(c)], np.int32).tobytes()); f.write(c.tobytes())
        f.write(pose_info.tobytes())
        f.write(np.ascontiguousarray(q_bl, np.float64).tobytes()); f.write(np.ascontiguousarray(t_bl, np.float64).tobytes())


def run_demo_map(path, device=0, env=None):
    """-> dict(n_voxels, checksum (loop_checksum of the map), n_points_total, radix_passes, pcl_index_overflow, n_frames, add_device_ms)"""
    import json
    r = subprocess.run([build_demo_map(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_map failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w and w[0] == "map":
            out.update(n_voxels=int(w[1]), checksum=int(w[2], 16), n_points_total=int(w[3]), radix_passes=int(w[4]), pcl_index_overflow=bool(int(w[5])), n_frames=int(w[6]))
        elif ln.startswith("{"):
            out.update(json.loads(ln))
    return out


DEMO_POSE_GRAPH = os.path.join(HERE, "host_demo_pose_graph")


def build_demo_pose_graph(force=False):
    """The C++ pose-graph sequence (host_demo_pose_graph.cpp over glio::GlobalGraph / glio::PoseGraph, glio_posegraph_backend.hpp)."""
    src = [os.path.join(HERE, "host_demo_pose_graph.cpp"), os.path.join(HERE, "glio_posegraph_backend.hpp")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_POSE_GRAPH) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_POSE_GRAPH) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_POSE_GRAPH])
    return DEMO_POSE_GRAPH


def write_pose_graph_case(path, pose_each_frame, keyframe_id_in_frame, W, latest_keyframe, closest_keyframe, rel, var, gps):
    """int32 F NK W n_gps latest closest 0 0 | pose_each_frame [F][7] = t, q | keyframe_id_in_frame [NK] int32, padded to a multiple of 2 | rel [7] var [6] |
    n_gps x (frame, xyz[3], var[3]) doubles"""
    P = np.ascontiguousarray(pose_each_frame, np.float64).reshape(-1, 7)
    kf = np.ascontiguousarray(keyframe_id_in_frame, np.int32)
    with open(path, "wb") as f:
        f.write(np.array([len(P), len(kf), W, len(gps), latest_keyframe, closest_keyframe, 0, 0], np.int32).tobytes())
        f.write(P.tobytes())
        f.write(kf.tobytes() + (b"\0\0\0\0" if len(kf) & 1 else b""))
        f.write(np.ascontiguousarray(rel, np.float64).reshape(7).tobytes()); f.write(np.ascontiguousarray(var, np.float64).reshape(6).tobytes())
        for node, xyz, v in gps:
            f.write(np.array([float(node), *xyz, *v], np.float64).tobytes())


def run_demo_pose_graph(path, device=0, env=None, damped=False, keep_stdout=False):
    """-> dict(iterations, termination, error_before, initial_error, final_error, separators, segments, poses [n][7], calls [(n_keyframes, first, last)], n_keyframe_poses)
    damped: the loop closed by glio_pgraph_solve_damped; also accepted, rejected, invalid, trials, final_radius, history [trials][4].  keep_stdout: the demo's output as `stdout`."""
    r = subprocess.run([build_demo_pose_graph(), path, str(device)] + (["damped=1"] if damped else []), capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_pose_graph failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out, poses, calls, hist = ({"stdout": r.stdout} if keep_stdout else {}), [], [], []
    for ln in r.stdout.splitlines():
        w = ln.split()
        if not w:
            continue
        if w[0] == "solve":
            out.update(iterations=int(w[1]), termination=int(w[2]), error_before=float.fromhex(w[3]), initial_error=float.fromhex(w[4]),
                       final_error=float.fromhex(w[5]), separators=int(w[6]), segments=int(w[7]))
        elif w[0] == "pose":
            poses.append([float.fromhex(x) for x in w[2:9]])
        elif w[0] == "call":
            calls.append((int(w[1]), int(w[3]), int(w[5])))
        elif w[0] == "keyframes":
            out["n_keyframe_poses"] = int(w[1])
        elif w[0] == "damped":
            out.update(accepted=int(w[1]), rejected=int(w[2]), invalid=int(w[3]), trials=int(w[4]), final_radius=float.fromhex(w[5]))
        elif w[0] == "trial":
            hist.append([float.fromhex(x) for x in w[2:5]] + [float(w[5])])
    if damped:
        out["history"] = np.array(hist, np.float64).reshape(-1, 4)
    out.update(poses=np.array(poses), calls=calls)
    return out


DEMO_TRAJECTORY = os.path.join(HERE, "host_demo_trajectory")


def build_demo_trajectory(force=False):
    """The C++ every-frame trajectory (host_demo_trajectory.cpp over glio::Trajectory, glio_trajectory_backend.hpp, into glio::GlobalGraph)."""
    src = [os.path.join(HERE, "host_demo_trajectory.cpp"), os.path.join(HERE, "glio_trajectory_backend.hpp"), os.path.join(HERE, "glio_posegraph_backend.hpp"),
           os.path.join(HERE, "..", "..", "include", "glio_traj.h")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_TRAJECTORY) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_TRAJECTORY) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_TRAJECTORY])
    return DEMO_TRAJECTORY


def write_trajectory_case(path, imu, frame_stamps, keyframe_id_in_frame, imu_idx_in_kf, W, keyframe_poses, start_states, corrected):
    """int32 n_imu F NK W 0 0 0 0 | imu [n_imu][7] = stamp, acc, gyr | frame_stamps [F] | keyframe_id_in_frame [NK] int32, padded to a multiple of 2 |
    imu_idx_in_kf [NK] int32, padded | keyframe_poses [NK][7] | start_states [NK][15] | corrected [NK][7]"""
    imu = np.ascontiguousarray(imu, np.float64).reshape(-1, 7)
    fs = np.ascontiguousarray(frame_stamps, np.float64)
    kf = np.ascontiguousarray(keyframe_id_in_frame, np.int32)
    idx = np.ascontiguousarray(imu_idx_in_kf, np.int32)
    pad = b"\0\0\0\0" if len(kf) & 1 else b""
    with open(path, "wb") as f:
        f.write(np.array([len(imu), len(fs), len(kf), W, 0, 0, 0, 0], np.int32).tobytes())
        f.write(imu.tobytes()); f.write(fs.tobytes())
        f.write(kf.tobytes() + pad); f.write(idx.tobytes() + pad)
        f.write(np.ascontiguousarray(keyframe_poses, np.float64).reshape(len(kf), 7).tobytes())
        f.write(np.ascontiguousarray(start_states, np.float64).reshape(len(kf), 15).tobytes())
        f.write(np.ascontiguousarray(corrected, np.float64).reshape(len(kf), 7).tobytes())


def run_demo_trajectory(path, device=0, env=None):
    """-> dict(frames [F][7], nodes [n][7], resolved [F][7], calls [(n, gap, n_frames, termination, iterations)], graph [(n, first, last)],
    resolves [(termination, iterations)])"""
    r = subprocess.run([build_demo_trajectory(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_trajectory failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    rows = {"frame": [], "node": [], "resolved": []}
    calls, graph, resolves = [], [], []
    for ln in r.stdout.splitlines():
        w = ln.split()
        if not w:
            continue
        if w[0] in rows:
            rows[w[0]].append([float.fromhex(x) for x in w[2:9]])
        elif w[0] == "call":
            calls.append((int(w[1]), int(w[3]), int(w[5]), int(w[7]), int(w[9])))
        elif w[0] == "graph":
            graph.append((int(w[1]), int(w[3]), int(w[5])))
        elif w[0] == "resolve":
            resolves.append((int(w[3]), int(w[5])))
    return dict(frames=np.array(rows["frame"]), nodes=np.array(rows["node"]), resolved=np.array(rows["resolved"]), calls=calls, graph=graph, resolves=resolves)


DEMO_BATCH_COV = os.path.join(HERE, "host_demo_batch_cov")


def build_demo_batch_cov(force=False):
    """The C++ per-keyframe covariance of the batch stage (host_demo_batch_cov.cpp over glio::BatchBackend::covariance)."""
    src = [os.path.join(HERE, "host_demo_batch_cov.cpp"), os.path.join(HERE, "glio_batch_backend.hpp"), os.path.join(HERE, "..", "..", "include", "glio_batch_cov.h")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_BATCH_COV) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_BATCH_COV) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_BATCH_COV])
    return DEMO_BATCH_COV


def write_batch_cov_case(path, K, band, anchor, cross, poses, speed_bias, con, dq, frame, dd, imu, gravity):
    """the case file of host_demo_batch_cov.cpp (layout in its header); imu: a list of dicts of synth.preintegrate or GlioPreint, or None"""
    import ctypes as C
    from .. import ctypes_types as T
    from .. import synth
    ci, cj, cp, nc, score = con
    nc = np.ascontiguousarray(nc, np.float64)
    imu = list(imu or [])
    with open(path, "wb") as f:
        f.write(np.array([K, band, anchor, 1 if cross else 0, len(dq[0]), len(dd), len(imu), nc.size // max(len(ci), 1)], np.int32).tobytes())
        f.write(np.array([len(ci)], np.int64).tobytes())
        f.write(np.ascontiguousarray(poses, np.float64).tobytes())
        if imu:
            f.write(np.ascontiguousarray(speed_bias, np.float64).tobytes())
        f.write(np.ascontiguousarray(ci, np.int32).tobytes()); f.write(np.ascontiguousarray(cj, np.int32).tobytes())
        f.write(np.ascontiguousarray(cp, np.float32).tobytes()); f.write(nc.tobytes()); f.write(np.ascontiguousarray(score, np.float64).tobytes())
        f.write(np.ascontiguousarray(dq[0], np.int32).tobytes()); f.write(np.ascontiguousarray(dq[1], np.int32).tobytes()); f.write(np.ascontiguousarray(dq[2], np.float64).tobytes())
        f.write(bytes(frame))
        for d in dd:
            f.write(C.string_at(C.addressof(d), C.sizeof(d)))
        for d in imu:
            if not isinstance(d, T.GlioPreint):
                r = T.GlioPreint(); synth.fill_preint(r, d); d = r
            f.write(C.string_at(C.addressof(d), C.sizeof(d)))
        f.write(np.array([gravity], np.float64).tobytes())


def run_demo_batch_cov(path, device=0, env=None):
    """-> dict(diag, next (when asked), info: the result's bytes; B, levels, bad_keyframe)"""
    r = subprocess.run([build_demo_batch_cov(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_batch_cov failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if len(w) == 2 and w[0] in ("diag", "next", "info"):
            out[w[0]] = bytes.fromhex(w[1])
        elif w[:1] == ["B"]:
            out.update({w[i]: int(w[i + 1]) for i in range(0, len(w) - 1, 2)})
    return out


DEMO_POSE_GRAPH_COV = os.path.join(HERE, "host_demo_pose_graph_cov")


def build_demo_pose_graph_cov(force=False):
    """The C++ covariance of every pose-graph node (host_demo_pose_graph_cov.cpp over glio::PoseGraph::marginalCovariances)."""
    src = [os.path.join(HERE, "host_demo_pose_graph_cov.cpp"), os.path.join(HERE, "glio_posegraph_backend.hpp"),
           os.path.join(HERE, "..", "..", "include", "glio_pgraph_cov.h")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_POSE_GRAPH_COV) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_POSE_GRAPH_COV) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_POSE_GRAPH_COV])
    return DEMO_POSE_GRAPH_COV


def write_pose_graph_cov_case(path, poses, loops, gps, segment_nodes, prior=True, solve=True):
    """the case file of host_demo_pose_graph_cov.cpp (layout in its header); loops: (i, j, rel [7], var [6]); gps: (node, xyz [3], var [3])"""
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    with open(path, "wb") as f:
        f.write(np.array([len(P), len(loops), len(gps), segment_nodes, 1 if prior else 0, 1 if solve else 0, 0, 0], np.int32).tobytes())
        f.write(P.tobytes())
        for i, j, rel, var in loops:
            f.write(np.array([float(i), float(j), *rel, *var], np.float64).tobytes())
        for node, xyz, v in gps:
            f.write(np.array([float(node), *xyz, *v], np.float64).tobytes())


def run_demo_pose_graph_cov(path, device=0, env=None):
    """-> dict(diag, next, info: the result's bytes; nodes, separators, full_row_separators, bad_node)"""
    r = subprocess.run([build_demo_pose_graph_cov(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_pose_graph_cov failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[:1] == ["nodes"]:
            out.update({w[i]: int(w[i + 1]) for i in range(0, len(w) - 1, 2)})
        elif w and w[0] in ("diag", "next", "info"):
            out[w[0]] = bytes.fromhex(w[1]) if len(w) > 1 else b""
    return out


DEMO_ALIGN = os.path.join(HERE, "host_demo_align")


def build_demo_align(force=False):
    """The C++ GNSS frame estimate (host_demo_align.cpp over glio::GnssAlignment, glio_align_backend.hpp)."""
    src = [os.path.join(HERE, "host_demo_align.cpp"), os.path.join(HERE, "glio_align_backend.hpp"), os.path.join(HERE, "..", "..", "include", "glio_align.h")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_ALIGN) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_ALIGN) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_ALIGN])
    return DEMO_ALIGN


def write_align_case(path, opts, start, dd, positions):
    """int32 n_dd n_pos stride 0 | glio_align_opts | glio_gnss_frame start | glio_dd_psr [n_dd] | double positions [n_pos][stride]"""
    import ctypes as C
    pos = np.ascontiguousarray(positions, np.float64)
    with open(path, "wb") as f:
        f.write(np.array([len(dd), pos.shape[0], pos.shape[1], 0], np.int32).tobytes())
        f.write(bytes(opts)); f.write(bytes(start))
        for d in dd:
            f.write(C.string_at(C.addressof(d), C.sizeof(d)))
        f.write(pos.tobytes())


def run_demo_align(path, device=0, env=None):
    """-> dict(frame, info, coarse, cost: the result's bytes; status, rows, downweighted)"""
    r = subprocess.run([build_demo_align(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_align failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if len(w) == 2 and w[0] in ("frame", "info", "coarse", "cost"):
            out[w[0]] = bytes.fromhex(w[1])
        elif w and w[0] == "status":
            out.update(status=int(w[1]), rows=int(w[3]), downweighted=int(w[5]))
    return out


DEMO_PLACE = os.path.join(HERE, "host_demo_place")


def build_demo_place(force=False):
    """The C++ place recognition (host_demo_place.cpp over glio::PlaceRecognition, glio_place_backend.hpp)."""
    src = [os.path.join(HERE, "host_demo_place.cpp"), os.path.join(HERE, "glio_place_backend.hpp"), os.path.join(HERE, "..", "..", "include", "glio_place.h")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_PLACE) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_PLACE) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_PLACE])
    return DEMO_PLACE


def write_place_case(path, opts, cap, top_k, min_time_gap, clouds, times, attitudes, pose_closest):
    """int32 K cap top_k 0 | glio_place_opts | double min_time_gap | K x (n, cloud) | double times[K] | double attitude[K][4] | double pose_closest[7]"""
    K = len(clouds)
    times, att = np.ascontiguousarray(times, np.float64), np.ascontiguousarray(attitudes, np.float64)
    assert times.shape == (K,) and att.shape == (K, 4)
    with open(path, "wb") as f:
        f.write(np.array([K, cap, top_k, 0], np.int32).tobytes())
        f.write(bytes(opts)); f.write(np.array([min_time_gap], np.float64).tobytes())
        for c in clouds:
            c = np.ascontiguousarray(c, np.float32).reshape(-1, 4)
            f.write(np.array([len(c)], np.int32).tobytes()); f.write(c.tobytes())
        f.write(times.tobytes()); f.write(att.tobytes()); f.write(np.ascontiguousarray(pose_closest, np.float64).reshape(7).tobytes())


def run_demo_place(path, device=0, env=None):
    """-> dict(name: the bytes host_demo_place printed under that name; candidate: int; mask<k>: int)"""
    r = subprocess.run([build_demo_place(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_place failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if not w:
            continue
        if w[0] == "candidate":
            out["candidate"] = int(w[1])
        elif w[0].startswith("mask"):
            out[w[0]] = int(w[1], 16)
        else:
            out[w[0]] = bytes.fromhex(w[1]) if len(w) > 1 else b""
    return out


DEMO_STATIC_MAP = os.path.join(HERE, "host_demo_static_map")


def build_demo_static_map(force=False):
    """The C++ static map (host_demo_static_map.cpp over glio::StaticClouds, glio_static_backend.hpp, and glio::GlobalMap on it)."""
    src = [os.path.join(HERE, "host_demo_static_map.cpp"), os.path.join(HERE, "glio_static_backend.hpp"), os.path.join(HERE, "glio_map_backend.hpp"),
           os.path.join(HERE, "..", "..", "include", "glio_static.h"), os.path.join(HERE, "..", "..", "include", "glio_dense.h")] + _ABI_HEADERS
    if force or not os.path.exists(DEMO_STATIC_MAP) or any(os.path.getmtime(s) > os.path.getmtime(DEMO_STATIC_MAP) for s in src):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", src[0], "-I" + os.path.join(HERE, "..", "..", "include"),
                               "-L" + os.path.join(HERE, "..", "lib"), "-lglio_hip", "-Wl,-rpath,$ORIGIN/../lib", "-o", DEMO_STATIC_MAP])
    return DEMO_STATIC_MAP


def write_static_map_case(path, opts, gmap_opts, cap, half_window, min_baseline, clouds, poses):
    """int32 K cap half_window 0 | glio_static_opts | glio_gmap_opts | double min_baseline | K x (n, cloud) | double poses[K][7]"""
    K = len(clouds)
    poses = np.ascontiguousarray(poses, np.float64)
    assert poses.shape == (K, 7)
    with open(path, "wb") as f:
        f.write(np.array([K, cap, half_window, 0], np.int32).tobytes())
        f.write(bytes(opts)); f.write(bytes(gmap_opts)); f.write(np.array([min_baseline], np.float64).tobytes())
        for c in clouds:
            c = np.ascontiguousarray(c, np.float32).reshape(-1, 4)
            f.write(np.array([len(c)], np.int32).tobytes()); f.write(c.tobytes())
        f.write(poses.tobytes())


def run_demo_static_map(path, device=0, env=None):
    """-> dict(name: the bytes host_demo_static_map printed under that name)"""
    r = subprocess.run([build_demo_static_map(), path, str(device)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("host_demo_static_map failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w:
            out[w[0]] = bytes.fromhex(w[1]) if len(w) > 1 else b""
    return out
