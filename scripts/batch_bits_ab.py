"""Bits of the batch stage, for A/B runs of two builds of the library (GLIO_HIP_LIB selects one; a fresh process per build): one sha256 per case over
every byte the stage hands back -- Hg of a linearisation, the poses and the model decrease of a step, poses / speed-bias / summary of a trust-region
solve.  Two builds that compute the same print the same lines.
Linearisation: K = 14, band 3, a pair list whose pairs hold 1, 63, 64, 65, 129 records and one pair none (lanes past the end, the prefetch's re-read
on the last trip, two and three trips), through the sorted index arrays (glio_batch_set_constraints_dev) and through the pair list; streamed (mode 0),
by moments (1), moments evaluated at moved poses (2); again after update_constraints_pairs with two pairs marked changed; again with explicit record
offsets that leave gaps.
Pose solve (step): (K, band) = (37, 3) -- 36 x 36 nodes, ragged last super-block -- and (50, 12) -- 72 x 72 -- under set_solver(1) and (0).
Trust-region solve with the IMU chain (12 iterations, per_kf 100): band 6 at K = 13 on one rank and K = 43 on three virtual ranks; band 12 (the
reference's end windows) at K = 50 on one rank and on two.
GLIO_BCR_ELIM is read when the library loads: run the script once per value (unset, 0, 1); BB_ONLY=solve leaves the linearisation cases out (they do
not depend on it).
    GLIO_HIP_LIB=<library> [GLIO_BCR_ELIM=0|1] [BB_ONLY=solve] python scripts/batch_bits_ab.py > bits.txt"""
import ctypes as C, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from glio_amd import batch, capi
from glio_amd import ctypes_types as T
lib = capi.load()
elim = os.environ.get("GLIO_BCR_ELIM", "unset")


def sha(*parts):
    m = hashlib.sha256()
    for p in parts:
        m.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return m.hexdigest()[:16]


def summary_bytes(s):
    return json.dumps(sorted((k, repr(v)) for k, v in s.as_dict().items())).encode()


# ------------------------------------------------------------------ linearisation
def pool(K, band, seed):
    """every pair of the band with at least 129 records to choose from"""
    gt, init = batch.make_poses(K, seed=seed)
    ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 150 * 2 * band, band, seed=seed, device="cuda:0")
    return gt, init, ci, cj, cp, nc, score


def pick(ci, cj, counts, from_end=()):
    """record indices of a pair-major selection: the first counts[p] records of pair p (the last ones for the pairs in `from_end`)"""
    key = ci.astype(np.int64) * 1000 + cj
    pairs = np.unique(key)
    assert len(pairs) == len(counts)
    idx = []
    for p, (k, c) in enumerate(zip(pairs, counts)):
        own = np.nonzero(key == k)[0]
        assert len(own) >= c
        idx.append(own[len(own) - c:] if p in from_end else own[:c])
    return (pairs // 1000).astype(np.int32), (pairs % 1000).astype(np.int32), np.concatenate(idx)


def linearisation_cases():
    K, band = 14, 3
    gt, init, ci, cj, cp, nc, score = pool(K, band, 17)
    npairs = len(np.unique(ci.astype(np.int64) * 1000 + cj))
    counts = np.array([(1, 63, 64, 65, 129, 0)[p] if p < 6 else 3 + (7 * p) % 70 for p in range(npairs)], np.int64)
    pci, pcj, idx = pick(ci, cj, counts)
    sel = torch.as_tensor(idx, device="cuda:0")
    rcp, rnc, rsc = cp[sel].contiguous(), nc[sel].contiguous(), score[sel].contiguous()
    st = batch.BatchStage(K, band, len(idx))
    Hg = st.new_hg()

    def modes(tag):
        st.linearize_mode(init, Hg, 0); h0 = sha(Hg.cpu().numpy())
        st.linearize_mode(init, Hg, 1); h1 = sha(Hg.cpu().numpy())
        st.linearize_mode(gt, Hg, 2); h2 = sha(Hg.cpu().numpy())
        print("linearise K14 band3 %s streamed / moments / moments at moved poses: %s %s %s" % (tag, h0, h1, h2))

    st.set_constraints(ci[idx], cj[idx], rcp, rnc, rsc)           # the sorted index arrays (the empty pair does not appear)
    st.linearize(init, Hg)
    print("linearise K14 band3 index arrays, linearize: %s" % sha(Hg.cpu().numpy()))
    modes("index arrays")
    st.set_constraints_pairs(pci, pcj, counts, rcp, rnc, rsc)
    modes("pair list")
    # two pairs replaced (other records, same counts), marked changed: the moments of the others are kept
    _, _, idx2 = pick(ci, cj, counts, from_end=(2, 9))
    sel2 = torch.as_tensor(idx2, device="cuda:0")
    ucp, unc, usc = cp[sel2].contiguous(), nc[sel2].contiguous(), score[sel2].contiguous()
    changed = np.zeros(npairs, np.uint8); changed[[2, 9]] = 1
    st.set_constraints_pairs(pci, pcj, counts, ucp, unc, usc, changed=changed)
    modes("two pairs changed")
    # explicit record offsets with gaps (glio_batch_update_constraints_pairs_at_dev)
    gaps = np.array([5 + 3 * (p % 4) for p in range(npairs)], np.int64)
    offs = np.cumsum(counts + gaps) - counts
    total = int(offs[-1] + counts[-1] + 8)
    gcp = torch.zeros(total, 4, dtype=torch.float32, device="cuda:0"); gnc = torch.zeros(total, 6, dtype=torch.float64, device="cuda:0")
    gsc = torch.zeros(total, dtype=torch.float64, device="cuda:0")
    run = 0
    for p in range(npairs):
        c = int(counts[p]); o = int(offs[p])
        gcp[o:o + c] = ucp[run:run + c]; gnc[o:o + c] = unc[run:run + c]; gsc[o:o + c] = usc[run:run + c]
        run += c
    torch.cuda.synchronize()
    st._keep = (gcp, gnc, gsc)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    offs = np.ascontiguousarray(offs, np.int64)
    capi._check(lib.glio_batch_update_constraints_pairs_at_dev(st._h, npairs, T.iptr(pci), T.iptr(pcj), i64(counts), i64(offs), C.c_void_p(gcp.data_ptr()),
                                                               C.c_void_p(gnc.data_ptr()), C.c_void_p(gsc.data_ptr()), None))
    modes("record offsets with gaps")
    st.close()


# ------------------------------------------------------------------ pose solve
def step_cases():
    for K, band in ((37, 3), (50, 12)):
        gt, init = batch.make_poses(K, seed=21 + K)
        ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 200, band, seed=21 + K, device="cuda:0")
        st = batch.BatchStage(K, band, len(ci))
        st.set_constraints(ci, cj, cp, nc, score)
        Hg = st.new_hg()
        st.linearize(init, Hg)
        out = []
        for mode in (1, 0):
            st.set_solver(mode)
            new, m = st.step(Hg, 1e-4, init)
            out.append(sha(new, np.float64(m)))
        st.close()
        print("step K%d band%d elim %s block cyclic reduction / sequential: %s %s" % (K, band, elim, out[0], out[1]))


# ------------------------------------------------------------------ trust-region solve with the IMU chain
def solve_on(K, band, world, con, dq, dd, frame, imu, init, sb0):
    from test_hip_batch_tr import _stage
    opts = T.batch_tr_opts(max_iterations=12)
    if world == 1:
        st = _stage(K, band, con, dq, dd, frame, imu=imu)
        res = [st.solve_tr(init, opts, speed_bias=sb0)]
        st.close()
    else:
        stages = [_stage(K, band, con, dq, dd, frame, imu=imu, rank=r, world=world) for r in range(world)]
        ranks = batch.ThreadRanks(world, sync=torch.cuda.synchronize)
        res = ranks.run(lambda r, d: stages[r].solve_tr(init, opts, d, speed_bias=sb0))
        for s_ in stages:
            s_.close()
    return " ".join(sha(p, sb, summary_bytes(sm)) for p, sb, sm in res), res[0][2].iterations


def tr_cases():
    from test_hip_batch_tr import _imu_problem
    for K, world in ((13, 1), (43, 3)):
        gt, init, con, dq, dd, frame, imu, sb0 = _imu_problem(K, 6, per_kf=100, seed=59)
        h, it = solve_on(K, 6, world, con, dq, dd, frame, imu, init, sb0)
        print("solve_tr K%d band6 ranks %d elim %s iterations %d: %s" % (K, world, elim, it, h))
    for K, world in ((50, 1), (50, 2)):
        band, sr = 12, 6
        gt, init = batch.make_poses(K, seed=77 + K, perturb=(0.08, 0.004))
        ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 100, band, seed=77 + K, search_range=sr)
        con = (ci, cj, cp.numpy(), nc.numpy(), score.numpy())
        rng = np.random.default_rng(77 + K)
        odo = gt.copy(); odo[:, :3] += rng.normal(0, 0.02, (K, 3))
        dq = batch.delta_q_pairs(odo, sr)
        dd, frame = batch.make_batch_gnss(gt, seed=77 + K)
        for f in dd:
            f.threshold = 10.0
        imu, _, sb0 = batch.make_batch_imu(K, seed=77 + K)
        h, it = solve_on(K, band, world, con, dq, dd, frame, imu, init, sb0)
        print("solve_tr K%d band12 ranks %d elim %s iterations %d: %s" % (K, world, elim, it, h))


if os.environ.get("BB_ONLY") != "solve":
    linearisation_cases()
step_cases()
tr_cases()
