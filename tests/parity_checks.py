"""The comparisons the GPU parity tests share: rel_err and assert_pose_parity (H, g, cost per linearisation to 1e-10 relative; poses per solve to
1e-4 m / 1e-5 rad, BASELINE.json north_star) and check_root (what the next window consumes of a marginalization root, 1e-8 relative)."""
import numpy as np

from glio_amd import synth


def rel_err(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def rot_angle(qa, qb):
    d = synth.qmul(synth.qconj(qa), qb)
    return 2 * np.arctan2(np.linalg.norm(d[1:]), abs(d[0]))


def assert_pose_parity(sa, sb, tol_t=1e-4, tol_r=1e-5):
    dt = np.linalg.norm(sa.trans - sb.trans, axis=1).max()
    dr = max(rot_angle(sa.quat[i], sb.quat[i]) for i in range(sa.W))
    assert dt <= tol_t, f"translation parity {dt:.3e} m"
    assert dr <= tol_r, f"rotation parity {dr:.3e} rad"
    return dt, dr


def check_root(out_h, out_o):
    Jh, rh, Jo, ro = out_h["lin_jac"], out_h["lin_res"], out_o["lin_jac"], out_o["lin_res"]
    assert rel_err(Jh.T @ Jh, Jo.T @ Jo) <= 1e-8
    assert rel_err(Jh.T @ rh, Jo.T @ ro) <= 1e-8
    assert abs(rh @ rh - ro @ ro) <= 1e-7 * max(ro @ ro, 1e-30)
    assert np.allclose(Jh, np.triu(Jh)), "Cholesky root is upper triangular"
    for k in ("blk_slot", "blk_kind", "blk_idx"):
        assert np.array_equal(out_h[k], out_o[k])
    assert np.array_equal(out_h["blk_x0"], out_o["blk_x0"])
