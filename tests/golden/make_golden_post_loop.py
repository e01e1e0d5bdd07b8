"""Generates tests/golden/post_loop_marg.npz: the windows after a loop closure as THE REFERENCE'S OWN MarginalizationInfo sees them
(oracle/_ref/libglio_ref.so, the reference's MarginalizationFactor.cpp compiled unmodified; recipe oracle/ref_shim/Makefile).  For W = 2 .. 5 the
scenario of tests/marg_layout_restated.py: the first window carries SpeedBiasPriorFactorAutoDiff on slots 0 .. W-2 (as a synthetic prior, which is the
same residual and Jacobian) and no marginalization prior; every later window takes the reference's own output as its prior.  The reference tree does not
exist on the GPU box, so these vectors are how it travels there.

    python tests/golden/make_golden_post_loop.py      # needs the reference tree; rewrites post_loop_marg.npz

Per window `W{W}_k{k}_*`: start / solved state (the oracle's solve), then the reference's result with its columns in the kept layout's order: n, lin_jac,
lin_res, blk_slot, blk_kind, blk_idx, blk_x0."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

FIELDS = ("n", "lin_jac", "lin_res", "blk_slot", "blk_kind", "blk_idx", "blk_x0")


def generate():
    import marg_layout_restated as mr
    from oracle import pyoracle as po
    out = {}
    for W in sorted(mr.SHAPES):
        win, corr = mr.scenario_window(W)
        prob = po.Problem(win, corr, use_gnss=False, use_prior=False)
        rows = mr.run_transient(win, corr, lambda st, pr, ns: mr.canonical(mr.reference_marginalize(win, prob, st, pr), W))
        for k, (start, sol, summ, _, res) in enumerate(rows):
            p = "W%d_k%d_" % (W, k)
            for name, st in (("start", start), ("sol", sol)):
                out[p + name + "_trans"], out[p + name + "_quat"], out[p + name + "_sb"] = st.trans.copy(), st.quat.copy(), st.speed_bias.copy()
            out[p + "iterations"] = np.int32(summ.iterations)
            for f in FIELDS:
                out[p + f] = np.asarray(res[f])
    return out


def load(path=None):
    return dict(np.load(path or os.path.join(HERE, "post_loop_marg.npz")))


def prior_of(G, W, k):
    p = "W%d_k%d_" % (W, k)
    d = {f: G[p + f] for f in FIELDS}
    d["n"] = int(d["n"])
    d["lin_jac"] = np.ascontiguousarray(d["lin_jac"]); d["blk_x0"] = np.ascontiguousarray(d["blk_x0"])
    d["S"] = d["lin_jac"].T @ d["lin_jac"]; d["bs"] = d["lin_jac"].T @ d["lin_res"]
    return d


def state_of(G, W, k, which, like):
    p = "W%d_k%d_%s_" % (W, k, which)
    st = like.copy()
    st.trans[:], st.quat[:], st.speed_bias[:] = G[p + "trans"], G[p + "quat"], G[p + "sb"]
    st.n_ddt = 0
    return st


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(os.path.join(HERE, "post_loop_marg.npz"), **data)
    print("wrote post_loop_marg.npz:", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "post_loop_marg.npz")), "bytes")
