"""The host arithmetic of the window context (glio_amd/csrc/window_tables.h) as a program of its own (glio_amd/host/host_window_tables_test.cpp),
built by a plain host compiler twice -- as it is, and with the address and undefined-behaviour sanitizers -- and run as a program.  Every expected
value below is stated here, in Python, not taken from the header: the GNSS tables from `sorted` + `itertools.groupby`, the kept layouts from
tests/marg_layout_restated.py, the arena's offsets as numbers.

One refusal of glio_set_gnss has no case: "more than W^2 groups".  A group is a distinct (slot_i, slot_j) with both slots in [0, W) and
slot_i != slot_j -- anything else is a bad factor -- so there are at most W (W - 1) of them; the check cannot fire behind the validation."""
import itertools
import os
import random
import subprocess

import pytest

import marg_layout_restated as mr
from glio_amd import ctypes_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "glio_amd", "host", "host_window_tables_test.cpp")
MAX_WINDOW = 64          # GLIO_MAX_WINDOW
E_ARG, E_STATE = -1, -3
OFF = {T.BLK_TRANS: 0, T.BLK_QUAT: 3, T.BLK_SPEEDBIAS: 6}
SIZE = {T.BLK_TRANS: 3, T.BLK_QUAT: 3, T.BLK_SPEEDBIAS: 9}


# ------------------------------------------------------------------------------------------------ the cases: (script, expected output lines)
def ints(name, v):
    return (name + " " + " ".join(str(int(x)) for x in v)).rstrip() if len(v) else name


def gnss_script(W, nmax, dd, dop):
    return "\n".join([f"gnss {W} {nmax} {len(dd)} {len(dop)}"] + [" ".join(map(str, f)) for f in dd] + [" ".join(map(str, f)) for f in dop])


def gnss_expect(W, nmax, dd, dop):
    """dd: (slot_i, slot_j, n_sat, master, tag), dop: (slot_i, slot_j, epoch, tag); valid input"""
    key = lambda f: f[0] * W + f[1]
    sdd, sdop = sorted(dd, key=key), sorted(dop, key=lambda f: (key(f), f[2]))          # (sorted is stable)
    keys = sorted(set(map(key, dd)) | set(map(key, dop)))
    dd_rng, dop_rng, runs, run_rng = {}, {}, [], {}
    at = 0
    for k, g in itertools.groupby(sdd, key):
        n = len(list(g)); dd_rng[k] = (at, at + n); at += n
    at = 0
    for (k, ep), g in itertools.groupby(sdop, lambda f: (key(f), f[2])):
        n = len(list(g))
        lo, hi = dop_rng.get(k, (at, at)); dop_rng[k] = (lo, at + n)
        lo, hi = run_rng.get(k, (len(runs), len(runs))); run_rng[k] = (lo, len(runs) + 1)
        runs.append((at, at + n, ep, keys.index(k))); at += n
    groups, a, b, r = [], 0, 0, 0
    for k in keys:          # an absent range is empty at the running position
        d0, d1 = dd_rng.get(k, (a, a)); p0, p1 = dop_rng.get(k, (b, b)); r0, r1 = run_rng.get(k, (r, r))
        groups.append((k // W, k % W, d0, d1, p0, p1, r0, r1)); a, b, r = d1, p1, r1
    es = [(-1, -1)] * max(1, nmax)
    per = [[] for _ in range(W)]
    for (_, _, ep, g) in runs:
        lo, hi = sorted(groups[g][:2]); es[ep] = (lo, hi); per[lo].append(ep); per[hi].append(ep)
    off = [0]
    for p in per:
        off.append(off[-1] + len(p))
    ok = int(all(abs(groups[g][1] - groups[g][0]) == 1 for (_, _, _, g) in runs))
    chain = int(all(g[1] - g[0] == 1 for g in groups))
    return [f"ok {int(sdd != list(dd))} {int(sdop != list(dop))}", ints("groups", [x for g in groups for x in g]), ints("runs", [x for r_ in runs for x in r_]),
            ints("es", [x for s in es for x in s]), ints("off", off), ints("list", [e for p in per for e in p]),
            f"flags {ok} {chain} {max([r_[2] for r_ in runs], default=-1)}", ints("ddorder", [f[4] for f in sdd]), ints("doporder", [f[3] for f in sdop])]


def gnss_cases():
    cases = []
    for W in (2, 3, 5):
        for nmax in (0, 1, 8):
            dd, dop, tag = [], [], 0
            pairs = [(i, i + 1) for i in range(W - 1)]
            for (i, j) in pairs:
                for _ in range(2):
                    dd.append((i, j, 5, 1, tag)); tag += 1
            for ep in range(nmax):          # epoch ep under pair ep % (W - 1): three rows each
                i, j = pairs[ep % len(pairs)]
                for _ in range(3):
                    dop.append((i, j, ep, tag)); tag += 1
            dop.sort(key=lambda f: (f[0] * W + f[1], f[2]))
            sh_dd, sh_dop = dd[:], dop[:]
            random.Random(7).shuffle(sh_dd); random.Random(8).shuffle(sh_dop)
            for a, b in ((dd, dop), (dd[::-1], dop[::-1]), (sh_dd, sh_dop)):
                cases.append((W, nmax, a, b))
            assert gnss_expect(W, nmax, dd, dop)[0] == "ok 0 0"          # the sorted input: nothing copied
    cases += [(3, 4, [], []),                                                                   # empty
              (3, 4, [(0, 1, 2, 0, 0), (1, 2, 20, 19, 1)], []),                               # DD only
              (3, 4, [], [(0, 1, 0, 0), (0, 1, 0, 1), (1, 2, 3, 2)]),                           # Doppler only
              (3, 4, [(2, 1, 4, 0, 0)], [(2, 1, 1, 1)]),                                        # upper keyframe first
              (3, 4, [(0, 2, 4, 0, 0)], [(0, 2, 2, 1), (0, 1, 0, 2)]),                          # a pair that skips a keyframe
              (3, 4, [(0, 1, 4, 0, 0)], [(0, 1, 0, 1), (0, 1, 1, 2), (0, 1, 0, 3), (1, 2, 2, 4)])]   # one epoch in two stretches under one pair: one run, input order kept
    out = [(gnss_script(*c), gnss_expect(*c)) for c in cases]
    # every refusal: code and text
    good = (0, 1, 4, 1, 0)
    for bad in ((-1, 1, 4, 1, 0), (3, 1, 4, 1, 0), (0, -1, 4, 1, 0), (0, 3, 4, 1, 0), (1, 1, 4, 1, 0), (0, 1, 1, 0, 0), (0, 1, 21, 1, 0), (0, 1, 4, -1, 0), (0, 1, 4, 4, 0)):
        out.append((gnss_script(3, 4, [good, bad], []), [f"refused {E_ARG} bad DD factor"]))
    for bad in ((-1, 1, 0, 0), (3, 1, 0, 0), (0, -1, 0, 0), (0, 3, 0, 0), (2, 2, 0, 0), (0, 1, -1, 0), (0, 1, 4, 0)):
        out.append((gnss_script(3, 4, [good], [(0, 1, 0, 0), bad]), [f"refused {E_ARG} bad Doppler factor (epoch {bad[2]}, max_ddt_epochs 4)"]))
    out.append((gnss_script(3, 0, [], [(0, 1, 0, 0)]), [f"refused {E_ARG} bad Doppler factor (epoch 0, max_ddt_epochs 0)"]))
    out.append((gnss_script(3, 4, [], [(0, 1, 2, 0), (1, 2, 2, 1)]), [f"refused {E_ARG} epoch 2 appears under two keyframe pairs"]))
    return out


def blocks_script(head, blocks):
    return "\n".join([head] + [f"{s} {k} {c}" for s, k, c in blocks])


def index_tables(W, n, blocks):
    index, colblk = [-1] * (15 * W), [-1] * n
    for b, (s, k, c) in enumerate(blocks):
        for j in range(SIZE[k]):
            index[15 * s + OFF[k] + j] = c + j; colblk[c + j] = b
    return index, colblk


def installed_prior(W):
    """a prior as an earlier marginalization leaves it, with speed-bias blocks at every odd slot >= 3 before the shift: at slots 2, 4, ... of the window"""
    fake = dict(blk_slot=[s for s in range(3, W) if s % 2 == 1], blk_kind=[T.BLK_SPEEDBIAS] * len([s for s in range(3, W) if s % 2 == 1]))
    blocks, _ = mr.kept_blocks(W, fake, 0)
    return [(s - 1, k, c) for s, k, c in blocks]


def marg_cases():
    out = []
    for W in range(2, MAX_WINDOW + 1):
        np_limit, nb_limit = min(max(6 * W + 9, 15 * (W - 1)), 6 * MAX_WINDOW + 9), min(max(2 * W + 1, 3 * (W - 1)), 2 * MAX_WINDOW + 1)
        for prior in (None, installed_prior(W)):
            pd = dict(blk_slot=[b[0] for b in prior], blk_kind=[b[1] for b in prior]) if prior else None
            if prior:
                assert W < 4 or any(k == T.BLK_SPEEDBIAS and s >= 2 for s, k, _ in prior)
            for sbp_n in range(W):
                kept, n = mr.kept_blocks(W, pd, sbp_n)
                ne = len(mr.extra_slots(W, pd, sbp_n))
                assert n == 6 * (W - 1) + 9 + 9 * ne and len(kept) == 2 * (W - 1) + 1 + ne
                tables = [(s - 1, k, c) for s, k, c in kept]
                x0 = []
                for s, k, _ in kept:
                    vals = {T.BLK_TRANS: [1000 + 3 * s + j for j in range(3)], T.BLK_QUAT: [2000 + 4 * s + j for j in range(4)], T.BLK_SPEEDBIAS: [3000 + 9 * s + j for j in range(9)]}[k]
                    x0 += vals + [0] * (9 - len(vals))
                index, colblk = index_tables(W, n, tables)
                out.append((blocks_script(f"marg {W} {sbp_n} {len(prior) if prior else 0}", prior or []),
                            [f"size {n} {len(kept)} {ne} {int(n <= np_limit and len(kept) <= nb_limit)}", ints("slot", [b[0] for b in tables]), ints("kind", [b[1] for b in tables]),
                             ints("idx", [b[2] for b in tables]), ints("x0", x0), ints("index", index), ints("colblk", colblk)]))
    return out


def prior_cases():
    Tr, Q, SB = T.BLK_TRANS, T.BLK_QUAT, T.BLK_SPEEDBIAS
    out = []
    good = [(0, Tr, 0), (0, Q, 3), (0, SB, 6), (1, Tr, 15), (1, Q, 18)]
    index, colblk = index_tables(2, 21, good)
    out.append((blocks_script("prior 2 21 5", good), ["ok 1 0", ints("index", index), ints("colblk", colblk)]))
    two_sb = [(0, SB, 0), (2, SB, 9)]          # two speed-bias blocks, one beyond slot 1
    index, colblk = index_tables(3, 18, two_sb)
    out.append((blocks_script("prior 3 18 2", two_sb), ["ok 0 1", ints("index", index), ints("colblk", colblk)]))
    for blocks, n, text in (([(0, Tr, 0), (0, 3, 3)], 6, "prior block 1: unknown kind 3"),
                            ([(2, Tr, 0)], 3, "prior block out of range"), ([(-1, Tr, 0)], 3, "prior block out of range"),
                            ([(0, Tr, -1)], 3, "prior block out of range"), ([(0, SB, 0)], 8, "prior block out of range"),
                            ([(0, Tr, 0), (0, Tr, 3)], 6, "prior: two blocks for slot 0 kind 0"),
                            ([(0, Tr, 0), (1, Tr, 2)], 6, "prior: blocks 0 and 1 overlap at column 2"),
                            ([(0, Tr, 0), (1, Tr, 4)], 7, "prior column 3 not covered by a block")):
        out.append((blocks_script(f"prior 2 {n} {len(blocks)}", blocks), [f"refused {E_ARG} {text}"]))
    # chain test: two keyframes with three columns each; J0 = I (+ one entry).  J0^T J0 (a, b) relative to the column norms: eps / sqrt(1 + eps^2)
    def chain(entries):
        J = [[float(i == j) for j in range(6)] for i in range(6)]
        for (i, j), v in entries.items():
            J[i][j] = v
        return blocks_script("chain 6 2", [(0, Tr, 0), (1, Tr, 3)]) + "\n" + " ".join(repr(v) for r in J for v in r)
    out += [(chain({}), ["chain 1"]), (chain({(0, 1): 0.5}), ["chain 1"]),          # block diagonal; a coupling inside one keyframe
            (chain({(0, 3): 2e-13}), ["chain 0"]), (chain({(0, 3): 5e-14}), ["chain 1"])]          # between two keyframes, above and below the 1e-13 of the code
    return out


def stage_cases():
    over = f"refused {E_STATE} upload arena overflow"
    big = 16384 + 4          # STAGE_DIRECT_BYTES + 4
    return [
        # 33 tables of four bytes: the 32nd is accepted, the 33rd refused; every offset a multiple of 64, none below 1024
        ("stage 8192 -1\n" + "up 4\n" * 33 + "end", [f"seg {1024 + 64 * k} 1 {k + 1}" for k in range(32)] + [over, f"used {1024 + 64 * 31 + 4} top 8192 block {1024 + 64 * 34}"]),
        ("stage 8192 -1\nup 6\nup 8\nd2d 6\nend", [over, "seg 1024 1 1", over, "used 1032 top 8192 block 3200"]),
        ("stage 8192 -1\n" + "d2d 8\n" * 33 + "end", [f"d2d {k + 1}" for k in range(32)] + [over, "used 1024 top 8192 block 3200"]),
        # a large table: its own copy from the top of an ordinary block, a segment of an early one
        (f"stage 65536 -1\nup {big}\nup 8\nend", [f"direct {65536 - 16448}", "seg 1024 1 1", f"used 1032 top {65536 - 16448} block 3200"]),
        (f"stage 65536 0\nup {big}\nup 8\nend", ["seg 1024 1 1", f"seg {1024 + 16448} 1 2", f"used {1024 + 16448 + 8} top 65536 block 3200"]),
        # top meeting used, from either side
        ("stage 40000 -1\nup 20000\nup 20000\nup 18960\nup 4\nend", ["direct 19968", over, over, "seg 1024 1 1", "used 1028 top 19968 block 3200"]),
        ("stage 4100 -1\nup 2048\nup 1024\nup 4\nword\nend", ["seg 1024 1 1", "seg 3072 1 2", over, "word none", "used 4096 top 4096 block 3200"]),
        # the result word: on the next 64-byte line behind the last payload
        ("stage 4096 -1\nup 100\nword\nend", ["seg 1024 1 1", "word 1152", "used 1156 top 4096 block 3200"]),
        ("stage 4096 -1\nup 128\nword\nend", ["seg 1024 1 1", "word 1152", "used 1156 top 4096 block 3200"]),
    ]


def imu_cases():
    def cov(diag, offd=0.0):
        return [[diag[i] if i == j else offd * 1e-3 / (1 + abs(i - j)) for j in range(15)] for i in range(15)]
    spd = cov([1e-3 * (k + 1) for k in range(15)], 0.1)
    head = [10, 11, 12, 50, 51, 52, 53, 20, 21, 22, 30, 31, 32, 40, 41, 42, 60]
    jac = [100 + 15 * (r0 + r) + c0 + c for (r0, c0) in ((0, 9), (0, 12), (3, 12), (6, 9), (6, 12)) for r in range(3) for c in range(3)]
    script = lambda slot, m: f"imu {slot}\n" + " ".join(repr(float(v)) for r in m for v in r)
    return [(script(3, spd), ["digest 1", ints("head", head), ints("jac", jac), "slot 3 pad 0 below 0 diag 15"]),
            (script(0, cov([0.0] * 15)), ["digest 0"]),                                                  # singular
            (script(0, cov([1e-3] * 14 + [0.0])), ["digest 0"]),                                         # singular in one direction
            (script(0, cov([1e-3] * 7 + [-1e-3] + [1e-3] * 7)), ["digest 0"])]                           # indefinite


@pytest.fixture(scope="module")
def cases():
    return gnss_cases() + prior_cases() + marg_cases() + stage_cases() + imu_cases()


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_window_tables_program(tmp_path, cases, flags):
    exe = str(tmp_path / "host_window_tables_test")
    subprocess.check_call(["g++", "-std=c++17"] + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], input="\n".join(c[0] for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("--\n")
    assert got[-1] == "" and len(got) == len(cases) + 1
    for (script, want), text in zip(cases, got):
        assert text.splitlines() == want, script[:300]
