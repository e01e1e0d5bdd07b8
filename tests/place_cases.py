"""The query cases of tests/test_hip_place.py, built and vetted on the CPU with the restatement (tests/place_restated.py): banks of host descriptors that go
into the device store with glio_place_set_descriptor, and the check that every argmin over shifts and every rank the tests look at is separated by more than
twice the gate -- so that shift and place are exact and only the distance carries a tolerance."""
import numpy as np

import place_restated as R

EPS32 = 2.0 ** -24                     # float32's unit roundoff
GATE = 64 * EPS32                      # 3.8e-6 absolute, on distances: a 20-term dot product of unit float vectors, two normalisations and a mean of <= 60 terms
#                                        are bounded by about 30 eps; the gate doubles that
LARGEST = {"deviation": 0.0}           # the largest |device - restated| distance the GPU tests have compared so far (they print it)


def within_gate(device_distance, restated_distance):
    """notes the deviation, then holds it to the gate"""
    dev = abs(float(device_distance) - float(restated_distance))
    LARGEST["deviation"] = max(LARGEST["deviation"], dev)
    return dev <= GATE
RUN = 16                               # candidates per wavefront of the pair kernel: the banks have sizes on both sides of it and of twice it


def random_descriptor(rng, absent=0):
    """heights uniform in [0, 6) with `absent` columns without a point (their heights zero, as the device writes them)"""
    h = rng.uniform(0.0, 6.0, (R.RINGS, R.SECTORS)).astype(np.float32)
    mask = R.MASK60
    for j in rng.choice(R.SECTORS, absent, replace=False):
        h[:, j] = 0
        mask &= ~(1 << int(j))
    return h, mask


def revisit(rng, h, mask, k, noise=0.8):
    """the place seen again with the sensor turned: columns rolled by k, heights disturbed"""
    h2 = np.roll(h, k, axis=1) + rng.uniform(-noise, noise, h.shape).astype(np.float32)
    h2 = np.where(np.roll(h, k, axis=1) == 0, np.float32(0), h2).astype(np.float32)
    return h2, R.rotated_mask(mask, (R.SECTORS - k) % R.SECTORS)


def bank(n_places, seed, gaps=()):
    """[(place, heights, mask, time)]: n_places descriptors at consecutive indices except that the indices in `gaps` are left out (invalid slots between valid
    ones).  A third of the bank are revisits of the entry two before them at shifts that include 0 and 59; some have absent columns; one is all-absent."""
    rng = np.random.default_rng(seed)
    out, idx, shifts = [], 0, [0, 59, 1, 30, 17, 44]
    while len(out) < n_places:
        if idx in gaps:
            idx += 1
            continue
        i = len(out)
        if i >= 3 and i % 3 == 0:
            src = out[i - 2]
            h, m = revisit(rng, src[1], src[2], shifts[(i // 3) % len(shifts)])
        elif i == 5:
            h, m = np.zeros((R.RINGS, R.SECTORS), np.float32), 0             # all-absent: distance exactly 1 to everything
        else:
            h, m = random_descriptor(rng, absent=(0, 7, 25)[i % 3])
        out.append((idx, h, m, float(idx)))
        idx += 1
    return out


def restated_store(entries, n_slots):
    st = R.Store(n_slots)
    for place, h, m, t in entries:
        st.set(place, h, m, t)
    return st


def separated(st, q, min_time_gap, top_k, earlier_only=False):
    """True when, for query q, every candidate's argmin over shifts and the first top_k + 1 ranks are more than 2 GATE apart (the all-absent place, whose 60
    shifts tie at exactly 1 by rule, is exempt from the shift check)"""
    uq, pq, _ = st.places[q]
    ds = []
    for c in st.candidates(q, min_time_gap, earlier_only):
        d = np.sort(R.shift_distances(uq, pq, st.places[c][0], st.places[c][1]).astype(np.float64))
        if not (pq == 0 or st.places[c][1] == 0) and not d[1] - d[0] > 2 * GATE:
            return False
        ds.append(d[0])
    ds = np.sort(np.array(ds))[:top_k + 1]
    return bool(np.all(np.diff(ds) > 2 * GATE))
