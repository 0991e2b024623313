"""CPU: the uniform frame of the packed scan kernels (cudasw4_amd/csrc/sw_dp_kernel.hpp: sw_scan_kernel, dp_step<UNI>) restated
in numpy and checked against the oracle's scalar DP.

A cell of step t of stripe s is kept raised by a*(u + 1 + class), u = t_g mod K, t_g = t + LANES*s (a = -gex): the same
level in every lane of a wave.  The model runs the kernel's schedule — lanes in lock-step on anti-diagonals, R rows per lane
in P row classes, the hand-off to the next lane one step later (F lowered by a*lastClass, row 0's profile entry raised by
a*(2 - lastClass)), stripes that hand their last lane's (H, F) to the next stripe's lane 0 through a border ring without
correction, and the frame lowered by a*K in every lane after the last step of each period — with exact integers, and
reads the best score out of the frame with the wave-uniform levels.  tests/test_gpu_uniform_frame.py checks the kernels."""
import numpy as np
import pytest

import oracle_lib as O

NONE = -(1 << 40)   # F of the head lane (bound_ctrl zero fill): below every level
EMPTY = 0           # a border pair that was never produced: the kind's unraised zero (int16: the bias), the frame's level 0


def uniform_frame_score(q, s, m21, gop, gex, lanes, R, P, K, head_extra=1):
    a = -gex
    gopa = gop + a                      # ScanParams::gop of the OFFS kernels: gop - gex
    last = (R - 1) % P                  # class of a lane's last row
    sub = m21.reshape(-1, 21).astype(np.int64)
    stripe_rows = lanes * R
    ns = max(1, -(-len(q) // stripe_rows))
    qp = np.full(ns * stripe_rows, 20, dtype=np.int64)
    qp[:len(q)] = q
    L = len(s)
    nquads = (L + lanes - 1 + 3) // 4
    T = 4 * nquads
    letters = np.full(T + lanes, 20, dtype=np.int64)
    letters[:L] = s
    r_idx = np.arange(R)
    cls = r_idx % P
    above = np.where(r_idx == 0, R - 1, r_idx - 1) % P
    head = (r_idx == 0).astype(np.int64)
    best = 0
    ring = None                         # (H, F) per column from the stripe above
    for st in range(ns):
        rows = qp[st * stripe_rows:(st + 1) * stripe_rows].reshape(lanes, R)
        prof = sub[rows] + a * (1 + head_extra * head + cls - above)[None, :, None]   # [lane, row, letter]: sw_build_profile_kernel
        u0 = (lanes * st) % K
        H = np.tile(a * (u0 + cls), (lanes, 1))                           # the step before the first: zw[class]
        E = np.tile(a * (u0 + cls + 1), (lanes, 1))                       # the first step's level: zw[class + 1]
        upH_prev = np.full(lanes, a * (u0 - 1 + last))                   # H(row above, column before): two steps back
        Hlast = np.full(lanes, a * (u0 + last))
        Fout = np.full(lanes, a * u0)
        out = np.full((T, 2), EMPTY, dtype=np.int64)
        lane = np.arange(lanes)
        for t in range(T):
            u = (t + lanes * st) % K
            lvl = a * (u + 1 + cls)                                       # zero level of this step's cells, per class
            zop = lvl + a
            j = t - lane                                                  # each lane's column
            if ring is None:
                hH, hF = a * (u + last), NONE                             # local boundary (first_stripe_pairs) / bound_ctrl zero
            else:
                hH, hF = ring[t]
            upH = np.concatenate([[hH], Hlast[:-1]])
            F = np.concatenate([[hF], Fout[:-1]])
            diag = upH_prev
            upH_prev = upH
            lt = letters[np.maximum(j, 0)]
            lt = np.where(j < 0, 20, lt)
            sc = prof[lane, :, lt]                                        # [lane, row]
            Hold = H.copy()
            for r in range(R):
                tv = (diag if r == 0 else Hold[:, r - 1]) + sc[:, r]
                h = np.maximum(np.maximum(tv, E[:, r]), F)
                hg = h + gopa
                fm = np.maximum(np.maximum(F, hg), zop[r])
                E[:, r] = np.maximum(np.maximum(E[:, r], hg), zop[r])
                if r == R - 1:
                    F = fm - a * last
                elif cls[r] == P - 1:
                    F = fm - a * P
                else:
                    F = fm
                H[:, r] = h
                best = max(best, int((h - lvl[r]).max()))
            Hlast = H[:, R - 1].copy()
            Fout = F
            if (t + lanes * st + 1) % K == 0:                             # uniform lowering, before the ring store
                H, E, Hlast, Fout = H - a * K, E - a * K, Hlast - a * K, Fout - a * K
                upH_prev = np.maximum(upH_prev - a * K, EMPTY - a)         # int16: the floor of lane 0's diagonal
            out[t] = (Hlast[-1], Fout[-1])
        # the next stripe's lane 0 takes column j at its step j: what the last lane emitted at step j + lanes - 1
        nxt = np.full((T, 2), EMPTY, dtype=np.int64)
        nxt[:T - (lanes - 1)] = out[lanes - 1:]
        ring = nxt
    return best


def random_case(rng, qlen, slen):
    q = rng.integers(0, 20, qlen).astype(np.int8)
    s = rng.integers(0, 20, slen).astype(np.int8)
    copy = [int(c) for c in q for _ in range(1 if rng.random() > 0.1 else 0)]   # a gapped relative of the query
    for _ in range(3):
        at = int(rng.integers(0, max(1, len(copy))))
        copy[at:at] = rng.integers(0, 20, int(rng.integers(1, 9))).tolist()
    copy = np.array(copy[:slen], dtype=np.int8)
    at = int(rng.integers(0, slen - len(copy) + 1))
    s[at:at + len(copy)] = copy
    return q, s


# (lanes, R, P, K): single- and multi-stripe, 4/8/16/64-lane groups, periods shorter than the subjects (lowering mid-subject,
# inside a border block: a 16-lane block is 32 steps, K = 64 lowers in every second one), odd classes of the last row
SHAPES = [(16, 4, 2, 64), (16, 5, 2, 64), (16, 3, 1, 64), (8, 4, 2, 32), (4, 6, 3, 16), (64, 2, 1, 256), (16, 8, 4, 128)]


@pytest.mark.parametrize("lanes,R,P,K", SHAPES)
@pytest.mark.parametrize("gop,gex", [(-11, -1), (-10, -2), (-5, -5)])
def test_uniform_frame_matches_the_oracle(lanes, R, P, K, gop, gex):
    rng = np.random.default_rng(lanes * 1000 + R * 10 + P + abs(gex))
    m21 = O.blosum21(62)
    stripe = lanes * R
    for qlen, slen in ((stripe - 3, 2 * K + 37), (2 * stripe + 5, K + 5), (3 * stripe, 3 * K // 2 + 1), (5, 4)):
        q, s = random_case(rng, max(1, qlen), max(1, slen))
        chars, offsets, lengths = O.make_db([s])
        want = int(O.scan(q, chars, offsets, lengths, gop=gop, gex=gex)[0])
        assert uniform_frame_score(q, s, m21, gop, gex, lanes, R, P, K) == want, (qlen, slen)


def test_the_column_frame_profile_does_not_fit_the_uniform_frame():
    """row 0's diagonal comes from the previous lane two steps back: without the profile's extra a (head_extra = 0, the
    profile of the column frame) the uniform frame scores wrongly"""
    rng = np.random.default_rng(7)
    m21 = O.blosum21(62)
    differs = 0
    for _ in range(6):
        q, s = random_case(rng, 60, 90)
        chars, offsets, lengths = O.make_db([s])
        want = int(O.scan(q, chars, offsets, lengths)[0])
        assert uniform_frame_score(q, s, m21, -11, -1, 16, 4, 2, 64) == want
        differs += uniform_frame_score(q, s, m21, -11, -1, 16, 4, 2, 64, head_extra=0) != want
    assert differs > 0
