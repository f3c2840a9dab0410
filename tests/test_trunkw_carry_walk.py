"""CPU test of trunkw_kernel's step lists under the producers' CARRY (csrc/uva_wino.hip.h kloop_carry): the lists are the ones
tests/test_trunkw_schedule.py walks with the six-row A-ring, unchanged; here every workgroup's list is walked the way the
kernel with the carry does -- a FOUR-row A-ring that holds only a step's new input rows, six accumulator rows per step of which
rows 0 and 1 go on from what the step above left in rows 4 and 5 -- with row identities in place of pixel data.  An intermediate
row counts as valid only if its sum is made of exactly its three input rows of its own strip IN ORDER (dy = 0, 1, 2: the order
that makes the fp32 sums the bits of the six-row k-loop); every stored output row must come from three valid intermediate rows,
every plane pixel must be stored exactly once.  A segment start hands on whatever the segment above left (garbage), a
workgroup's first step either nothing or, with entry bit 25, the sums of the two extra rows (carry_in)."""
import numpy as np
import pytest

from test_trunkw_schedule import BROWS, SW, locate, schedule


@pytest.mark.parametrize("h,w,tile,border", [
    (1080, 1920, 960, 10), (1080, 1920, 0, 0), (24, 40, 0, 0), (70, 75, 32, 10), (5, 3, 0, 0), (131, 61, 64, 10), (1, 1, 0, 0),
    (96, 128, 64, 10), (256, 256, 32, 10), (200, 70, 0, 0), (13, 124, 62, 10)] + [(hh, 61, 0, 0) for hh in (1, 2, 3, 4, 5, 7, 8, 9, 13)])
@pytest.mark.parametrize("six", [0, 1, -1])
def test_walking_the_lists_with_carried_sums(uva, h, w, tile, border, six, monkeypatch):
    if six >= 0:
        monkeypatch.setenv("UVA_TW_SIX", str(six))
    else:
        monkeypatch.delenv("UVA_TW_SIX", raising=False)
    steps, nsteps, planes, guard = schedule(uva, h, w, tile, border)
    cover = [np.zeros((int(p[0]), int(p[1])), np.int32) for p in planes]
    for b in range(steps.shape[0]):
        n = int(nsteps[b])
        dec = []
        for g in range(n):
            a, bb = steps[b, g, :4], steps[b, g, 4:]
            fold = (int(a[1]) >> 27) & 1
            pi = int(a[2]) >> 24 if fold else int(a[3])
            pi2 = -1
            if fold:
                delta = int(np.uint32(a[3])) + 2048
                pi2 = [j for j in range(len(planes)) if int(planes[j, 3]) == int(planes[pi, 3]) + delta // 128][0]
            row, col = locate(int(a[0]) | ((int(a[1]) & 0xff) << 32), planes, guard, pi)
            dec.append((pi, row - 2, col + 1, bb, (int(a[1]) >> 25) & 1, pi2))
        aring = [None] * 4
        bring = [None] * BROWS
        carry = [[], []]                 # the sums handed down: rows 4 and 5 of the step above, as lists of input rows
        b10 = 0

        def put_rows(g):
            pi, yA, x0 = dec[g][:3]
            for wv in range(4):
                aring[wv] = (pi, x0, yA + 1 + wv)
        if n:
            put_rows(0)
            pi, yA, x0, _, six_rows, _ = dec[0]
            if six_rows:                 # carry_in: window rows 0 and 1 feed rows 0 (dy = 0, 1) and 1 (dy = 0)
                carry = [[(pi, x0, yA - 1), (pi, x0, yA)], [(pi, x0, yA)]]
        for it in range(n + 1):
            if it < n:
                pi, yA, x0 = dec[it][:3]
                ph = int(planes[pi, 0])
                acc = [list(carry[0]), list(carry[1]), None, None, None, None]
                for r in range(4):       # fragment row r = window row R: rows n = R - dy; dy = 0 starts a sum afresh
                    for nn in range(6):
                        dy = r + 2 - nn
                        if dy == 0:
                            acc[nn] = [aring[r]]
                        elif 0 < dy <= 2:
                            acc[nn].append(aring[r])
                for nn in range(4):
                    valid = acc[nn] == [(pi, x0, yA + nn - 1 + d) for d in range(3)]
                    inside = 0 <= yA + nn < ph
                    bring[(b10 + nn) % BROWS] = (pi, x0, yA + nn, valid or not inside)
                assert len(acc[4]) == 2 and len(acc[5]) == 1
                carry = [acc[4], acc[5]]
                if it + 1 < n:
                    put_rows(it + 1)
            if 1 <= it <= n:
                pi, yA, x0, bb, _, pi2 = dec[it - 1]
                if (int(bb[1]) >> 24) & 1:
                    pw = int(planes[pi, 1])
                    vy, vx, v0 = (int(bb[1]) >> 8) & 7, (int(bb[1]) >> 11) & 63, (int(bb[1]) >> 17) & 7
                    assert vx == min(SW, pw - x0)
                    yo = yA - 1
                    bp = (b10 - 4 - 2) % BROWS
                    win = [bring[(bp + r) % BROWS] for r in range(6)]
                    for nn in range(v0, vy):
                        for d in range(3):
                            e = win[nn + d]
                            assert e is not None and e[:3] == (pi, x0, yo + nn - 1 + d) and e[3], (b, it, nn, d, e)
                    cover[pi][yo + v0:yo + vy, x0:x0 + vx] += 1
                    if pi2 >= 0:
                        cover[pi2][yo + v0:yo + vy, x0:x0 + vx] += 1
            b10 = (b10 + 4) % BROWS
    for c in cover:
        assert c.min() == 1 and c.max() == 1
