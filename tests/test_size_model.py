"""CPU: the size mode's deal as tests/size_model.py states it, on hand-made tables -- equal q in all chunks, chunks of
one plane, a chunk whose whole stream is under 8 bits, constant chunks, chunks without a plane -- dealt at W around
every breakpoint (the sum of F_c at a candidate threshold, one bit below and above) and in between.

  form       budgets are multiples of 8, at least 8 and at most end_c[0] (the 8-bit floor, one payload byte, stands
             above a shorter stream); 0 for a constant chunk
  fit        the sum is <= W, and > W - 8 #nonconst unless every chunk is coded in full: the rounding to bytes (under 8
             bits a chunk) and the floors of the shares (under a bit a tied chunk, inside the same 8) are all that is lost
  monotone   no chunk's budget falls when W grows
  ties       chunks that share the plane the rest goes to get it in proportion to their planes' sizes
  refusal    W < 8 #nonconst"""
import numpy as np
import pytest

import size_model as sm

TABLES = sm.hand_tables()


def full_depth(table, budgets):
    q, nbp, end, ic = table
    return all(ic[c] or budgets[c] == max(8, (int(end[c][0]) // 8) * 8 if nbp[c] > 0 else 0) for c in range(len(q)))


@pytest.mark.parametrize("name", sorted(TABLES))
def test_form_fit_and_monotony(name):
    table = TABLES[name]
    q, nbp, end, ic = table
    n = len(q)
    nonconst = int(n - np.count_nonzero(ic))
    prev = None
    for W in sm.probe_budgets(table):
        res = sm.deal(table, W)
        if W < 8 * nonconst:
            assert res is None, W
            continue
        budgets, star, nxt = res
        for c in range(n):
            if ic[c]:
                assert budgets[c] == 0
                continue
            full = int(end[c][0]) if nbp[c] > 0 else 0
            assert budgets[c] % 8 == 0 and budgets[c] >= 8 and budgets[c] <= max(8, full), (W, c, budgets[c], full)
        assert sum(budgets) <= W, (W, budgets)
        if not full_depth(table, budgets):
            assert sum(budgets) > W - 8 * nonconst, (W, sum(budgets), budgets)
        if prev is not None:
            assert all(b >= a for a, b in zip(prev, budgets)), (W, prev, budgets)
        prev = budgets


def test_refused_below_a_byte_per_chunk():
    table = TABLES["spread_q"]
    assert sm.deal(table, 8 * 5 - 1) is None
    assert sm.deal(table, 8 * 5)[0] == [8] * 5
    assert sm.payload_bits(20 + 4 * 5 + 26 * 5 + 4, 5, 0) is None
    assert sm.payload_bits(20 + 4 * 5 + 26 * 5 + 5, 5, 0) == 40
    assert sm.payload_bits(14 + 4 + 17, 1, 1) == 0 and sm.payload_bits(14 + 4 + 16, 1, 1) is None


def test_all_constant_and_no_planes():
    assert sm.deal(TABLES["all_const"], 0)[0] == [0, 0]
    b, star, nxt = sm.deal(TABLES["no_planes"], 10 ** 6)
    assert b[0] == 8 and b[1] == (int(TABLES["no_planes"][2][1][0]) // 8) * 8 and nxt is None


def test_a_breakpoint_moves_the_threshold():
    """One bit below a breakpoint the tied chunks hold all but their last bits of the plane; at it, T* is the next
    candidate and every chunk holds F_c of it."""
    table = TABLES["spread_q"]
    cand = sm.candidates(table)
    for k in range(1, len(cand)):
        S = sum(sm.floor_bits(table, cand[k]))
        at, below = sm.deal(table, S), sm.deal(table, S - 1)
        assert at[1] == cand[k], k
        assert at[0] == [max(8, (min(f, int(table[2][c][0])) // 8) * 8) for c, f in enumerate(sm.floor_bits(table, cand[k]))]
        assert below[1] == cand[k - 1] and below[2] == cand[k], k


def test_tied_chunks_share_in_proportion():
    table = TABLES["tied_pairs"]
    q, nbp, end, ic = table
    cand = sm.candidates(table)
    seen = 0
    for k in range(len(cand) - 1):
        base, grown = sm.floor_bits(table, cand[k]), sm.floor_bits(table, cand[k + 1])
        plane = [g - b for g, b in zip(grown, base)]
        tied = [c for c in range(4) if plane[c]]
        if len(tied) < 2:
            continue
        rem = sum(plane) // 2
        budgets = sm.deal(table, sum(base) + rem)[0]
        for c in range(4):
            want = base[c] + rem * plane[c] // sum(plane)
            assert budgets[c] == max(8, (min(want, int(end[c][0])) // 8) * 8), (k, c)
        a, b = tied[0], tied[1]
        # in proportion: the shares' ratio is the planes', up to the bytes' rounding
        assert abs((budgets[a] - base[a]) * plane[b] - (budgets[b] - base[b]) * plane[a]) <= 16 * max(plane), (k, budgets)
        seen += 1
    assert seen >= 4


def test_equal_q_comes_out_even():
    """equal steps and rows of like size: the budgets follow the planes' sizes, chunk by chunk"""
    table = TABLES["equal_q"]
    for W in (2000, 20000):
        budgets, star, nxt = sm.deal(table, W)
        thr = [t for t, _ in sm.last_plane_threshold(table, budgets) if t is not None]
        assert len(set(thr)) <= 1, (W, thr)
