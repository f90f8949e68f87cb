"""The size mode's deal in numpy (no GPU): sperr_amd/csrc/budget.h stated again, the plain way -- all candidate
thresholds in a sorted list, walked from the top -- where the header bisects over bit patterns.  Both are exact
statements of one rule, so tests compare every budget (tests/test_size_host.py: the header as host C++;
tests/test_gpu_size.py: the kernel).

  table     q float64 [n], nbp int [n], end uint64 [n][32] (bits at the end of plane p under an unlimited budget, zeros
            from nbp on), is_const bool [n]
  W         payload_bits(target, n, #const) = 8 (target - header - 26 #nonconst - 17 #const); None: refused
  P_c(T)    the smallest p >= 0 with ldexp(q_c, p) >= T, capped at nbp_c;  F_c(T) = max(8, end_c[P_c(T)]), end_c[nbp_c] = 0
  T*        the last of (+inf, then every distinct ldexp(q_c, p), p < nbp_c, descending) with sum F_c(T*) <= W
  the rest  W - sum F_c(T*) to the chunks whose F grows at the next candidate T', floor(rem plane_c / sum plane) each
  rounding  max(8, 8 floor(min(F_c(T*) + share_c, end_c[0]) / 8)); 0 for a constant chunk"""
import numpy as np

PLANES = 32


def header_bytes(nchunks):
    return (20 if nchunks > 1 else 14) + 4 * nchunks


def payload_bits(target_bytes, nchunks, nconst):
    nonconst = nchunks - nconst
    fixed = header_bytes(nchunks) + 26 * nonconst + 17 * nconst
    if target_bytes < fixed or target_bytes - fixed < nonconst:
        return None
    return 8 * (target_bytes - fixed)


def depth(q, nbp, T):
    """P_c(T) of every chunk"""
    q = np.asarray(q, dtype=np.float64)
    nbp = np.asarray(nbp, dtype=np.int64)
    P = nbp.copy()
    for p in range(PLANES - 1, -1, -1):   # the smallest p that passes wins: walk down
        with np.errstate(over="ignore"):
            ok = (np.ldexp(q, p) >= T) & (p < nbp)
        P[ok] = p
    return P


def floor_bits(table, T):
    """F_c(T) as python ints (0 for a constant chunk)"""
    q, nbp, end, is_const = table
    P = depth(q, nbp, T)
    out = []
    for c in range(len(q)):
        if is_const[c]:
            out.append(0)
        else:
            e = int(end[c][P[c]]) if P[c] < nbp[c] else 0
            out.append(max(8, e))
    return out


def candidates(table):
    q, nbp, end, is_const = table
    vals = set()
    for c in range(len(q)):
        if is_const[c] or not q[c] > 0.0 or nbp[c] <= 0:
            continue
        top = float(np.ldexp(np.float64(q[c]), int(nbp[c]) - 1))
        if not np.isfinite(top):
            continue
        for p in range(int(nbp[c])):
            vals.add(float(np.ldexp(np.float64(q[c]), p)))
    return [np.inf] + sorted(vals, reverse=True)


def deal(table, W):
    """-> (budgets as a list of python ints, T*, T' or None); None when W < 8 #nonconst"""
    q, nbp, end, is_const = table
    n = len(q)
    nonconst = sum(1 for c in range(n) if not is_const[c])
    if W < 8 * nonconst:
        return None
    cand = candidates(table)
    k = 0
    while k + 1 < len(cand) and sum(floor_bits(table, cand[k + 1])) <= W:
        k += 1
    star = cand[k]
    nxt = cand[k + 1] if k + 1 < len(cand) else None
    base = floor_bits(table, star)
    budgets = list(base)
    if nxt is not None:
        grown = floor_bits(table, nxt)
        plane = [g - b for g, b in zip(grown, base)]
        rem, tot = W - sum(base), sum(plane)
        if tot:
            for c in range(n):
                budgets[c] += min(plane[c], rem * plane[c] // tot)
    for c in range(n):
        if is_const[c]:
            budgets[c] = 0
            continue
        full = int(end[c][0]) if nbp[c] > 0 else 0
        budgets[c] = max(8, (min(budgets[c], full) // 8) * 8)
    return budgets, star, nxt


def make_table(q, ends, is_const=None):
    """a table from per-chunk lists of end[p] (p = 0 first, each of its chunk's nbp entries)"""
    n = len(q)
    end = np.zeros((n, PLANES), dtype=np.uint64)
    nbp = np.zeros(n, dtype=np.int64)
    for c, row in enumerate(ends):
        nbp[c] = len(row)
        end[c, :len(row)] = np.asarray(row, dtype=np.uint64)
    ic = np.zeros(n, dtype=bool) if is_const is None else np.asarray(is_const, dtype=bool)
    return np.asarray(q, dtype=np.float64), nbp, end, ic


def last_plane_threshold(table, budgets):
    """per chunk: q_c 2^p of the last plane its budget completes (up to the rounding to bytes), None where no plane
    is complete (the 8-bit floor) -- and whether the chunk is at full depth"""
    q, nbp, end, is_const = table
    out = []
    for c in range(len(q)):
        if is_const[c] or nbp[c] <= 0:
            out.append((None, False))
            continue
        done = [p for p in range(int(nbp[c])) if (int(end[c][p]) // 8) * 8 <= budgets[c]]
        if not done:
            out.append((None, False))
        else:
            p = min(done)
            out.append((float(np.ldexp(np.float64(q[c]), p)), p == 0))
    return out


# ---- hand-made tables (tests/test_size_model.py, tests/test_size_host.py) ------------------------------------------

def _row(nbp, top, growth, seed):
    """end[p] for p = 0 .. nbp - 1: `top` bits for the top plane, each lower plane `growth` times the one above plus a
    hashed few bits (so that no two rows are proportional)"""
    sizes, s = [], float(top)
    for k in range(nbp):
        sizes.append(int(s) + (seed * 2654435761 + k * 40503) % 13)
        s *= growth
    ends, run = [], 0
    for v in sizes:
        run += v
        ends.append(run)
    return ends[::-1]   # (p = 0 first: the whole stream)


def hand_tables():
    """{name: table}"""
    t = {}
    t["equal_q"] = make_table([0.25] * 4, [_row(12, 40, 1.7, k) for k in range(4)])
    t["spread_q"] = make_table([1.0, 0.1, 1e-3, 1e-3, 3e-4], [_row(14, 30, 1.8, 10 + k) for k in range(5)])
    t["one_plane"] = make_table([2.0, 0.5, 0.37], [_row(10, 25, 1.6, 20), [97], _row(9, 60, 1.5, 22)])
    t["tiny_chunk"] = make_table([1.0, 1.0 / 3.0], [_row(8, 50, 1.9, 30), [5, 3]])          # end[0] < 8
    t["with_const"] = make_table([0.5, 0.0, 0.02, 0.0], [_row(11, 33, 1.75, 40), [], _row(13, 21, 1.65, 42), []],
                                 is_const=[False, True, False, True])
    t["all_const"] = make_table([0.0, 0.0], [[], []], is_const=[True, True])
    t["no_planes"] = make_table([0.0, 1.5], [[], _row(6, 44, 1.5, 50)])                       # all-zero coefficients
    t["tied_pairs"] = make_table([0.125, 0.125, 4.0, 4.0], [_row(10, 35, 1.7, 60), _row(10, 70, 1.7, 61),
                                                            _row(7, 20, 2.0, 62), _row(7, 20, 2.0, 63)])
    return t


def breakpoints(table):
    """sum F_c(T) at every candidate, ascending: the W at which T* moves"""
    return sorted({sum(floor_bits(table, T)) for T in candidates(table)})


def write_table(path, table):
    """the file tests/cpp/size_check.cpp reads"""
    q, nbp, end, is_const = table
    with open(path, "wb") as f:
        f.write(np.uint64(len(q)).tobytes())
        f.write(np.asarray(q, dtype=np.float64).tobytes())
        f.write(np.asarray(nbp, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(end, dtype=np.uint64).tobytes())
        f.write(np.asarray(is_const, dtype=np.uint8).tobytes())


def probe_budgets(table):
    """the W a table is dealt at: around every breakpoint, and a spread in between and beyond"""
    n = sum(1 for c in table[3] if not c)
    ws = {8 * n, 8 * n + 1, 8 * n + 8}
    bps = breakpoints(table)
    for b in bps:
        ws.update((b - 1, b, b + 1, b + 7, b + 8, b + 9))
    top = bps[-1] if bps else 0
    for k in range(1, 40):
        ws.add(8 * n + (top * k) // 37)
    ws.update((top + 1000, 2 * top + 64))
    return sorted(w for w in ws if w >= 0)
