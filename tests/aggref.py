"""Host model of the independent sets and the aggregation (pem_tiled_mis / pem_tiled_aggregate), written
from the contract on top of colourref: the sequential greedy maximal independent set at distance 1 or 2 in "beats" order, the
round-synchronous version the device runs (two-hop propagation of maxima over the edge list, never a ball per vertex), the two
assignment passes of the MIS(2) aggregation, and the checks of what a set and an aggregation must be."""
import numpy as np

import colourref as cr

IN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INT32_MAX = 2 ** 31 - 1


def edges(n, I, J, symmetric=False):
    """(src, dst): src sees dst.  Every stored off-diagonal (i, j) lets i see j and, unless symmetric=True (the row orientation only,
    what the device reads under that promise), j see i"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    off = I != J
    I, J = I[off], J[off]
    if symmetric:
        return I, J
    return np.concatenate([I, J]), np.concatenate([J, I])


def beat_keys(prio):
    """a uint64 per vertex, never 0: u beats v exactly where key[u] > key[v]"""
    n = len(prio)
    return (np.asarray(prio, np.uint64) << np.uint64(31) | (np.uint64(INT32_MAX) - np.arange(n, dtype=np.uint64))) + np.uint64(1)


def greedy_mis(adj, prio, distance):
    """the sequential set: the vertices in "beats" order, v enters iff no vertex already in the set lies within `distance`"""
    n = len(adj)
    order, _ = cr._ranks(prio)
    blocked, in_set = np.zeros(n, bool), np.zeros(n, np.uint8)
    for v in order:
        if blocked[v]:
            continue
        in_set[v] = 1
        for u in adj[v]:
            blocked[u] = True
            if distance == 2:
                for w in adj[u]:
                    blocked[w] = True
    return in_set


def _spread(n, src, dst, val):
    """out[v] = the maximum of val over v and the vertices v sees"""
    out = val.copy()
    if len(src):
        np.maximum.at(out, src, val[dst])
    return out


def rounds_mis(n, src, dst, prio, distance):
    """(in_set, rounds) by rounds on undecided / in / out, every round from one snapshot: an undecided vertex with an in vertex within
    `distance` turns out; otherwise one that no undecided vertex within `distance` beats turns in.  Out vertices relay.  Stops after
    the first round without an undecided vertex, or after round n (a false symmetric=True promise): what is undecided then is 0."""
    beat = beat_keys(prio)
    key = beat.copy()                       # 0: out, IN_KEY: in, else undecided
    r = 0
    while r < n:
        m =_spread(n, src, dst, key)
        if distance == 2:
            m = _spread(n, src, dst, m)
        und = (key != 0) & (key != IN_KEY)
        new = key.copy()
        new[und & (m == IN_KEY)] = 0
        new[und & (m == key)] = IN_KEY
        key = new
        r += 1
        if not np.any((key != 0) & (key != IN_KEY)):
            break
    return (key == IN_KEY).astype(np.uint8), r


def assign_pass(n, src, dst, prio, agg):
    """one assignment pass: a vertex without an aggregate takes the aggregate of the placed vertex it sees that beats the others"""
    beat = beat_keys(prio)
    cand = np.where(agg >= 0, beat, np.uint64(0))
    best = np.zeros(n, np.uint64)
    if len(src):
        np.maximum.at(best, src, cand[dst])
    out = agg.copy()
    take = (agg < 0) & (best != 0)
    winner = INT32_MAX - ((best[take] - np.uint64(1)) & np.uint64(INT32_MAX)).astype(np.int64)
    out[take] = agg[winner]
    return out


def aggregate_from(n, src, dst, prio, in_set):
    """(agg, roots, naggregates): the roots numbered in ascending vertex order, then the two passes"""
    roots = np.flatnonzero(in_set).astype(np.int32)
    agg = np.full(n, -1, np.int32)
    agg[roots] = np.arange(len(roots), dtype=np.int32)
    agg = assign_pass(n, src, dst, prio, agg)
    agg = assign_pass(n, src, dst, prio, agg)
    return agg, roots, len(roots)


def _prio(n, seed, priority):
    return cr.hash_priority(n, seed) if priority is None else np.asarray(priority, np.uint32)


def mis(n, I, J, distance=2, seed=0, priority=None, symmetric=False):
    """what Tiled.mis returns, on the host: (in_set, count, rounds)"""
    src, dst = edges(n, I, J, symmetric)
    s, r = rounds_mis(n, src, dst, _prio(n, seed, priority), distance)
    return s, int(s.sum()), r


def aggregate(n, I, J, seed=0, priority=None, symmetric=False):
    """what Tiled.aggregate returns, on the host: (agg, roots, naggregates, rounds)"""
    src, dst = edges(n, I, J, symmetric)
    prio = _prio(n, seed, priority)
    s, r = rounds_mis(n, src, dst, prio, 2)
    agg, roots, nc = aggregate_from(n, src, dst, prio, s)
    return agg, roots, nc, r


def within(adj, v, distance):
    """the vertices at distance 1 .. `distance` of v"""
    ball = set(adj[v])
    if distance == 2:
        for u in adj[v]:
            ball |= adj[u]
    ball.discard(v)
    return ball


def is_mis(adj, in_set, distance):
    """independent (no two members within `distance`) and maximal (every other vertex has a member within `distance`)"""
    for v in range(len(adj)):
        hit = any(in_set[u] for u in within(adj, v, distance))
        if bool(in_set[v]) == hit:
            return False
    return True


def check_aggregation(adj, agg, roots, nc):
    """no -1, exactly one root per aggregate, ids ascending by root, every member within 2 of its root inside the aggregate"""
    n = len(adj)
    assert len(roots) == nc and np.all(np.diff(roots) > 0)
    assert n == 0 or (agg.min() >= 0 and agg.max() == nc - 1)
    assert np.array_equal(agg[roots], np.arange(nc))
    for v in range(n):
        c, r = agg[v], roots[agg[v]]
        if v == r or r in adj[v]:
            continue
        assert any(agg[u] == c and r in adj[u] for u in adj[v]), (v, c, r)


def grid_one_way(k=40):
    """the k x k five-point grid, vertex k r + c, only (v, v + 1) and (v, v + k) stored"""
    v = np.arange(k * k).reshape(k, k)
    I = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]).astype(np.int32)
    J = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()]).astype(np.int32)
    return k * k, I, J


def graphs(cases):
    """name -> (n, I, J): the colouring's list, colourref's built graphs and the grid"""
    names = ("one_entry", "empty_matrix", "diag_100", "ragged_37", "dense_tile", "dense_48", "empty_rows", "rand_300", "powerlaw_600",
             "hub_row_4000", "band_1500")
    out = {name: (cases[name][0], cases[name][2], cases[name][3]) for name in names}
    out.update(cr.built_graphs())
    out["grid_40_one_way"] = grid_one_way(40)
    return out


def priority_array(n, which):
    """the uint32 array of a priority choice: a seed (hashed), "equal", or "ties" (test_gpu_colour.py's: four values, most tie)"""
    if which == "equal":
        return np.full(n, 0x80000000, np.uint32)
    if which == "ties":
        return np.random.default_rng(n + 5).integers(0, 4, n).astype(np.uint32) * np.uint32(0x40000001)
    return cr.hash_priority(n, which)
