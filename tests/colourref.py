"""Host model of the graph colouring (pem_tiled_colour / pem_colour_order), written from the contract:
the hash, the adjacency of a COO pattern under both `symmetric` readings, the sequential greedy colouring in priority order with the
round of every vertex, the round-synchronous Jones-Plassmann colouring the device runs, and the stable colour order."""
import numpy as np

M32 = 0xFFFFFFFF


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def hash_priority(n, seed):
    """the priority of every vertex under d_priority = NULL"""
    return np.array([fmix32(v + seed * 0x9E3779B9) for v in range(n)], np.uint32)


def hash_priority_at(idx, seed):
    """hash_priority(n, seed)[idx] for any n above every index, computed for those vertices alone"""
    h = (np.asarray(idx, np.uint64) + np.uint64((seed * 0x9E3779B9) & M32)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def adjacency(n, I, J, symmetric=False):
    """a list of neighbour sets: every stored off-diagonal (i, j) is the edge {i, j}; symmetric=True reads what the device reads under
    that promise, the row orientation only (vertex i sees j, and j sees i only if (j, i) is stored too)"""
    adj = [set() for _ in range(n)]
    for i, j in zip(np.asarray(I).tolist(), np.asarray(J).tolist()):
        if i != j:
            adj[i].add(j)
            if not symmetric:
                adj[j].add(i)
    return adj


def _ranks(prio):
    """(order, rank): the vertices in descending (priority, -index) order, and every vertex's position in it -- u beats v where
    rank[u] < rank[v]"""
    order = sorted(range(len(prio)), key=lambda v: (-int(prio[v]), v))
    rank = [0] * len(order)
    for k, v in enumerate(order):
        rank[v] = k
    return order, rank


def greedy(adj, prio):
    """(colour, round, ncolours, rounds): the sequential greedy colouring in descending (priority, -index) order -- the smallest
    colour no neighbour of higher priority holds -- and round[v] = 1 + the largest round of such a neighbour (the vertices on the
    longest chain of falling priority that ends in v)"""
    n = len(adj)
    order, rank = _ranks(prio)
    colour, rnd = [-1] * n, [0] * n
    for v in order:
        higher = [u for u in adj[v] if rank[u] < rank[v]]
        used = {colour[u] for u in higher}
        c = 0
        while c in used:
            c += 1
        colour[v] = c
        rnd[v] = 1 + max((rnd[u] for u in higher), default=0)
    return np.array(colour, np.int32), np.array(rnd, np.int32), max(colour, default=-1) + 1, max(rnd, default=0)


def jones_plassmann(adj, prio):
    """(colour, round, ncolours, rounds) by rounds: every uncoloured vertex no uncoloured neighbour beats takes the smallest colour its
    coloured neighbours leave free, all of a round from the colours of the round before"""
    n = len(adj)
    _, rank = _ranks(prio)
    colour, rnd = [-1] * n, [0] * n
    left, r = set(range(n)), 0
    while left:
        r += 1
        new = {}
        for v in left:
            if any(colour[u] < 0 and rank[u] < rank[v] for u in adj[v]):
                continue
            used = {colour[u] for u in adj[v] if colour[u] >= 0}
            c = 0
            while c in used:
                c += 1
            new[v] = c
        assert new, "a round must colour the best uncoloured vertex"
        for v, c in new.items():
            colour[v], rnd[v] = c, r
        left -= set(new)
    return np.array(colour, np.int32), np.array(rnd, np.int32), max(colour, default=-1) + 1, r


def colouring(n, I, J, seed=0, priority=None, symmetric=False):
    """what Tiled.colour returns, on the host: (colours, ncolours, rounds)"""
    prio = hash_priority(n, seed) if priority is None else np.asarray(priority, np.uint32)
    c, _, nc, rounds = greedy(adjacency(n, I, J, symmetric), prio)
    return c, nc, rounds


def is_valid(n, I, J, colour):
    """no stored off-diagonal entry joins two vertices of one colour; every colour is in [0, n)"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    off = I != J
    return bool(np.all(colour[I[off]] != colour[J[off]])) and bool(np.all((colour >= 0) & (colour < max(n, 1))))


def colour_order(colour, ncolours):
    """(perm, offsets): the stable sort by colour and the cumulative histogram"""
    colour = np.asarray(colour)
    perm = np.argsort(colour, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=ncolours))]).astype(np.int32)
    return perm, offsets


def symmetrised(I, J):
    """the pattern united with its transpose: (I, J) without duplicates"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    m = int(max(I.max(initial=0), J.max(initial=0))) + 1
    key = np.unique(np.concatenate([I * m + J, J * m + I]))
    return (key // m).astype(np.int32), (key % m).astype(np.int32)


def built_graphs():
    """name -> (n, I, J): the three graphs the tests build themselves"""
    out = {}
    i, j = np.meshgrid(np.arange(70), np.arange(70), indexing="ij")
    out["k70_in_75"] = (75, i.ravel().astype(np.int32), j.ravel().astype(np.int32))       # diagonal stored too: no edge
    i, j = np.meshgrid(np.arange(131), np.arange(131), indexing="ij")
    off = i != j
    out["k131"] = (131, i[off].astype(np.int32), j[off].astype(np.int32))                 # 17 030 entries
    p = np.arange(202, dtype=np.int32)
    out["path_203_one_way"] = (203, p, p + 1)                                             # 0-1-...-202, (i, i + 1) only
    return out
