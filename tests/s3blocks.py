"""Layout for step 3's two-pair blocks: later pairs walked two at a time, a visit's second product gathered beside its first.

The shallow entry-per-lane kernel (step3.hip, s3_pair_block) takes the pairs of an entry's C tile two per block: records of both,
then the first product of both (and the first pair's second product), then the sums in order.  spec() puts the edges of that
into one layout -- later-pair counts 1 to 7, last blocks half filled, lanes of 1, 2, 4 and 7 pairs in one trip, the staging
limit on both sides, a partial last trip, a tile split across trips and waves -- as tests/s3batch.py does for the batched
fetch.  Its many-pair tiles are CRAFTED: a crafted tile's entries lie in columns 0-3, and pair j gives entry (r, c) exactly
counts[j][r, c] products (0 to 4), whatever the other entries and pairs get -- so dead visits, visits with 1, 2, 3 and 4
products in every position of a block, and the rare combinations the kernel's product loops branch on are there by
construction.  products() restates the counts from the operands' masks, for the host-only test to show that they are.
"""
import numpy as np

import s3cases
from s3cases import _pad_to

SEED = 13
CRAFT = "craft"
_DRAW = (0, 0, 0, 1, 1, 2, 3, 4)      # products of one (entry, pair) visit of a crafted tile


def spec():
    """(entries, pairs[, empty_rows[, dead[, CRAFT]]]) per C tile; fewer than two pairs per tile overall, dead pairs included"""
    s = []
    # one tile per trip: the trip's lanes all have 3 .. 9 pairs, i.e. 1 .. 7 later pairs (odd counts: a half-filled last block)
    s += [(64, n, (), 0, CRAFT) for n in (3, 4, 5, 6)]
    s += [(64, n, (), 0, CRAFT) for n in (7, 8, 9)]
    _pad_to(s, 256)
    # mixed trip: lanes of one-pair, two-pair, 4-pair and 7-pair tiles side by side (blocks where only some lanes are on, and
    # where some of those have no second pair)
    s += [(10, 1), (10, 2), (12, 4, (), 0, CRAFT), (12, 7, (), 0, CRAFT), (10, 1), (10, 2)]
    _pad_to(s, 256)
    # small tiles of 3 to 9 pairs between one- and two-pair tiles: several many-pair tiles in a trip, lanes leaving block by block
    for rep in range(3):
        s += [t for n in range(3, 10) for t in ((5 - rep, n, (), 0, CRAFT), (2, 1), (3, 2))]
    _pad_to(s, 256)
    # staging limit (s3cases.shallow_spec's constructions with a 5-pair tile): one trip of 64 lanes with Pn == 64, one with 65
    s += [(5, 5)] + [(1, 1)] * 59
    _pad_to(s, 256)
    s += [(4, 5)] + [(1, 1)] * 60
    _pad_to(s, 256)
    # split tile: 256 entries and 5 pairs from entry 100 of a wave on -- across trips, and across waves
    s += [(100, 1), (256, 5)]
    _pad_to(s, 256)
    # dead pairs behind live ones (kept by prune = 0: inside a block, and blocks of dead pairs only)
    s += [(10, 3, (), 2), (7, 1, (), 1), (9, 4, (), 3), (12, 2, (), 4)]
    _pad_to(s, 256)
    # one-pair tiles keep the plan shallow (npairs < 2 * ntc, dead pairs counted)
    tiles, pairs = len(s) + 1, sum(t[1] + (t[3] if len(t) > 3 else 0) for t in s) + 5
    s += [(1, 1)] * max(0, pairs - 2 * tiles + 8)
    _pad_to(s, 64)
    # partial trip: the last valid lane belongs to a 5-pair tile, the lanes behind it are idle
    s += [(11, 5)]
    return s


SPEC = spec()
FORMS = {
    # name: (options, the form plus-times takes)
    "decode_idx32_mark": ((), "decode,idx32,mark"),
    "decode_idx32": ((("s3_mark", 0),), "decode,idx32"),
    "decode_mark": ((("s3_idx64", 1),), "decode,mark"),
    "decode": ((("s3_idx64", 1), ("s3_mark", 0)), "decode"),
    "wide": ((("s3_decode", 0),), "wide"),
    "unpruned": ((("prune", 0),), "decode,idx32"),
}


def crafted(rng, n, npairs, force=()):
    """a tile of n entries (row-major in columns 0-3) and npairs pairs; -> (pairs for s3cases.build, counts[pair, entry])

    Column c of B holds inner indices 4c .. 4c+3 and row r of A holds the lowest counts[j, e] of them, e = 4r + c: the visit
    (entry e, pair j) has exactly counts[j, e] products.  force: (entry, counts per pair) rows set as given."""
    assert 0 < n <= 64
    cnt = rng.choice(_DRAW, size=(npairs, n))
    for e, col in force:
        cnt[:, e] = col
    for e in np.nonzero(cnt.sum(0) == 0)[0]:          # every entry is in C: a product somewhere
        cnt[int(rng.integers(npairs)), e] = 1
    for j in np.nonzero(cnt.sum(1) == 0)[0]:          # every pair is alive
        cnt[j, int(rng.integers(n))] = 1
    pairs = []
    for j in range(npairs):
        arow = [0] * 16
        for e in range(n):
            arow[e // 4] |= ((1 << int(cnt[j, e])) - 1) << (4 * (e % 4))
        bcol = [0xF << (4 * c) if c < 4 else 0 for c in range(16)]
        pairs.append((arow, bcol))
    return pairs, cnt


def _force(n, npairs):
    """the combinations a random draw may miss, in the 64-entry tile of seven pairs"""
    if (n, npairs) != (64, 7):
        return ()
    return ((0, (0, 2, 0, 0, 0, 0, 0)),               # a dead first pair beside a second pair with two products
            (1, (0, 0, 0, 0, 0, 0, 1)),               # the only product comes from the last pair of an odd count
            (2, (1, 0, 3, 2, 0, 0, 0)),               # products in both pairs of a later block
            (3, (4, 4, 4, 4, 0, 0, 0)), (4, (3, 3, 3, 3, 0, 0, 0)), (5, (2, 2, 2, 2, 0, 0, 0)), (6, (1, 1, 1, 1, 0, 0, 0)))


_TILES = None


def tiles():
    """the layout's tiles for s3cases.build(): s3cases._layout's, the crafted ones put in their places"""
    global _TILES
    if _TILES is None:
        out = s3cases._layout(np.random.default_rng(1000 + SEED), SPEC)
        rng = np.random.default_rng(2000 + SEED)
        for t, s in enumerate(SPEC):
            if len(s) > 4 and s[4] == CRAFT:
                out[t] = crafted(rng, s[0], s[1], _force(s[0], s[1]))[0]
        _TILES = out
    return _TILES


def case(name):
    opts, _ = FORMS[name]
    c = s3cases._case("blocks_" + name, SPEC, SEED, opts, ())
    key = (id(SPEC), SEED)
    if key not in s3cases._OPS:                        # (operands() builds from the spec alone: the crafted tiles go in here)
        s3cases._OPS[key] = s3cases.build(tiles(), SEED)
    return c


def products(ps):
    """counts[pair, entry] of one tile's pairs [(a_rows[16], b_cols[16])]: products of every visit, entries row-major over the
    tile's pattern (the union of the pairs' products)"""
    k = np.array([[[bin(arow[r] & bcol[c]).count("1") for c in range(16)] for r in range(16)] for arow, bcol in ps])
    return k.reshape(len(ps), 256)[:, k.sum(0).reshape(256) > 0]
