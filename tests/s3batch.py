"""Layouts for step 3's batched record fetch (PEM_OPT_S3_BATCH) and a walk of the trips they give.

The shallow entry-per-lane kernel fetches the records of a trip's third and later pairs S3_BATCH_R = 3 pairs at a time into a
wave-private LDS strip.  spec() puts every edge of that into one layout, section by section, each section starting on a wave
(256 entries); trips() restates from pairs_offset and c_tile_nnz_ptr which lanes, pair counts and pair range every trip of the
kernel has (as s3cases.model does, but trip by trip), so that a test can show the layout reaches the edge it was built for.
"""
import numpy as np

import s3cases
from s3cases import INT_MAX, S3_CHUNK, _pad_to

S3_BATCH_R = 3        # step3.hip: pairs per batch
SEED = 11


def spec():
    """(entries, pairs[, empty_rows[, dead]]) per C tile; fewer than two pairs per tile overall, dead pairs included"""
    s = []
    # batch edges: one tile per trip, so a trip's deepest lane has exactly 3, 4, 5 (one batch, partly and wholly filled),
    # 6 (a second batch of one round), 8 (two full batches) and 9 pairs (a third batch)
    s += [(64, 3), (64, 4), (64, 5), (64, 6)]
    s += [(64, 8), (64, 9)]
    _pad_to(s, 256)
    # mixed trip: lanes of one-pair, two-pair, 5-pair and 9-pair tiles together (rounds where only some lanes are on)
    s += [(10, 1), (10, 2), (12, 5), (12, 9), (10, 1), (10, 2)]
    _pad_to(s, 256)
    # staging limit (s3cases.shallow_spec's constructions with a 5-pair tile): one trip of 64 lanes with Pn == 64, one with 65
    s += [(5, 5)] + [(1, 1)] * 59
    _pad_to(s, 256)
    s += [(4, 5)] + [(1, 1)] * 60
    _pad_to(s, 256)
    # split tile: 256 entries and 5 pairs from entry 100 of a wave on -- across trips, and across waves
    s += [(100, 1), (256, 5)]
    _pad_to(s, 256)
    # dead pairs behind live ones (kept by prune = 0: inside a batch, and a batch of dead pairs only)
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
    # name: (options, mask, the form plus-times takes)
    "decode_idx32_mark": ((), None, "decode,idx32,mark"),
    "decode_idx32": ((("s3_mark", 0),), None, "decode,idx32"),
    "decode_mark": ((("s3_idx64", 1),), None, "decode,mark"),
    "decode": ((("s3_idx64", 1), ("s3_mark", 0)), None, "decode"),
    "wide": ((("s3_decode", 0),), None, "wide"),
    "complement": ((), "complement", "decode,idx32"),
    "unpruned": ((("prune", 0),), None, "decode,idx32"),
}


def case(name):
    opts, mask, _ = FORMS[name]
    return s3cases._case("batch_" + name, SPEC, SEED, opts, (), mask=mask)


def tiles():
    """the layout's tiles as s3cases.operands() builds them: per C tile its pairs (a_rows[16], b_cols[16])"""
    return s3cases._layout(np.random.default_rng(1000 + SEED), SPEC)


def trips(pairs_offset, c_tile_nnz_ptr, epw=S3_CHUNK):
    """every trip of the entry-per-lane kernel: dict(nvalid, n_of = pairs of each valid lane's tile, tile = its tile, Pn, staged)"""
    po = np.asarray(pairs_offset, np.int64)
    off = np.asarray(c_tile_nnz_ptr, np.int64)
    ntc = len(po) - 1
    nnz = int(off[-1])
    npt = np.diff(po)
    chunk_tile = np.searchsorted(off, np.arange(0, nnz, S3_CHUNK), side="right") - 1
    lanes = np.arange(64)
    out = []
    for wave in range((nnz + epw - 1) // epw):
        e_lo, e_hi = wave * epw, min(wave * epw + epw, nnz)
        t0 = int(chunk_tile[wave * (epw // S3_CHUNK)])
        while t0 < ntc:
            lane_off = np.where(t0 + lanes < ntc, off[np.minimum(t0 + lanes, ntc)], INT_MAX)
            tend = min(t0 + 64, ntc)
            first = int(lane_off[0])
            if first >= e_hi:
                break
            chunk_end = int(off[tend])
            for ebase in range(max(first, e_lo), min(chunk_end, e_hi), 64):
                nvalid = min(64, min(chunk_end, e_hi) - ebase)
                e = ebase + lanes[:nvalid]
                t = t0 + np.searchsorted(lane_off, e, side="right") - 1
                n_of = npt[t]
                Pn = int(po[t[-1] + 1] - po[t[0]])
                out.append(dict(nvalid=nvalid, n_of=n_of, tile=t, Pn=Pn, staged=bool((n_of > 2).any()) and Pn <= 64))
            if chunk_end >= e_hi:
                break
            t0 += 64
    return out


def later_pair_products(tl):
    """(lanes' later pairs that meet in no product, later pairs that give an entry two or more products) over the layout"""
    none = multi = 0
    for ps in tl:
        if len(ps) < 3:
            continue
        arow0, bcol0 = ps[0]
        entries = [(r, c) for r in range(16) for c in range(16) if arow0[r] & bcol0[c]]   # pair 0 carries the whole pattern
        for arow, bcol in ps[2:]:
            for r, c in entries:
                k = bin(arow[r] & bcol[c]).count("1")
                none += k == 0
                multi += k >= 2
    return none, multi
