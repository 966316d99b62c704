"""Step 3's kernel paths: operands built C tile by C tile, and a model of where step 3's waves and trips fall.

The entry-per-lane kernel (step3.hip, s3_accumulate_wide_kernel) and the many-pair kernel (s3_band_kernel) branch on how C
tiles, their pairs and their entries fall across a wave's 64-entry trips and 64-tile windows.  Whether a random matrix reaches
a branch is luck; here the layout is built for it.

build(tiles)     C tile t is (t, t) and owns its k tiles alone, so every tile's pair count, entry pattern and position in C
                 are exactly what the caller asked for.  A is 16T x 16K and B is 16K x 16T (K: the pairs of all tiles).
model(...)       restates, from the plan's pairs_offset and c_tile_nnz_ptr, what s3_launch and the two kernels compute: the
                 form, the waves' first tiles, each trip's lanes, pair range and staging, the band kernel's tiles -- and
                 returns the set of PATHS the plan takes.  A witness of coverage only: values are checked against the oracle.
cases()          named layouts with their options and the paths each must reach; together they reach every path.
"""
import numpy as np

from matgen import _vals

S3_CHUNK = 256        # spgemm_internal.h: C entries per chunk of step 3's work index
S3_BAND_MIN = 8       # step3.hip: C tiles with this many pairs go to s3_band_kernel (deep plans, band on)
INT_MAX = 0x7FFFFFFF
# PEM_OPT_S3_POISON's fill (0x7FF4 in every 16-bit half): a NaN as fp64 and as fp32
POISON = {np.dtype(np.float64): np.uint64(0x7FF47FF47FF47FF4), np.dtype(np.float32): np.uint32(0x7FF47FF4)}


def poisoned(v):
    """entries of C (fp64 or fp32 values) that hold the fill: no step-3 kernel wrote them"""
    v = np.asarray(v)
    return v.view(np.uint64 if v.dtype == np.float64 else np.uint32) == POISON[v.dtype]

DEFAULTS = dict(prune=1, step1_global_sort=0, wide=1, s3_band=1, s3_decode=1, s3_epw=0, s3_idx64=0, s3_mark=1, s3_xcd=1)

# every path of gap 1 (what test_s3_cover_cpu.py requires the cases to reach, each on both sides of its edge)
PATHS = {
    # launch forms (s3_launch) and the work split
    "form:base": "16 lanes per tile (PEM_OPT_WIDE = 0)",
    "form:wide": "entry per lane, Ctiles_rowColIdx (PEM_OPT_S3_DECODE = 0)",
    "form:decode": "entry per lane, decode, 64-bit, shuffle search",
    "form:decode,idx32": "entry per lane, decode, 32-bit offsets, shuffle search",
    "form:decode,idx32,mark": "entry per lane, decode, 32-bit offsets, marked tile lookup",
    "form:decode,mark": "entry per lane, decode, 64-bit, marked tile lookup",
    "form:deep": "four pairs per trip (PEM_OPT_S3_BAND = 0)",
    "form:deep,band": "four pairs per trip + the wave-per-tile kernel",
    "epw:256": "256 entries per wave", "epw:512": "512 entries per wave", "epw:1024": "1024 entries per wave",
    "xcd:0": "waves in block order", "xcd:1": "XCD x takes the x-th eighth of C",
    # waves and windows of the entry-per-lane kernel
    "wave_starts_at_tile": "a wave's first entry is its tile's first",
    "wave_starts_mid_tile": "a wave's first entry lies inside a tile (chunk_tile from step 2)",
    "tile_split_across_waves": "a tile's entries go to two waves",
    "tile_split_across_trips": "a tile's entries go to two trips of one wave",
    "wave_one_window": "a wave's entries lie in one 64-tile window",
    "wave_crosses_window": "a wave's entries cross the 64-tile register window (t0 += 64)",
    "trip_full": "a trip with 64 valid lanes", "trip_partial": "a trip with fewer than 64 valid lanes",
    "empty_tile_inside_trip": "a C tile without entries between a trip's entries",
    # MARK
    "mark_tile_starts_trip": "MARK: a tile starts at the trip's first entry (before == 0)",
    "mark_trip_starts_inside_tile": "MARK: the trip's first entry lies inside a tile (before >= 1)",
    "mark_no_tile_starts": "MARK: no tile starts in the trip",
    "mark_tiles_start": "MARK: tiles start in the trip",
    # DECODE
    "decode_skips_empty_row": "DECODE: a tile with an empty row below a row with entries",
    "decode_full_tile": "DECODE: a 256-entry tile",
    "decode_partial_tile": "DECODE: a tile of fewer than 256 entries",
    # shallow pairs
    "sh_one_pair": "shallow: an entry of a one-pair tile (has1 only)",
    "sh_two_pairs": "shallow: an entry of a two-pair tile (has1, has2)",
    "sh_staged": "shallow: a lane with 3+ pairs, trip pair range Pn <= 64 (staged)",
    "sh_staged_pn64": "shallow: staged with Pn == 64",
    "sh_unstaged": "shallow: a lane with 3+ pairs, Pn > 64 (the unstaged loop)",
    "sh_unstaged_pn65": "shallow: unstaged with Pn == 65",
    "sh_no_third_pair": "shallow: a trip whose lanes have at most 2 pairs",
    # deep
    "deep_quad_more": "deep: a group of four with the next four loaded (more)",
    "deep_quad_last": "deep: a group of four without a next one (!more)",
    "deep_rem0": "deep: no pairs after the groups of four", "deep_rem1": "deep: 1 pair after the groups",
    "deep_rem2": "deep: 2 pairs after the groups", "deep_rem3": "deep: 3 pairs after the groups",
    "deep_leaves_band_tile": "deep,band: a lane whose tile has 8+ pairs leaves it to the band kernel",
    "deep_keeps_np7": "deep,band: a tile of 7 pairs stays in the entry-per-lane kernel",
    # band
    "band_np8": "band: a tile of exactly S3_BAND_MIN pairs",
    "band_pad": "band: pair count not a multiple of 4 (M4 padding)",
    "band_np_mult4": "band: pair count a multiple of 4",
    "band_np16": "band: 16 pairs, one stage", "band_np17": "band: 17 pairs, a second stage of one pair",
    "band_np_gt64": "band: more than 64 pairs",
    "band_one_sub": "band: at most 64 entries", "band_sub_trips": "band: more than 64 entries (the sub loop)",
    "band_several_tiles_in_wave": "band: several many-pair tiles in one wave",
    "band_grid_tail": "band: a many-pair tile in a wave that reaches past the last C tile",
}


# ------------------------------------------------------------------------------------------------------------------------
# the builder
# ------------------------------------------------------------------------------------------------------------------------
def pattern(rng, n, empty_rows=()):
    """16 row masks of a C tile with n entries at random positions of the rows not in empty_rows"""
    rows = [r for r in range(16) if r not in empty_rows]
    assert 0 <= n <= 16 * len(rows)
    pos = rng.choice(16 * len(rows), size=n, replace=False)
    S = [0] * 16
    for p in pos:
        S[rows[p // 16]] |= 1 << int(p % 16)
    return S


def pairs_for(rng, S, npairs, multi=0.3, dead=0):
    """npairs live pairs whose product pattern is exactly S (16 row masks), then `dead` pairs whose A and B tiles never meet.

    Pair j: A row r holds bit k (inner index k of the pair's k tile) and B row k holds pattern S[k] (a part of it for j > 0), so
    A row r times B meets only where some k with S[k] inside S[r] is in A's row: bit r always (pair 0), and with probability
    `multi` further k, which gives an entry two or more products in one pair.  Returns [(a_rows[16], b_cols[16])]."""
    nz = [r for r in range(16) if S[r]]
    out = []
    for j in range(npairs):
        arow, brow = [0] * 16, [0] * 16
        for k in nz:
            brow[k] = S[k] if j == 0 else S[k] & int(rng.integers(0, 1 << 16))
        for r in nz:
            if j == 0 or rng.random() < 0.8:
                arow[r] |= 1 << r
            for k in nz:
                if k != r and S[k] & ~S[r] == 0 and rng.random() < multi:
                    arow[r] |= 1 << k
        if not any(arow[r] & sum(1 << k for k in range(16) if brow[k]) for r in range(16)):   # keep the pair alive
            r = nz[int(rng.integers(len(nz)))]
            arow[r] |= 1 << r
            brow[r] = S[r]
        if rng.random() < 0.3:                   # an A entry whose B row is empty: a product that never meets
            free = [k for k in range(16) if not brow[k]]
            if free:
                arow[nz[0]] |= 1 << free[0]
        out.append((arow, _cols(brow)))
    for _ in range(dead):                        # A's only column (k = 0) is none of B's rows (k = 1): pruned, or empty
        arow, brow = [0] * 16, [0] * 16
        arow[int(rng.integers(16))] = 1
        brow[1] = 1 << int(rng.integers(16))
        out.append((arow, _cols(brow)))
    return out


def _cols(brow):
    """B tile rows -> its column masks (bit k of column c: B(k, c) stored)"""
    return [sum(1 << k for k in range(16) if (brow[k] >> c) & 1) for c in range(16)]


def build(tiles, seed):
    """tiles: per C tile a list of pairs (a_rows[16], b_cols[16]) -> dict(A=(rows, cols, I, J, V), B=..., T, K, pairs per tile)"""
    rng = np.random.default_rng(seed)
    T = len(tiles)
    am = np.array([p[0] for ps in tiles for p in ps], np.int64).reshape(-1, 16)      # [pair, row r] -> mask over the k tile
    bm = np.array([p[1] for ps in tiles for p in ps], np.int64).reshape(-1, 16)      # [pair, col c] -> mask over the k tile
    K = len(am)
    t_of = np.repeat(np.arange(T), [len(ps) for ps in tiles])
    bit = (am[:, :, None] >> np.arange(16)) & 1                                      # [pair, r, b]
    p, r, b = np.nonzero(bit)
    AI, AJ = 16 * t_of[p] + r, 16 * p + b
    bit = (bm[:, :, None] >> np.arange(16)) & 1                                      # [pair, c, b]
    p, c, b = np.nonzero(bit)
    BI, BJ = 16 * p + b, 16 * t_of[p] + c
    A = (16 * T, 16 * K, AI.astype(np.int32), AJ.astype(np.int32), _vals(rng, len(AI)))
    B = (16 * K, 16 * T, BI.astype(np.int32), BJ.astype(np.int32), _vals(rng, len(BI)))
    return dict(A=A, B=B, T=T, K=K, pairs=[len(ps) for ps in tiles])


def permute_k(ops, perm_tiles):
    """the same product through a reordered inner dimension: (A P)(P^T B) with P moving k tile q to perm_tiles[q]"""
    rows, cols, I, J, V = ops["A"]
    brows, bcols, BI, BJ, BV = ops["B"]
    perm = np.asarray(perm_tiles, np.int64)
    A = (rows, cols, I, (16 * perm[J // 16] + J % 16).astype(np.int32), V)
    B = (brows, bcols, (16 * perm[BI // 16] + BI % 16).astype(np.int32), BJ, BV)
    return dict(ops, A=A, B=B)


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
SEMIRING_SFX = dict(plus_times="", min_plus=",min_plus", max_plus=",max_plus", max_times=",max_times", plus_pair=",plus_pair",
                    lor_land=",lor_land")


def form_of(npairs, ntc, opts, semiring="plus_times", masked=False):
    o = dict(DEFAULTS, **dict(opts))
    if ntc == 0:
        return None
    deep = npairs >= 2 * ntc
    wide = (o["wide"] and not o["step1_global_sort"]) or masked
    if wide and deep:
        return "deep,band" if o["s3_band"] else "deep"
    if wide and o["s3_decode"]:
        if semiring != "plus_times":                 # the other semirings: 64-bit, shuffle search only
            return "decode"
        mark = o["s3_mark"] and o["prune"] and not masked
        idx32 = not o["s3_idx64"]                    # (every array is far below 4 GiB here)
        return "decode" + (",idx32" if idx32 else "") + (",mark" if mark else "")
    return "wide" if wide else "base"


def kernel_names(form, vt, semiring="plus_times"):
    """the step-3 kernel names of a form (s3_launch, PEM_S3_NAMES)"""
    if form is None:
        return []
    s = SEMIRING_SFX[semiring]
    if form == "base":
        return [f"s3_accumulate_kernel<{vt}{s}>"]
    if form == "wide":
        return [f"s3_accumulate_wide_kernel<{vt}{s}>"]
    if form == "deep,band":
        return sorted([f"s3_accumulate_wide_kernel<{vt},deep,band{s}>", f"s3_band_kernel<{vt}{s}>"])
    return [f"s3_accumulate_wide_kernel<{vt},{form}{s}>"]


def natural_epw_units(nnz_c, ntc, deep, cu_count=256):
    """step3_impl's choice of entries per wave / 256 without PEM_OPT_S3_EPW: 2 only where C holds 16.7 M+ entries on 256 CUs"""
    s3_many = nnz_c >= 4 * (cu_count * 32) * (2 * S3_CHUNK)
    return 2 if (ntc > 0 and nnz_c >= 8 * ntc and not deep and s3_many) else 1


def model(pairs_offset, c_tile_nnz_ptr, opts=(), semiring="plus_times", masked=False, c_mask=None, cu_count=256):
    """-> dict(form, epw, natural_epw, paths): the paths of gap 1 this plan takes (PATHS' keys)"""
    o = dict(DEFAULTS, **dict(opts))
    po = np.asarray(pairs_offset, np.int64)
    off = np.asarray(c_tile_nnz_ptr, np.int64)
    ntc = len(po) - 1
    nnz = int(off[-1]) if ntc >= 0 and len(off) else 0
    npairs = int(po[-1]) if len(po) else 0
    deep = npairs >= 2 * ntc
    form = form_of(npairs, ntc, o, semiring, masked)
    nat = natural_epw_units(nnz, ntc, deep, cu_count)
    units = o["s3_epw"] if o["s3_epw"] > 0 else nat
    epw = S3_CHUNK * units
    paths = set()
    out = dict(form=form, epw=epw, natural_epw=S3_CHUNK * nat, paths=paths)
    if form is None:
        return out
    paths.add("form:" + form)
    if form == "base" or nnz == 0:
        return out
    paths.add(f"epw:{epw}")
    paths.add(f"xcd:{int(bool(o['s3_xcd']))}")
    npt = np.diff(po)
    ent = np.diff(off)
    band = form == "deep,band"
    mark = form.endswith(",mark")
    decode = form.startswith("decode")
    if decode and c_mask is not None:
        w = np.asarray(c_mask, np.uint32).reshape(-1, 8)
        rows = np.empty((len(w), 16), np.uint32)
        rows[:, 0::2], rows[:, 1::2] = w >> 16, w & 0xFFFF
        nz = rows != 0
        last_nz = np.where(nz.any(1), 15 - np.argmax(nz[:, ::-1], axis=1), -1)
        skips_row = np.array([bool((~nz[t, :last_nz[t]]).any()) if last_nz[t] > 0 else False for t in range(len(w))])
    # tiles split across waves / trips: from the tiles' side
    for t in np.nonzero(ent > 0)[0]:
        if off[t] // epw != (off[t + 1] - 1) // epw:
            paths.add("tile_split_across_waves")
    chunk_tile = np.searchsorted(off, np.arange(0, nnz, S3_CHUNK), side="right") - 1   # step 2d: the tile entry ch * 256 lies in
    lanes = np.arange(64)
    for wave in range((nnz + epw - 1) // epw):
        e_lo, e_hi = wave * epw, min(wave * epw + epw, nnz)
        lo = int(chunk_tile[wave * (epw // S3_CHUNK)])
        assert off[lo] <= e_lo < off[lo + 1]
        paths.add("wave_starts_mid_tile" if e_lo > off[lo] else "wave_starts_at_tile")
        windows = 0
        t0 = lo
        while t0 < ntc:
            lane_off = np.where(t0 + lanes < ntc, off[np.minimum(t0 + lanes, ntc)], INT_MAX)
            tend = min(t0 + 64, ntc)
            first = int(lane_off[0])
            if first >= e_hi:
                break
            chunk_end = int(off[tend])
            e_begin, e_end = max(first, e_lo), min(chunk_end, e_hi)
            windows += e_begin < e_end
            for ebase in range(e_begin, e_end, 64):
                nvalid = min(64, e_end - ebase)
                e = ebase + lanes
                valid = lanes < nvalid
                ti = np.searchsorted(lane_off, e, side="right") - 1                      # the shuffle search
                t = t0 + ti
                tv = t[valid]
                paths.add("trip_full" if nvalid == 64 else "trip_partial")
                inner = np.nonzero((ent[t0:tend] == 0) & (lane_off[:tend - t0] > ebase) & (lane_off[:tend - t0] < ebase + nvalid))[0]
                if len(inner):
                    paths.add("empty_tile_inside_trip")
                if mark:
                    st = lane_off - ebase
                    marks = (st >= 0) & (st < 64)
                    before = int((lane_off < ebase).sum())
                    ti_mark = before - 1 + np.cumsum(np.bincount(st[marks], minlength=64)[:64])
                    assert np.array_equal(ti_mark[valid], ti[valid]), "the marked lookup disagrees with the search"
                    paths.add("mark_tile_starts_trip" if before == 0 else "mark_trip_starts_inside_tile")
                    paths.add("mark_tiles_start" if marks.any() else "mark_no_tile_starts")
                if decode and c_mask is not None:
                    for u in np.unique(tv):
                        paths.add("decode_full_tile" if ent[u] == 256 else "decode_partial_tile")
                        if skips_row[u]:
                            paths.add("decode_skips_empty_row")
                n_of = npt[tv]
                if not deep:
                    if (n_of == 1).any():
                        paths.add("sh_one_pair")
                    if (n_of == 2).any():
                        paths.add("sh_two_pairs")
                    P0 = po[tv[0]]
                    Pn = int(po[tv[-1] + 1] - P0)
                    if (n_of > 2).any():
                        if Pn <= 64:
                            paths.add("sh_staged")
                            if Pn == 64:
                                paths.add("sh_staged_pn64")
                        else:
                            paths.add("sh_unstaged")
                            if Pn == 65:
                                paths.add("sh_unstaged_pn65")
                    else:
                        paths.add("sh_no_third_pair")
                else:
                    for n in np.unique(n_of):
                        if band and n >= S3_BAND_MIN:
                            paths.add("deep_leaves_band_tile")
                            continue
                        if band and n == S3_BAND_MIN - 1:
                            paths.add("deep_keeps_np7")
                        if n >= 8:
                            paths.add("deep_quad_more")
                        if n >= 4:
                            paths.add("deep_quad_last")
                        paths.add(f"deep_rem{n % 4}")
            if chunk_end >= e_hi:
                break
            t0 += 64
        paths.add("wave_crosses_window" if windows >= 2 else "wave_one_window")
    # a tile whose entries lie in two trips of one wave: trips start at the wave's first entry, then every 64 within a window
    for t in np.nonzero(ent > 64)[0]:
        if off[t] // epw == (off[t + 1] - 1) // epw:
            paths.add("tile_split_across_trips")
    if band:
        nblocks = ((max(1, -(-ntc // 256))) + 7) & ~7
        for w in range(nblocks * 4):
            ts = np.arange(64 * w, 64 * w + 64)
            inr = ts[ts < ntc]
            big = inr[npt[inr] >= S3_BAND_MIN]
            if len(big) >= 2:
                paths.add("band_several_tiles_in_wave")
            if len(big) and len(inr) < 64:
                paths.add("band_grid_tail")
            for t in big:
                n, m = int(npt[t]), int(ent[t])
                if n == S3_BAND_MIN:
                    paths.add("band_np8")
                paths.add("band_pad" if n % 4 else "band_np_mult4")
                if n == 16:
                    paths.add("band_np16")
                if n == 17:
                    paths.add("band_np17")
                if n > 64:
                    paths.add("band_np_gt64")
                paths.add("band_sub_trips" if m > 64 else "band_one_sub")
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
def _layout(rng, spec):
    """spec: list of (entries, pairs[, empty_rows[, dead]]) per C tile -> tiles for build()"""
    tiles = []
    for s in spec:
        n, npairs = s[0], s[1]
        empty_rows = s[2] if len(s) > 2 else ()
        dead = s[3] if len(s) > 3 else 0
        if n == 0:                                   # a C tile of dead pairs only: empty when unpruned, gone when pruned
            tiles.append(pairs_for(rng, [0] * 16, 0, dead=max(dead, 1)))
            continue
        S = pattern(rng, n, empty_rows)
        tiles.append(pairs_for(rng, S, npairs, multi=0.3 if n < 200 else 0.15, dead=dead))
    return tiles


def _pad_to(spec, boundary, pairs=1):
    """one-pair tiles (at most 128 entries each) up to the next multiple of `boundary` entries"""
    n = sum(s[0] for s in spec)
    gap = (-n) % boundary
    while gap:
        k = min(gap, 128)
        spec.append((k, pairs))
        gap -= k
    return spec


def shallow_spec():
    """fewer than two pairs per tile: every shallow path, edges on both sides"""
    s = [(64, 1), (200, 2, (1, 5, 6))]                   # tile 1 crosses entry 256: wave 1 starts in it; a trip inside it marks nothing
    s += [(1, 1 + (i % 2)) for i in range(248)]          # 248 one-entry tiles: wave 1 spans four windows
    _pad_to(s, 256)
    s += [(3, 3)] + [(1, 1)] * 61                        # one trip of 64 lanes, Pn == 64: staged
    _pad_to(s, 256)
    s += [(2, 3)] + [(1, 1)] * 62                        # one trip of 64 lanes, Pn == 65: unstaged
    _pad_to(s, 256)
    s += [(256, 3), (256, 1, ()), (130, 2, (0, 15))]     # full tiles (staged, Pn == 3); empty first and last rows
    s += [(17, 5), (40, 1, (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)), (9, 4), (5, 2)] * 6
    s += [(1, 1)] * 70 + [(11, 3)]                       # ends in a partial trip
    return s


def deep_spec():
    """two or more pairs per tile: groups of four with and without a next group, remainders 0-3, band edges"""
    s = []
    for n in range(1, 14):                               # pair counts 1..13 (7 and 8 on the band edge)
        s += [(1 + (7 * n) % 60, n), (64 + n, n, (2,))]
    s += [(256, 8), (65, 10), (40, 12), (130, 16), (200, 17), (23, 70, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)), (256, 9)]
    s += [(30 + n, 2 + n % 5) for n in range(60)]        # the next waves of the band grid
    s += [(70, 11), (12, 8), (5, 3)]                     # many-pair tiles in the last (partial) 64-tile group
    return s


def unpruned_spec():
    """prune 0: dead pairs, and C tiles made only of them (empty tiles inside trips)"""
    s = []
    for i in range(120):
        s.append((1 + (i * 5) % 23, 1 + (i % 3 == 0), (), 1 if i % 4 == 0 else 0))
        if i % 9 == 4:
            s.append((0, 0))
    return s


def _c_pattern(ops):
    """C's (row, col) keys from the operands (boolean product)"""
    rows, kcols, AI, AJ, _ = ops["A"]
    _, cols, BI, BJ, _ = ops["B"]
    order = np.argsort(BI, kind="stable")
    BI, BJ = BI[order], BJ[order]
    start = np.searchsorted(BI, np.arange(kcols + 1))
    cnt = start[AJ + 1] - start[AJ]
    r = np.repeat(AI.astype(np.int64), cnt)
    idx = np.repeat(start[AJ] - np.cumsum(np.r_[0, cnt[:-1]]), cnt) + np.arange(int(cnt.sum()))
    return np.unique(r * cols + BJ[idx].astype(np.int64))


def mask_complement_for(ops, every=5):
    keys = _c_pattern(ops)
    cols = ops["B"][1]
    r, c = keys // cols, keys % cols
    t = r // 16
    assert np.array_equal(t, c // 16)
    keep_exact = t % every == 2                          # M = C's own entries: the complement keeps an empty tile
    MI, MJ = [r[keep_exact]], [c[keep_exact]]
    full_t = np.unique(t[t % every == 3])                # M holds all 256: the complement drops the tile
    rr, cc = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    for u in full_t:
        MI.append(16 * u + rr.ravel())
        MJ.append(16 * u + cc.ravel())
    return np.concatenate(MI).astype(np.int32), np.concatenate(MJ).astype(np.int32)


def _case(name, spec, seed, opts=(), reach=(), tile_rows=None, mask=None):
    return dict(name=name, spec=spec, seed=seed, opts=tuple(opts), reach=set(reach), tile_rows=tile_rows, mask=mask)


SHALLOW_REACH = {"wave_starts_at_tile", "wave_starts_mid_tile", "tile_split_across_waves", "tile_split_across_trips",
                 "wave_crosses_window", "wave_one_window", "trip_full", "trip_partial", "sh_one_pair", "sh_two_pairs",
                 "sh_staged", "sh_staged_pn64", "sh_unstaged", "sh_unstaged_pn65", "sh_no_third_pair"}
DECODE_REACH = {"decode_skips_empty_row", "decode_full_tile", "decode_partial_tile"}
MARK_REACH = {"mark_tile_starts_trip", "mark_trip_starts_inside_tile", "mark_no_tile_starts", "mark_tiles_start"}
DEEP_REACH = {"deep_quad_last", "deep_rem0", "deep_rem1", "deep_rem2", "deep_rem3", "wave_starts_mid_tile", "trip_partial"}


def cases():
    """name -> case dict (spec, seed, options, paths it must reach, tile-row range, mask)"""
    sh, dp = shallow_spec(), deep_spec()
    out = [
        _case("shallow", sh, 1, (), {"form:decode,idx32,mark", "epw:256", "xcd:1"} | SHALLOW_REACH | DECODE_REACH | MARK_REACH),
        _case("shallow_epw1_xcd0", sh, 1, (("s3_epw", 1), ("s3_xcd", 0)), {"epw:256", "xcd:0"} | SHALLOW_REACH),
        _case("shallow_epw2_xcd0", sh, 1, (("s3_epw", 2), ("s3_xcd", 0)),
              {"epw:512", "xcd:0", "wave_crosses_window", "sh_staged", "sh_unstaged", "wave_starts_mid_tile"}),
        _case("shallow_epw2_xcd1", sh, 1, (("s3_epw", 2),), {"epw:512", "xcd:1", "form:decode,idx32,mark"}),
        _case("shallow_epw4", sh, 1, (("s3_epw", 4),), {"epw:1024", "wave_crosses_window", "mark_no_tile_starts"}),
        _case("shallow_epw4_xcd0", sh, 1, (("s3_epw", 4), ("s3_xcd", 0)), {"epw:1024", "xcd:0"}),
        _case("shallow_nomark", sh, 1, (("s3_mark", 0),), {"form:decode,idx32"} | SHALLOW_REACH | DECODE_REACH),
        _case("shallow_idx64", sh, 1, (("s3_idx64", 1),), {"form:decode,mark", "sh_staged", "sh_unstaged"} | DECODE_REACH | MARK_REACH),
        _case("shallow_idx64_nomark", sh, 1, (("s3_idx64", 1), ("s3_mark", 0)), {"form:decode", "sh_staged", "sh_unstaged"} | DECODE_REACH),
        _case("shallow_nodecode", sh, 1, (("s3_decode", 0),), {"form:wide"} | SHALLOW_REACH),
        _case("shallow_base", sh, 1, (("wide", 0),), {"form:base"}),
        _case("deep_band", dp, 2, (), {"form:deep,band", "deep_leaves_band_tile", "deep_keeps_np7", "band_np8", "band_pad",
                                       "band_np_mult4", "band_np16", "band_np17", "band_np_gt64", "band_one_sub", "band_sub_trips",
                                       "band_several_tiles_in_wave", "band_grid_tail"} | DEEP_REACH),
        _case("deep_noband", dp, 2, (("s3_band", 0),), {"form:deep", "deep_quad_more"} | DEEP_REACH),
        _case("deep_noband_epw1", dp, 2, (("s3_band", 0), ("s3_epw", 1)), {"form:deep", "epw:256", "xcd:1", "deep_quad_more"}),
        _case("deep_band_epw2_xcd0", dp, 2, (("s3_epw", 2), ("s3_xcd", 0)), {"form:deep,band", "epw:512", "xcd:0"}),
        _case("unpruned", unpruned_spec(), 3, (("prune", 0),), {"form:decode,idx32", "empty_tile_inside_trip", "sh_one_pair",
                                                                "sh_two_pairs"}),
        _case("complement", sh, 4, (), {"form:decode,idx32", "empty_tile_inside_trip", "sh_staged", "sh_unstaged"},
              mask="complement"),
        _case("row_range", sh, 5, (), {"form:decode,idx32,mark", "wave_crosses_window", "sh_staged"}, tile_rows=(7, 400)),
        _case("row_range_deep", dp, 6, (), {"form:deep,band", "band_np_gt64"}, tile_rows=(3, 60)),
    ]
    return {c["name"]: c for c in out}


_OPS = {}


def operands(case):
    """(dict(A, B, T, K), mask (MI, MJ) or None) of a case, built once per (spec, seed)"""
    key = (id(case["spec"]), case["seed"])
    if key not in _OPS:
        rng = np.random.default_rng(1000 + case["seed"])
        _OPS[key] = build(_layout(rng, case["spec"]), case["seed"])
    ops = _OPS[key]
    mask = mask_complement_for(ops) if case["mask"] == "complement" else None
    return ops, mask


def plan_arrays(oracle, case):
    """the plan arrays step 3 works from, as the oracle's plan (pruned by prune_ref, masked by maskref) gives them"""
    import maskref
    import prune_ref
    ops, mask = operands(case)
    oA, oB = oracle.Tiled(*ops["A"]), oracle.Tiled(*ops["B"])
    lo, hi = case["tile_rows"] or (0, None)
    op = oracle.Plan(oA, oB, lo, hi)
    want, _ = prune_ref.expected(op, oA, oB, prune=bool(dict(DEFAULTS, **dict(case["opts"]))["prune"]))
    if mask is not None:
        n = 16 * ops["T"]
        M = oracle.Tiled(n, n, mask[0], mask[1], np.ones(len(mask[0])))
        want = maskref.restate(dict(want, tr_lo=op.tr_lo), M, complement=True)
    return want


def model_of(oracle, case, semiring="plus_times"):
    arr = plan_arrays(oracle, case)
    return model(arr["pairs_offset"], arr["c_tile_nnz_ptr"], case["opts"], semiring, case["mask"] is not None, arr["c_mask"])
