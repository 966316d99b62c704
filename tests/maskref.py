"""numpy restatement of the masked product's filter and AND (mask.hip, s2_tiles_kernel<.., MASKED>).

`restate(plan, M, complement)` works from the arrays of an UNMASKED plan (the device's, or the tiled oracle's) and the tiled
arrays of M, and gives every array the masked plan must hold: the C tiles whose (row, column) M holds (complement: does not hold,
or holds with fewer than 256 entries), their pairs, their masks ANDed with M's tile there (complement: with its inverse), the
entry offsets and M's tile id per kept tile.  `filter_csr` is the same product on a CSR C: its entries at M's stored positions.
"""
import numpy as np


def _get(obj, name):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


def m_packed(m_masks):
    """M's 16 row masks per tile -> the C-mask packing (uint32 word q = row 2q << 16 | row 2q+1), shape (T, 8)"""
    m = np.asarray(m_masks, np.uint32).reshape(-1, 16)
    return (m[:, 0::2] << 16) | m[:, 1::2]


def m_tile_lookup(M, rows, cols):
    """M's tile id at tile (rows[k], cols[k]), -1 where M has none"""
    rowptr, colidx = np.asarray(_get(M, "tile_rowptr"), np.int64), np.asarray(_get(M, "tile_colidx"), np.int64)
    width = int(_get(M, "tile_cols")) + 1
    mrow = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    mkey = mrow * width + colidx                        # ascending: rows ascend, columns ascend inside a row
    key = np.asarray(rows, np.int64) * width + np.asarray(cols, np.int64)
    pos = np.searchsorted(mkey, key)
    found = pos < len(mkey)
    found[found] = mkey[pos[found]] == key[found]
    return np.where(found, pos, -1)


def rowcolidx(c_mask):
    """Ctiles_rowColIdx: the (r << 4 | c) bytes of every tile's entries, row-major, from the packed masks"""
    w = np.asarray(c_mask, np.uint32).reshape(-1, 8)
    rows = np.empty((len(w), 16), np.uint32)
    rows[:, 0::2], rows[:, 1::2] = w >> 16, w & 0xFFFF
    bits = (rows[:, :, None] >> np.arange(16, dtype=np.uint32)) & 1          # [tile, r, c]
    t, r, c = np.nonzero(bits)
    return ((r << 4) | c).astype(np.uint8)


def popcounts(c_mask):
    w = np.asarray(c_mask, np.uint32).reshape(-1, 8)
    return np.unpackbits(w.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


def restate(plan, M, complement=False, tr_lo=None):
    """The masked plan's arrays from an unmasked plan's (dict or object with the pem_cplan_array names)."""
    rowptr = np.asarray(_get(plan, "c_tile_rowptr"), np.int64)
    colidx = np.asarray(_get(plan, "c_tile_colidx"), np.int64)
    poff = np.asarray(_get(plan, "pairs_offset"), np.int64)
    pa, pb = np.asarray(_get(plan, "pairs_a"), np.int32), np.asarray(_get(plan, "pairs_b"), np.int32)
    cmask = np.asarray(_get(plan, "c_mask"), np.uint32).reshape(-1, 8)
    if tr_lo is None:
        tr_lo = int(_get(plan, "tr_lo")) if not isinstance(plan, dict) else int(plan.get("tr_lo", 0))
    TC = len(colidx)
    trow = tr_lo + np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    mt = m_tile_lookup(M, trow, colidx)
    mp = m_packed(_get(M, "masks"))
    if complement:
        full = np.zeros(TC, bool)
        full[mt >= 0] = np.all(mp[mt[mt >= 0]] == 0xFFFFFFFF, axis=1)
        keep = ~full
    else:
        keep = mt >= 0
    kept = np.nonzero(keep)[0]
    # pairs of the kept tiles, in order
    npair = np.diff(poff)[kept]
    first = poff[:-1][kept]
    sel = np.repeat(first - np.concatenate(([0], np.cumsum(npair)[:-1])), npair) + np.arange(int(npair.sum()))
    sel = sel.astype(np.int64)
    # masks ANDed with M's tile (complement: its inverse; no M tile: nothing to AND)
    m = cmask[kept].copy()
    kmt = mt[kept]
    has = kmt >= 0
    mw = mp[kmt[has]]
    m[has] &= ~mw if complement else mw
    cnt = popcounts(m)
    keep_scan = np.concatenate(([0], np.cumsum(keep)))
    out = dict(
        c_tile_rowptr=keep_scan[rowptr].astype(np.int32),
        c_tile_rowidx=trow[kept].astype(np.int32),
        c_tile_colidx=colidx[kept].astype(np.int32),
        pairs_offset=np.concatenate(([0], np.cumsum(npair))).astype(np.int32),
        pairs_a=pa[sel], pairs_b=pb[sel],
        c_mask=m.reshape(-1).astype(np.uint32),
        c_tile_nnz_ptr=np.concatenate(([0], np.cumsum(cnt))).astype(np.int32),
        c_mtile=kmt.astype(np.int32),
    )
    out["c_rowcolidx"] = rowcolidx(out["c_mask"])
    out.update(ntiles_c=len(kept), npairs=len(sel), nnz_c=int(cnt.sum()))
    return out


def pattern_keys(rows, cols, ncols):
    return np.asarray(rows, np.int64) * int(ncols) + np.asarray(cols, np.int64)


def filter_csr(rowptr, colidx, vals, m_rows, m_cols, ncols, complement=False, row0=0):
    """CSR C (rows row0..) restricted to M's stored positions (complement: to the others) -> CSR"""
    rowptr = np.asarray(rowptr, np.int64)
    r = row0 + np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    inm = np.isin(pattern_keys(r, colidx, ncols), pattern_keys(m_rows, m_cols, ncols))
    keep = ~inm if complement else inm
    counts = np.bincount(r[keep] - row0, minlength=len(rowptr) - 1)
    return (np.concatenate(([0], np.cumsum(counts))).astype(np.int32), np.asarray(colidx)[keep].astype(np.int32),
            np.asarray(vals)[keep])
