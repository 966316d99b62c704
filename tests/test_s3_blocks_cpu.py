"""Host only: the layout of tests/s3blocks.py reaches every situation the two-pair blocks of step 3 branch on.

From the oracle's plan arrays (s3cases.plan_arrays) and the trip walk of tests/s3batch.py: which lanes, pair counts and pair
ranges the kernel's trips have; from the operands' masks (s3blocks.products): how many products every (entry, pair) visit has.
A green test_gpu_s3_blocks.py is then not luck.
"""
import numpy as np

import s3batch
import s3blocks
import s3cases


def _plan(oracle, name="decode_idx32_mark"):
    arr = s3cases.plan_arrays(oracle, s3blocks.case(name))
    return arr, np.asarray(arr["pairs_offset"], np.int64), np.asarray(arr["c_tile_nnz_ptr"], np.int64)


def test_pair_and_entry_counts_are_the_spec_s(oracle):
    """every C tile owns its k tiles: the pruned plan has the spec's pairs and entries per tile, crafted tiles included"""
    _, po, off = _plan(oracle)
    assert 200 <= len(s3blocks.SPEC) <= 600
    assert np.array_equal(np.diff(po), [s[1] for s in s3blocks.SPEC])
    assert np.array_equal(np.diff(off), [s[0] for s in s3blocks.SPEC])
    assert po[-1] < 2 * (len(po) - 1), "the layout must be shallow"
    for t, ps in enumerate(s3blocks.tiles()):
        k = s3blocks.products(ps)
        live = int((k.sum(1) > 0).sum())
        assert k.shape[1] == s3blocks.SPEC[t][0] and live == s3blocks.SPEC[t][1], t


def test_layout_reaches_the_later_pair_cases(oracle):
    arr, po, off = _plan(oracle)
    tr = s3batch.trips(po, off)
    staged = [t for t in tr if t["staged"]]
    # tiles of 3 to 9 pairs alone in a trip: later-pair counts 1-7, the odd ones with a half-filled last block
    alone = {int(t["n_of"][0]) for t in staged if t["nvalid"] == 64 and len(set(t["tile"].tolist())) == 1}
    assert set(range(3, 10)) <= alone, alone
    assert {n - 2 for n in alone} >= set(range(1, 8))
    assert any(int(t["n_of"].max()) % 2 == 1 for t in staged)
    # lanes of 1, 2, 4 and 7 pairs side by side
    assert any({1, 2, 4, 7} <= set(t["n_of"].tolist()) for t in staged)
    # the staging limit on both sides
    assert any(t["Pn"] == 64 and t["staged"] and 5 in t["n_of"] and t["nvalid"] == 64 for t in tr)
    assert any(t["Pn"] == 65 and not t["staged"] and 5 in t["n_of"] for t in tr)
    # a partial last trip ending in a five-pair tile
    assert tr[-1]["nvalid"] < 64 and tr[-1]["staged"] and tr[-1]["n_of"][-1] == 5
    # a 256-entry five-pair tile split across trips and across two waves
    ent, npt = np.diff(off), np.diff(po)
    split = [u for u in np.nonzero((ent == 256) & (npt == 5))[0] if off[u] // 256 != (off[u + 1] - 1) // 256]
    assert split, "no 256-entry 5-pair tile across two waves"
    assert sum(1 for t in staged if split[0] in t["tile"]) >= 4
    m = s3cases.model(po, off, (), "plus_times", False, arr["c_mask"])
    assert {"sh_staged_pn64", "sh_unstaged_pn65", "tile_split_across_waves", "tile_split_across_trips", "trip_partial",
            "sh_one_pair", "sh_two_pairs", "sh_no_third_pair"} <= m["paths"]
    # prune = 0 keeps the dead pairs: blocks with dead pairs behind live ones, and blocks of dead pairs only; still shallow
    un = s3cases.plan_arrays(oracle, s3blocks.case("unpruned"))
    upo = np.asarray(un["pairs_offset"], np.int64)
    assert upo[-1] > po[-1] and upo[-1] < 2 * (len(upo) - 1)
    ut = s3batch.trips(upo, un["c_tile_nnz_ptr"])
    dead = [i for i, s in enumerate(s3blocks.SPEC) if len(s) > 3 and s[3]]
    assert np.array_equal(np.diff(upo)[dead], [s3blocks.SPEC[i][1] + s3blocks.SPEC[i][3] for i in dead])
    assert any(t["staged"] and {5, 7, 6} <= set(t["n_of"].tolist()) for t in ut)


def test_layout_reaches_the_live_positions_and_product_counts(oracle):
    """over the tiles that staged trips walk: where the products of an entry's visits lie, and how many a visit has"""
    _, po, off = _plan(oracle)
    in_staged = set()
    for t in s3batch.trips(po, off):
        if t["staged"]:
            in_staged |= set(t["tile"].tolist())
    all_tiles = s3blocks.tiles()
    seen = {pos: set() for pos in ("pair1", "pair2", "later_first", "later_second")}
    dead_later = only_last_odd = both_of_block = dead_first_two_second = 0
    for u in sorted(in_staged):
        k = s3blocks.products(all_tiles[u])                        # [pair, entry]
        n = len(k)
        seen["pair1"] |= set(k[0].tolist())
        if n > 1:
            seen["pair2"] |= set(k[1].tolist())
            dead_first_two_second += int(((k[0] == 0) & (k[1] == 2)).sum())
        for j in range(2, n):
            seen["later_first" if j % 2 == 0 else "later_second"] |= set(k[j].tolist())
            dead_later += int((k[j] == 0).sum())
        for j in range(2, n - 1, 2):
            both_of_block += int(((k[j] > 0) & (k[j + 1] > 0)).sum())
        if n >= 3 and n % 2 == 1:
            only_last_odd += int(((k[:-1].sum(0) == 0) & (k[-1] > 0)).sum())
    for pos, counts in seen.items():
        assert {1, 2, 3} <= counts and max(counts) >= 4, (pos, counts)    # visits with 1, 2, 3 and 4 or more products
        assert 0 in counts or pos == "pair1", (pos, counts)
    assert 0 in seen["pair1"]                                      # (a dead first pair: crafted tiles only)
    assert dead_later > 0, "no later pair meets nowhere"
    assert only_last_odd > 0, "no entry whose only product comes from the last pair of an odd count"
    assert both_of_block > 0, "no entry with products in both pairs of a later block"
    assert dead_first_two_second > 0, "no dead first pair beside a second pair with two products"
