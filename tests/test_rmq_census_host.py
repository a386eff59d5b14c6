"""The inputs of tests/test_gpu_rmq_edges.py reach what they are there for -- asserted on the CPU, with the oracle and the plain model of
tests/_rmq_census.py only, so that the GPU tests cannot quietly stop reaching a regime of k_rmq_sort / k_rmq_dp.

1. The model (mg_lchain_rmq's fill restated without the trees) gives the oracle's f, p and v (orc.rmq_fill) in every pass that it runs
   to the end, on every input under every option set the GPU test uses.  That is what makes its predictions trustworthy.
2. Every class of the census has a count above 0 on the input and option set named in NEEDS, in a pass that ends without an event,
   i.e. on a read the device must chain itself (`python tests/_rmq_census.py` prints the table below).
3. The host is the exception: under every option set at most a quarter of a world's reads are predicted HOST / HOST_ALL, except under
   the sets made for the events, where HOST_READS names every such read.

Run time: 2.8 min on the CPU (tests/test_chain_census_host.py: 1.8 min on the same machine); the census script alone: 50 s.

The census (per read for the read, sort, rescue and event classes, per anchor of the passes that run to the end for the others):

| class | edges_ont default | edges_asm20 default | edges_asm20 cap_100 | edges_asm20 inner_0 | edges_ont rescue_ratio_1 | edges_ont cap_neg | edges_asm5 default | edges_hifi default | wide_ont gap_16000 | wide_asm20 gap_16000 | wide_asm20 gap_16000_cap_1000 | arrays_ont default | arrays_ont gap_scale_0_inner_0 | arrays_asm20 gap_scale_0_inner_0 | arrays_hifi default | arrays_hifi gap_scale_0 |
|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|
| reads | 19 | 22 | 22 | 22 | 19 | 19 | 22 | 21 | 3 | 3 | 3 | 10 | 10 | 8 | 8 | 8 |
| anchors | 24159 | 49537 | 49537 | 46410 | 23191 | 0 | 42012 | 20417 | 41945 | 66917 | 66917 | 3897 | 10342 | 7707 | 2947 | 1565 |
| n_le_64 | 1 | 3 | 3 | 3 | 0 | 0 | 3 | 1 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 |
| n_not_mult_64 | 12 | 32 | 32 | 31 | 10 | 0 | 32 | 15 | 3 | 6 | 6 | 3 | 5 | 5 | 4 | 2 |
| n_gt_512 | 12 | 28 | 28 | 28 | 11 | 0 | 28 | 14 | 3 | 6 | 6 | 3 | 5 | 5 | 4 | 2 |
| n_gt_2048 | 5 | 7 | 7 | 6 | 5 | 0 | 3 | 2 | 3 | 6 | 6 | 0 | 3 | 1 | 0 | 0 |
| strand_change | 11 | 26 | 26 | 26 | 10 | 0 | 26 | 13 | 3 | 6 | 6 | 0 | 0 | 0 | 0 | 0 |
| run_ge_2 | 6 | 16 | 16 | 16 | 6 | 0 | 16 | 8 | 3 | 6 | 6 | 3 | 5 | 4 | 4 | 2 |
| run_cross_64 | 2 | 9 | 9 | 9 | 2 | 0 | 11 | 5 | 3 | 6 | 6 | 3 | 5 | 3 | 4 | 2 |
| sort_le_64 | 1 | 1 | 1 | 1 | 0 | 1 | 1 | 1 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 |
| sort_gt_64 | 15 | 17 | 17 | 17 | 13 | 15 | 17 | 17 | 3 | 3 | 3 | 9 | 9 | 1 | 6 | 6 |
| sort_gt_stage | 5 | 3 | 3 | 2 | 5 | 5 | 1 | 2 | 3 | 3 | 3 | 3 | 3 | 0 | 1 | 1 |
| rescue_size | 13 | 15 | 15 | 15 | 13 | 13 | 16 | 16 | 3 | 3 | 3 | 0 | 0 | 0 | 0 | 0 |
| rescue_ratio_only | 3 | 3 | 3 | 3 | 0 | 3 | 2 | 2 | 0 | 0 | 0 | 9 | 9 | 1 | 6 | 6 |
| rescue_no | 0 | 0 | 0 | 0 | 3 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 |
| one_chain | 3 | 1 | 1 | 1 | 3 | 3 | 1 | 3 | 0 | 0 | 0 | 1 | 1 | 4 | 2 | 2 |
| win_empty | 213 | 663 | 663 | 663 | 190 | 0 | 733 | 309 | 34 | 62 | 62 | 3 | 5 | 6 | 4 | 2 |
| win_no_block | 12463 | 20348 | 31745 | 20319 | 12151 | 0 | 18200 | 9367 | 6670 | 10476 | 10476 | 189 | 315 | 378 | 252 | 126 |
| win_blocks | 11483 | 28526 | 17129 | 25428 | 10850 | 0 | 23079 | 10741 | 35241 | 56379 | 56379 | 3705 | 10022 | 7323 | 2691 | 1437 |
| blk_inside | 62241 | 146859 | 12899 | 122557 | 58830 | 0 | 129470 | 73626 | 348767 | 567912 | 331160 | 26147 | 98543 | 57209 | 10512 | 5787 |
| blk_cut_lo | 0 | 276 | 0 | 276 | 0 | 0 | 224 | 0 | 13692 | 17205 | 13965 | 0 | 0 | 0 | 0 | 0 |
| blk_cut_hi | 4807 | 23609 | 3958 | 17392 | 4797 | 0 | 16447 | 4011 | 67098 | 175982 | 142121 | 13308 | 63502 | 29530 | 5192 | 3095 |
| blk_outside | 5101 | 9110 | 272 | 5715 | 5081 | 0 | 6249 | 2574 | 16228 | 58560 | 39692 | 1587 | 5432 | 2267 | 305 | 249 |
| blk_btie_not_min | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 587 | 670 | 0 | 192 |
| win_hbm_prefix | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 9903 | 10405 | 0 | 0 | 1473 | 121 | 0 | 0 |
| winner_in_prefix | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 65 | 487 | 0 | 0 | 0 | 0 | 0 | 0 |
| cap_moves_st | 0 | 0 | 26837 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 23847 | 0 | 0 | 0 | 0 | 0 |
| cap_moves_st_in | 0 | 0 | 11587 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 |
| winner_none | 710 | 1796 | 1869 | 1796 | 679 | 0 | 1828 | 793 | 348 | 533 | 548 | 3 | 5 | 6 | 4 | 2 |
| winner_near | 23422 | 47416 | 47668 | 44174 | 22485 | 0 | 39899 | 19572 | 41406 | 63696 | 64998 | 3040 | 7648 | 6241 | 2943 | 1563 |
| winner_far | 27 | 325 | 0 | 440 | 27 | 0 | 285 | 52 | 191 | 2688 | 1371 | 854 | 2689 | 1460 | 0 | 0 |
| winner_width_rejected | 0 | 3282 | 2069 | 4251 | 0 | 0 | 2937 | 0 | 0 | 4803 | 4150 | 0 | 0 | 1947 | 0 | 0 |
| winner_exact | 16201 | 32334 | 33450 | 29327 | 15469 | 0 | 27857 | 14820 | 29303 | 44831 | 45733 | 2120 | 5073 | 4729 | 1645 | 887 |
| winner_eq_y_j0 | 3 | 14 | 14 | 14 | 3 | 0 | 13 | 2 | 2 | 1 | 1 | 0 | 0 | 0 | 0 | 0 |
| inner_off | 0 | 0 | 0 | 15287 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 5264 | 2972 | 0 | 0 |
| inner_ascending | 4860 | 9482 | 8623 | 0 | 4668 | 0 | 6447 | 2606 | 3475 | 8474 | 7825 | 76 | 0 | 0 | 141 | 44 |
| inner_checked | 1736 | 3926 | 3706 | 0 | 1731 | 0 | 3655 | 1456 | 8084 | 11645 | 11383 | 26 | 0 | 0 | 43 | 13 |
| inner_sorted | 62 | 319 | 246 | 0 | 62 | 0 | 472 | 161 | 80 | 172 | 171 | 1672 | 0 | 0 | 1114 | 619 |
| inner_gt_64 | 1734 | 4727 | 3502 | 0 | 1638 | 0 | 1865 | 424 | 1844 | 5370 | 4852 | 1488 | 0 | 0 | 811 | 467 |
| break_first_batch | 1974 | 5600 | 4659 | 0 | 1867 | 0 | 2664 | 671 | 4186 | 7967 | 7353 | 614 | 0 | 0 | 821 | 358 |
| break_later_batch | 126 | 161 | 148 | 0 | 126 | 0 | 73 | 58 | 233 | 286 | 286 | 120 | 0 | 0 | 173 | 143 |
| skip_carried | 130 | 161 | 161 | 0 | 130 | 0 | 120 | 105 | 422 | 466 | 448 | 65 | 0 | 0 | 153 | 120 |
| break_lane_0 | 13 | 23 | 23 | 0 | 13 | 0 | 6 | 2 | 44 | 39 | 37 | 3 | 0 | 0 | 7 | 3 |
| break_lane_63 | 2 | 10 | 10 | 0 | 2 | 0 | 6 | 1 | 40 | 40 | 41 | 3 | 0 | 0 | 4 | 3 |
| walk_improves | 469 | 2578 | 1296 | 0 | 469 | 0 | 2148 | 276 | 1124 | 4163 | 3242 | 24 | 0 | 0 | 269 | 16 |
| tie_lane | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 3 | 2 | 0 | 2 |
| tie_summary | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 1 | 1 | 0 | 1 |
| tie_btie | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 1 | 0 | 0 | 0 |
| tie_hbm | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 |
| inner_capacity | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 6 | 0 | 0 | 2 | 1 |
| cap_negative | 0 | 0 | 0 | 0 | 0 | 16 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 0 |

Not reached by any input:
  tie_hbm    two equal minimal priorities of which one lies in the HBM prefix of the window, more than RQ_WRING - WAVE = 1984 anchors
             back.  The minimal priority belongs to the anchor with the largest f + 0.5 pen_gap (x + y); an anchor 1984 places back in
             x loses to the continuation of its own chain unless every anchor since lies outside the y range, and then two such anchors
             must still agree in all 53 bits.  None of the 200 tandem reads, of the wide reads or of the edge reads has one under any
             option set here (chain_gap_scale = 0 included); the HBM prefix itself and a winner inside it are reached (win_hbm_prefix,
             winner_in_prefix), and the tie rule there is the lane-level one.
Sizes: the primary pass (asm20) sees exactly 1, 64, 65, 511, 512, 513, 2047, 2048 and 2049 anchors.  The long-join pass cannot see 1
(two chains of min_cnt = 3 anchors at least), and its count moves in steps with the read's length (a chain enters or leaves whole): map-ont
gets 64, 65, 511, 512, 513 and 2048, map-hifi 64 to 513 and 2047, 2048, 2049."""
import collections

import pytest

import _rmq_census as RC
import _rmq_worlds as W

RUN_IDS = [(world, opts) for world, sets in W.RUNS.items() for opts in sets]


def _total(world, opts):
    tot = collections.Counter()
    for pd in W.predictions(world, opts):
        tot.update(pd["census"])
    return tot


@pytest.mark.parametrize("world,opts", RUN_IDS, ids=lambda x: x)
def test_model_is_the_oracles_fill(built, world, opts):
    """(the comparison itself sits in W.predictions, so that no prediction is ever used unchecked)"""
    pds = W.predictions(world, opts)
    n_cmp = sum(len(a) for pd in pds for _, a, _, r in pd["passes"] if r["event"] is None)
    n_ev = sum(r["event"] is not None for pd in pds for _, _, _, r in pd["passes"])
    assert n_cmp > 1000 or (opts in W.EVENT_SETS or opts == "cap_0") and n_cmp + n_ev > 0, (world, opts, n_cmp, n_ev)


# class -> (world, option set): where the class must occur
_E, _A, _G = ("edges_ont", "default"), ("edges_asm20", "default"), ("arrays_ont", "gap_scale_0_inner_0")
NEEDS = dict(
    [(key, _E) for key in RC.READ_KEYS if key != "n_le_64"] + [("n_le_64", _A)]
    + [("sort_le_64", _A), ("sort_gt_64", _E), ("sort_gt_stage", _E)]
    + [("rescue_size", _E), ("rescue_ratio_only", _E), ("one_chain", _E), ("rescue_no", ("edges_ont", "rescue_ratio_1"))]
    + [(key, _E) for key in ("win_empty", "win_no_block", "win_blocks", "blk_inside", "blk_cut_hi", "blk_outside")]
    + [("blk_cut_lo", _A), ("blk_btie_not_min", _G), ("win_hbm_prefix", ("wide_ont", "gap_16000")), ("winner_in_prefix", ("wide_ont", "gap_16000")),
       ("cap_moves_st", ("edges_ont", "cap_100")), ("cap_moves_st_in", ("edges_ont", "cap_100"))]
    + [(key, _E) for key in ("winner_none", "winner_near", "winner_far", "winner_exact", "winner_eq_y_j0")] + [("winner_width_rejected", _A)]
    + [(key, _E) for key in RC.INNER_KEYS if key != "inner_off"] + [("inner_off", ("edges_ont", "inner_0"))]
    + [("tie_lane", _G), ("tie_summary", _G), ("tie_btie", _G), ("inner_capacity", ("arrays_ont", "default")), ("cap_negative", ("edges_ont", "cap_neg"))])
NOT_REACHED = ("tie_hbm",)
# the same classes where another world or option set is what makes them
ALSO = [("win_hbm_prefix", "wide_ont", "gap_12000"), ("win_hbm_prefix", "wide_ont", "gap_20000"), ("win_hbm_prefix", "wide_asm20", "gap_16000"),
        ("winner_in_prefix", "wide_asm20", "gap_16000"), ("n_gt_2048", "wide_asm20", "gap_16000"), ("cap_moves_st", "wide_ont", "gap_16000_cap_1000"),
        ("cap_moves_st", "edges_asm20", "cap_1"), ("cap_moves_st", "edges_ont", "cap_1000"), ("cap_moves_st_in", "edges_asm20", "cap_100"),
        ("winner_far", "edges_asm20", "default"), ("winner_far", "edges_asm5", "default"), ("winner_far", "edges_hifi", "default"),
        ("inner_off", "edges_asm20", "inner_0"), ("inner_sorted", "arrays_hifi", "default"), ("inner_sorted", "edges_asm20", "default"),
        ("skip_carried", "edges_ont", "skip_60"), ("break_first_batch", "edges_ont", "skip_0"), ("rescue_no", "edges_ont", "rescue_size_100000"),
        ("rescue_ratio_only", "edges_ont", "rescue_ratio_0"), ("rescue_size", "edges_ont", "rescue_size_0"),
        ("tie_lane", "edges_ont", "gap_scale_0"), ("tie_lane", "edges_asm20", "gap_scale_0"), ("tie_summary", "arrays_hifi", "gap_scale_0"),
        ("tie_summary", "arrays_asm20", "gap_scale_0_inner_0"), ("inner_capacity", "edges_asm20", "inner_20000"),
        ("inner_capacity", "arrays_hifi", "default"), ("cap_negative", "edges_asm20", "cap_neg")]


def test_every_class_is_reached(built):
    assert set(NEEDS) | set(NOT_REACHED) == set(RC.ALL_KEYS) and not set(NEEDS) & set(NOT_REACHED)
    for key, (world, opts) in NEEDS.items():
        assert _total(world, opts)[key] > 0, (key, world, opts)
    for key, world, opts in ALSO:
        assert _total(world, opts)[key] > 0, (key, world, opts)
    for world, opts in RUN_IDS:
        for key in NOT_REACHED:
            assert _total(world, opts)[key] == 0, (key, world, opts)      # (it moves into NEEDS the day an input reaches it)


def test_every_size_is_seen(built):
    seen = lambda world: {len(pd["passes"][0][1]) for pd in W.predictions(world, "default") if pd["passes"]}
    assert set(W.SIZES) <= seen("edges_asm20")
    assert {64, 65, 511, 512, 513, 2048} <= seen("edges_ont")
    assert {64, 65, 511, 512, 513, 2047, 2048, 2049} <= seen("edges_hifi")
    for world in ("edges_ont", "edges_asm20"):
        names = list(W.WORLDS[world]()["reads"])
        pds = W.predictions(world, "default")
        for nm in ("random", "empty", "tiny"):                            # reads without anchors: no pass, nothing counted
            pd = pds[names.index(nm)]
            assert pd["state"] == RC.KEEP and not pd["passes"] and not any(pd["stats"].values()), (world, nm)


# every read the device must hand to the host under the sets made for the events and on the tandem reads, by name
HOST_READS = {
    ("edges_ont", "cap_neg"): "plain_fwd plain_rev chimera deletion insertion transposed duplicated sv0 sv1 sv2 n_64 n_65 n_511 n_512 n_513 n_2048",
    ("edges_ont", "inner_20000"): "plain_fwd plain_rev deletion insertion transposed duplicated sv0 sv1 n_511 n_512 n_513 n_2048",
    ("edges_ont", "gap_scale_0"): "plain_fwd plain_rev deletion insertion transposed duplicated sv0 sv1 sv2 n_2048",
    ("edges_asm20", "cap_neg"): "plain_fwd plain_rev chimera deletion insertion transposed duplicated sv0 sv1 sv2 n_1 n_64 n_65 n_511 n_512 n_513 n_2047 n_2048 n_2049",
    ("edges_asm20", "inner_20000"): "plain_fwd plain_rev deletion insertion transposed duplicated sv0 sv1 n_511 n_512 n_513 n_2047 n_2048 n_2049",
    ("edges_asm20", "gap_scale_0"): "plain_fwd plain_rev chimera deletion insertion transposed duplicated sv0 sv1 sv2 n_2047 n_2048 n_2049",
    ("arrays_ont", "default"): "t3 t26 t28 t57 t111 t127",
    ("arrays_ont", "gap_scale_0_inner_0"): "t3 t7 t57 t127",
    ("arrays_asm20", "default"): "t3 t111 t127",
    ("arrays_asm20", "gap_scale_0_inner_0"): "t3 t127 t151",
    ("arrays_hifi", "default"): "t76 t127",
    ("arrays_hifi", "gap_scale_0"): "t9 t21 t76 t127",
}


@pytest.mark.parametrize("world,opts", RUN_IDS, ids=lambda x: x)
def test_the_host_is_the_exception(built, world, opts):
    names = list(W.WORLDS[world]()["reads"])
    pds = W.predictions(world, opts)
    host = [nm for nm, pd in zip(names, pds) if pd["state"] >= RC.HOST]
    if (world, opts) in HOST_READS:
        assert opts in W.EVENT_SETS or world.startswith("arrays_")
        assert host == HOST_READS[(world, opts)].split(), (world, opts, host)
    else:
        assert opts not in W.EVENT_SETS and 4 * len(host) <= len(names), (world, opts, host)
    # MM_F_RMQ presets hand a read over whole (HOST_ALL) when the primary pass meets the event, the others after the sort (HOST)
    primary = W.PRESET[world.split("_")[1]] in ("asm20", "asm5")
    for pd in pds:
        if pd["state"] >= RC.HOST:
            assert (pd["state"] == RC.HOST_ALL) == (primary and pd["passes"][-1][0] == "primary")


def test_one_batch_mixes_keep_done_and_host(built):
    for world, opts in (("arrays_hifi", "default"), ("arrays_ont", "gap_scale_0_inner_0"), ("edges_ont", "gap_scale_0"), ("edges_asm20", "inner_20000")):
        states = {pd["state"] for pd in W.predictions(world, opts)}
        assert {RC.KEEP, RC.DONE} <= states and states & {RC.HOST, RC.HOST_ALL}, (world, opts, states)
