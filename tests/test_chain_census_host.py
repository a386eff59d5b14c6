"""The inputs of tests/test_gpu_chain_edges.py reach what they are there for -- asserted on the CPU, with the oracle and the plain model of
tests/_chain_census.py only, so that the GPU tests cannot quietly stop reaching a branch of the chain-fill kernels.

1. The model's literal half (mg_lchain_dp's fill restated in Python, float32 mg_log2 included) gives the oracle's f, p, v and t on every
   input under every option set the GPU test uses.
2. Every class of the census has a count above 0 on the input and option set named in NEEDS (`python tests/_chain_census.py` prints the
   whole table).
3. The mark ring on the mosaic read.  tw[] keeps 15 bits of the marking anchor in 8192 slots; a slot none of whose aliases (s + 8192 k)
   is written for 32768 anchors answers "marked" for s + 32768 at anchor i + 32768.  How often that happens depends on WHEN the marks are
   written.  In the order of the reference loop (one mark per j walked, none behind a break) the read gives false answers under
   max_chain_skip = 1, and two anchors get another f / p.  The wave writes the marks of all 64 lanes of a batch before it reads any, the
   lanes behind a break included, so in a co-linear stretch every slot is rewritten by the next anchors and a mark last written at anchor
   i belongs to a j at least a batch's reach behind i: with max_chain_skip = 1 the scan has broken long before it gets that far, and the
   kernel's own order gives no false answer on this read under that set or the default.  It does where the window, not the break, ends
   the scan: max_chain_iter = 3 with max_chain_skip = 0 gives 56 false answers and two anchors (131377, 131378) with another f / p.
   Clearing the table whenever (i & 0x7fff) == 0 (CLEARED_RING, what the kernel does now) gives none under any of the sets; that run is
   at the same time the literal fill that is compared with the oracle.

The census (`python tests/_chain_census.py`, about a minute on the CPU; counts over the anchors of segments of more than 32 anchors, the
segment classes over all segments):

| class | stages default | stages iter_40 | stages skip_60 | arrays default | arrays iter_8000 | arrays skip_1 | mosaic skip_1 |
|---|---|---|---|---|---|---|---|
| anchors | 14458 | 14458 | 14458 | 15333 | 15333 | 15333 | 150312 |
| seg_1 | 47 | 47 | 47 | 3 | 3 | 3 | 4 |
| seg_2_31 | 203 | 203 | 203 | 0 | 0 | 0 | 4 |
| seg_32 | 2 | 2 | 2 | 0 | 0 | 0 | 0 |
| seg_33 | 2 | 2 | 2 | 0 | 0 | 0 | 0 |
| seg_longer | 88 | 88 | 88 | 4 | 4 | 4 | 1 |
| start_lane_63 | 2 | 2 | 2 | 0 | 0 | 0 | 0 |
| last_end_next_64 | 61 | 61 | 61 | 0 | 0 | 0 | 0 |
| last_end_beyond_512 | 2 | 2 | 2 | 4 | 4 | 4 | 1 |
| last_end_beyond_chunk | 2 | 2 | 2 | 1 | 1 | 1 | 1 |
| last_end_read_end | 2 | 2 | 2 | 3 | 3 | 3 | 0 |
| read_multi_chunk | 2 | 2 | 2 | 1 | 1 | 1 | 1 |
| win_le_128 | 9425 | 12598 | 9425 | 516 | 516 | 516 | 129 |
| win_129_896 | 3173 | 0 | 3173 | 3072 | 3072 | 3072 | 768 |
| win_gt_896 | 0 | 0 | 0 | 11742 | 11742 | 11742 | 149403 |
| st_jump_64 | 26 | 0 | 26 | 0 | 1 | 0 | 0 |
| iter_clamp | 0 | 8171 | 0 | 4651 | 1123 | 4651 | 0 |
| batches_1 | 9604 | 12508 | 7786 | 3953 | 3953 | 15020 | 70450 |
| batches_2 | 2290 | 0 | 3651 | 1831 | 1831 | 161 | 1281 |
| batches_3up | 614 | 0 | 1071 | 9542 | 9542 | 145 | 78568 |
| break_first_batch | 3803 | 2375 | 1492 | 3849 | 3849 | 15012 | 70388 |
| break_later_batch | 862 | 0 | 973 | 10605 | 10605 | 193 | 34838 |
| break_lane_0 | 45 | 0 | 37 | 153 | 153 | 4 | 548 |
| break_lane_63 | 58 | 0 | 50 | 167 | 167 | 13 | 574 |
| skip_carried | 2656 | 0 | 4474 | 11275 | 11275 | 137 | 32188 |
| reflect | 0 | 0 | 0 | 8 | 8 | 3 | 0 |
| tie_in_batch | 4632 | 4632 | 4632 | 12359 | 12359 | 13078 | 71567 |
| far_batch | 614 | 0 | 1071 | 9542 | 9542 | 145 | 78568 |
| rescan | 50 | 49 | 50 | 0 | 0 | 0 | 0 |
| rescan_tie | 1 | 1 | 1 | 0 | 0 | 0 | 0 |
| rescue_wins | 0 | 0 | 0 | 0 | 0 | 43 | 4 |
| maxii_gt_128 | 0 | 0 | 0 | 1156 | 1156 | 1561 | 313 |
| maxii_gt_896 | 0 | 0 | 0 | 388 | 388 | 388 | 0 |
| v_far | 4 | 0 | 4 | 32 | 32 | 16 | 10956 |
| idx_ge_32768 | 0 | 0 | 0 | 0 | 0 | 0 | 117532 |

Not reached by any input: none.  max_chain_iter = 8000 is reached as a clamp of st (iter_clamp on the tiled read) but no scan there runs
5000 anchors far before it breaks, so no f or p depends on the value (test_option_sets_reach_the_fill)."""
import functools

import numpy as np
import pytest

import _chain_census as CC
import _chain_worlds as W


def _equal(r, orc, a, qlen, label):
    ef, ep, ev, et = orc.chain_fill(a, qlen)
    assert np.array_equal(r["f"], ef), label
    assert np.array_equal(r["p"], ep), label
    assert np.array_equal(r["v"], ev), label
    assert np.array_equal(r["t"], et), label
    return ef, ep


@functools.lru_cache(maxsize=None)
def _census(world, opts, k=None, w=None):
    """read name -> census counts of `world` under the option set `opts`; the restatement is compared with the oracle on the way"""
    wd = W.WORLDS[world]()
    orc = W.oracle_for(wd, W.OPTION_SETS[opts], k, w)
    out = {}
    for name, rd in wd["reads"].items():
        c, a, r = CC.census(orc, rd)
        _equal(r, orc, a, len(rd), (world, opts, k, w, name))
        out[name] = c
    return out


def _total(world, opts):
    tot = CC.collections.Counter()
    for c in _census(world, opts).values():
        tot.update(c)
    return tot


@pytest.mark.parametrize("opts", list(W.OPTION_SETS))
def test_restatement_is_the_oracles_fill(built, opts):
    for world in W.WORLDS:
        assert sum(c["anchors"] for c in _census(world, opts).values()) > 10000


@pytest.mark.parametrize("kw", W.KW_SETS, ids=lambda kw: "k%d_w%d" % kw)
def test_restatement_other_k_w(built, kw):
    cs = _census("arrays", "default", *kw)
    assert sum(c["anchors"] for c in cs.values()) > 3000 and sum(c["seg_longer"] for c in cs.values()) >= 4


# class -> (world, option set): where the class must occur
NEEDS = dict([(key, ("stages", "default")) for key in CC.SEGMENT_KEYS] + [
    ("win_le_128", ("stages", "default")), ("win_129_896", ("stages", "default")), ("win_gt_896", ("arrays", "default")),
    ("st_jump_64", ("stages", "default")), ("iter_clamp", ("arrays", "default")),
    ("batches_1", ("stages", "default")), ("batches_2", ("stages", "default")), ("batches_3up", ("stages", "default")),
    ("break_first_batch", ("stages", "default")), ("break_later_batch", ("stages", "default")),
    ("break_lane_0", ("stages", "default")), ("break_lane_63", ("stages", "default")), ("skip_carried", ("stages", "default")),
    ("reflect", ("arrays", "default")), ("tie_in_batch", ("stages", "default")), ("far_batch", ("stages", "default")),
    ("rescan", ("stages", "default")), ("rescan_tie", ("stages", "default")), ("rescue_wins", ("arrays", "skip_1")),
    ("maxii_gt_128", ("arrays", "default")), ("maxii_gt_896", ("arrays", "default")), ("v_far", ("stages", "default"))])
# the same classes where another option set is what makes them: the clamp at every max_chain_iter, the carried n_skip at its largest
ALSO = [("iter_clamp", "arrays", "iter_8000"), ("iter_clamp", "stages", "iter_40"), ("iter_clamp", "stages", "iter_200"),
        ("win_gt_896", "arrays", "iter_8000"), ("skip_carried", "stages", "skip_60"), ("break_first_batch", "stages", "skip_0"),
        ("rescue_wins", "arrays", "skip_0"), ("rescue_wins", "arrays", "skip_3")]


def test_every_class_is_reached(built):
    assert set(NEEDS) == set(CC.ALL_KEYS) - set(CC.RING_KEYS)
    for key, (world, opts) in NEEDS.items():
        assert _total(world, opts)[key] > 0, (key, world, opts)
    for key, world, opts in ALSO:
        assert _total(world, opts)[key] > 0, (key, world, opts)
    # the tiled read alone: windows of more than 5000 and of more than 8000 anchors
    assert _census("arrays", "default")["tiled"]["iter_clamp"] > 1000 and _census("arrays", "iter_8000")["tiled"]["iter_clamp"] > 100


def test_option_sets_reach_the_fill(built):
    """every option set but three changes the f or p of some anchor of the two worlds (the oracle's fill against its fill under the
    defaults).  max_frag_len = 800 lies below every read's length, so max_dist_x falls back to max_gap and nothing may change.
    max_frag_len = 20000 lifts max_dist_x of the reads shorter than 15 kb; max_dist_y and bw still refuse every j that far back, so f and
    p stay, but k_chain_segments cuts fewer, longer segments.
    max_chain_iter = 8000 moves st on the tiled read (the census: iter_clamp under either value), but every scan there has broken long
    before it gets 5000 anchors far, so no f or p depends on it: nothing is claimed for it"""
    for opts, fields in W.OPTION_SETS.items():
        if opts in ("default", "iter_8000"):
            continue
        n_diff = 0
        for world in W.WORLDS:
            wd = W.WORLDS[world]()
            o0, o1 = W.oracle_for(wd), W.oracle_for(wd, fields)
            for rd in wd["reads"].values():
                a = o0.anchors(rd, sorted_=True)[0]
                f0, p0, _, _ = o0.chain_fill(a, len(rd))
                f1, p1, _, _ = o1.chain_fill(a, len(rd))
                n_diff += int(((f0 != f1) | (p0 != p1)).sum())
        if opts == "frag_20000":
            n_seg = lambda name: sum(c[key] for c in _census("stages", name).values() for key in CC.SEGMENT_KEYS[:5])
            assert n_diff == 0 and n_seg(opts) < n_seg("default") - 20, (n_diff, n_seg(opts), n_seg("default"))
            continue
        assert (n_diff == 0) == (opts == "frag_800"), (opts, n_diff)


@pytest.mark.parametrize("opts", list(W.MOSAIC_SETS))
def test_mosaic_mark_ring(built, opts):
    wd = W.mosaic_world()
    rd = wd["reads"]["mosaic"]
    orc = W.oracle_for(wd, W.MOSAIC_SETS[opts])
    a = orc.anchors(rd, sorted_=True)[0]
    # the cleared table beside the literal marks: no answer differs, so this run is the literal fill as well -- compared with the oracle
    c = CC.collections.Counter()
    r = CC.fill(a, len(rd), orc.mo, orc.k, ring=CC.CLEARED_RING, census=c)
    assert r["false_marks"] == 0, opts
    ef, ep = _equal(r, orc, a, len(rd), ("mosaic", opts))
    assert len(a) > 140000 and c["idx_ge_32768"] > 100000, (opts, len(a), c["idx_ge_32768"])
    differ = lambda x: int(((x["f"] != ef) | (x["p"] != ep)).sum())
    if opts == "skip_1":
        x = CC.fill(a, len(rd), orc.mo, orc.k, ring=CC.SEQUENTIAL_RING)        # the 15-bit table written in the reference loop's order
        assert x["false_marks"] > 0 and differ(x) >= 1, (opts, x["false_marks"], differ(x))
        x = CC.fill(a, len(rd), orc.mo, orc.k, ring=CC.KERNEL_RING)            # ... and in the wave's order
        assert x["false_marks"] == 0 and differ(x) == 0, (opts, x["false_marks"], differ(x))
    if opts.startswith("iter_"):
        x = CC.fill(a, len(rd), orc.mo, orc.k, ring=CC.KERNEL_RING)
        assert x["false_marks"] > 0 and differ(x) >= 1, (opts, x["false_marks"], differ(x))
