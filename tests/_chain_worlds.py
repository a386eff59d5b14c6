"""The inputs of the chain-fill tests (tests/test_chain_census_host.py asserts on the CPU what they reach, tests/test_gpu_chain_edges.py
runs them through k_chain_segments / k_chain_small / k_chain_big) and the option sets they run under.  Built once per process.

stages   six reads of the world of tests/test_gpu_stages.py, picked (by the census, smallest anchor total first) so that between them
         they hold every segment class of k_chain_segments -- segments of exactly 32 and 33 anchors, a start on lane 63, ends in the
         next strip, beyond the first look-ahead step, beyond the 4096-anchor chunk and at the read's end -- and the ordinary scan classes
arrays   the tandem-array genome of tests/test_gpu_stages.py::_tandem_world with three of its reads (interleaved diagonals: the
         reflected n_skip walk, max_ii rescues, a max_ii hundreds of anchors back) and one read of 14 copies of the 350-base unit whose
         array has 11: more than 8000 anchors within max_gap of each other, so the window is cut by max_chain_iter at 5000 and at 8000
mosaic   one 396-kb read of a genome sown with 4000 30-mers at 9 places each: about 150 000 anchors, nearly all in one segment, half of
         them off the diagonal and nobody's predecessor -- the input on which a mark of tw[] can outlive 32768 anchors"""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

from oracle import oracle as O
import synthdata as S

PRESET = "map-ont"

# name -> MapOpt fields, written into the product's and the oracle's record alike
OPTION_SETS = dict([
    ("default", {}),
    ("iter_40", dict(max_chain_iter=40)), ("iter_200", dict(max_chain_iter=200)), ("iter_8000", dict(max_chain_iter=8000)),
    ("skip_0", dict(max_chain_skip=0)), ("skip_1", dict(max_chain_skip=1)), ("skip_3", dict(max_chain_skip=3)), ("skip_60", dict(max_chain_skip=60)),
    ("bw_8000", dict(bw=8000)), ("gap_800", dict(max_gap=800)), ("gap_ref_1500", dict(max_gap_ref=1500)),
    ("frag_800", dict(max_frag_len=800)), ("frag_20000", dict(max_frag_len=20000)),
    ("gap_scale_0.3", dict(chain_gap_scale=0.3)), ("gap_scale_2", dict(chain_gap_scale=2.0)),
    ("skip_scale_0.5", dict(chain_skip_scale=0.5)), ("skip_scale_0.5_gap_scale_2", dict(chain_skip_scale=0.5, chain_gap_scale=2.0)),
])
KW_SETS = ((19, 19), (21, 11))                      # other k / w (another q_span), on the arrays world
CHAINS_SETS = ("iter_200", "skip_1", "skip_scale_0.5_gap_scale_2")       # the option sets the backtrack runs behind as well
# the mosaic read: the two sets it was made for, and the one under which the kernel's own order of writing the marks lets one survive
# (tests/test_chain_census_host.py::test_mosaic_mark_ring)
MOSAIC_SETS = dict([("skip_1", dict(max_chain_skip=1)), ("default", {}), ("iter_3_skip_0", dict(max_chain_iter=3, max_chain_skip=0))])


def _dir(prefix):
    td = tempfile.mkdtemp(prefix=prefix)
    atexit.register(shutil.rmtree, td, True)
    return td


def set_opts(mo, fields):
    for k, v in fields.items():
        setattr(mo, k, v)


def oracle_for(world, fields=None, k=None, w=None):
    orc = O.OracleAligner(world["fa"], preset=PRESET, k=k, w=w)
    set_opts(orc.mo, fields or {})
    return orc


STAGES_READS = (30, 42, 43, 63, 80, 117)


@functools.lru_cache(maxsize=None)
def stages_world():
    g = S.make_genome(31, [400000, 250000], repeats=((4000, 6, 0.01), (900, 40, 0.02), (300, 120, 0.05)), n_runs=3)
    td = _dir("chain_stages_")
    fa = os.path.join(td, "ref.fa")
    S.write_fasta(fa, g, ["chrA", "chrB"])
    reads, _ = S.make_reads(32, g, 160, n50=5000, lo=200)
    return dict(fa=fa, dir=td, reads={"r%d" % i: reads[i] for i in STAGES_READS})


ARRAY_READS = (3, 111, 127)
TILED_ARRAY, TILED_COPIES = 2, 14                   # the third array (a 350-base unit, 11 exact copies) and the copies the tiled read has of it


@functools.lru_cache(maxsize=None)
def arrays_world():
    rng = np.random.default_rng(5)
    bg = S.random_codes(rng, 300000)
    pieces, arrays, pos, at = [], [], 0, 0
    for k in range(12):
        seg = bg[pos:pos + 20000]; pos += 20000
        unit = S.random_codes(rng, int(rng.choice([171, 350, 700])))
        ncopy = int(rng.integers(3, 12))
        arr = np.concatenate([S.mutate(unit, rng, 0.0 if k % 2 == 0 else 0.01, 0, 0) for _ in range(ncopy)])
        pieces += [seg, arr]
        arrays.append((at + len(seg), unit, ncopy))
        at += len(seg) + len(arr)
    g = np.concatenate(pieces).astype(np.uint8)
    td = _dir("chain_arrays_")
    fa = os.path.join(td, "tandem.fa")
    S.write_fasta(fa, [g], ["chrT"])
    reads = []
    for i in range(200):
        st = int(rng.integers(0, len(g) - 9000)); ln = int(rng.integers(2000, 9000))
        err = 0.0 if i % 2 == 0 else 0.01
        reads.append(S.codes_to_str(S.mutate(g[st:st + ln], rng, err, err / 2, err / 2)))
    out = {"t%d" % i: reads[i] for i in ARRAY_READS}
    at, unit, ncopy = arrays[TILED_ARRAY]
    assert (len(unit), ncopy) == (350, 11)
    rng = np.random.default_rng(55)
    end = at + len(unit) * ncopy
    # (3 kb of unique sequence on either side: without them mm_seed_mz_flt takes the array's minimizers, 14 of each among too few, out of the read)
    out["tiled"] = S.codes_to_str(np.concatenate([g[at - 3000:at], S.mutate(np.tile(unit, TILED_COPIES), rng, 0.005, 0.002, 0.002), g[end:end + 3000]]))
    return dict(fa=fa, dir=td, reads=out)


@functools.lru_cache(maxsize=None)
def mosaic_world():
    rng = np.random.default_rng(9)
    g = S.random_codes(rng, 400000)
    for _ in range(4000):
        u = S.random_codes(rng, 30)
        for pos in rng.integers(0, 400000 - 30, 9):
            g[pos:pos + 30] = u
    td = _dir("chain_mosaic_")
    fa = os.path.join(td, "mosaic.fa")
    S.write_fasta(fa, [g], ["mosaic"])
    return dict(fa=fa, dir=td, reads={"mosaic": S.codes_to_str(S.mutate(g[2000:398000], rng, 0.005, 0.002, 0.002))})


WORLDS = dict(stages=stages_world, arrays=arrays_world)      # the worlds every option set runs on (the mosaic read has its own sets)
