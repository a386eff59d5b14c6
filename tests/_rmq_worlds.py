"""The inputs of the RMQ chainer tests (tests/test_rmq_census_host.py asserts on the CPU what they reach, tests/test_gpu_rmq_edges.py runs
them through k_rmq_sort / k_rmq_dp / k_rmq_backtrack) and the option sets they run under.  Built once per process.

Two genomes, those of tests/_chain_worlds.py: `stages` (two contigs with three repeat families) and `arrays` (tandem arrays).  A world is
a genome, a preset and a list of reads:

edges_*   short reads of the stages genome, one world per preset (map-ont: the long-join pass only; asm20 and asm5: mg_lchain_rmq as the
          primary chainer, then the long join; map-hifi).  Ordinary reads of both strands and contigs, a chimera of two contigs, reads with a
          deletion, an inserted block or an inversion (tests/test_gpu_stages.py::_sv_reads: more than one chain, so the rescue test
          runs), a transposed read (reference A C B, read A B C': for the first anchors of B the 3 kb of C in front of them lie above
          y_i, the winner is the last anchor of A, more than RQ_RING - WAVE back), a read with a duplicated block (two diagonals that
          interleave in x but keep the order of y), reads without anchors, and reads trimmed until the pass under test sees exactly
          1, 64, 65, 511, 512, 513, 2047, 2048 and 2049 anchors.  Every option set runs on these.
wide_*    three long reads (30 to 50 kb, each with a deletion, so that map-ont re-chains them) under max_gap 12000 to 20000: windows of
          more than RQ_WRING - WAVE anchors (the HBM prefix), reads of more than 2048 anchors (the reuse of the summary slots).
arrays_*  eight to ten of the tandem-array reads of tests/test_gpu_stages.py::_tandem_world per preset: interleaved diagonals (the sorted redo
          of the inner walk) and inner sets that outgrow the rings (inner_capacity: what hands these reads to the host under the default
          options -- none of the 200 reads has two equal minimal priorities there).  Under chain_gap_scale = 0 the priority is -f and
          chains of equal score tie: lane by lane, through a block summary, inside one summarised block (t57 under map-ont); other
          reads (t26, t28) hold such a block that is never the minimum and stay on the device."""
import functools
import pathlib

import numpy as np

import synthdata as S
import _chain_worlds as CW
import _rmq_census as RC
from oracle import oracle as O
from test_gpu_stages import _sv_reads

# name -> MapOpt fields, written into the product's and the oracle's record alike
OPTION_SETS = dict([
    ("default", {}),
    ("cap_0", dict(rmq_size_cap=0)), ("cap_1", dict(rmq_size_cap=1)), ("cap_100", dict(rmq_size_cap=100)), ("cap_1000", dict(rmq_size_cap=1000)),
    ("cap_neg", dict(rmq_size_cap=-1)),
    ("inner_0", dict(rmq_inner_dist=0)), ("inner_50", dict(rmq_inner_dist=50)), ("inner_20000", dict(rmq_inner_dist=20000)),
    ("skip_0", dict(max_chain_skip=0)), ("skip_1", dict(max_chain_skip=1)), ("skip_60", dict(max_chain_skip=60)),
    ("rescue_size_0", dict(rmq_rescue_size=0)), ("rescue_size_100000", dict(rmq_rescue_size=100000)),
    ("rescue_ratio_0", dict(rmq_rescue_size=100000, rmq_rescue_ratio=0.0)), ("rescue_ratio_1", dict(rmq_rescue_ratio=1.0)),
    ("bw_long_2000", dict(bw_long=2000)), ("bw_long_100000", dict(bw_long=100000)), ("gap_200", dict(max_gap=200)),
    ("gap_scale_0.3", dict(chain_gap_scale=0.3)), ("gap_scale_2", dict(chain_gap_scale=2.0)), ("skip_scale_0.5", dict(chain_skip_scale=0.5)),
    ("gap_12000", dict(max_gap=12000)), ("gap_16000", dict(max_gap=16000)), ("gap_20000", dict(max_gap=20000)),
    ("gap_16000_cap_1000", dict(max_gap=16000, rmq_size_cap=1000)),
    # pen_gap = 0: the priority is -f alone, and two chains of equal score tie (the event no ordinary option set produces on these inputs)
    ("gap_scale_0", dict(chain_gap_scale=0.0)), ("gap_scale_0_inner_0", dict(chain_gap_scale=0.0, rmq_inner_dist=0)),
])
FIELDS = ("flag", "bw", "bw_long", "max_gap", "max_chain_skip", "min_cnt", "min_chain_score", "chain_gap_scale", "chain_skip_scale",
          "rmq_size_cap", "rmq_inner_dist", "rmq_rescue_size", "rmq_rescue_ratio")      # what mg_lchain_rmq and its call sites read
SIZES = (1, 64, 65, 511, 512, 513, 2047, 2048, 2049)
WIDE_SETS = ("gap_12000", "gap_16000", "gap_20000", "gap_16000_cap_1000")
EDGE_SETS = tuple(k for k in OPTION_SETS if k not in WIDE_SETS and k != "gap_scale_0_inner_0")
# the sets made for the events: every read they hand to the host is named in tests/test_rmq_census_host.py::HOST_READS.  (Under
# rmq_inner_dist = 20000, clamped to max_gap = 5000, the inner set of every read of more than RQ_RING - 2 * WAVE anchors outgrows the rings.)
EVENT_SETS = ("cap_neg", "inner_20000", "gap_scale_0", "gap_scale_0_inner_0")
# world -> the option sets it runs under
# (the rescue test is the same code under every preset: its sets run under map-ont only)
RUNS = dict([("edges_ont", EDGE_SETS), ("edges_asm20", tuple(k for k in EDGE_SETS if not k.startswith("rescue_") and k != "bw_long_100000")), ("edges_asm5", ("default", "inner_0", "cap_100")),
             ("edges_hifi", ("default", "skip_1")), ("wide_ont", WIDE_SETS), ("wide_asm20", ("gap_16000", "gap_16000_cap_1000")),
             ("arrays_ont", ("default", "gap_scale_0_inner_0")), ("arrays_asm20", ("default", "gap_scale_0_inner_0")),
             ("arrays_hifi", ("default", "gap_scale_0"))])
# the census table of `python tests/_rmq_census.py`
TABLE = (("edges_ont", "default"), ("edges_asm20", "default"), ("edges_asm20", "cap_100"), ("edges_asm20", "inner_0"), ("edges_ont", "rescue_ratio_1"), ("edges_ont", "cap_neg"),
         ("edges_asm5", "default"), ("edges_hifi", "default"), ("wide_ont", "gap_16000"), ("wide_asm20", "gap_16000"),
         ("wide_asm20", "gap_16000_cap_1000"), ("arrays_ont", "default"), ("arrays_ont", "gap_scale_0_inner_0"), ("arrays_asm20", "gap_scale_0_inner_0"),
         ("arrays_hifi", "default"), ("arrays_hifi", "gap_scale_0"))

PRESET = dict(ont="map-ont", asm20="asm20", asm5="asm5", hifi="map-hifi")
DIVERGENCE = dict(ont=0.02, asm20=0.02, asm5=0.002, hifi=0.002)


@functools.lru_cache(maxsize=None)
def _stages_genome():
    return S.make_genome(31, [400000, 250000], repeats=((4000, 6, 0.01), (900, 40, 0.02), (300, 120, 0.05)), n_runs=3)


def _comp(c):
    return np.where(c < 4, 3 - c, 4).astype(np.uint8)[::-1]


def oracle_for(world, fields=None):
    wd = WORLDS[world]() if isinstance(world, str) else world
    orc = O.OracleAligner(wd["fa"], preset=wd["preset"])
    CW.set_opts(orc.mo, fields or {})
    return orc


def _pass_anchors(orc, rd):
    """number of anchors the first mg_lchain_rmq pass of this read sees (primary: all of them; long join: the chained ones, 0 if it
    does not run)"""
    if len(rd) == 0:
        return 0
    a = orc.anchors(rd, sorted_=True)[0]
    if orc.mo.flag & RC.MM_F_RMQ:
        return len(a)
    u, b = orc.chains(a, len(rd))
    return len(b) if (RC.rescue(u, b, len(rd), orc.mo) or (False,))[0] else 0


def _trim_to(orc, codes, want):
    """a piece of the read whose first mg_lchain_rmq pass sees exactly `want` anchors (None if none is found): the count grows with the
    length of a prefix, in steps (a minimizer of a repeat family brings all its anchors at once), so bisect, look around, and where the
    count steps over `want` try again without the read's first bases"""
    for skip in range(0, 12 * 37, 37):
        piece = codes[skip:]
        count = lambda ln: _pass_anchors(orc, S.codes_to_str(piece[:ln]))
        lo, hi = 0, len(piece)
        while lo < hi:
            mid = (lo + hi) // 2
            if count(mid) < want:
                lo = mid + 1
            else:
                hi = mid
        for ln in range(max(lo - 60, 1), min(lo + 60, len(piece) + 1)):
            if count(ln) == want:
                return S.codes_to_str(piece[:ln])
    return None


def _edge_reads(key):
    g = _stages_genome()
    div = DIVERGENCE[key]
    mut = lambda c, rng: S.mutate(c, rng, div, div / 4, div / 4)
    rng = np.random.default_rng(301)
    A, B = g[0], g[1]
    out = [("plain_fwd", mut(A[20000:26000], rng)), ("plain_rev", mut(_comp(B[90000:97000]), rng)),
           ("chimera", mut(np.concatenate([A[50000:53000], _comp(B[30000:33500])]), rng)),
           ("deletion", mut(np.concatenate([A[120000:124000], A[127000:131000]]), rng)),
           ("insertion", mut(np.concatenate([A[200000:203000], S.random_codes(rng, 1800), A[203000:207000]]), rng)),
           ("transposed", mut(np.concatenate([A[300000:305000], A[308000:313000], A[305000:308000]]), rng)),
           ("duplicated", mut(np.concatenate([A[340000:344000], A[342000:347000]]), rng)),
           ("random", S.random_codes(rng, 1500))]
    out = [(n, S.codes_to_str(c)) for n, c in out]
    out += [("sv%d" % i, rd) for i, rd in enumerate(_sv_reads(g, np.random.default_rng(91), n_each=1))]
    out += [("empty", ""), ("tiny", "ACGT")]
    return out


@functools.lru_cache(maxsize=None)
def _edges(key):
    fa = CW.stages_world()["fa"]
    wd = dict(fa=fa, preset=PRESET[key])
    reads = _edge_reads(key)
    # the sized reads: prefixes of a read with a deletion (the long join re-chains it under map-ont) whose pass sees exactly SIZES anchors
    g = _stages_genome()
    div = DIVERGENCE[key]
    rng = np.random.default_rng(302)
    base = S.mutate(np.concatenate([g[0][60000:60250], g[0][63500:90000]]), rng, div, div / 4, div / 4)
    orc = oracle_for(wd)
    for want in SIZES:
        rd = _trim_to(orc, base, want)
        if rd is not None:
            reads.append(("n_%d" % want, rd))
    wd["reads"] = dict(reads)
    return wd


@functools.lru_cache(maxsize=None)
def _wide(key):
    g = _stages_genome()
    div = 0.015
    rng = np.random.default_rng(303)
    mut = lambda c: S.codes_to_str(S.mutate(c, rng, div, div / 4, div / 4))
    A, B = g[0], g[1]
    reads = dict([("w50", mut(np.concatenate([A[10000:30000], A[33000:63000]]))),
                  ("w30_rev", mut(_comp(np.concatenate([B[100000:112000], B[114500:132500]])))),
                  ("w40", mut(np.concatenate([A[150000:152000], A[155000:193000]])))])
    return dict(fa=CW.stages_world()["fa"], preset=PRESET[key], reads=reads)


ARRAY_READS = dict(ont=(3, 7, 8, 14, 26, 28, 42, 57, 111, 127), asm20=(3, 8, 14, 40, 42, 111, 127, 151), hifi=(3, 8, 9, 21, 40, 76, 118, 127))


@functools.lru_cache(maxsize=None)
def _arrays(key):
    from test_gpu_stages import _tandem_world
    fa, reads = _tandem_world(pathlib.Path(CW._dir("rmq_arrays_")))
    return dict(fa=fa, preset=PRESET[key], reads={"t%d" % i: reads[i] for i in ARRAY_READS[key]})


WORLDS = dict([("edges_" + k, functools.partial(_edges, k)) for k in PRESET] + [("wide_" + k, functools.partial(_wide, k)) for k in ("ont", "asm20")]
              + [("arrays_" + k, functools.partial(_arrays, k)) for k in ("ont", "asm20", "hifi")])


@functools.lru_cache(maxsize=None)
def anchors_of(world):
    """the oracle's sorted anchors of every read of the world (no option set here touches the seed stage)"""
    wd = WORLDS[world]()
    orc = oracle_for(wd)
    return [orc.anchors(rd, sorted_=True)[0] if len(rd) else np.zeros((0, 2), np.uint64) for rd in wd["reads"].values()]      # (the oracle's sketch refuses an empty read)


@functools.lru_cache(maxsize=None)
def predictions(world, opts):
    """RC.predict of every read of `world` under the option set `opts`, in the order of the world's reads"""
    wd = WORLDS[world]()
    orc = oracle_for(wd, OPTION_SETS[opts])
    out = []
    for rd, a in zip(wd["reads"].values(), anchors_of(world)):
        pd = RC.predict(orc, rd, anchors=a)
        for kind, pa, bw, r in pd["passes"]:                 # the model against the oracle's fill, wherever it ran to the end
            if r["event"] is None:
                ef, ep, ev = orc.rmq_fill(pa, bw)
                assert np.array_equal(r["f"], ef) and np.array_equal(r["p"], ep) and np.array_equal(r["v"], ev), (world, opts, kind)
        out.append(pd)
    return out
