"""The inputs of the seed-edge tests (tests/test_seed_edges_host.py asserts on the CPU what they reach, tests/test_gpu_seed_edges.py runs them
through the kernels): a 2.9-kb genome whose flat table wraps, a 40-base contig whose table has two lines, and one 0.5-Mbp world with the
repeat structure that sends streaks of high-occurrence hits through every branch of mm_seed_select.  Built once per process."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

from oracle import oracle as O
import synthdata as S

NO_DIAG, NO_DUAL, FOR_ONLY, REV_ONLY = 1, 2, 0x100000, 0x200000
MID_OCC = 20
# the option sets of the select world (written into the product's and the oracle's MapOpt alike)
OPTION_SETS = dict(default={}, max_max_occ_30=dict(max_max_occ=30), occ_dist_0=dict(occ_dist=0), occ_dist_100=dict(occ_dist=100))


def comp(c):
    return np.where(c < 4, 3 - c, 4).astype(np.uint8)[::-1]


def _dir(prefix):
    td = tempfile.mkdtemp(prefix=prefix)
    atexit.register(shutil.rmtree, td, True)
    return td


def set_opts(mo, fields, flag=0):
    """the fields of an option set (and extra flag bits) into one MapOpt record; mid_occ is fixed for the select world"""
    mo.mid_occ = MID_OCC
    for k, v in fields.items():
        setattr(mo, k, v)
    mo.flag |= flag


# ------------------------------------------------------------------ the table that wraps
WRAP_SEED, WRAP_LEN = 6, 2900


@functools.lru_cache(maxsize=None)
def wrap_world():
    """2900 random bases at k15 w10: a table of 128 lines about half full in which the run of full lines at the end carries entries round to
    line 0.  Reads: the genome, its reverse complement, a 4 % mutated copy, and random reads whose minimizers are absent keys homed in every
    line many times over."""
    g = S.random_codes(np.random.default_rng(WRAP_SEED), WRAP_LEN)
    td = _dir("seed_wrap_")
    fa = os.path.join(td, "wrap.fa")
    S.write_fasta(fa, [g], ["wrap"])
    rng = np.random.default_rng(600)
    reads = [S.codes_to_str(g), S.codes_to_str(comp(g)), S.codes_to_str(S.mutate(g, rng, 0.02, 0.01, 0.01))]
    reads += [S.codes_to_str(S.random_codes(rng, n)) for n in (30000, 9000, 1100, 383)]
    return dict(fa=fa, genome=g, seq=S.codes_to_str(g), reads=reads, dir=td)


@functools.lru_cache(maxsize=None)
def two_line_world():
    """one 40-base contig: a handful of keys, a table of two lines (line_mask == 1)"""
    rng = np.random.default_rng(41)
    g = S.random_codes(rng, 40)
    td = _dir("seed_two_")
    fa = os.path.join(td, "two.fa")
    S.write_fasta(fa, [g], ["two"])
    reads = [S.codes_to_str(g), S.codes_to_str(comp(g)), S.codes_to_str(np.concatenate([S.random_codes(rng, 300), g, S.random_codes(rng, 500)])),
             S.codes_to_str(S.random_codes(rng, 2000))]
    return dict(fa=fa, genome=g, seq=S.codes_to_str(g), reads=reads, dir=td)


# ------------------------------------------------------------------ the world of the select branches
MAIN_LEN = 470000
LONG_READ = 430000                  # the long read is main[0:LONG_READ]: hit 65536 falls at about base 353600, inside the tandem array
ARRAY_AT, ARRAY_UNIT, ARRAY_COPIES = 352500, 61, 70
FAM_LEN, FAM_EXACT, FAM_DIVERGED = 2000, 10, 30
ELEMENT_LEN, ELEMENT_EVERY = 40, 3000


@functools.lru_cache(maxsize=None)
def select_world():
    """contigs: `zmain` (470 kb: a unique background, a 2-kb family of 10 exact and 30 diverged (1-3 %) copies on either strand, a tandem
    array of a 61-base unit where hit 65536 of the long read falls, a 40-base element every 3 kb, a 1-kb low-copy repeat), `selfie` (9 kb with
    a family copy and a 300-base block twice: a read of this name and length is its own copy) and `aaa` (5 kb with a family copy and a piece of `selfie`; its name sorts before every read's).
    reads: dict name -> sequence."""
    rng = np.random.default_rng(2025)
    main = S.random_codes(rng, MAIN_LEN)
    fam = S.random_codes(rng, FAM_LEN)
    element = S.random_codes(rng, ELEMENT_LEN)
    low = S.random_codes(rng, 1000)
    unit = S.random_codes(rng, ARRAY_UNIT)
    # family copies every 5 kb from 4 kb on (exact and diverged interleaved, every third on the reverse strand)
    for at in range(2500, MAIN_LEN - ELEMENT_LEN, ELEMENT_EVERY):       # (first: what follows overwrites the elements it meets)
        main[at:at + ELEMENT_LEN] = element
    kinds = [0.0] * FAM_EXACT + [float(d) for d in rng.uniform(0.01, 0.03, FAM_DIVERGED)]
    rng.shuffle(kinds)
    fam_at = []
    for i, div in enumerate(kinds):
        at = 4000 + 5000 * i
        c = fam if div == 0.0 else S.mutate(fam, rng, div, 0.0, 0.0)[:FAM_LEN]
        main[at:at + FAM_LEN] = comp(c) if i % 3 == 2 else c
        fam_at.append((at, div, i % 3 == 2))
    for i in range(5):                                  # low-copy repeat: kept seeds with 5 occurrences on both strands
        at = 1500 + 85000 * i
        main[at:at + 1000] = comp(low) if i & 1 else low
    main[ARRAY_AT:ARRAY_AT + ARRAY_UNIT * ARRAY_COPIES] = np.tile(unit, ARRAY_COPIES)
    dup = S.random_codes(rng, 300)                     # twice in `selfie`: anchors of the read on its own contig off the diagonal (MM_SEED_SELF)
    selfie = np.concatenate([S.random_codes(rng, 1500), dup, S.random_codes(rng, 1700), S.mutate(fam, rng, 0.02, 0.0, 0.0)[:FAM_LEN],
                             S.random_codes(rng, 1700), dup, S.random_codes(rng, 1500)])
    aaa = np.concatenate([S.random_codes(rng, 1000), S.mutate(selfie[200:1400], rng, 0.01, 0.0, 0.0), fam, S.random_codes(rng, 1000)])
    td = _dir("seed_select_")
    fa = os.path.join(td, "select.fa")
    S.write_fasta(fa, [main, selfie, aaa], ["zmain", "selfie", "aaa"])

    def island(parts):
        """unique pieces of zmain (between the family copies' end and the array, clear of the 40-base elements), stretches that hit nothing, and short pieces of the family: streaks that may keep all of their hits"""
        out = []
        for kind, a, b in parts:
            out.append(main[a:b] if kind == "u" else fam[a:b] if kind == "f" else S.random_codes(rng, b - a))
        return S.codes_to_str(np.concatenate(out))

    reads = {}
    reads["long"] = S.codes_to_str(main[:LONG_READ])
    # 70 kb of exact copies of the unit's inside with an N between them: every minimizer of the read is then the least of a full window of
    # family k-mers, so a minimizer of every exact copy too (across a plain junction some are minimizers only by the grace of what follows
    # them: low counts that cut the streak).  One streak, clamp at 128
    reads["clamp"] = S.codes_to_str(np.tile(np.concatenate([fam[100:1900], np.array([4], np.uint8)]), 39))
    at9 = [a for a, d, rev in fam_at if d == 0 and not rev][2]               # across an exact copy: one long streak
    atd = [a for a, d, rev in fam_at if d > 0 and not rev][2]                # across a diverged copy: its private bases cut the streak short
    reads["nine"] = S.codes_to_str(S.mutate(main[at9 - 3500:at9 + 5500], rng, 0.02, 0.01, 0.01))
    # islands: a family piece first (st == 0), in the middle between stretches that hit nothing, and last (en == n_m0)
    reads["isle_a"] = island([("f", 300, 332), ("x", 0, 1600), ("u", 300000, 301000), ("x", 0, 1600), ("f", 900, 934), ("x", 0, 1600),
                              ("u", 306000, 307000), ("x", 0, 1800), ("f", 1500, 1532)])
    reads["isle_b"] = island([("x", 0, 1700), ("f", 1200, 1236), ("x", 0, 1800)])                   # every hit in one streak: st == 0 and en == n_m0
    reads["isle_c"] = island([("u", 288000, 288800), ("x", 0, 1700), ("f", 600, 634), ("x", 0, 1700), ("u", 291000, 291800),
                              ("x", 0, 2000), ("f", 100, 140), ("x", 0, 2000), ("u", 294000, 294700)])
    reads["selfie"] = S.codes_to_str(selfie)
    # mm_seed_mz_flt: a tandem read whose few minimizer values each make up more than 1 % of its > 2048 minimizers, in front of unique sequence
    reads["tandem"] = S.codes_to_str(np.concatenate([np.tile(main[30000:30037], 700), main[40000:43000]]))
    reads["revnine"] = S.codes_to_str(comp(S.mutate(main[atd - 1000:atd + 3000], rng, 0.01, 0.005, 0.005)))
    return dict(fa=fa, dir=td, reads=reads, contigs=dict(zmain=main, selfie=selfie, aaa=aaa))


def oracle_for(world, opts=None, flag=0):
    """the oracle of a world's FASTA (default options, k15 w10) with an option set written in"""
    orc = O.OracleAligner(world["fa"])
    if opts is not None:
        set_opts(orc.mo, opts, flag)
    return orc
