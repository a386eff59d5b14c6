"""One mm355_stage_dp call per launch unit of mm355_dp.hip's table (a unit = one kernel launch over a contiguous range of launch groups):
three or four problems that all plan into that unit, results against the oracle, and the per-group statistics -- launches and cells on exactly
the groups present, elapsed time on exactly the unit's timer slot (its first group: 8 for groups 8-9, 10 for 10-13).  A wrong row of the table
(kernel, group range, list offset, timer slot) fails the one call that uses it.  Also k_ksw_band2's two half lists, the second run of band
problems whose proof fails (one per redo class), and rounds with nothing to align.
The row-sweep and band units need MM355_DP_BAND=0 / MM355_DP_BAND_FORCE, which the library reads once: those cases run in a child process,
as tests/test_gpu_map.py::test_dp_band_kernels_forced does."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import synthdata as S
import _dp_problems as D

APPROX, RIGHT, DROP, EXTZ, REV = 0x08, 0x02, 0x10, 0x40, 0x80
NEG_INF = -0x40000000
REDO = 23


def similar(rng, ql, tl):
    """a target of tl bases and a query of exactly ql: the target (repeated when shorter) with 0.5 % substitutions and a 4-base shift (close enough for every band proof to hold)"""
    t = S.random_codes(rng, tl)
    q = np.resize(t, ql).copy()
    sub = rng.random(ql) < 0.005
    q[sub] = (q[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    if ql > 40:
        q = np.concatenate([q[:ql // 2], q[ql // 2 + 4:], S.random_codes(rng, 4)])
    return q.astype(np.uint8), t.astype(np.uint8)


def unrelated(rng, ql, tl):
    return S.random_codes(rng, ql).astype(np.uint8), S.random_codes(rng, tl).astype(np.uint8)


def reg(tl, exact):
    """three problems of the register class of targets around tl: band-limited (w = 50), so that no approximate one is a full-band fill"""
    fl = (0, EXTZ, EXTZ | RIGHT | REV) if exact else (APPROX, APPROX | RIGHT, APPROX | DROP)
    return [(tl - 10, tl, 50, 400, -1, fl[0]), (tl, tl - 3, 50, 400, 10, fl[1]), (tl + 20, tl, 50, 400, -1, fl[2])]


def fills(shapes):
    """full-band approximate gap fills: the problems row_class gives to the row sweep and the band kernels"""
    return [(ql, tl, ql + tl, 400, -1, APPROX | (RIGHT if i % 2 else 0) | (REV if i == 2 else 0)) for i, (ql, tl) in enumerate(shapes)]


# name -> (environment, jobs, groups that must launch, timer slots that must show time)
UNITS = {
    "reg1_approx": ({}, reg(100, False), {0}, {0}), "reg1_exact": ({}, reg(100, True), {1}, {1}),
    "reg2_approx": ({}, reg(200, False), {2}, {2}), "reg2_exact": ({}, reg(200, True), {3}, {3}),
    "reg4_approx": ({}, reg(400, False), {4}, {4}), "reg4_exact": ({}, reg(400, True), {5}, {5}),
    "reg8_approx": ({}, reg(900, False), {6}, {6}), "reg8_exact": ({}, reg(900, True), {7}, {7}),
    # k_ksw_extd2<512>, LDS state of 4096 positions: w = 833 keeps the exact ones off k_ksw_regw
    "lds4096_exact": ({}, [(300, 1040, 833, 400, -1, 0), (1200, 1500, 833, 400, 10, EXTZ), (250, 4096, 833, 400, -1, RIGHT)], {9}, {8}),
    "lds4096_mixed": ({}, [(300, 1040, 833, 400, -1, APPROX), (1200, 1500, 833, 400, -1, EXTZ), (250, 4096, 833, 400, -1, APPROX | RIGHT)], {8, 9}, {8}),
    # ... of 12288 positions, and state in HBM beyond
    "lds12288_exact": ({}, [(300, 4100, 833, 400, -1, 0), (200, 12288, 833, 400, -1, EXTZ), (200, 12300, 833, 400, -1, RIGHT)], {11, 13}, {10}),
    "lds12288_mixed": ({}, [(300, 5000, 833, 400, -1, APPROX), (250, 8000, 833, 400, -1, EXTZ), (200, 12300, 833, 400, -1, APPROX | RIGHT),
                            (200, 12300, 833, 400, -1, 0)], {10, 11, 12, 13}, {10}),
    "regw8": ({}, [(1100, 1100, 751, 400, -1, EXTZ), (1000, 1100, 751, 400, 10, 0), (1900, 2000, 300, 400, -1, RIGHT)], {18}, {18}),
    # full-band fills too far off the diagonal for any band: the eight-wave row sweep
    "rowl": ({}, fills([(700, 1300), (2100, 1400), (600, 1290)]), {17}, {17}),
    "row2": ({"MM355_DP_BAND": "0"}, fills([(90, 100), (250, 256), (300, 200)]), {14}, {14}),
    "row4": ({"MM355_DP_BAND": "0"}, fills([(257, 257), (500, 512), (300, 400)]), {15}, {15}),
    "row8": ({"MM355_DP_BAND": "0"}, fills([(513, 513), (1000, 1024), (700, 900)]), {16}, {16}),
    "band128": ({"MM355_DP_BAND_FORCE": "1"}, fills([(300, 300), (280, 320), (500, 450)]), {19}, {19}),
    "band256": ({"MM355_DP_BAND_FORCE": "2"}, fills([(600, 600), (560, 640), (1300, 1250)]), {20}, {20}),
    "band512": ({"MM355_DP_BAND_FORCE": "4"}, fills([(700, 700), (900, 1000), (1500, 1400)]), {21}, {21}),
    "band64": ({"MM355_DP_BAND_FORCE": "64"}, fills([(200, 200), (300, 310), (1200, 1190)]), {22}, {22}),
}
ENVS = [{}, {"MM355_DP_BAND": "0"}, {"MM355_DP_BAND_FORCE": "1"}, {"MM355_DP_BAND_FORCE": "2"}, {"MM355_DP_BAND_FORCE": "4"}, {"MM355_DP_BAND_FORCE": "64"}]
SWITCHES = ("MM355_DP_BAND", "MM355_DP_BAND_FORCE")


def env_id(env):
    return "-".join("%s=%s" % kv for kv in env.items()) or "default"


def here(env):
    return {k: os.environ[k] for k in SWITCHES if k in os.environ} == env


def in_child(test, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_dp_groups.py::%s[%s]" % (test, env_id(env)), "-x", "-q"],
                       cwd=root, env=dict(e, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def al(built, tmp_path_factory):
    """a map-ont aligner over a 20-kb genome: the stage entry needs a context and the preset's options, nothing of the index"""
    import mappy_rs
    fa = str(tmp_path_factory.mktemp("dpg") / "ref.fa")
    S.write_fasta(fa, S.make_genome(3, [20000]), ["chrG"])
    return mappy_rs.Aligner(fa, preset="map-ont")


def run(al, jobs, seqs, tag):
    """one launch; results against the oracle; returns (launches, cells, ms) per group and (n_dp_band, n_dp_band_redo)"""
    qs, ts = [s[0] for s in seqs], [s[1] for s in seqs]
    res, cig, sr = D.run_stage_dp(al, al._mo, jobs, qs, ts)
    st = sr.stats()
    out = list(st.n_launch_group), list(st.dp_cells_group), list(st.ms_dp_group), (st.n_dp_band, st.n_dp_band_redo)
    sr.close()
    D.check_against_oracle(al._mo, jobs, qs, ts, res, cig, tag=tag)
    return out


def check_stats(tag, launches, cells, ms, groups, slots):
    assert [g for g in range(24) if launches[g]] == sorted(groups) and all(launches[g] == 1 for g in groups), (tag, launches)
    assert all(cells[g] > 0 for g in groups), (tag, cells)
    assert [g for g in range(24) if ms[g] > 0] == sorted(slots) and all(m >= 0 for m in ms), (tag, ms)


@pytest.mark.parametrize("env", ENVS, ids=env_id)
def test_each_launch_unit_alone(al, env):
    if not here(env):
        return in_child("test_each_launch_unit_alone", env)
    rng = np.random.default_rng(41)
    for name, (e, jobs, groups, slots) in UNITS.items():
        if e != env:
            continue
        launches, cells, ms, (n_band, n_redo) = run(al, jobs, [similar(rng, j[0], j[1]) for j in jobs], name)
        assert n_redo == 0 and n_band == (len(jobs) if min(groups) >= 19 else 0), (name, n_band, n_redo)   # (similar sequences: every proof holds)
        check_stats(name, launches, cells, ms, groups, slots)


@pytest.mark.parametrize("env", [{"MM355_DP_BAND_FORCE": "64"}], ids=env_id)
def test_band2_half_lists(al, env):
    """k_ksw_band2 pairs neighbours of its list, and a pair shares KSW_EZ_RIGHT: the list is launched as two halves"""
    if not here(env):
        return in_child("test_band2_half_lists", env)
    rng = np.random.default_rng(43)
    shapes = [(200, 200), (300, 310), (260, 250), (400, 400)]
    for name, rights in (("right_only", (1, 1, 1)), ("left_only", (0, 0, 0)), ("odd_halves", (1, 0, 1, 1))):
        jobs = [(ql, tl, ql + tl, 400, -1, APPROX | (RIGHT if r else 0)) for (ql, tl), r in zip(shapes, rights)]
        launches, cells, ms, (n_band, n_redo) = run(al, jobs, [similar(rng, j[0], j[1]) for j in jobs], name)
        assert (n_band, n_redo) == (len(jobs), 0), (name, n_band, n_redo)
        check_stats(name, launches, cells, ms, {22}, {22})
        assert cells[22] == sum(j[0] * j[1] for j in jobs), (name, cells[22])


@pytest.mark.parametrize("env", [{"MM355_DP_BAND_FORCE": "64"}], ids=env_id)
def test_failed_proofs_run_again_in_every_redo_class(al, env):
    """unrelated sequences on a forced 64-diagonal band: the end score is far below the bound that proves the band (about 2 n - 175 for n bases
    with map-ont's scoring), so each of them runs again on the full matrix -- k_ksw_row<2>, <4>, <8> and k_ksw_rowl, one problem each --
    beside one similar pair per class whose proof holds"""
    if not here(env):
        return in_child("test_failed_proofs_run_again_in_every_redo_class", env)
    rng = np.random.default_rng(47)
    shapes = [(200, 210), (400, 390), (800, 800), (1200, 1210)]
    jobs = fills(shapes + shapes)
    seqs = [unrelated(rng, ql, tl) for ql, tl in shapes] + [similar(rng, ql, tl) for ql, tl in shapes]
    launches, cells, ms, (n_band, n_redo) = run(al, jobs, seqs, "redo")
    assert (n_band, n_redo) == (8, 4), (n_band, n_redo)
    check_stats("redo", launches, cells, ms, {22, REDO}, {22, REDO})
    assert cells[REDO] == sum(ql * tl for ql, tl in shapes), cells[REDO]


def test_rounds_with_nothing_to_align(al):
    """no job at all, and jobs that are all skipped (no query, no target, qlen * tlen beyond max_sw_mat): empty and skipped jobs ride in
    group 0's list, whose kernel writes their results"""
    from mappy_rs import _ffi
    L = _ffi.lib()
    sr = al._stage_runner()
    res = (_ffi.DpRes * 1)(); cig = np.zeros(4, np.uint32); none = np.zeros(1, np.uint8)
    _ffi.check(L.mm355_stage_dp(sr.ctx, C.byref(al._mo), 0, (_ffi.DpJob * 1)(), none.ctypes.data, 0, none.ctypes.data, 0, res, cig.ctypes.data, 4))
    st = sr.stats()
    assert not any(st.n_launch_group) and not any(st.dp_cells_group) and not any(st.ms_dp_group) and (st.n_dp_jobs, st.n_launch_dp, st.dp_cells) == (0, 0, 0)
    sr.close()
    rng = np.random.default_rng(53)
    assert 0 < al._mo.max_sw_mat < 20000 * 20000
    jobs = [(0, 300, 100, 400, -1, 0), (300, 0, 100, 400, -1, APPROX), (20000, 20000, 751, 400, -1, EXTZ)]
    seqs = [(np.zeros(0, np.uint8), S.random_codes(rng, 300).astype(np.uint8)), (S.random_codes(rng, 300).astype(np.uint8), np.zeros(0, np.uint8)),
            unrelated(rng, 20000, 20000)]
    res, cig, sr = D.run_stage_dp(al, al._mo, jobs, [s[0] for s in seqs], [s[1] for s in seqs])
    st = sr.stats()
    got = [(r.max, r.zdropped, r.max_q, r.max_t, r.mqe, r.mqe_t, r.mte, r.mte_q, r.score, r.reach_end, r.n_cigar) for r in res]
    launches, cells, ms = list(st.n_launch_group), list(st.dp_cells_group), list(st.ms_dp_group)
    tot = (st.n_dp_jobs, st.n_launch_dp, st.dp_cells, st.n_dp_band, st.n_dp_band_redo)
    sr.close()
    assert got == [(0, zd, -1, -1, NEG_INF, -1, NEG_INF, -1, NEG_INF, 0, 0) for zd in (0, 0, 1)], got
    assert launches == [1] + [0] * 23 and not any(cells) and [g for g in range(24) if ms[g] > 0] == [0], (launches, cells, ms)
    assert tot == (3, 1, 0, 0, 0), tot
