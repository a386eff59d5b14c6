"""The extension kernels against the oracle across the int8 domain of U:ksw2_extd2_sse.c (mappy-rs_amd/csrc/mm355_dpdomain.h).  The oracle keeps
the SSE kernel's int8 wrap-around; the literal kernels (k_ksw_reg, k_ksw_regw, k_ksw_extd2) copy it, the row sweep and the band kernels compute
the plain recurrence and may only take a problem inside the domain.  Here: the problem set of test_gpu_map.py::test_dp_kernel_parity under
scorings where the int8 lanes wrap (gap sum (q + e) + (q2 + e2) of 129 / 134 / 150, match score 121, a = 100 with q + e = 40, swapped pieces)
and at the last scorings inside (gap sum 128, a + q + 2e = 128); a band-range pin (in-band values far below ROW_NEG); end-to-end parity for
asm5 / map-ont scorings on both sides of the edge; and the option fuzzer's wide mode, whose scorings span the whole int8 range."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import synthdata as S
import _dp_problems as D
from test_gpu_map import check_reads, ont  # noqa: F401  (ont: the module fixture -- genome, map-ont aligner, oracle)

ROW_GROUPS = (14, 15, 16, 17)              # k_ksw_row<2 | 4 | 8>, k_ksw_rowl
BAND_GROUPS = (19, 20, 21, 22)             # k_ksw_band<1 | 2 | 4>, k_ksw_band2
REG_GROUPS, LDS_GROUPS, REGW_GROUP = tuple(range(0, 8)), tuple(range(8, 14)), 18

# ((a, b, sc_ambi, q, e, q2, e2), inside the int8 domain)
SCORINGS = [((1, 19, 1, 40, 3, 85, 1), False),     # gap sum 129 (asm5 with q = 40)
            ((1, 19, 1, 45, 3, 85, 1), False),     # gap sum 134
            ((2, 4, 1, 40, 30, 60, 20), False),    # gap sum 150
            ((121, 4, 1, 4, 2, 24, 1), False),     # match score 121: a + q + 2e = 129
            ((100, 4, 1, 30, 10, 77, 1), False),   # a = 100 with q + e = 40
            ((2, 4, 1, 88, 1, 30, 10), False),     # gap sum 129 with the pieces swapped (ksw2 re-orders them)
            ((1, 19, 1, 39, 3, 85, 1), True),      # gap sum 128: the last one inside
            ((120, 4, 1, 4, 2, 24, 1), True)]      # a + q + 2e = 128: the last one inside


def with_scoring(mo, cfg):
    mo = copy.copy(mo)
    mo.a, mo.b, mo.sc_ambi, mo.q, mo.e, mo.q2, mo.e2 = cfg
    return mo


@pytest.mark.parametrize("cfg,inside", SCORINGS, ids=["-".join(map(str, c)) for c, _ in SCORINGS])
def test_dp_kernels_under_scorings_near_the_int8_edge(ont, cfg, inside):
    """every ez field and the CIGAR of the ~1100 problems of test_dp_kernel_parity equal the oracle's; outside the domain nothing runs on the
    row / band kernels and the literal classes take everything, inside the row kernels run (the two 65-KB targets: first scoring only)"""
    al = ont["al"]
    jobs, qs, ts, _n_short, _n_rowl = D.parity_problems()
    if cfg != SCORINGS[0][0]:                                           # the two 65-KB targets (in front of the 24 border paths): oracle time
        keep = [i for i in range(len(jobs)) if jobs[i][1] < 60000]
        assert len(keep) == len(jobs) - 2
        jobs, qs, ts = [jobs[i] for i in keep], [qs[i] for i in keep], [ts[i] for i in keep]
    mo = with_scoring(al._mo, cfg)
    res, cig, sr = D.run_stage_dp(al, mo, jobs, qs, ts)
    groups = list(sr.stats().n_launch_group)
    sr.close()
    D.check_against_oracle(mo, jobs, qs, ts, res, cig, tag=cfg)
    if inside:
        assert sum(groups[g] for g in ROW_GROUPS) > 0, (groups, cfg)
    else:
        assert sum(groups[g] for g in ROW_GROUPS + BAND_GROUPS) == 0, (groups, cfg)
        assert sum(groups[g] for g in REG_GROUPS) > 0 and sum(groups[g] for g in LDS_GROUPS) > 0 and groups[REGW_GROUP] > 0, (groups, cfg)


def test_dp_band_problems_below_row_neg(ont):
    """full-band fills of 3000..3250 bases with no match at all (poly-A against poly-C) and unrelated pairs under (2,16,1,4,4,115,1) -- inside
    the domain (gap sum 124): band_plan admits them, and the best path inside a band scores about -18000, below ROW_NEG.  Results equal the
    oracle's; with MM355_DP_BAND_FORCE (the child processes below) they run on the forced band kernel first"""
    rng = np.random.default_rng(77)
    cfg = (2, 16, 1, 4, 4, 115, 1)
    qs, ts, jobs = [], [], []
    for i, (ql, tl) in enumerate([(3000, 3000), (3100, 3120), (3250, 3210), (3000, 3040), (3200, 3200), (3050, 3150), (3240, 3250), (3000, 3100)]):
        for unrelated in (False, True):
            x = S.random_codes(rng, ql) if unrelated else np.zeros(ql, np.uint8)              # poly-A ...
            t = S.random_codes(rng, tl) if unrelated else np.ones(tl, np.uint8)               # ... against poly-C
            fl = 8 | (2 if (i + unrelated) % 2 else 0)
            qs.append(x.astype(np.uint8)); ts.append(t.astype(np.uint8)); jobs.append((ql, tl, ql + tl + 1, 400, -1, fl))
    al = ont["al"]
    mo = with_scoring(al._mo, cfg)
    res, cig, sr = D.run_stage_dp(al, mo, jobs, qs, ts)
    st = sr.stats()
    groups, n_band = list(st.n_launch_group), st.n_dp_band
    sr.close()
    D.check_against_oracle(mo, jobs, qs, ts, res, cig, tag=cfg)
    force = os.environ.get("MM355_DP_BAND_FORCE")
    if force:
        k = {"64": 22, "1": 19, "2": 20, "4": 21}[force]
        assert groups[k] > 0 and n_band > 0, (groups, n_band)


@pytest.mark.parametrize("force", ["64", "1", "2", "4"])
def test_dp_band_range_forced(built, force):
    """the band-range pin once more in a child process (the switch is read once) with every fill pushed onto a band of 64 / 128 / 256 / 512 diagonals"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_dp_scoring.py", "-x", "-q", "-k", "test_dp_band_problems_below_row_neg"],
                       cwd=root, env=dict(os.environ, MM355_DP_BAND_FORCE=force), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("preset,scoring", [("asm5", (1, 19, 40, 3, 85, 1)), ("asm5", (1, 19, 39, 3, 85, 1)), ("map-ont", (121, 4, 4, 2, 24, 1))],
                         ids=["asm5-gap129", "asm5-gap128", "map-ont-a121"])
def test_map_parity_scorings_near_the_int8_edge(ont, preset, scoring):
    """whole records (every field, cs, MD, and the device k_extra pass) against the oracle on both sides of the domain's edge"""
    import mappy_rs
    kw = dict(preset=preset, scoring=scoring)
    al = mappy_rs.Aligner(ont["fa"], **kw)
    orc = O.OracleAligner(ont["fa"], **kw)
    err = dict(sub=0.004, ins=0.002, dele=0.002) if preset == "asm5" else {}     # asm5 (mismatch 19, min_dp_max 200) maps near-identical reads
    reads, _ = S.make_reads(91, ont["g"], 40, n50=4000, lo=500, **err)
    n_hits, _ = check_reads(al, orc, reads)
    # at gap sum 129 upstream keeps no hit of these reads (its wrapped DP scores); the records -- none per read -- must still be the oracle's
    assert n_hits >= (0 if scoring[2] == 40 else 30), n_hits


def test_option_fuzz_wide_scorings(built, tmp_path):
    """tools/optfuzz.py's wide mode: random option sets whose scorings span ksw2's whole int8 range, bit-exact against the oracle"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("optfuzz", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "optfuzz.py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    n_cfg, n_hits, n_bad = fz.run(7, 8, str(tmp_path / "fzw.fa"), wide=True)
    assert n_bad == 0 and n_hits > 150, (n_hits, n_bad)
