"""The int8 domain of U:ksw2_extd2_sse.c (mappy-rs_amd/csrc/mm355_dpdomain.h), the predicate row_class asks before it sends a full-band gap
fill to the plain-recurrence kernels (k_ksw_row / k_ksw_rowl, the band kernels), held against the oracle on the CPU.  The product's own header
is compiled with g++ (tests/host_harness/dp_domain_host.cpp); for every scoring it accepts with a regular cost -- the only costs row_class
routes there -- the row-sweep model of test_row_sweep_model.py and, where the band proof holds, the band model of test_band_model.py must give
the oracle's score and CIGAR on every problem: 1-base targets, unrelated sequences, N runs, long indels, left- and right-aligned gaps.
Scorings swept: the presets, families around gap sums (q + e) + (q2 + e2) of 126..131 with several splits and swapped pieces, match scores
118..127, b at its ceiling 2 (q + e), sc_ambi 0 and large, and 200 seeded random tuples over the whole int8 range.
Where the predicate sits: exactly ON the observed edge for the two conditions that bind.  Gap sum 128 is accepted and agrees, 129 is
rejected and disagrees on nearly every problem ((1,19,1,39,3,85,1) vs (1,19,1,40,3,85,1)); with q = 4, e = 2 the match score 120
(a + q + 2e = 128) is accepted and agrees, 121 is rejected and disagrees.  The rejected scorings of the random sweep mostly disagree too
(asserted below for a share of them), so the domain is not much wider than the predicate."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
import _capi
import synthdata as S
from test_row_sweep_model import consts, row_sweep, backtrack, REGULAR
from test_band_model import band_sweep, plan


# (a, b, sc_ambi, q, e, q2, e2) of the long-read presets (oracle/mmo_options.c)
PRESETS = {"map-ont": (2, 4, 1, 4, 2, 24, 1), "map-hifi": (1, 4, 1, 6, 2, 26, 1), "asm5": (1, 19, 1, 39, 3, 81, 1), "asm10": (1, 9, 1, 16, 2, 41, 1),
           "asm20": (1, 4, 1, 6, 2, 26, 1)}
# scorings that pass dc.valid and are regular, but whose int8 lanes wrap: the plain recurrence disagrees with the SSE kernel
WRAPS = [(1, 19, 1, 40, 3, 85, 1), (1, 19, 1, 45, 3, 85, 1), (2, 4, 1, 30, 10, 88, 1), (2, 4, 1, 40, 30, 60, 20), (121, 4, 1, 4, 2, 24, 1),
         (100, 4, 1, 30, 10, 77, 1)]
EDGES = [(1, 19, 1, 39, 3, 85, 1), (120, 4, 1, 4, 2, 24, 1)]          # the last scorings inside: gap sum 128, a + q + 2e = 128


@pytest.fixture(scope="module")
def domain():
    L = _capi.build_harness("dp_domain_host", ["-Wall"], ["mm355_dpdomain.h"])
    L.dp_domain_host.argtypes = [C.c_int] * 7
    L.dp_domain_host.restype = C.c_int
    return lambda cfg: bool(L.dp_domain_host(*cfg))


def regular(cfg):
    _a, _b, _amb, q, e, q2, e2 = cfg
    qq, ee, qq2, ee2, _lt, _ld = consts(q, e, q2, e2)
    return ee > ee2 or (ee == ee2 and qq == qq2)


def valid(cfg):
    """ksw_extd2_sse aligns at all (dc.valid): the lowest substitution score is not below -2 (q + e) after the ordering"""
    _a, b, amb, q, e, q2, e2 = cfg
    qq, ee = consts(q, e, q2, e2)[:2]
    sc_n = -e2 if amb == 0 else -abs(amb)
    return -min(-abs(b), sc_n) <= 2 * (qq + ee)


def problems(rng, n):
    """(query, target, right) of gap-fill shape; every kind of problem where an int8 lane reaches an end of its range"""
    out = []
    for it in range(n):
        k = it % 8
        tl = 1 if k == 0 else int(rng.integers(2, 150))
        t = S.random_codes(rng, tl)
        x = S.mutate(t, rng, 0.06, 0.03, 0.03)
        if k == 0: x = S.random_codes(rng, int(rng.integers(1, 40)))                          # a 1-base target
        if k == 1: x = S.random_codes(rng, int(rng.integers(1, 160)))                         # unrelated sequences
        if k == 2 and len(x) > 50:                                                              # a long deletion (the second gap piece)
            cut = int(rng.integers(5, len(x) - 40)); x = np.concatenate([x[:cut], x[cut + int(rng.integers(20, 40)):]])
        if k == 3:                                                                               # a long insertion
            cut = int(rng.integers(0, len(x) + 1)); x = np.concatenate([x[:cut], S.random_codes(rng, int(rng.integers(20, 60))), x[cut:]])
        if k == 4 and len(x) > 8: x[len(x) // 3:len(x) // 3 + 5] = 4                           # an N run in the query ...
        if k == 5 and tl > 8: t[tl // 2:tl // 2 + 4] = 4                                         # ... and in the target
        if k == 6: x = x[:max(1, len(x) // 4)]                                                  # a query much shorter than the target
        if len(x) == 0: x = S.random_codes(rng, 1)
        out.append((x.astype(np.uint8), t.astype(np.uint8), it % 2 == 1))
    return out


def mismatches(cfg, probs, with_band=True):
    """problems on which the row-sweep model (and the band model, where its proof holds) differ from the oracle"""
    a, b, amb, q, e, q2, e2 = cfg
    qq, ee, qq2, ee2 = consts(q, e, q2, e2)[:4]
    OL = O.lib()
    mat = np.zeros(25, np.int8); OL.mmo_ksw_gen_simple_mat(5, mat.ctypes.data, a, b, amb)
    bad = n_band = 0
    for x, t, right in probs:
        ez = O.Extz()
        OL.mmo_ksw_extd2(len(x), x.ctypes.data, len(t), t.ctypes.data, 5, mat.ctypes.data, q, e, q2, e2, len(x) + len(t) + 5, 400, -1,
                         8 | (2 if right else 0), C.byref(ez))
        exp = [ez.cigar[k] for k in range(ez.n_cigar)]
        if ez.n_cigar: OL.free(ez.cigar)
        sc, P = row_sweep(x, t, a, b, amb, q, e, q2, e2, right)
        ok = sc == ez.score and backtrack(P, len(x), len(t)) == exp
        if with_band and ok:
            pl = plan(len(x), len(t), 64, a, qq, ee, qq2, ee2)
            if pl is not None:
                h_end, bsc, BP = band_sweep(x, t, a, b, amb, q, e, q2, e2, right, pl[0], 64)
                if h_end >= pl[1]:
                    n_band += 1
                    ok = bsc == ez.score and backtrack(BP, len(x), len(t)) == exp
        bad += not ok
    return bad, n_band


def boundary_families():
    """gap sums 126..131 in several (q + e) / (q2 + e2) splits, each also given with the pieces swapped (ksw2 re-orders them)"""
    out = []
    for gs in range(126, 132):
        for qe in (20, 42, 60, 64):
            qe2 = gs - qe
            if qe2 < qe or qe2 > 127: continue
            e, e2 = max(2, qe // 12), 1
            cfg = (1, min(2 * qe, 19), 1, qe - e, e, qe2 - e2, e2)
            out.append(cfg)
            out.append(cfg[:3] + (qe2 - e2, e2, qe - e, e))                                   # swapped pieces
    return out


def match_families():
    """match scores 118..127 against several gap costs"""
    return [(a, 4, 1, q, e, q2, e2) for a in range(118, 128) for (q, e, q2, e2) in ((4, 2, 24, 1), (2, 1, 10, 0), (1, 2, 20, 1))]


def special():
    return [(1, 126, 1, 60, 3, 64, 1), (1, 126, 1, 64, 1, 60, 3), (2, 12, 1, 4, 2, 24, 1), (3, 2 * 40, 1, 30, 10, 77, 1),   # b = 2 (q + e)
            (2, 4, 0, 4, 2, 24, 1), (1, 19, 0, 39, 3, 85, 1), (1, 19, 0, 40, 3, 85, 1), (2, 4, 0, 4, 2, 24, 7),               # sc_ambi 0: sc_N = -e2
            (2, 8, 127, 40, 24, 60, 4), (2, 8, 100, 40, 24, 60, 4), (2, 6, 40, 14, 6, 60, 2)]                                 # large sc_ambi


def random_tuples(rng, n):
    """every parameter in 1..127 with q + e <= 127, q2 + e2 <= 127, b <= 2 (q + e): most fall outside the domain"""
    out = []
    while len(out) < n:
        q, e, q2, e2 = (int(v) for v in rng.integers(1, 128, 4))
        if q + e > 127 or q2 + e2 > 127: continue
        a, amb = int(rng.integers(1, 128)), int(rng.integers(0, 128))
        b = int(rng.integers(1, min(127, 2 * min(q + e, q2 + e2)) + 1))
        out.append((a, b, amb, q, e, q2, e2))
    return out


def random_inside(rng, n, domain):
    """random scorings the predicate accepts with a regular cost: small match scores and gap costs near the edges"""
    out = []
    while len(out) < n:
        e2 = int(rng.integers(0, 4)); e = int(rng.integers(e2 + 1, 12))
        q = int(rng.integers(1, 60)); q2 = int(rng.integers(q + e - e2, 124))
        a = int(rng.integers(1, 128 - q - 2 * e)) if rng.random() < 0.5 else int(rng.integers(1, 6))
        b = int(rng.integers(1, min(127, 2 * (q + e)) + 1)); amb = int(rng.integers(0, 2 * (q + e) + 1)) if rng.random() < 0.3 else 1
        cfg = (a, b, amb, q, e, q2, e2) if rng.random() < 0.8 else (a, b, amb, q2, e2, q, e)
        if domain(cfg) and regular(cfg) and valid(cfg): out.append(cfg)
    return out


def test_presets_and_regular_costs_are_inside(domain):
    """preset routing (and speed) is unchanged: every preset and every tuple the row-sweep model already holds against the oracle"""
    for name, cfg in PRESETS.items():
        assert domain(cfg), name
    for cfg in REGULAR:
        assert domain(cfg), cfg


def test_the_observed_wrap_scorings_are_rejected(built, domain):
    """the scorings whose plain recurrence is seen to differ from the SSE kernel are outside -- and they do differ (the table of the issue)"""
    rng = np.random.default_rng(5)
    for cfg in WRAPS:
        assert valid(cfg) and regular(cfg) and not domain(cfg), cfg
        assert mismatches(cfg, problems(rng, 16), with_band=False)[0] >= 4, cfg
    for cfg in EDGES:
        assert domain(cfg) and mismatches(cfg, problems(rng, 16))[0] == 0, cfg


@pytest.mark.parametrize("family", ["presets", "gap_sum", "match", "special"])
def test_inside_the_domain_the_plain_recurrence_is_the_sse_kernel(built, domain, family):
    cfgs = {"presets": list(PRESETS.values()) + REGULAR, "gap_sum": boundary_families(), "match": match_families(), "special": special()}[family]
    rng = np.random.default_rng(17 + len(family))
    n_in = n_out = n_band = 0
    for cfg in cfgs:
        if not (valid(cfg) and regular(cfg)):
            continue
        if domain(cfg):
            bad, nb = mismatches(cfg, problems(rng, 16))
            assert bad == 0, cfg
            n_in += 1; n_band += nb
        else:
            n_out += 1
    assert n_in >= 4 and n_band > 0, (n_in, n_band)
    if family in ("gap_sum", "match"):
        assert n_out >= 4, n_out                                       # both sides of the edge are in the sweep


def test_random_scorings(built, domain):
    """200 seeded random tuples over the whole int8 range (the predicate decides; the accepted regular ones must agree) plus 40 drawn inside
    the domain near its edges; a share of the rejected regular ones is run too: most of those disagree"""
    rng = np.random.default_rng(2026)
    tup = random_tuples(rng, 200)
    inside = [c for c in tup if domain(c) and regular(c) and valid(c)] + random_inside(rng, 40, domain)
    for cfg in inside:
        assert mismatches(cfg, problems(rng, 16))[0] == 0, cfg
    rejected = [c for c in tup if not domain(c) and regular(c) and valid(c)][:12]
    assert len(rejected) >= 8
    n_differ = sum(mismatches(cfg, problems(rng, 16), with_band=False)[0] > 0 for cfg in rejected)
    assert n_differ >= len(rejected) // 2, (n_differ, len(rejected))
