"""The extension problems of tests/test_gpu_map.py::test_dp_kernel_parity -- every kernel class of mm355_dp.hip, at the borders of its
size classes -- and the two steps every DP parity test takes with them: one mm355_stage_dp launch, and the field-by-field comparison with
the oracle's restatement of U:ksw2_extd2_sse.c.  Shared by test_gpu_map.py and test_gpu_dp_scoring.py (the same set under other scorings)."""
import ctypes as C

import numpy as np

from oracle import oracle as O
import synthdata as S


def parity_problems(seed=9):
    """(jobs, qs, ts, n_short, n_rowl): jobs[i] = (qlen, tlen, w, zdrop, end_bonus, flag); jobs[n_short:n_rowl] are the full-band fills of
    targets 1025..8192 (k_ksw_rowl), the last two jobs the 65-KB targets of the eight-wave register kernel"""
    rng = np.random.default_rng(seed)
    jobs, qs, ts = [], [], []
    EXTZ, RIGHT, REV, APPROX = 0x40, 0x02, 0x80, 0x08
    APPROX_DROP = 0x10
    kinds = [(EXTZ, 751, 400), (EXTZ | RIGHT | REV, 751, 200), (APPROX, 30001, 400), (0, None, 400), (APPROX | RIGHT, 30001, 400),
             (EXTZ | APPROX | APPROX_DROP, 751, 100), (RIGHT, None, 400), (APPROX, None, 400), (EXTZ, None, 60)]
    spans = [(1, 40), (100, 140), (240, 270), (500, 530), (1000, 1040), (1, 700), (900, 2600)]   # around the size-class borders
    for i in range(540):
        lo, hi = spans[i % len(spans)]
        tl = int(rng.integers(lo, hi))
        t = S.random_codes(rng, tl)
        q = S.mutate(t, rng, 0.05, 0.03, 0.03)
        if i % 11 == 0 and len(q) > 20:
            q[len(q) // 2:len(q) // 2 + 3] = 4
        if i % 17 == 0 and tl > 30:
            t[tl // 3:tl // 3 + 2] = 4
        if i % 13 == 0:
            q = np.concatenate([q[:len(q) // 2], S.random_codes(rng, 300)])   # forces z-drop
        if i % 19 == 0:
            q = q[:max(1, len(q) // 3)]                                       # query much shorter than the target
        if len(q) == 0:
            q = S.random_codes(rng, 5)
        flag, w, zd = kinds[i % len(kinds)]
        if w is None:
            w = int(rng.integers(5, 200))
        jobs.append((len(q), tl, w, zd, -1 if i % 5 else 10, flag)); qs.append(q.astype(np.uint8)); ts.append(t.astype(np.uint8))
    # gap fills whose band never binds (KSW_EZ_APPROX_MAX, w >= qlen + tlen, targets <= 1024): the row-sweep kernel k_ksw_row -- every
    # register-set border (128 / 256 / ... / 1024), query much longer / shorter than the target, ambiguous bases, left- and right-aligned
    # gaps, reversed CIGARs, long indels (the second gap piece), empty-ish problems
    for i in range(420):
        tl = int(rng.choice([1, 2, 3, 17, 127, 128, 129, 200, 255, 256, 257, 300, 383, 384, 385, 511, 512, 513, 640, 767, 768, 769, 1023, 1024])) if i % 3 == 0 else int(rng.integers(1, 1025))
        t = S.random_codes(rng, tl)
        q = S.mutate(t, rng, 0.06, 0.03, 0.03)
        if i % 7 == 0 and len(q) > 40:
            cut = int(rng.integers(5, len(q) - 30)); q = np.concatenate([q[:cut], q[cut + int(rng.integers(1, 30)):]])        # deletion
        if i % 7 == 3:
            cut = int(rng.integers(0, len(q) + 1)); q = np.concatenate([q[:cut], S.random_codes(rng, int(rng.integers(1, 120))), q[cut:]])   # insertion
        if i % 10 == 0:
            q = S.random_codes(rng, int(rng.integers(1, 900)))                 # unrelated query, any length ratio
        if i % 11 == 0 and len(q) > 6:
            q[len(q) // 2:len(q) // 2 + 3] = 4
        if i % 13 == 0 and tl > 6:
            t[tl // 3:tl // 3 + 2] = 4
        if len(q) == 0:
            q = S.random_codes(rng, 1)
        flag = APPROX | (RIGHT if i % 2 else 0) | (REV if i % 4 == 1 else 0)
        jobs.append((len(q), tl, len(q) + tl + int(rng.integers(0, 50)), 400, -1, flag)); qs.append(q.astype(np.uint8)); ts.append(t.astype(np.uint8))
    # the same with targets of 1025..4096 bases: the eight-wave row sweep k_ksw_rowl (one 512-column panel per wave, 64-row batches):
    # every panel border, one to eight panels, queries shorter than / equal to / just over one batch and up to the LDS limit of 5120 rows
    n_short = len(jobs)
    for i in range(52):   # (the last eight: targets beyond 4096 -- a wave takes a second panel)
        tl = int([1025, 1536, 1537, 2047, 2048, 2049, 2560, 2561, 3000, 3583, 3584, 3585, 4000, 4095, 4096][i % 15]) if i < 30 else int(rng.integers(1025, 4097)) if i < 44 else \
             int([4097, 4608, 4609, 5000, 5120, 6000, 7000, 8192][i - 44])
        t = S.random_codes(rng, tl)
        q = S.mutate(t, rng, 0.06, 0.03, 0.03)
        if i % 5 == 0:
            cut = int(rng.integers(5, len(q) - 600)); q = np.concatenate([q[:cut], q[cut + int(rng.integers(1, 500)):]])        # deletion
        if i % 5 == 3:
            cut = int(rng.integers(0, len(q) + 1)); q = np.concatenate([q[:cut], S.random_codes(rng, int(rng.integers(1, 700))), q[cut:]])   # insertion
        if i % 8 == 1:
            q = q[:int([1, 63, 64, 65, 128, 700][(i // 8) % 6])]               # a few rows only
        if i % 8 == 6:
            q = S.random_codes(rng, int(rng.integers(1, 5121)))                # unrelated query, any length ratio
        if len(q) > 5120:
            q = q[:5120]                                                       # the kernel's row limit (its LDS column buffers)
        if i % 6 == 0:
            q[len(q) // 2:len(q) // 2 + 3] = 4
        if i % 7 == 0:
            t[tl // 3:tl // 3 + 2] = 4
        flag = APPROX | (RIGHT if i % 2 else 0) | (REV if i % 4 == 1 else 0)
        jobs.append((len(q), tl, len(q) + tl + int(rng.integers(0, 50)), 400, -1, flag)); qs.append(q.astype(np.uint8)); ts.append(t.astype(np.uint8))
    # exact sweeps with a narrow band over long targets: k_ksw_regw, the register kernel whose 1024-position window follows the band
    # (extensions of read ends: w = 751; the widest band it takes, 832; narrow ones; band-limited global fills; z-drop half way; queries
    # much shorter / longer than the target, so that the band leaves the matrix early; ambiguous bases across a window move)
    n_rowl = len(jobs)
    for i in range(40):
        tl = int([1025, 1100, 1151, 1152, 1153, 2000, 2047, 2048, 3000, 5000, 7000, 9000][i % 12]) if i < 24 else int(rng.integers(1025, 6000))
        t = S.random_codes(rng, tl)
        q = S.mutate(t, rng, 0.05, 0.03, 0.03)
        if i % 6 == 1:
            cut = int(rng.integers(400, len(q) - 400)); q = np.concatenate([q[:cut], q[cut + int(rng.integers(20, 300)):]])        # deletion: the path moves off the main diagonal
        if i % 6 == 4:
            cut = int(rng.integers(400, len(q) - 400)); q = np.concatenate([q[:cut], S.random_codes(rng, int(rng.integers(20, 300))), q[cut:]])
        if i % 7 == 2:
            q = np.concatenate([q[:len(q) * 2 // 3], S.random_codes(rng, 900)])      # z-drop after two thirds
        if i % 9 == 3:
            q = q[:int(rng.integers(1, 900))]                                      # short query: band limited by the query
        if i % 9 == 5:
            q = np.concatenate([q, S.random_codes(rng, 1500)])                     # query runs past the target
        if i % 5 == 0:
            q[len(q) // 2:len(q) // 2 + 3] = 4; t[tl // 2 + 100:tl // 2 + 102] = 4
        flag, w, zd = [(EXTZ, 751, 400), (EXTZ | RIGHT | REV, 751, 200), (0, 832, 400), (RIGHT, 300, 400), (EXTZ, 16, 100), (0, 751, 10000)][i % 6]
        jobs.append((len(q), tl, w, zd, -1 if i % 4 else 10, flag)); qs.append(q.astype(np.uint8)); ts.append(t.astype(np.uint8))
    # ... and two whose query + target need more than 64 KB of LDS (the eight-wave kernel stages both sequences there: dynamic LDS beyond the
    # default limit, opted into per launch); qlen * tlen stays below max_sw_mat (beyond it the stage answers "z-dropped" without aligning)
    for tl, fl in ((65000, EXTZ), (64800, EXTZ | RIGHT | REV)):
        t = S.random_codes(rng, tl)
        q = S.mutate(t[:1450], rng, 0.05, 0.03, 0.03)[:1500]
        jobs.append((len(q), tl, 751, 100000, -1, fl)); qs.append(q.astype(np.uint8)); ts.append(t.astype(np.uint8))
    # paths along the matrix border and along the band edge while the band spans five or more 128-cell blocks (the catch-all instance
    # of the register kernels): a global alignment that opens with a 560-base deletion runs through the top-row cells t = r >= 512, whose
    # y / u are boundary values; one that opens with a (w - 1)-base insertion rides the lower band edge, where x[st - 1] / v[st - 1] are
    # defaults whenever st did not move
    for i in range(24):
        tl = int([1020, 1000, 900, 3000, 2500, 5000][i % 6])
        t = S.random_codes(rng, tl)
        m = S.mutate(t, rng, 0.03, 0.01, 0.01)
        w = 751
        if i % 4 == 0: q = m[int([560, 600, 700, 520][(i // 4) % 4]):]
        elif i % 4 == 1: q = np.concatenate([S.random_codes(rng, w - 1 - (i // 4) % 3), m])
        elif i % 4 == 2: q = np.concatenate([m[:len(m) // 2], S.random_codes(rng, 700), m[len(m) // 2:]])   # the same in the middle of the matrix
        else: q = np.concatenate([m[:len(m) // 3], m[len(m) // 3 + 650:]])
        flag = [0, RIGHT, EXTZ, EXTZ | RIGHT | REV][(i // 2) % 4]
        jobs.append((len(q), tl, w, 100000, -1, flag)); qs.append(q.astype(np.uint8)); ts.append(t.astype(np.uint8))
    return jobs, qs, ts, n_short, n_rowl


def run_stage_dp(al, mo, jobs, qs, ts):
    """one mm355_stage_dp launch of the jobs under the options mo (a ctypes mapopt, e.g. a copy of al._mo with another scoring):
    (res, cig, sr) -- the caller reads sr.stats() and closes sr"""
    from mappy_rs import _ffi
    L = _ffi.lib()
    qcat = np.concatenate(qs); tcat = np.concatenate(ts)
    ja = (_ffi.DpJob * len(jobs))()
    qo = to = 0
    for i, (ql, tl, w, zd, eb, fl) in enumerate(jobs):
        ja[i].qlen, ja[i].tlen, ja[i].qoff, ja[i].toff, ja[i].w, ja[i].zdrop, ja[i].end_bonus, ja[i].flag = ql, tl, qo, to, w, zd, eb, fl
        qo += ql; to += tl
    res = (_ffi.DpRes * len(jobs))()
    cap = int(qcat.size + tcat.size + 4 * len(jobs))
    cig = np.zeros(cap, np.uint32)
    sr = al._stage_runner()
    _ffi.check(L.mm355_stage_dp(sr.ctx, C.byref(mo), len(jobs), ja, qcat.ctypes.data, qcat.size, tcat.ctypes.data, tcat.size, res, cig.ctypes.data, cap))
    return res, cig, sr


def check_against_oracle(mo, jobs, qs, ts, res, cig, tag=None):
    """every ez field and the CIGAR of every job equal the oracle's; returns the number of z-dropped problems"""
    OL = O.lib()
    mat = np.zeros(25, np.int8)
    OL.mmo_ksw_gen_simple_mat(5, mat.ctypes.data, mo.a, mo.b, mo.sc_ambi)
    n_zd = 0
    for i, (ql, tl, w, zd, eb, fl) in enumerate(jobs):
        ez = O.Extz()
        OL.mmo_ksw_extd2(ql, qs[i].ctypes.data, tl, ts[i].ctypes.data, 5, mat.ctypes.data, mo.q, mo.e, mo.q2, mo.e2, w, zd, eb, fl, C.byref(ez))
        emax, ezd = ez.max_zd & 0x7fffffff, ez.max_zd >> 31
        r = res[i]
        assert (r.max, r.zdropped, r.max_q, r.max_t, r.mqe, r.mqe_t, r.mte, r.mte_q, r.score, r.reach_end, r.n_cigar) == \
               (emax, ezd, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score, ez.reach_end, ez.n_cigar), (tag, i, jobs[i])
        exp = [ez.cigar[k] for k in range(ez.n_cigar)]
        assert list(cig[r.cigar_off:r.cigar_off + r.n_cigar]) == exp, (tag, i)
        n_zd += ezd
        if ez.n_cigar: OL.free(ez.cigar)
    return n_zd
