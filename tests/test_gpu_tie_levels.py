"""The literal radix_sort_128x emulation (k_sort_level_mw / k_sort_tasks, mappy-rs_amd/csrc/mm355_kernels.hip) read by read against the oracle.
 * E. coli-scale genome, MM355_FAST_SORT=0: every read takes the emulation on its whole array -- with the default size classes (wave tasks
   and, for the anchor-rich reads, the 256-thread levels) and with both thresholds at their floor of 65, where every bucket of more than 65
   elements, whole arrays included, goes through the 1024-thread level kernel and hands its children on level by level;
 * mid-scale human-like genome, the default route (cull + segmented sort + emulation of the reads with equal keys) with the thresholds at 65.
A regression net for the existing emulation: of what it runs, this change touches the wave priority of the two kernels only.  That the level
kernels ran is asserted from the stage timers of sr.stats() (ms_kernel[7] / [20] / [21]): n_a_literal counts the tie path of the cull route only,
and is asserted there.  The switches are read once per process, so every configuration is a child process (as test_gpu_human.py::test_anchor_cull_in_many_passes)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONT = dict(n50=10000, sigma=0.75, lo=500, hi=100000)
N_READS = 48
# the reads of the E. coli-scale case: those of block 0 with equal-x neighbours (few reads of a bacterial genome span two copies of a repeat;
# found with the oracle alone, and asserted with it below), five of them with more than 2048 anchors, and the block's first 37
PICK = [178, 720, 913, 966, 1079, 1119, 1177, 1189, 1252, 2491, 2620] + list(range(37))


def _device_index(L, _ffi, g, names):
    io, mo = _ffi.IdxOpt(), _ffi.MapOpt()
    L.mm355_set_opt(None, C.byref(io), C.byref(mo))
    _ffi.check(L.mm355_set_opt(b"map-ont", C.byref(io), C.byref(mo))); mo.flag |= 4
    ptrs = (C.c_char_p * len(g))(*[C.cast(c.ctypes.data, C.c_char_p) for c in g])
    lens = (C.c_int64 * len(g))(*[len(c) for c in g]); nm = (C.c_char_p * len(g))(*[n.encode() for n in names])
    idx = C.c_void_p()
    _ffi.check(L.mm355_index_build_device(C.byref(io), len(g), ptrs, lens, nm, 0, C.byref(idx)))
    L.mm355_mapopt_update(C.byref(mo), idx)
    return idx, mo


def _n_ties(exp):
    return int((exp[1:, 0] == exp[:-1, 0]).sum()) if len(exp) > 1 else 0


def literal_case():
    """child: every read through the emulation (MM355_FAST_SORT=0), sorted = 1 against the oracle"""
    from mappy_rs import _ffi
    from oracle import oracle as O
    import synthdata as S
    L = _ffi.lib()
    g = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01)))
    names = ["chrE"]
    block, _ = S.make_read_block(4, 0, g, **ONT)
    reads = [block[i] for i in PICK]
    assert len(reads) == N_READS
    orc = O.OracleAligner(codes=g, names=names, preset="map-ont", n_threads=16)
    exp = [orc.anchors(rd, sorted_=True)[0] for rd in reads]
    n_tie_reads = sum(_n_ties(e) > 0 for e in exp)
    assert n_tie_reads >= 2, n_tie_reads                         # the order of equal keys is what the emulation is for
    idx, mo = _device_index(L, _ffi, g, names)
    sr = _ffi.StageRunner(idx, mo, 0)
    try:
        got, _, _ = sr.anchors(reads, sorted_=1)
        st = sr.stats()
        assert st.n_sort_fast_reads == 0, st.n_sort_fast_reads   # nobody took the segmented sort
        mk = list(st.ms_kernel)                                  # [7]: the levels above the heavy threshold, [20]: the 256-thread levels, [21]: the wave tasks
        assert mk[7] + mk[20] > 0 and mk[21] > 0, (mk[7], mk[20], mk[21])
        if os.environ.get("MM355_SORT_HEAVY_MIN") == "65":
            assert mk[7] > 0, mk[7]                              # every whole array of more than 65 anchors starts in the 1024-thread class
        n_big = sum(len(e) > int(os.environ.get("MM355_SORT_MEDIUM_MIN", "2048")) for e in exp)
        assert n_big >= 2, n_big                                 # whole arrays that start in a block level
        assert len(got) == len(reads)
        for i in range(len(reads)):
            assert np.array_equal(got[i], exp[i]), i
    finally:
        sr.close()
        L.mm355_index_free(idx)
    print("literal-ok", n_tie_reads, n_big)


def cull_case():
    """child: cull + segmented sort + emulation of the reads with equal keys; sorted = 1, sorted = 2 and the chains against the oracle"""
    from mappy_rs import _ffi
    from oracle import oracle as O
    import synthdata as S
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_human import _check_culled
    L = _ffi.lib()
    g, names = S.make_human_like(3, 0.05)
    reads, _ = S.make_read_block(4, 2, g, **ONT)
    reads = reads[:64]
    orc = O.OracleAligner(codes=g, names=names, preset="map-ont", n_threads=16)
    idx, mo = _device_index(L, _ffi, g, names)
    sr = _ffi.StageRunner(idx, mo, 0)
    try:
        full_g, _, _ = sr.anchors(reads, sorted_=1, cap=40_000_000)
        st = sr.stats()
        assert st.n_sort_fast_reads == len(reads) and st.n_a_kept == st.n_a and st.n_a_literal > 0, (st.n_sort_fast_reads, st.n_a_kept, st.n_a, st.n_a_literal)
        cul_g, _, _ = sr.anchors(reads, sorted_=2, cap=40_000_000)
        st = sr.stats()
        assert st.n_sort_fast_reads == len(reads) and 0 < st.n_a_kept < 0.9 * st.n_a, (st.n_a_kept, st.n_a)
        assert st.n_sort_tie_reads >= 1 and st.n_a_literal > 0, (st.n_sort_tie_reads, st.n_a_literal)
        n_tie_reads = n_culled = 0
        exp_all = []
        for i, rd in enumerate(reads):
            exp, _, _, _ = orc.anchors(rd, sorted_=True)
            exp_all.append(exp)
            assert np.array_equal(full_g[i], exp), i
            n_tie_reads += _n_ties(exp) > 0
            n_culled += _check_culled(exp, cul_g[i], mo.max_gap, 3)
        assert n_tie_reads >= 2 and n_culled == st.n_a - st.n_a_kept, (n_tie_reads, n_culled, st.n_a - st.n_a_kept)
        ch = sr.chains(reads, cap=40_000_000)
        for i, rd in enumerate(reads):
            eu, eb = orc.chains(exp_all[i], len(rd))
            assert np.array_equal(ch[i][0], eu), i
            assert np.array_equal(ch[i][1], eb), i
    finally:
        sr.close()
        L.mm355_index_free(idx)
    print("cull-ok", n_tie_reads)


def _child(func, **switches):
    code = "import sys; sys.path[:0] = %r; import tests.test_gpu_tie_levels as T; T.%s()" % ([ROOT, os.path.join(ROOT, "mappy-rs_amd")], func)
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("switches", [dict(), dict(MM355_SORT_HEAVY_MIN="65", MM355_SORT_MEDIUM_MIN="65")], ids=["default-classes", "thresholds-65"])
def test_literal_emulation_read_by_read(built, switches):
    _child("literal_case", MM355_FAST_SORT="0", **switches)


def test_cull_and_tie_path_with_small_thresholds(built):
    _child("cull_case", MM355_SORT_HEAVY_MIN="65", MM355_SORT_MEDIUM_MIN="65")
