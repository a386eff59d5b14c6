"""Contexts on the GPU: ten at once on one device (eight on the device's stream pool, two with streams of their own), destroyed and made
again; and the stage / kernel timers of a call that records many event pairs.  Reads of the fixture genome (tests/golden/test.fa), map-ont
with CIGAR and cs; nothing is written."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _capi

pytestmark = pytest.mark.gpu

OUT_CS = 1          # MM355_OUT_CS (include/mm355.h)
KT_SKETCH = 0       # first slot of mm355_stats_t::ms_kernel (mm355_dev.h)
STAGE_MS = ("ms_sketch", "ms_seed", "ms_seed_lookup", "ms_seed_expand", "ms_sort", "ms_chain", "ms_backtrack", "ms_rmq", "ms_dp", "ms_host", "ms_total")


def _fixture_reads(golden_dir, n):
    """n reads cut from the four contigs of the fixture genome: windows of 150 bases and more, a substitution every 41st base, every other read
    reverse-complemented"""
    contigs, cur = [], []
    for line in open(os.path.join(golden_dir, "test.fa")):
        if line.startswith(">"):
            cur = []; contigs.append(cur)
        else:
            cur.append(line.strip())
    contigs = ["".join(c).upper() for c in contigs]
    rng = np.random.default_rng(355)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    reads = []
    for i in range(n):
        s = contigs[i % len(contigs)]
        ln = int(rng.integers(150, len(s) + 1))
        a = int(rng.integers(0, len(s) - ln + 1))
        r = list(s[a:a + ln])
        for j in range(7 + i % 5, ln, 41):
            r[j] = comp.get(r[j], "A")
        r = "".join(r)
        reads.append("".join(comp.get(c, "N") for c in reversed(r)) if i & 1 else r)
    return reads


@pytest.fixture(scope="module")
def al(built, golden_dir):
    import mappy_rs
    return mappy_rs.Aligner(os.path.join(golden_dir, "test.fa"), preset="map-ont")


def _same(a, b):
    return (np.array_equal(a.off, b.off) and np.array_equal(a.status, b.status) and _capi.raw(a.hits) == _capi.raw(b.hits)
            and np.array_equal(a.cigar, b.cigar) and a.str == b.str)


def test_ten_contexts_on_one_device(al, golden_dir):
    """(run before the Aligner makes a context of its own, so that the ten start from the first free pool slot)"""
    from mappy_rs import _ffi
    L = al._L
    reads = _fixture_reads(golden_dir, 24)
    ref = None
    for n_ctx in (10, 3):       # ten at once (the pool has eight slots); then, with those gone, three more
        ctxs = []
        try:
            for _ in range(n_ctx):
                c = C.c_void_p()
                _ffi.check(L.mm355_ctx_create(al._idx, 0, C.byref(c)))
                ctxs.append(c)
            views = [_ffi.map_raw(L, c, al._mo, reads, OUT_CS) for c in ctxs]
        finally:
            for c in ctxs:
                L.mm355_ctx_destroy(c)
        ref = ref or views[0]
        assert len(ref.hits) >= 20 and len(ref.cigar) > 0 and len(ref.str) > 0
        assert len(views) == n_ctx and all(_same(v, ref) for v in views)
    assert _same(_capi.map_raw(al, reads, OUT_CS), ref)


def test_stats_of_a_call_with_many_pending_pairs(al, golden_dir, monkeypatch):
    """32 reads: timers are on.  With a budget of 1 MB the extension rounds are cut into many launches, and one call begins far more timer
    pairs than fit between two resolves.  Every time read back is a time; the records do not change."""
    reads = _fixture_reads(golden_dir, 32)
    ref = _capi.map_raw(al, reads, OUT_CS)
    monkeypatch.setenv("MM355_DP_BUDGET_MB", "1")
    cut = _capi.map_raw(al, reads, OUT_CS)
    st = _capi.stats(al)
    times = {"ms_kernel[%d]" % i: x for i, x in enumerate(st.ms_kernel)}
    times.update({"ms_dp_group[%d]" % i: x for i, x in enumerate(st.ms_dp_group)})
    times.update({k: getattr(st, k) for k in STAGE_MS})
    print(st.n_rounds_split, st.n_ext_rounds, {k: round(v, 4) for k, v in times.items() if v})
    bad = {k: v for k, v in times.items() if not (math.isfinite(v) and v >= 0)}
    assert not bad, bad
    assert st.ms_kernel[KT_SKETCH] > 0
    assert _same(cut, ref)
