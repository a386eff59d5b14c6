"""mm355_index_load_mmi_device (mm355_idxload.hip): an .mmi loaded straight into HBM is the index the host loader makes of the same file --
its dump, its statistics, its mid_occ and every mapping result are identical -- for minimap2's own file, the oracle's dumps and this
library's canonical ones, with pieces so small that buckets straddle them; the files and devices it refuses; Aligner(load_on_gpu=True)."""
import ctypes as C
import os
import random

import pytest

import _mmi
import _mmiload
from test_gpu_index_dump import _map_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ffi(built):
    from mappy_rs import _ffi
    _ffi.lib()
    return _ffi


def _host_canonical(ffi, src, dst):
    """this library's canonical dump of a file, through the host loader"""
    rc, h = _mmi.load(ffi, src, _mmi.idxopt(ffi, 15, 10, 0))
    assert rc == 0
    try:
        return _mmi.dump(ffi, h, dst)
    finally:
        ffi.lib().mm355_index_free(h)


@pytest.fixture(scope="module")
def world(ffi, golden_dir, tmp_path_factory):
    """name -> path: test.mmi, the oracle's dump of the repeat-rich reference at the four settings and the host's canonical dump of each"""
    d = tmp_path_factory.mktemp("gpuidxload")
    recs = _mmi.repeat_rich_records()
    fa = str(d / "rep.fa")
    _mmi.write_fasta(fa, recs)
    files = {"golden": os.path.join(golden_dir, "test.mmi")}
    for k, w, flag in _mmi.SETTINGS:
        name = "%d_%d_%d" % (k, w, flag)
        files["oracle_" + name] = str(d / ("oracle_%s.mmi" % name))
        _mmiload.oracle_dump(fa, k, w, flag, files["oracle_" + name])
        files["canon_" + name] = str(d / ("canon_%s.mmi" % name))
        _host_canonical(ffi, files["oracle_" + name], files["canon_" + name])
    files["canon_golden"] = str(d / "canon_golden.mmi")
    _host_canonical(ffi, files["golden"], files["canon_golden"])
    return dict(dir=d, recs=recs, fa=fa, files=files, reads=_mmi.make_reads(recs))


def load_dev(ffi, path, device=0):
    h = C.c_void_p()
    rc = ffi.lib().mm355_index_load_mmi_device(str(path).encode(), device, C.byref(h))
    return rc, h


def _facts(ffi, h):
    """mm355_index_info, mm355_index_stat and the mid_occ mm355_mapopt_update computes (default and a fraction that reaches into the counts)"""
    L = ffi.lib()
    k, w, b, fl, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint32()
    assert L.mm355_index_info(h, C.byref(k), C.byref(w), C.byref(b), C.byref(fl), C.byref(n)) == 0
    st = [C.c_int64() for _ in range(4)]
    assert L.mm355_index_stat(h, *[C.byref(x) for x in st]) == 0
    mids = []
    for frac in (2e-4, 0.01, 0.2):
        io, mo = ffi.IdxOpt(), ffi.MapOpt()
        L.mm355_set_opt(None, C.byref(io), C.byref(mo))
        mo.mid_occ_frac, mo.min_mid_occ = frac, 1
        assert L.mm355_mapopt_update(C.byref(mo), h) == 0
        mids.append(mo.mid_occ)
    names = [(L.mm355_index_seq_name(h, i), L.mm355_index_seq_len(h, i)) for i in range(n.value)]
    return (k.value, w.value, b.value, fl.value, n.value), tuple(x.value for x in st), tuple(mids), names


def _same_as_host_load(ffi, path, tmp_path, canonical=False):
    """the device-loaded index of `path` against the host-loaded one"""
    L = ffi.lib()
    rc, hh = _mmi.load(ffi, path, _mmi.idxopt(ffi, 15, 10, 0))
    assert rc == 0
    rc, hd = load_dev(ffi, path)
    assert rc == 0 and hd
    try:
        assert L.mm355_index_get(hd, 0, None, 0) == ffi.MM355_EUNSUP            # device-resident: no host table
        assert L.mm355_index_get(hh, 0, None, 0) >= 0
        want = _mmi.dump(ffi, hh, tmp_path / "host.mmi")
        got = _mmi.dump(ffi, hd, tmp_path / "dev.mmi")
        assert got == want
        if canonical:
            assert got == open(path, "rb").read()
        assert _facts(ffi, hd) == _facts(ffi, hh)
    finally:
        L.mm355_index_free(hd); L.mm355_index_free(hh)
    return got


# ------------------------------------------------------------------ 1. dump equality
FILES = ["golden", "canon_golden"] + [p + "%d_%d_%d" % s for s in _mmi.SETTINGS for p in ("oracle_", "canon_")]


@pytest.mark.parametrize("name", FILES)
def test_dump_equals_host_load(ffi, world, tmp_path, name, monkeypatch):
    monkeypatch.delenv("MM355_IDXLOAD_PIECE", raising=False)
    _same_as_host_load(ffi, world["files"][name], tmp_path, canonical=name.startswith("canon_"))


# ------------------------------------------------------------------ 2. small pieces
@pytest.mark.parametrize("piece", [256, 4096])
@pytest.mark.parametrize("name", [p + s for s in ("15_10_0", "6_3_0") for p in ("oracle_", "canon_")])
def test_small_pieces(ffi, world, tmp_path, monkeypatch, name, piece):
    """buckets across three or more pieces, split pair segments (tests/test_mmi_walk_host.py asserts that of the plan at 256)"""
    monkeypatch.setenv("MM355_IDXLOAD_PIECE", str(piece))
    _same_as_host_load(ffi, world["files"][name], tmp_path, canonical=name.startswith("canon_"))


def test_small_pieces_long_run_beside_short_runs(ffi, tmp_path, monkeypatch):
    """the skewed reference of test_gpu_index_dump.py::test_long_run_beside_short_runs: a run above 4096 positions (eight and more pieces of
    4096 bytes) beside thousands of runs of 2-3"""
    rng = random.Random(5)
    a = _mmi._rand(rng, 15000)
    s = _mmi._rand(rng, 4000) + a + _mmi._rand(rng, 3000) + _mmi._rand(rng, 50) * 5000 + a + _mmi._rand(rng, 2500) + a[:7500] + _mmi._rand(rng, 500)
    h = _mmi.build(ffi, [("skew", s)], _mmi.idxopt(ffi, 15, 10, 0))
    try:
        src = _mmi.dump(ffi, h, tmp_path / "skew.mmi")
    finally:
        ffi.lib().mm355_index_free(h)
    runs = [int(v) & 0xffffffff for _, pairs in _mmi.parse_mmi(src)["buckets"] for key, v in pairs if not int(key) & 1]
    assert max(runs) > 4096 and sum(1 for r in runs if r <= 3) > 1000
    monkeypatch.setenv("MM355_IDXLOAD_PIECE", "4096")
    _same_as_host_load(ffi, tmp_path / "skew.mmi", tmp_path, canonical=True)


# ------------------------------------------------------------------ 3. mapping parity
@pytest.mark.parametrize("name", ["oracle_15_10_0", "canon_15_10_0"])
def test_maps_like_the_host_loaded_index(ffi, world, name, monkeypatch):
    monkeypatch.delenv("MM355_IDXLOAD_PIECE", raising=False)
    L = ffi.lib()
    path = world["files"][name]
    rc, hh = _mmi.load(ffi, path, _mmi.idxopt(ffi, 15, 10, 0))
    assert rc == 0
    try:
        want = _map_all(ffi, hh, world["reads"])
    finally:
        L.mm355_index_free(hh)
    rc, hd = load_dev(ffi, path)
    assert rc == 0
    try:
        assert _map_all(ffi, hd, world["reads"]) == want
    finally:
        L.mm355_index_free(hd)


# ------------------------------------------------------------------ 4. MM_I_NO_SEQ
def test_no_seq_file(ffi, world, tmp_path, monkeypatch):
    monkeypatch.delenv("MM355_IDXLOAD_PIECE", raising=False)
    L = ffi.lib()
    f = tmp_path / "noseq.mmi"
    f.write_bytes(_mmiload.no_seq(open(world["files"]["oracle_15_10_0"], "rb").read()))
    _same_as_host_load(ffi, f, tmp_path)

    def chain_only(h):
        io, mo = ffi.IdxOpt(), ffi.MapOpt()
        L.mm355_set_opt(None, C.byref(io), C.byref(mo))
        ffi.check(L.mm355_set_opt(b"map-ont", C.byref(io), C.byref(mo)))
        ffi.check(L.mm355_mapopt_update(C.byref(mo), h))
        ctx = C.c_void_p()
        ffi.check(L.mm355_ctx_create(h, 0, C.byref(ctx)))
        try:
            v = ffi.map_raw(L, ctx, mo, world["reads"], 0)
            res = (mo.mid_occ, v.off.tobytes(), v.status.tobytes(), v.hits.view("u1").tobytes())
            mo.flag |= 4                                                          # MM_F_CIGAR needs the sequence
            rc, none = ffi.map_raw(L, ctx, mo, world["reads"], 0, raise_on_error=False)
            assert rc == ffi.MM355_EUNSUP and none is None
        finally:
            L.mm355_ctx_destroy(ctx)
        assert len(res[3]) > 32 * C.sizeof(ffi.Hit)
        return res

    rc, hh = _mmi.load(ffi, f, _mmi.idxopt(ffi, 15, 10, 0))
    assert rc == 0
    try:
        want = chain_only(hh)
    finally:
        L.mm355_index_free(hh)
    rc, hd = load_dev(ffi, f)
    assert rc == 0
    try:
        fl = C.c_int32()
        L.mm355_index_info(hd, None, None, None, C.byref(fl), None)
        assert fl.value & 2 and L.mm355_index_getseq(hd, 0, 0, 10, (C.c_uint8 * 10)()) == -1
        assert chain_only(hd) == want
    finally:
        L.mm355_index_free(hd)


# ------------------------------------------------------------------ 5. errors
def _bad_run(data):
    """one multi-occurrence pair patched so that start + count > n of its bucket"""
    lay = _mmiload.layout(data)
    raw = bytearray(data)
    for (off, n, size), (_, pairs) in zip(lay["buckets"], lay["m"]["buckets"]):
        for j, (key, val) in enumerate(pairs):
            if not int(key) & 1:
                at = off + 8 + 8 * n + 16 * j + 8
                raw[at:at + 8] = ((int(val) >> 32) << 32 | (n - (int(val) >> 32) + 1)).to_bytes(8, "little")
                return bytes(raw)
    raise AssertionError("no multi-occurrence pair")


def test_errors(ffi, world, tmp_path, monkeypatch):
    monkeypatch.delenv("MM355_IDXLOAD_PIECE", raising=False)
    L = ffi.lib()
    good = world["files"]["canon_15_10_0"]
    data = open(good, "rb").read()
    (tmp_path / "trunc.mmi").write_bytes(data[:len(data) // 2])
    (tmp_path / "badrun.mmi").write_bytes(_bad_run(data))
    cases = [(world["fa"], 0, ffi.MM355_EINVAL), (tmp_path / "missing.mmi", 0, ffi.MM355_EIO), (tmp_path / "trunc.mmi", 0, ffi.MM355_EIO),
             (tmp_path / "badrun.mmi", 0, ffi.MM355_EIO), (good, 1 << 20, ffi.MM355_ENODEV)]
    for what, raw in _mmiload.bad_files(data):
        f = tmp_path / ("bad%d.mmi" % len(cases))
        f.write_bytes(raw)
        cases.append((f, 0, ffi.MM355_EIO))
    for path, device, want in cases:
        rc, h = load_dev(ffi, path, device)
        assert rc == want and not h, (str(path), rc)
        rc, h = load_dev(ffi, good)                                               # a good load in the same process still succeeds
        assert rc == 0 and h
        try:
            assert _mmi.dump(ffi, h, tmp_path / "again.mmi") == data
        finally:
            L.mm355_index_free(h)


# ------------------------------------------------------------------ 6. Python
def test_aligner_load_on_gpu(ffi, world, tmp_path, monkeypatch):
    monkeypatch.delenv("MM355_IDXLOAD_PIECE", raising=False)
    import mappy_rs
    reads = world["reads"]
    saved = world["files"]["canon_15_10_0"]
    host = mappy_rs.Aligner(saved, preset="map-ont")
    dev = mappy_rs.Aligner(saved, preset="map-ont", load_on_gpu=True)
    assert host._L.mm355_index_get(host._idx, 0, None, 0) >= 0
    assert dev._L.mm355_index_get(dev._idx, 0, None, 0) == ffi.MM355_EUNSUP
    assert (dev.k, dev.w, dev.n_seq, dev.seq_names) == (host.k, host.w, host.n_seq, host.seq_names)

    def batch(al):
        al.enable_threading(2)
        got = {d["i"]: m for m, d in al.map_batch([{"seq": r, "i": i} for i, r in enumerate(reads)])}
        return [got[i] for i in range(len(reads))]

    def single(al):
        return [list(al.map(r, cs=True)) for r in reads]

    want_single, want_batch = single(host), batch(host)
    assert sum(len(ms) for ms in want_single) > 32 and sum(len(ms) for ms in want_batch) > 32
    assert single(dev) == want_single and batch(dev) == want_batch
    name = world["recs"][0][0]
    assert dev.seq(name, 5, 25) == world["recs"][0][1][5:25] == host.seq(name, 5, 25)
    out = str(tmp_path / "resaved.mmi")
    assert dev.save_index(out) is None
    assert open(out, "rb").read() == open(saved, "rb").read()
    # a FASTA is not an .mmi: the usual routes
    fa_host = mappy_rs.Aligner(world["fa"], preset="map-ont", load_on_gpu=True)
    assert fa_host._L.mm355_index_get(fa_host._idx, 0, None, 0) >= 0
    assert batch(fa_host) == batch(mappy_rs.Aligner(world["fa"], preset="map-ont")) == want_batch
    both = mappy_rs.Aligner(world["fa"], preset="map-ont", build_on_gpu=True, load_on_gpu=True)
    assert both._L.mm355_index_get(both._idx, 0, None, 0) == ffi.MM355_EUNSUP
    both_mmi = mappy_rs.Aligner(saved, preset="map-ont", build_on_gpu=True, load_on_gpu=True)
    assert both_mmi._L.mm355_index_get(both_mmi._idx, 0, None, 0) == ffi.MM355_EUNSUP
    assert batch(both) == want_batch
    with pytest.raises(RuntimeError, match="Did not create or open an index"):
        mappy_rs.Aligner(str(tmp_path / "missing.mmi"), load_on_gpu=True)
    (tmp_path / "trunc.mmi").write_bytes(open(saved, "rb").read()[:5000])
    with pytest.raises(RuntimeError, match="Did not create or open an index"):
        mappy_rs.Aligner(str(tmp_path / "trunc.mmi"), load_on_gpu=True)
