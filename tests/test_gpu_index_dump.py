"""mm355_index_dump of a device-resident index (mm355_idxdump.hip) and mm355_index_load_device: the file a device-built index writes is,
byte for byte, the file the host-built index of the same sequences writes; it loads and maps like the index it came from; the FASTA /
FASTQ / gzip / .mmi paths of mm355_index_load_device; Aligner(build_on_gpu=True) and save_index."""
import ctypes as C
import os
import random

import pytest

import _mmi
from _capi import raw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ffi(built):
    from mappy_rs import _ffi
    _ffi.lib()
    return _ffi


@pytest.fixture(scope="module")
def world(ffi, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpuidxdump")
    recs = _mmi.repeat_rich_records()
    fa, fq, gz = str(d / "rep.fa"), str(d / "rep.fq"), str(d / "rep.fa.gz")
    _mmi.write_fasta(fa, recs); _mmi.write_fastq(fq, recs); _mmi.write_gzip(gz, fa)
    return dict(dir=d, recs=recs, fa=fa, fq=fq, gz=gz, reads=_mmi.make_reads(recs), host_dump={})


def _host_dump(ffi, world, k, w, flag):
    """the host-built index's file of the repeat-rich reference, made once per setting"""
    key = (k, w, flag)
    if key not in world["host_dump"]:
        h = _mmi.build(ffi, world["recs"], _mmi.idxopt(ffi, k, w, flag))
        try:
            world["host_dump"][key] = _mmi.dump(ffi, h, world["dir"] / ("host_%d_%d_%d.mmi" % key))
        finally:
            ffi.lib().mm355_index_free(h)
    return world["host_dump"][key]


def _both(ffi, recs, k, w, flag, d):
    """(device dump, host dump) of the same sequences"""
    L = ffi.lib()
    io = _mmi.idxopt(ffi, k, w, flag)
    hd, hh = _mmi.build(ffi, recs, io, device=0), _mmi.build(ffi, recs, io)
    try:
        dev, host = _mmi.dump(ffi, hd, d / "dev.mmi"), _mmi.dump(ffi, hh, d / "host.mmi")
    finally:
        L.mm355_index_free(hd); L.mm355_index_free(hh)
    return dev, host


def _runs(m):
    return [int(v) & 0xffffffff for _, pairs in m["buckets"] for key, v in pairs if not int(key) & 1]


# ------------------------------------------------------------------ 1. device dump == host dump
@pytest.mark.parametrize("k,w,flag", _mmi.SETTINGS)
def test_repeat_rich(ffi, world, tmp_path, k, w, flag):
    L = ffi.lib()
    hd = _mmi.build(ffi, world["recs"], _mmi.idxopt(ffi, k, w, flag), device=0)
    try:
        dev = _mmi.dump(ffi, hd, tmp_path / "dev.mmi")
    finally:
        L.mm355_index_free(hd)
    assert dev == _host_dump(ffi, world, k, w, flag)
    m = _mmi.parse_mmi(dev)
    _mmi.assert_canonical(m)
    assert max(_runs(m)) >= 100


def test_no_multi_occurrence_key(ffi, golden_dir, tmp_path):
    """tests/golden/test.fa: every minimizer is a singleton, p[] is empty everywhere -- nothing to gather, no empty launch"""
    recs, name = [], None
    for line in open(os.path.join(golden_dir, "test.fa")):
        if line.startswith(">"):
            name = line[1:].split()[0]; recs.append([name, ""])
        else:
            recs[-1][1] += line.strip()
    dev, host = _both(ffi, [tuple(r) for r in recs], 15, 10, 0, tmp_path)
    assert dev == host
    m = _mmi.parse_mmi(dev)
    assert all(len(p) == 0 for p, _ in m["buckets"]) and sum(len(pairs) for _, pairs in m["buckets"]) > 0


def test_single_short_contig(ffi, tmp_path):
    rng = random.Random(3)
    dev, host = _both(ffi, [("one", _mmi._rand(rng, 300))], 15, 10, 0, tmp_path)
    assert dev == host
    dev, host = _both(ffi, [("mono", "A" * 300)], 15, 10, 0, tmp_path)     # one key, one run: a single multi-occurrence entry
    assert dev == host
    m = _mmi.parse_mmi(dev)
    assert sum(len(pairs) for _, pairs in m["buckets"]) == 1 and len(_runs(m)) == 1


def test_long_run_beside_short_runs(ffi, tmp_path):
    """a 50-mer x 5000 tandem repeat (runs above 4096: the block-per-chunk path) beside a segment present three times (thousands of runs of 2-3)"""
    rng = random.Random(5)
    a = _mmi._rand(rng, 15000)
    s = _mmi._rand(rng, 4000) + a + _mmi._rand(rng, 3000) + _mmi._rand(rng, 50) * 5000 + a + _mmi._rand(rng, 2500) + a[:7500] + _mmi._rand(rng, 500)
    dev, host = _both(ffi, [("skew", s)], 15, 10, 0, tmp_path)
    assert dev == host
    runs = _runs(_mmi.parse_mmi(dev))
    assert max(runs) > 4096 and sum(1 for r in runs if r <= 3) > 1000


def test_every_bucket_one_long_run(ffi, tmp_path):
    """1 Mbp at k = 6, w = 3: at most 4096 keys, one per bucket, runs of several hundred positions on average (every wave's 64 keys
    flatten to thousands of steps)"""
    rng = random.Random(6)
    s = "".join(rng.choices("ACGT", k=1000000))
    dev, host = _both(ffi, [("mega", s)], 6, 3, 0, tmp_path)
    assert dev == host
    m = _mmi.parse_mmi(dev)
    runs = _runs(m)
    assert m["b"] == 12 and all(len(pairs) <= 1 for _, pairs in m["buckets"]) and len(runs) > 1000 and max(runs) > 256 and sum(runs) > 200 * len(runs) > 200000


# ------------------------------------------------------------------ 2. the file works
def _map_all(ffi, h, reads):
    """the 64 reads on one index with and without CIGAR -> the raw result arrays"""
    L = ffi.lib()
    out = []
    for cigar in (True, False):
        io, mo = ffi.IdxOpt(), ffi.MapOpt()
        L.mm355_set_opt(None, C.byref(io), C.byref(mo))
        ffi.check(L.mm355_set_opt(b"map-ont", C.byref(io), C.byref(mo)))
        if cigar:
            mo.flag |= 4
        ffi.check(L.mm355_mapopt_update(C.byref(mo), h))
        ctx = C.c_void_p()
        ffi.check(L.mm355_ctx_create(h, 0, C.byref(ctx)))
        try:
            v = ffi.map_raw(L, ctx, mo, reads, ffi.OUT_CS if cigar else 0)
        finally:
            L.mm355_ctx_destroy(ctx)
        out.append((mo.mid_occ, v.off.tobytes(), v.status.tobytes(), raw(v.hits), v.cigar.tobytes(), v.str))
    assert len(out[0][3]) > 32 * C.sizeof(ffi.Hit) and len(out[0][4]) > 0 and len(out[0][5]) > 0 and len(out[1][3]) > 0
    return out


def test_dumped_file_maps_like_the_device_index(ffi, world, tmp_path):
    L = ffi.lib()
    io = _mmi.idxopt(ffi, 15, 10, 0)
    hd = _mmi.build(ffi, world["recs"], io, device=0)
    try:
        before = _map_all(ffi, hd, world["reads"])
        first = _mmi.dump(ffi, hd, tmp_path / "dev.mmi")
        assert _map_all(ffi, hd, world["reads"]) == before               # the index is unchanged by the dump
        assert _mmi.dump(ffi, hd, tmp_path / "dev2.mmi") == first
    finally:
        L.mm355_index_free(hd)
    rc, hl = _mmi.load(ffi, tmp_path / "dev.mmi", io)
    assert rc == 0
    try:
        assert _map_all(ffi, hl, world["reads"]) == before
    finally:
        L.mm355_index_free(hl)


# ------------------------------------------------------------------ 3. mm355_index_load_device
def test_load_device(ffi, world, tmp_path):
    L = ffi.lib()
    io = _mmi.idxopt(ffi, 15, 10, 0)
    want = _host_dump(ffi, world, 15, 10, 0)
    for src in ("fa", "gz", "fq"):
        rc, h = _mmi.load(ffi, world[src], io, device=0)
        assert rc == 0
        try:
            assert L.mm355_index_get(h, 0, None, 0) == ffi.MM355_EUNSUP        # device-resident: built on the GPU, not on the host
            assert _mmi.dump(ffi, h, tmp_path / (src + ".mmi")) == want
        finally:
            L.mm355_index_free(h)
    mmi = tmp_path / "fa.mmi"
    rc, h = _mmi.load(ffi, mmi, io, device=0)
    assert rc == 0
    try:
        assert L.mm355_index_get(h, 0, None, 0) >= 0                           # a host image: nothing was built
        assert _mmi.dump(ffi, h, tmp_path / "from_mmi.mmi") == want
    finally:
        L.mm355_index_free(h)
    rc, h = _mmi.load(ffi, tmp_path / "missing.fa", io, device=0)
    assert rc == ffi.MM355_EIO and not h
    rc, h = _mmi.load(ffi, world["fa"], io, device=1 << 20)
    assert rc == ffi.MM355_ENODEV and not h


# ------------------------------------------------------------------ 4. Python
def test_aligner_build_on_gpu(ffi, world, tmp_path):
    import mappy_rs
    reads = world["reads"]
    host = mappy_rs.Aligner(world["fa"], preset="map-ont")
    dev = mappy_rs.Aligner(world["fa"], preset="map-ont", build_on_gpu=True)
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
    saved = str(tmp_path / "saved.mmi")
    assert dev.save_index(saved) is None
    assert open(saved, "rb").read() == _host_dump(ffi, world, 15, 10, 0)
    assert batch(mappy_rs.Aligner(saved, preset="map-ont")) == want_batch
    assert batch(mappy_rs.Aligner(saved, preset="map-ont", build_on_gpu=True)) == want_batch      # an .mmi loads as before
    name = world["recs"][0][0]
    assert dev.seq(name, 5, 25) == world["recs"][0][1][5:25] == host.seq(name, 5, 25)
