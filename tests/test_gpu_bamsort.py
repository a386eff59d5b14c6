"""Coordinate-sorted BAM on the GPU (mm355_bam.hip: k_rec_key, rocPRIM's radix sort, k_rec_permute; mm355_map_batch_bam_run;
Aligner.map_bam(sort=True) and map_bam_file(sort=True)).  The rule everything is tested against: the sorted output is the STABLE sort, by the
key of include/mm355.h, of what the same call writes without `sort` -- for any sub-batch size, reader or formatter.
The stage by itself: the device against the host against the model of tests/_bamsort.py, byte for byte, on streams built with struct.
CPU side: tests/test_bamsort_host.py."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _bam
import _bamaux as A
import _bamsort as BS
import _inflate as I
from test_gpu_tags import world, _rc          # noqa: F401  (the fixture: its genome and reads)
from test_gpu_sam import _sam_reads
from test_gpu_bamaux import _tagged_bam, _file_records
from test_bamsort_host import _stage, _refused_streams

EINVAL = -2


@pytest.fixture(scope="module")
def al(world):
    import mappy_rs
    return mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])


# ---------------------------------------------------------------- the stage: device == host == model
def _streams():
    """(label, records): the key patterns crossed with the record counts; the 257-record streams carry the five large sizes; one stream of
    nothing but large records, descending, so that every one of them moves to another residue"""
    rng = np.random.default_rng(61)
    out = []
    for n in (0, 1, 2, 257, 5000):
        for name, fields in BS.patterns(n, rng).items():
            out.append(("%s-%d" % (name, n), BS.records_for(fields, rng, big=n == 257)))
    large = [BS.record(1, 100 - k, 16 * (k & 1), b"q" * (k % 17 + 1), size, rng) for k, size in enumerate(BS.BIG + BS.BIG[::-1])]
    out.append(("large", large))
    out.append(("one-large", [BS.record(0, 5, 0, b"x", 70000, rng)]))
    # names of 1 .. 17 bytes and nothing else: 37-byte records up, back to back
    out.append(("residues", [BS.record(k % 2, 40 - k, 0, b"n" * (k % 17 + 1), None, rng) for k in range(40)]))
    return out


def test_stage_device_equals_host_equals_model(al):
    from mappy_rs import _ffi
    L, ctx = al._L, al._context()
    n_moved, streams = 0, _streams()
    for label, recs in streams:
        data, off = BS.stream(recs)
        srt, keys = BS.model(recs)
        want = (b"".join(srt), keys, list(BS.stream(srt)[1]))
        host = _stage(L, ctx, data, off, len(recs), _ffi.PAF_HOST)
        assert host[:3] == want and host[3] == 0, label
        dev = _stage(L, ctx, data, off, len(recs), _ffi.PAF_DEVICE)
        assert dev[3] == (1 if recs else 0), label
        assert dev[1] == want[1] and dev[2] == want[2], label
        if dev[0] != want[0]:
            bad = next(i for i, (a, b) in enumerate(zip(dev[0], want[0])) if a != b)
            raise AssertionError((label, "first different byte", bad, "of", len(want[0]), dev[0][bad - 8:bad + 24].hex(), want[0][bad - 8:bad + 24].hex()))
        if label.startswith("equal"):
            assert dev[0] == data
        n_moved += sum(a != b for a, b in zip(srt, recs))
    assert n_moved > 10000
    sizes = {len(r) for _, recs in streams[-3:] for r in recs}
    assert set(BS.BIG) <= sizes and 38 in sizes


def test_refused_stream_then_a_valid_one(al):
    from mappy_rs import _ffi
    L, ctx = al._L, al._context()
    cases, (data, off, n, nb) = _refused_streams()
    want = b"".join(BS.model(_bam.cut(data))[0])
    for where in (_ffi.PAF_DEVICE, _ffi.PAF_HOST):
        for name, (d, o, k, b) in cases.items():
            assert _stage(L, ctx, d, o, k, where, n_bytes=b) == EINVAL, (where, name)
            assert _stage(L, ctx, data, off, n, where)[0] == want, (where, name)
    assert _stage(L, ctx, data, off, n, 3) == EINVAL and _stage(L, ctx, data, off, n, _ffi.PAF_DEVICE)[0] == want


# ---------------------------------------------------------------- the run call
def _run_call(al, reads, names, quals, aux, where, **kw):
    """mm355_map_batch_bam_run -> (rec, keys, offsets, on_device)"""
    import mappy_rs
    from mappy_rs import _ffi
    L = al._L
    packed, narr = _ffi.pack_reads(reads), _ffi.pack_names(names)
    qkeep = [None if q is None else q.encode() for q in quals]
    qarr = (C.c_char_p * len(qkeep))(*qkeep)
    ptrs = lens = mods = None
    if aux is not None:
        n = len(aux)
        keep, lens, mods = [None] * n, (C.c_int32 * n)(), (C.c_int32 * n)()
        for i, a in enumerate(aux):
            if a is not None:
                keep[i], mods[i] = mappy_rs.bam_aux_split(a)
                lens[i] = len(keep[i])
        ptrs = (C.c_void_p * n)(*[None if k is None else C.cast(C.c_char_p(k), C.c_void_p).value for k in keep])
    rp = C.POINTER(_ffi.Run)()
    sam_flags = (_ffi.SAM_SOFTCLIP if kw.get("softclip") else 0) | (_ffi.SAM_HIT_ONLY if kw.get("hit_only") else 0)
    _ffi.check(L.mm355_map_batch_bam_run(al._context(), C.byref(al._mo), len(reads), packed.arr, packed.lens, narr, qarr, ptrs, lens, mods, _ffi.OUT_CS, sam_flags,
                                         where, C.byref(rp)))
    try:
        r = rp.contents
        n = int(r.n_rec)
        return C.string_at(r.rec, r.n_bytes), [int(r.key[i]) for i in range(n)], [int(r.rec_off[i]) for i in range(n + 1)], int(r.on_device)
    finally:
        L.mm355_free_run(rp)


def test_run_call_is_the_stable_sort_of_the_unsorted_call(al, world):
    from mappy_rs import _ffi
    rng = np.random.default_rng(67)
    reads, names, quals = _sam_reads(world, n_plain=40)          # both strands, two contigs, supplementaries, reads without hits, an empty read
    auxes = [None if i % 4 == 3 or not r else A.mod_pair(len(r), rng) + A.tag("RG", "Z", b"g") for i, r in enumerate(reads)]
    for aux in (None, auxes):
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            for kw in ({}, {"softclip": True, "hit_only": True}):
                plain = _bam.cut(_bam.inflate(al.map_bam(reads, names=names, quals=quals, cs=True, where=where, aux=aux, **kw)))
                srt, keys = BS.model(plain)
                rec, got_keys, off, on = _run_call(al, reads, names, quals, aux, where, **kw)
                assert on == (where == _ffi.PAF_DEVICE)
                assert _bam.cut(rec) == srt and got_keys == keys == sorted(keys) and off == list(BS.stream(srt)[1]), (aux is not None, where, kw)
                flags = {struct.unpack_from("<H", r, 18)[0] & 0x914 for r in plain}
                assert srt != plain and {0, 0x10} <= flags and len({k >> 32 for k in keys}) >= 2 and (kw or 4 in flags)
                # the surface: one call's blocks, stored and deflated
                assert _bam.inflate(al.map_bam(reads, names=names, quals=quals, cs=True, where=where, aux=aux, sort=True, **kw)) == rec
                assert al.paf_on_device == (where == _ffi.PAF_DEVICE)
        assert gzip.decompress(al.map_bam(reads, names=names, quals=quals, cs=True, aux=aux, sort=True, compress=True)) == b"".join(BS.model(
            _bam.cut(_bam.inflate(al.map_bam(reads, names=names, quals=quals, cs=True, aux=aux))))[0])
    assert _run_call(al, [], [], [], None, _ffi.PAF_DEVICE)[:3] == (b"", [], [0]) and al.map_bam([], sort=True) == b""


# ---------------------------------------------------------------- the file
def _fastq(path, reads, names, quals):
    with gzip.open(path, "wt") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % t for t in zip(names, reads, quals)))


def _blocks_hold(blob):
    """every BGZF block of the file inflates to ISIZE bytes with the CRC-32 of its trailer; returns the payloads back to back"""
    import zlib
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        p = zlib.decompress(blob[at + 18:at + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", blob, at + bsize - 8)
        assert zlib.crc32(p) == crc and len(p) == isize <= 0x10000
        out.append(p)
        at += bsize
    assert at == len(blob)
    return b"".join(out)


@pytest.fixture(scope="module")
def file_world(world, tmp_path_factory):
    td = tmp_path_factory.mktemp("gbamsort")
    reads, _, _ = _sam_reads(world, n_plain=180)
    reads = reads[:-1]                                                   # (a FASTQ record has bases)
    names = ["r%03d" % i for i in range(len(reads))]
    quals = ["".join(chr(35 + (i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
    fq = str(td / "reads.fq.gz")
    _fastq(fq, reads, names, quals)
    return dict(td=td, fq=fq, reads=reads, names=names, quals=quals)


def test_map_bam_file_sorted(world, file_world, monkeypatch):
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(3)
    td, fq = file_world["td"], file_world["fq"]
    assert len(file_world["reads"]) >= 190
    out, spool = str(td / "out.bam"), td / "spool"
    spool.mkdir()
    res0 = al.map_bam_file(fq, out, cs=True, sub_batch_reads=64)
    unsorted = open(out, "rb").read()
    al.map_bam_file(fq, out, cs=True, sub_batch_reads=64, sort=False)
    assert open(out, "rb").read() == unsorted and "n_runs" not in res0
    head_u, plain = _file_records(out)
    want, keys = BS.model(plain)
    assert want != plain and len({k >> 32 for k in keys}) == 3 and len(keys) - len(set(keys)) > 0
    files = {}
    for sub, chunk, compress in ((7, 100_000, False), (64, mappy_rs.SORT_CHUNK_BYTES, False), (7, 100_000, True), (64, 1 << 20, True)):
        monkeypatch.setattr(mappy_rs, "SORT_CHUNK_BYTES", chunk)
        res = al.map_bam_file(fq, out, cs=True, sub_batch_reads=sub, sort=True, compress=compress, tmp_dir=str(spool))
        blob = open(out, "rb").read()
        head, got = _file_records(out)
        assert got == want, (sub, compress, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b))
        assert head.startswith(b"@HD\tVN:1.6\tSO:coordinate\n") and head.split(b"\n", 1)[1] == head_u.split(b"\n", 1)[1]
        assert blob[-28:] == _bam.EOF and os.listdir(str(spool)) == [] and not os.path.exists(out + ".part")
        assert res["n_runs"] == res["n_sub_batches"] == -(-len(file_world["reads"]) // sub) and res["n_tmp_bytes"] == sum(map(len, want))
        assert res["n_lines"] == len(want) and res["n_reads"] == res0["n_reads"] and res["seconds_merge"] > 0
        assert res.keys() - res0.keys() == ({"n_runs", "seconds_merge", "n_tmp_bytes"} | ({"n_bytes_out"} if compress else set()))
        payload = _blocks_hold(blob)
        assert payload == gzip.decompress(blob)
        if compress:
            assert res["n_bytes_out"] == len(blob) < len(unsorted)
        else:                                                          # the header by itself, then the whole sorted stream cut every 0xff00 bytes
            assert blob == al.bam_header(sort=True) + _bam.frame(b"".join(want)) + _bam.EOF
        assert files.setdefault(compress, blob) == blob, (sub, compress)      # the same bytes for either sub-batch and step size
    # the default tmp_dir is out_path's directory, and nothing stays there either
    before = sorted(os.listdir(str(td)))
    al.map_bam_file(fq, out, cs=True, sub_batch_reads=64, sort=True, softclip=True, hit_only=True)
    assert sorted(os.listdir(str(td))) == before
    al.map_bam_file(fq, str(td / "u.bam"), cs=True, sub_batch_reads=64, softclip=True, hit_only=True)
    assert _file_records(out)[1] == BS.model(_file_records(str(td / "u.bam"))[1])[0]


def test_map_bam_file_sorted_with_copied_tags(world, tmp_path):
    import mappy_rs
    rng = np.random.default_rng(71)
    all_reads, _, _ = _sam_reads(world, n_plain=90)
    reads = [r.replace("N", "A") for r in all_reads[-7:-1] + all_reads[70:100]]
    names = ["r%03d" % i for i in range(len(reads))]
    quals = ["".join(chr(35 + (i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
    blob, _ = _tagged_bam(reads, names, quals, rng)
    bam, out = str(tmp_path / "calls.bam"), str(tmp_path / "out.bam")
    open(bam, "wb").write(I.bgzf_file(blob, 0xff00))
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(2)
    res0 = al.map_bam_file(bam, out, cs=True, sub_batch_reads=9, copy_tags=True)
    head_u, plain = _file_records(out)
    want = BS.model(plain)[0]
    assert any(b"MMZ" in r for r in plain) and want != plain
    for kw in (dict(), dict(read_on_gpu=True), dict(read_on_gpu=True, compress=True, sub_batch_reads=5)):
        res = al.map_bam_file(bam, out, cs=True, copy_tags=True, sort=True, **{"sub_batch_reads": 9, **kw})
        head, got = _file_records(out)
        assert got == want, kw
        assert head == head_u.replace(b"SO:unsorted\tGO:query", b"SO:coordinate") and head.count(b"@RG") == 1
        assert res["n_aux_bytes"] == res0["n_aux_bytes"] and res.get("reader_on_device", False) == bool(kw.get("read_on_gpu"))
        _blocks_hold(open(out, "rb").read())


def test_map_bam_file_sorted_failure_leaves_the_old_file(world, file_world, tmp_path):
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(2)
    blob = open(file_world["fq"], "rb").read()
    cut = str(tmp_path / "cut.fq.gz")
    open(cut, "wb").write(blob[:len(blob) // 2])
    out, out2 = str(tmp_path / "out.bam"), str(tmp_path / "out2.bam")
    open(out, "wb").write(b"what was here before\n")
    for target in (out2, out):
        with pytest.raises(RuntimeError):
            al.map_bam_file(cut, target, cs=True, sub_batch_reads=16, sort=True)
        assert not os.path.exists(target + ".part")
    assert not os.path.exists(out2) and open(out, "rb").read() == b"what was here before\n" and sorted(os.listdir(str(tmp_path))) == ["cut.fq.gz", "out.bam"]
    with pytest.raises(OSError):                                         # a spool directory that does not exist: nothing has run, nothing is left
        al.map_bam_file(file_world["fq"], out2, sort=True, tmp_dir=str(tmp_path / "nowhere"))
    assert not os.path.exists(out2) and not os.path.exists(out2 + ".part")
    with pytest.raises(TypeError):
        al.map_file(file_world["fq"], out2, sort=True)                   # SAM and PAF have no `sort`
