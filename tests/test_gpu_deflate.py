"""The deflate stage of the BAM writer on the GPU (mm355_bam.hip: k_bgzf_deflate, the scan of the block sizes, k_bgzf_compact): the kernel
against the serial coder of mm355_deflate.h byte for byte on the payloads of tests/_deflate.py; deflated and stored blocks mixed in one
call; Aligner.map_bam / bam_header / map_bam_file with compress=True against the uncompressed calls through gzip; compress=False against
the calls without the keyword; the levels the entry points refuse.  CPU side: tests/test_deflate_host.py."""
import ctypes as C
import gzip
import os

import pytest

pytestmark = pytest.mark.gpu

import _bam
import _bam_sets as BS
import _deflate as D
import _sam_sets as SS
from test_gpu_tags import world, _rc          # noqa: F401  (the fixture: its genome and reads)
from test_gpu_bam import stage                # noqa: F401  (the fixture: an Aligner with the constructed sets' contigs)
from test_gpu_sam import _sam_reads, _write_fastq_gz

P = D.P


def _deflate(al, data, where, level=1, raw=False):
    """mm355_bgzf_deflate -> (blocks, on_device), or the return code alone"""
    from mappy_rs import _ffi
    tp = C.POINTER(_ffi.Text)()
    rc = al._L.mm355_bgzf_deflate(al._context(), data, len(data), where, level, C.byref(tp))
    if raw:
        assert not tp
        return rc
    _ffi.check(rc)
    try:
        t = tp.contents
        assert t.n_lines == (len(data) + P - 1) // P and t.n_reads == 0
        return bytes(_ffi.text_view(tp)), t.on_device
    finally:
        al._L.mm355_free_text(tp)


@pytest.fixture(scope="module")
def host_coded(stage):
    from mappy_rs import _ffi
    out = {}
    for name, data in D.payloads().items():
        got, on = _deflate(stage, data, _ffi.PAF_HOST)
        assert on == 0
        out[name] = got
    return out


def test_device_deflate_equals_host(stage, host_coded):
    from mappy_rs import _ffi
    pl = D.payloads()
    n_deflated = 0
    for name, data in pl.items():
        got, on = _deflate(stage, data, _ffi.PAF_DEVICE)
        want = host_coded[name]
        assert on == 1 and got == want, (name, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1))
        n_deflated += sum(not s for s in D.check(got, data))
    assert n_deflated >= 20
    assert len(host_coded["repeat_1000"]) < P // 4 and host_coded["random_%d" % P] == _bam.frame(pl["random_%d" % P])
    # AUTO is the host for the bare wrap; level 0 is the framing kernel's and the host's stored blocks
    data = pl["text_%d" % (P + 1)]
    assert _deflate(stage, data, _ffi.PAF_AUTO) == (host_coded["text_%d" % (P + 1)], 0)
    for where, on in ((_ffi.PAF_HOST, 0), (_ffi.PAF_DEVICE, 1)):
        assert _deflate(stage, data, where, level=0) == (_bam.frame(data), on)
    # a small call after a large one, and the large one again: nothing is taken from what a call left behind
    for name in ("text_259", "records", "zeros_1", "records"):
        assert _deflate(stage, pl[name], _ffi.PAF_DEVICE)[0] == host_coded[name], name


def test_deflated_and_stored_blocks_mix(stage):
    from mappy_rs import _ffi
    import mappy_rs
    data = D.mixed_blocks()
    got, on = _deflate(stage, data, _ffi.PAF_DEVICE)
    assert on == 1 and got == _deflate(stage, data, _ffi.PAF_HOST)[0] == mappy_rs.bgzf_wrap(data, compress=True)
    assert D.check(got, data) == [False, True, False, True, False, True]
    sizes = [len(b) for b in D.blocks(got)]
    assert any(sum(sizes[:k]) % 16 for k in range(1, 6))


def test_levels_that_do_not_exist_are_refused(stage):
    from mappy_rs import _ffi
    al, L = stage, stage._L
    s = BS.boundary_set()
    h, qn, sp, ql, qp, rl, keep = SS.sam_args(s)
    reads = ["ACGTACGTAC" * 30]
    packed = _ffi.pack_reads(reads)
    for level in (2, -1):
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            assert _deflate(al, b"abc", where, level=level, raw=True) == _ffi.MM355_EINVAL
            tp = C.POINTER(_ffi.Text)()
            assert L.mm355_bam_format_deflate(al._context(), C.byref(al._mo), C.byref(h), qn, sp, ql, qp, rl, s["sam_flags"], where, level, C.byref(tp)) == _ffi.MM355_EINVAL
            assert not tp
            assert L.mm355_map_batch_bam_deflate(al._context(), C.byref(al._mo), 1, packed.arr, packed.lens, None, None, 0, 0, where, level, C.byref(tp)) == _ffi.MM355_EINVAL
            assert not tp


def test_format_deflate_on_constructed_sets(stage, monkeypatch):
    """mm355_bam_format_deflate on result sets: level 1 inflates to level 0's records under HOST and DEVICE, the two give the same bytes,
    level 0 is mm355_bam_format's bytes, AUTO follows MM355_BAM_MIN_HITS, line_off is the unframed stream's"""
    from mappy_rs import _ffi
    al, L = stage, stage._L

    def fmt(s, where, level):
        h, qn, sp, ql, qp, rl, keep = SS.sam_args(s)
        tp = C.POINTER(_ffi.Text)()
        _ffi.check(L.mm355_bam_format_deflate(al._context(), C.byref(al._mo), C.byref(h), qn, sp, ql, qp, rl, s["sam_flags"], where, level, C.byref(tp)))
        try:
            t = tp.contents
            return bytes(_ffi.text_view(tp)), [t.line_off[i] for i in range(t.n_reads + 1)], t.on_device, t.n_lines
        finally:
            L.mm355_free_text(tp)

    sets = BS.random_sets(99, 40) + [BS.boundary_set(), SS.make_set([], [], [0, 0, 0], [0, SS.EEMPTY], ["a", None], ["ACGT", ""], [None, None], [3, 0], SS.HIT_ONLY)]
    for k, s in enumerate(sets):
        want, want_off = BS.expected(s)
        stream = b"".join(want)
        host, off, on, nl = fmt(s, _ffi.PAF_HOST, 1)
        assert on == 0 and off == want_off and nl == len(want), k
        D.check(host, stream)
        dev, off, on, nl = fmt(s, _ffi.PAF_DEVICE, 1)
        assert on == 1 and dev == host and off == want_off and nl == len(want), k
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            assert fmt(s, where, 0)[0] == _bam.frame(stream), k
    twelve = BS.boundary_set()
    for env, on in (("1", 1), ("13", 0), ("12", 1)):
        monkeypatch.setenv("MM355_BAM_MIN_HITS", env)
        assert fmt(twelve, _ffi.PAF_AUTO, 1)[2] == on


def test_map_bam_compress(world, monkeypatch):
    import mappy_rs
    from mappy_rs import _ffi
    al = mappy_rs.Aligner(world["fa"], preset="map-ont")
    reads, names, quals = _sam_reads(world)
    plain = al.map_bam(reads, names=names, quals=quals, cs=True, where=_ffi.PAF_HOST)
    records = _bam.inflate(plain)
    got = {}
    for where, on in ((_ffi.PAF_HOST, False), (_ffi.PAF_DEVICE, True)):
        got[where] = al.map_bam(reads, names=names, quals=quals, cs=True, where=where, compress=True)
        assert al.paf_on_device is on
        D.check(got[where], records)
        assert len(got[where]) < len(plain)
        # compress=False is the call without the keyword
        assert al.map_bam(reads, names=names, quals=quals, cs=True, where=where, compress=False) == plain
    assert got[_ffi.PAF_HOST] == got[_ffi.PAF_DEVICE]
    for env, on in (("1", True), ("1000000", False)):
        monkeypatch.setenv("MM355_BAM_MIN_HITS", env)
        assert al.map_bam(reads, names=names, quals=quals, cs=True, compress=True) == got[_ffi.PAF_HOST] and al.paf_on_device is on
    monkeypatch.delenv("MM355_BAM_MIN_HITS")
    # two calls, one behind the other, are a valid stream
    a = al.map_bam(reads[:7], names=names[:7], quals=quals[:7], cs=True, where=_ffi.PAF_DEVICE, compress=True)
    b = al.map_bam(reads[7:], names=names[7:], quals=quals[7:], cs=True, where=_ffi.PAF_DEVICE, compress=True)
    assert gzip.decompress(a + b) == records and _bam.cut(gzip.decompress(a + b)) == _bam.cut(records)
    assert al.bam_header(compress=False) == al.bam_header() and gzip.decompress(al.bam_header(compress=True)) == _bam.inflate(al.bam_header())
    assert len(al.bam_header(compress=True)) < len(al.bam_header())


def test_map_bam_file_compress(world, tmp_path):
    import mappy_rs
    from mappy_rs import _ffi
    reads, _, _ = _sam_reads(world, n_plain=120)
    reads = reads[:-1]                                                   # (a FASTQ record has bases)
    names = ["r%03d" % i for i in range(len(reads))]
    quals = ["@" + "".join(chr(35 + (i + j) % 50) for j in range(len(r) - 1)) for i, r in enumerate(reads)]
    fq = str(tmp_path / "reads.fq.gz")
    _write_fastq_gz(fq, reads, names, quals)
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", tags=True, devices=[0])
    al.enable_threading(3)
    plain, packed = str(tmp_path / "plain.bam"), str(tmp_path / "packed.bam")
    res0 = al.map_bam_file(fq, plain, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE)
    assert "n_bytes_out" not in res0
    want = open(plain, "rb").read()
    assert al.map_bam_file(fq, plain, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE, compress=False)["n_lines"] == res0["n_lines"]
    assert open(plain, "rb").read() == want
    for where, n_dev in ((_ffi.PAF_DEVICE, 3), (_ffi.PAF_HOST, 0)):
        res = al.map_bam_file(fq, packed, cs=True, sub_batch_reads=64, where=where, compress=True)
        got = open(packed, "rb").read()
        assert gzip.decompress(got) == gzip.decompress(want)
        assert len(got) < len(want) and got[-28:] == _bam.EOF and not os.path.exists(packed + ".part")
        assert res["n_bytes_out"] == len(got) == os.path.getsize(packed)
        assert (res["n_reads"], res["n_lines"], res["n_sub_batches"], res["n_on_device"]) == (len(reads), res0["n_lines"], 3, n_dev)
        # header, three sub-batches each a whole number of blocks, the EOF block
        assert got.startswith(al.bam_header(compress=True)) and len(D.blocks(got)) >= 5
