"""The PAF writer on the GPU (mm355_recdev.h with PafFmt: k_rec_len, the scan, k_rec_fields): the device formatter against the host formatter and
mappy_rs.paf_line, byte for byte -- on constructed result sets (tests/_paf_sets.py), end to end through Aligner.map_paf on the two-contig
world of tests/test_gpu_tags.py, and from a reads file to a PAF file through Aligner.map_file.  CPU side: tests/test_paf_host.py."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import synthdata as S
import _capi
import _paf_sets as PS
from test_gpu_tags import world          # noqa: F401  (the fixture: its genome and reads)

OUT_CS, OUT_MD, OUT_TAGS = 1, 2, 4


def _format(al, s, where, mo_cigar, mo_chain):
    """mm355_paf_format on the set -> (text, line_off, on_device)"""
    from mappy_rs import _ffi
    L = al._L
    h, qn, ql, keep = PS.hits_struct(s)
    tp = C.POINTER(_ffi.Text)()
    _ffi.check(L.mm355_paf_format(al._context(), C.byref(mo_cigar if s["has_cigar"] else mo_chain), C.byref(h), qn, ql, where, C.byref(tp)))
    try:
        t = tp.contents
        assert t.n_reads == len(s["qlens"]) and t.n_lines == len(s["hits"]) and t.ms_format >= 0.0
        return bytes(_ffi.text_view(tp)), [t.line_off[i] for i in range(t.n_reads + 1)], t.on_device
    finally:
        L.mm355_free_text(tp)


@pytest.fixture(scope="module")
def stage(built, tmp_path_factory):
    """an Aligner whose index has the contig names of the constructed sets (names of 1 and 255 bytes), and the two option records"""
    import mappy_rs
    from mappy_rs import _ffi
    fa = str(tmp_path_factory.mktemp("gpaf") / "three.fa")
    S.write_fasta(fa, S.make_genome(5, [3000, 3000, 3000]), PS.CONTIGS)
    al = mappy_rs.Aligner(fa, preset="map-ont")
    assert al.seq_names == PS.CONTIGS
    mo_chain = _ffi.MapOpt.from_buffer_copy(al._mo)
    mo_chain.flag &= ~4
    return al, al._mo, mo_chain


def test_device_formatter_equals_host_and_python(stage, monkeypatch):
    from mappy_rs import _ffi
    al, mo_c, mo_n = stage
    sets = PS.random_sets(355, 300)
    rng = np.random.default_rng(9)
    sets.append(PS.random_set(rng, n_cigar_ops=100000, max_reads=2))           # one hit of 100 000 operations
    sets.append(PS.make_set([], [], True, [0, 0, 0], [0, PS.EEMPTY], [100, 0], ["a", None], PS.CONTIGS))      # a batch with zero hits
    n_lines = 0
    for k, s in enumerate(sets):
        want, want_off = PS.expected(s)
        host, host_off, on = _format(al, s, _ffi.PAF_HOST, mo_c, mo_n)
        assert on == 0 and host == want and host_off == want_off, k
        dev, dev_off, on = _format(al, s, _ffi.PAF_DEVICE, mo_c, mo_n)
        assert on == 1, k
        assert dev == want, (k, dev[:200], want[:200])
        assert dev_off == want_off, k
        n_lines += len(s["hits"])
    assert n_lines > 600 and int(sets[-2]["hits"][0]["n_cigar"]) == 100000
    # MM355_PAF_AUTO: the hit count against MM355_PAF_MIN_HITS
    s = sets[0]
    monkeypatch.setenv("MM355_PAF_MIN_HITS", "1")
    assert _format(al, s, _ffi.PAF_AUTO, mo_c, mo_n)[2] == (1 if len(s["hits"]) else 0)
    monkeypatch.setenv("MM355_PAF_MIN_HITS", "1000000")
    assert _format(al, s, _ffi.PAF_AUTO, mo_c, mo_n)[2] == 0


def test_format_refuses_what_it_cannot_read(stage):
    """no tags array, a row that points past its arena, a contig that does not exist, a de with divisor zero: MM355_EINVAL from both formatters, nothing launched"""
    from mappy_rs import _ffi
    al, mo_c, mo_n = stage
    s = next(s for s in PS.random_sets(3, 40) if s["has_cigar"] and len(s["cigar"]) > 2)
    for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
        for broken in ("tags", "cigar", "rid", "de"):
            h, qn, ql, keep = PS.hits_struct(s)
            if broken == "tags":
                h.tags = None
            elif broken == "cigar":
                h.n_cigar -= 1
            elif broken == "rid":
                h.hits[0].rid = len(PS.CONTIGS)
            else:                                   # 1 - mlen / 0: paf_line raises ZeroDivisionError there
                h.hits[0].block_len = 7
                h.tags[0].n_ambi, h.tags[0].n_gap, h.tags[0].n_gapo = 1, 9, 1
            tp = C.POINTER(_ffi.Text)()
            assert al._L.mm355_paf_format(al._context(), C.byref(mo_c), C.byref(h), qn, ql, where, C.byref(tp)) == _ffi.MM355_EINVAL and not tp


def _expected_paf(al, reads, names, flags):
    import mappy_rs
    recs = al._map_many(reads, flags | OUT_TAGS, names=names)
    out = []
    for i, ms in enumerate(recs):
        if isinstance(ms, list):
            out += [mappy_rs.paf_line(m, PS.printed_name(names[i] if names else None), len(reads[i])) + "\n" for m in ms]
    return "".join(out).encode()


def _both_ways(al, reads, names, want, **kw):
    from mappy_rs import _ffi
    for where, on in ((_ffi.PAF_HOST, False), (_ffi.PAF_DEVICE, True)):
        got = al.map_paf(reads, names=names, where=where, **kw)
        assert al.paf_on_device is on
        assert got == want, (where, got[:300], want[:300])


def _cigar_reads(world):
    reads = world["cigar_reads"][True] + world["reads"][:80] + [""]              # inversions, Ns, ordinary reads, one empty sequence
    names = [None if i % 7 == 3 else "read%d comment %d" % (i, i) if i % 5 == 0 else "read%d" % i for i in range(len(reads))]
    return reads, names


@pytest.mark.parametrize("preset,kw,flags", [("map-ont", dict(cs=True), OUT_CS), ("map-ont", dict(MD=True), OUT_MD), ("map-hifi", {}, 0)],
                         ids=["map-ont-cs", "map-ont-MD", "map-hifi"])
def test_map_paf_cigar_mode(world, preset, kw, flags):
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset=preset)          # tagged whatever tags= was
    reads, names = _cigar_reads(world)
    if preset == "map-hifi":
        reads = world["cigar_reads"][False] + world["reads"][:40]
        names = names[:len(reads)]
    want = _expected_paf(al, reads, names, flags)
    assert want.count(b"\n") > len(reads) // 2 and (b"\tcs:Z:" in want) == bool(flags & OUT_CS) and (b"\tMD:Z:" in want) == bool(flags & OUT_MD)
    assert b"\ttp:A:I\t" in want or preset != "map-ont"
    _both_ways(al, reads, names, want, **kw)
    _both_ways(al, reads, None, _expected_paf(al, reads, None, flags), **kw)      # every read unnamed: "*"


def test_map_paf_ava_chain_only_on_its_own_reads(world, tmp_path):
    import mappy_rs
    reads = world["reads"][:150]
    names = ["r%03d" % i for i in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    with open(fa, "w") as f:
        f.write("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    al = mappy_rs.Aligner(fa, preset="ava-ont", cigar=False, tags=True)
    want = _expected_paf(al, reads, names, 0)
    assert want.count(b"\n") > 20 and b"\tdv:f:" in want and b"cg:Z:" not in want
    _both_ways(al, reads, names, want)
    with pytest.raises(ValueError):
        al.map_paf(reads[:2], cs=True)
    with pytest.raises(TypeError):
        al.map_paf([b"ACGT"])
    with pytest.raises(ValueError):
        al.map_paf(reads[:2], names=["one"])


def _write_fastq_gz(path, reads, names):
    with gzip.open(path, "wt") as f:
        for n, r in zip(names, reads):
            f.write("@%s ch=%d start_time=x\n%s\n+\n%s\n" % (n, len(r) % 512, r, "@" + "I" * (len(r) - 1)))


def test_map_file(world, tmp_path):
    """reads file in, PAF file out, in input order across three workers and sub-batches of 64 reads"""
    import mappy_rs
    reads = world["cigar_reads"][True][:40] + world["reads"][:110]
    names = ["r%03d" % i for i in range(len(reads))]
    fq = str(tmp_path / "reads.fq.gz")
    _write_fastq_gz(fq, reads, names)
    out = str(tmp_path / "out.paf")
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", tags=True, devices=[0])
    want = "".join(mappy_rs.paf_line(m, n, len(r)) + "\n" for n, r in zip(names, reads) for m in al.map(r, cs=True, name=n)).encode()
    al.enable_threading(3)
    from mappy_rs import _ffi
    open(out, "wb").write(b"what was here before\n")
    res = al.map_file(fq, out, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE)     # three workers, each formatting in its own context's buffers
    got = open(out, "rb").read()
    assert got == want, (len(got), len(want))
    assert res["n_on_device"] == res["n_sub_batches"] == 3 and not os.path.exists(out + ".part")
    res = al.map_file(fq, out, cs=True, sub_batch_reads=64, where=_ffi.PAF_HOST)
    assert open(out, "rb").read() == want and res["n_on_device"] == 0
    al.map_file(fq, out, cs=True, sub_batch_reads=64)                        # AUTO: whichever formatter the hit counts select
    assert open(out, "rb").read() == want
    assert (res["n_reads"], res["n_bases"], res["n_lines"], res["n_sub_batches"]) == (len(reads), sum(map(len, reads)), want.count(b"\n"), 3)
    assert res["seconds"] > 0 and res["n_lines"] > 100
    # chain-only: as many lines as hits
    al2 = mappy_rs.Aligner(world["fa"], preset="map-ont", cigar=False, devices=[0])
    n_hits = sum(len(ms) for ms in al2._map_many(reads, 0, names=names))
    out2 = str(tmp_path / "out2.paf")
    res2 = al2.map_file(fq, out2, n_threads=2, sub_batch_reads=64, where=_ffi.PAF_DEVICE)
    assert res2["n_lines"] == n_hits == open(out2, "rb").read().count(b"\n") and res2["n_reads"] == len(reads)
    with pytest.raises(ValueError):
        al2.map_file(fq, out2, cs=True)
    # failures leave no file: a path that cannot be written, a reads file that is cut in the middle
    bad = str(tmp_path / "no_such_dir" / "out.paf")
    with pytest.raises(OSError):
        al.map_file(fq, bad, cs=True)
    assert not os.path.exists(bad)
    cut = str(tmp_path / "cut.fq.gz")
    blob = open(fq, "rb").read()
    open(cut, "wb").write(blob[:len(blob) // 2])
    out3 = str(tmp_path / "out3.paf")
    with pytest.raises(RuntimeError):
        al.map_file(cut, out3, cs=True, sub_batch_reads=16)
    assert not os.path.exists(out3) and not os.path.exists(out3 + ".part")
    # ... and leave a file that was there alone, also when the reads file does not exist
    for reads_path in (cut, str(tmp_path / "missing.fq")):
        with pytest.raises(RuntimeError):
            al.map_file(reads_path, out, cs=True, sub_batch_reads=16)
        assert open(out, "rb").read() == want and not os.path.exists(out + ".part")


def test_a_paf_request_changes_nothing_else(world):
    """mm355_map_batch_named's raw hits, CIGAR words and string bytes are the same before and after a mm355_map_batch_paf call on the context"""
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont")
    reads, names = _cigar_reads(world)
    reads, names = reads[:60], names[:60]

    def raw():
        v = _capi.map_raw(al, reads, OUT_CS | OUT_TAGS, names, entry="named")
        return _capi.raw(v.hits), _capi.raw(v.tags), v.cigar.tobytes(), v.str, v.off.tobytes(), v.status.tobytes()
    before = raw()
    from mappy_rs import _ffi
    for where in (_ffi.PAF_DEVICE, _ffi.PAF_HOST):
        assert al.map_paf(reads, names=names, cs=True, where=where).count(b"\n") == len(before[0]) // _ffi._HIT_DTYPE.itemsize
        assert raw() == before
