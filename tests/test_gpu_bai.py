"""The .bai index on the GPU (mm355_bam.hip: k_rec_span behind the sort's permutation; mm355_bam_sort_span, mm355_map_batch_bam_run_span;
Aligner.map_bam_file(sort=True, index=True)).  The span stage: the device against the host against the model of tests/_bai.py on streams
built with struct.  The file: the .bai is the model's, built from the bytes of the .bam that was written, whatever the sub-batch and merge
step sizes, and regions answered through it are the brute-force overlap sets.  CPU side: tests/test_bai_host.py."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _bai as B
import _baidata as D
import _bam
import _bamaux as A
import _bamsort as BS
import _inflate as I
from test_gpu_tags import world, _rc          # noqa: F401  (the fixture: its genome and reads)
from test_gpu_sam import _sam_reads
from test_gpu_bamaux import _tagged_bam, _file_records
from test_gpu_bamsort import al, file_world     # noqa: F401  (fixtures)
from test_bai_host import _stage, span_cases, _regions

EINVAL = -2
WORDS = (0, 1, 63, 64, 65, 129, 4097, 65535)     # around the wave's 64 lanes, two rounds and a word, many rounds, the most a record holds


def _rand_rec(rng, k, n_words, name_len, big=True):
    top = 2**28 if big else 3000
    words = (rng.integers(1, top, n_words, dtype=np.int64) << 4 | rng.integers(0, 16, n_words, dtype=np.int64)).tolist()
    return D.rec(int(rng.integers(-1, 3)), int(rng.integers(0, 100000)), int(rng.choice([0, 16, 4, 0x100])), words, b"n" * name_len)


def _streams():
    rng = np.random.default_rng(73)
    out = []
    # every residue of the words' start (names of 1 .. 17 bytes with their NUL) at every word count; lengths up to 2^28 - 1: sums above 2^32
    out.append(("words-residues", [_rand_rec(rng, k, WORDS[k % 8], (k // 8) % 17) for k in range(8 * 17)]))
    out.append(("hand-made", [r for r, w in span_cases().values() if w is not None]))
    for n in (0, 1, 2, 257, 5000):
        out.append(("count-%d" % n, [_rand_rec(rng, k, int(rng.integers(0, 70)), k % 17) for k in range(n)]))
    return out


def test_span_stage_device_equals_host_equals_model(al):
    from mappy_rs import _ffi
    L, ctx = al._L, al._context()
    for label, recs in _streams():
        data, off = BS.stream(recs)
        srt, keys = BS.model(recs)
        want = (b"".join(srt), keys, list(BS.stream(srt)[1]), [B.span_of(r) for r in srt])
        host = _stage(L, L.mm355_bam_sort_span, data, off, len(recs), _ffi.PAF_HOST, ctx)
        dev = _stage(L, L.mm355_bam_sort_span, data, off, len(recs), _ffi.PAF_DEVICE, ctx)
        assert host == want, label
        assert dev[:3] == want[:3], label
        bad = [i for i, (a, b) in enumerate(zip(dev[3], want[3])) if a != b]
        assert not bad and len(dev[3]) == len(want[3]), (label, bad[:5], [(dev[3][i], want[3][i], len(srt[i])) for i in bad[:5]])
        plain = _stage(L, L.mm355_bam_sort, data, off, len(recs), _ffi.PAF_DEVICE, ctx)
        assert plain == want[:3] + (None,), label
        if label == "words-residues":
            assert {(struct.unpack_from("<H", r, 16)[0], r[12]) for r in recs} == {(w, l) for w in WORDS for l in range(1, 18)}
            assert max(s >> 1 for s in want[3]) > 2**32
        if label == "hand-made":
            assert any(struct.unpack_from("<H", r, 16)[0] == 2 and b"CGBI" in r for r in recs)       # the long form


def test_refused_stream_then_a_valid_one_with_spans(al):
    from mappy_rs import _ffi
    L, ctx = al._L, al._context()
    good = [D.rec(1, 50 - k, 0, [(k + 1) << 4 | D.M] * k, b"g" * (k % 5)) for k in range(30)]
    bad = span_cases()["words pass the record"][0]
    want = (b"".join(BS.model(good)[0]), [B.span_of(r) for r in BS.model(good)[0]])
    for where in (_ffi.PAF_DEVICE, _ffi.PAF_HOST):
        data, off = BS.stream(good[:7] + [bad] + good[7:])
        assert _stage(L, L.mm355_bam_sort_span, data, off, len(good) + 1, where, ctx) == EINVAL
        got = _stage(L, L.mm355_bam_sort_span, *BS.stream(good), len(good), where, ctx)
        assert (got[0], got[3]) == want


# ---------------------------------------------------------------- the run call
def _run_call(al, fn, reads, names, quals, aux, where, **kw):
    """mm355_map_batch_bam_run / _span -> (rec, keys, offsets, spans or None)"""
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
    _ffi.check(fn(al._context(), C.byref(al._mo), len(reads), packed.arr, packed.lens, narr, qarr, ptrs, lens, mods, _ffi.OUT_CS, sam_flags, where, C.byref(rp)))
    try:
        r = rp.contents
        n = int(r.n_rec)
        return (C.string_at(r.rec, r.n_bytes), [int(r.key[i]) for i in range(n)], [int(r.rec_off[i]) for i in range(n + 1)],
                [int(r.span[i]) for i in range(n)] if r.span else None)
    finally:
        L.mm355_free_run(rp)


def test_run_call_with_spans(al, world):
    from mappy_rs import _ffi
    L = al._L
    rng = np.random.default_rng(79)
    reads, names, quals = _sam_reads(world, n_plain=40)
    auxes = [None if i % 4 == 3 or not r else A.mod_pair(len(r), rng) + A.tag("RG", "Z", b"g") for i, r in enumerate(reads)]
    for aux in (None, auxes):
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            old = _run_call(al, L.mm355_map_batch_bam_run, reads, names, quals, aux, where)
            new = _run_call(al, L.mm355_map_batch_bam_run_span, reads, names, quals, aux, where)
            assert old[3] is None and new[:3] == old[:3], (aux is not None, where)
            recs = _bam.cut(new[0])
            assert new[3] == [B.span_of(r) for r in recs] and len(recs) > 40
            assert any(s & 1 for s in new[3]) and len({s >> 1 for s in new[3]}) > 30
    empty = _run_call(al, L.mm355_map_batch_bam_run_span, [], [], [], None, _ffi.PAF_DEVICE)
    assert empty == (b"", [], [0], [])


# ---------------------------------------------------------------- the file
def _index_of(path):
    blob, bai = open(path, "rb").read(), open(path + ".bai", "rb").read()
    bam = B.Bam(blob)
    return blob, bai, bam


def test_map_bam_file_index_is_the_models(world, file_world, monkeypatch):
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(3)
    td, fq = file_world["td"], file_world["fq"]
    out, ref_out = str(td / "ix.bam"), str(td / "noix.bam")
    rng = np.random.default_rng(83)
    seen = {}
    for sub, chunk, compress in ((7, 100_000, False), (64, 64 << 20, False), (7, 100_000, True), (64, 64 << 20, True)):
        monkeypatch.setattr(mappy_rs, "SORT_CHUNK_BYTES", chunk)
        res = al.map_bam_file(fq, out, cs=True, sub_batch_reads=sub, sort=True, compress=compress, index=True)
        blob, bai, bam = _index_of(out)
        assert bai == B.build(bam), (sub, chunk, compress)
        assert res["n_index_bytes"] == len(bai) and res["seconds_index"] > 0
        assert sorted(p for p in os.listdir(str(td)) if p.startswith("ix.")) == ["ix.bam", "ix.bam.bai"]
        assert seen.setdefault(compress, (blob, bai)) == (blob, bai), (sub, chunk, compress)     # the same bytes for either sub-batch and step size
        if sub == 64:
            # without the keyword: no index, the same BAM, the dict of today
            res0 = al.map_bam_file(fq, ref_out, cs=True, sub_batch_reads=sub, sort=True, compress=compress)
            assert open(ref_out, "rb").read() == blob and not os.path.exists(ref_out + ".bai")
            assert res.keys() - res0.keys() == {"n_index_bytes", "seconds_index"}
            idx = B.parse(bai)
            assert idx[1] == sum(1 for r in bam.recs if r[0] < 0) > 0                          # n_no_coor: the reads without hits
            assert sum(1 for bins, _ in idx[0] if bins) >= 2
            n_hit = 0
            for ref, b, e in _regions(bam, rng, 200):
                got, want = B.query(bam, idx, ref, b, e), B.brute(bam, ref, b, e)
                assert got == want, (ref, b, e)
                n_hit += bool(want)
            assert n_hit > 40
    assert seen[False][1] != seen[True][1]                                                     # (other blocks, other offsets)


def test_map_bam_file_index_with_copied_tags(world, tmp_path):
    import mappy_rs
    rng = np.random.default_rng(89)
    all_reads, _, _ = _sam_reads(world, n_plain=90)
    reads = [r.replace("N", "A") for r in all_reads[-7:-1] + all_reads[70:100]]
    names = ["r%03d" % i for i in range(len(reads))]
    quals = ["".join(chr(35 + (i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
    blob, _ = _tagged_bam(reads, names, quals, rng)
    src, out = str(tmp_path / "calls.bam"), str(tmp_path / "out.bam")
    open(src, "wb").write(I.bgzf_file(blob, 0xff00))
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(2)
    for kw in (dict(), dict(read_on_gpu=True, compress=True, sub_batch_reads=5)):
        al.map_bam_file(src, out, cs=True, copy_tags=True, sort=True, index=True, **{"sub_batch_reads": 9, **kw})
        data, bai, bam = _index_of(out)
        assert bai == B.build(bam), kw
        assert any(b"MMZ" in r[6] for r in bam.recs)


def test_map_bam_file_index_refusals_and_failure(world, file_world, tmp_path, monkeypatch):
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(2)
    fq = file_world["fq"]
    out = str(tmp_path / "out.bam")
    with pytest.raises(ValueError, match="sort"):
        al.map_bam_file(fq, out, index=True)
    with pytest.raises(ValueError, match="sort"):
        al.map_bam_file(str(tmp_path / "no such reads"), out, index=True)         # before anything is opened
    first = al._names()[0]
    monkeypatch.setattr(mappy_rs, "BAI_MAX_LEN", 1000)                            # (a contig of 2^29 bases would take minutes to index)
    with pytest.raises(ValueError, match=str(first)):
        al.map_bam_file(str(tmp_path / "no such reads"), out, sort=True, index=True)
    monkeypatch.undo()
    assert os.listdir(str(tmp_path)) == []
    blob = open(fq, "rb").read()
    cut = str(tmp_path / "cut.fq.gz")
    open(cut, "wb").write(blob[:len(blob) // 2])
    open(out, "wb").write(b"what was here before\n")
    open(out + ".bai", "wb").write(b"and its index\n")
    out2 = str(tmp_path / "out2.bam")
    for target in (out2, out):
        with pytest.raises(RuntimeError):
            al.map_bam_file(cut, target, cs=True, sub_batch_reads=16, sort=True, index=True)
    assert sorted(os.listdir(str(tmp_path))) == ["cut.fq.gz", "out.bam", "out.bam.bai"]
    assert open(out, "rb").read() == b"what was here before\n" and open(out + ".bai", "rb").read() == b"and its index\n"
    with pytest.raises(TypeError):
        al.map_file(fq, out2, index=True)                                         # SAM and PAF have no `index`
