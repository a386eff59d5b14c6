"""Compressed runs on the GPU (mm355_bam.hip: k_rec_gather between k_bgzf_inflate and the deflate or framing kernels; mm355_bam_merge_step,
mm355_map_batch_bam_run_packed; Aligner.map_bam_file(sort=True, tmp_compress=True)).  The step: the device against the host against the model
of tests/_bammerge.py, byte for byte, on the steps of _bammerge.steps():
  1, 2, 3 (one of which gives no record) and 257 slices; records of 37, 4095, 4096, 4097, 8193 and 70 000 bytes (the last straddles three
  members); a slice whose first record starts mid-member at each residue 0 .. 15; a carry of 0, 1, 15, 16 and 0xfeff bytes, so that source
  and destination are misaligned against each other in every way; a step smaller than one payload (no block, all carry); final steps with a
  short last payload; stored spool members (random bytes) beside deflated ones; level 0 and level 1.
The packed run call: _run_span plus mm355_bgzf_deflate.  The file: the same .bam and .bai bytes as without the keyword.
CPU side: tests/test_bammerge_host.py."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _bam
import _bamaux as A
import _bammerge as M
import _inflate as I
from test_gpu_tags import world, _rc          # noqa: F401  (the fixture: its genome and reads)
from test_gpu_sam import _sam_reads
from test_gpu_bamaux import _tagged_bam
from test_gpu_bamsort import al, file_world     # noqa: F401  (fixtures)
from test_gpu_bai import _run_call
from test_bammerge_host import all_steps, call_step, check_blocks     # noqa: F401  (all_steps: a fixture)

P = M.P


# ---------------------------------------------------------------- the step: device == host == model
def test_step_device_equals_host_equals_model(al, all_steps):
    from mappy_rs import _ffi
    L, ctx = al._L, al._context()
    n_blocks_out = {0: 0, 1: 0}
    for label, (s, want) in all_steps.items():
        host = call_step(L, ctx, s, _ffi.PAF_HOST)
        dev = call_step(L, ctx, s, _ffi.PAF_DEVICE)
        assert host[3] == 0 and dev[3] == 1, label
        check_blocks(label, host[0], host[1], host[2], want, s.level)
        if dev[:3] != host[:3]:
            raw_d = b"".join(M.members(dev[0])) + dev[2]
            raw_h = want[0] + want[1]
            bad = next((i for i, (a, b) in enumerate(zip(raw_d, raw_h)) if a != b), min(len(raw_d), len(raw_h)))
            raise AssertionError((label, "first different raw byte", bad, "of", len(raw_h), len(raw_d), raw_d[bad - 8:bad + 24].hex(), raw_h[bad - 8:bad + 24].hex()))
        n_blocks_out[s.level] += dev[1]
    assert min(n_blocks_out.values()) > 30
    # what the steps reach
    steps = [s for s, _ in all_steps.values()]
    assert {len(s.slices) for s in steps} >= {0, 1, 2, 3, 257}
    assert {n for s in steps for _, _, n in s.recs} >= set(M.BIG)
    assert {len(s.carry) for s in steps} >= set(M.CARRIES)
    firsts = {(s.recs[0][1] - s.slices[0][2]) % 16 for label, (s, _) in all_steps.items() if label.startswith("residue")}
    assert firsts == set(range(16))                                             # the first record's place in the inflated bytes, every residue
    assert all_steps["small-final-0"][1][0] == b"" and all_steps["small-final-1"][1][1] == b""
    assert any(len(w[0]) % P for s, w in all_steps.values() if s.final)         # a short last payload
    assert any(len(s.slices) > len({r[0] for r in s.recs}) for s in steps if s.recs)                     # a slice that gives no record
    kinds = set()
    for s in steps[:5]:
        at, n, _ = s.slices[0]
        blob, k = s.spool[at:at + n], 0
        while k < len(blob):
            size = int.from_bytes(blob[k + 16:k + 18], "little") + 1
            kinds.add(blob[k + 18] >> 1 & 3)                                    # BTYPE of the member's first deflate block
            k += size
    assert 0 in kinds and kinds - {0}, kinds                                    # stored members beside deflated ones


def test_steps_in_a_row_on_the_device(al):
    """a merge in steps on the device: the carry goes from step to step, and the blocks are mm355_bgzf_deflate of the merged stream"""
    import mappy_rs
    from mappy_rs import _ffi
    L, ctx = al._L, al._context()
    rng = np.random.default_rng(13)
    runs = [M.Run(rng, [int(x) for x in rng.integers(37, 9000, 60)], levels=(6, 0, 1), kinds=(0, 0, 1)) for _ in range(3)]
    spool = M.spool_of(runs)
    merged = [(r, k) for k in range(60) for r in range(3)]
    stream = b"".join(runs[r].recs[k] for r, k in merged)
    for level in (0, 1):
        want = mappy_rs.bgzf_wrap(stream, compress=bool(level))
        for per_step in (7, 180):
            got, carry = b"", b""
            for i in range(0, len(merged), per_step):
                part = merged[i:i + per_step]
                takes = [(r, min(k for q, k in part if q == r), max(k for q, k in part if q == r) + 1) for r in range(3) if any(q == r for q, _ in part)]
                slot = {t[0]: n for n, t in enumerate(takes)}
                order = [(slot[r], k - takes[slot[r]][1]) for r, k in part]
                s = M.step_of(runs, spool, takes, order, carry=carry, final=i + per_step >= len(merged), level=level)
                blocks, _, carry, on = call_step(L, ctx, s, _ffi.PAF_DEVICE)
                assert on == 1
                got += blocks
            assert got == want and carry == b"", (level, per_step)


def test_refused_step_then_a_valid_one(al):
    from mappy_rs import _ffi
    L, ctx = al._L, al._context()
    cases = M.refusals()
    good = cases["good"][0]
    want = M.model(good)
    for where in (_ffi.PAF_DEVICE, _ffi.PAF_HOST):
        for label in ("a record passes its slice's payloads", "a member's CRC-32 is wrong", "rec_slice == n_slice", "a slice ends inside a member", "n_carry == 0xff00"):
            s, code = cases[label]
            assert call_step(L, ctx, s, where) == code, (where, label)
            blocks, n_blocks, left, on = call_step(L, ctx, good, where)
            assert on == (where == _ffi.PAF_DEVICE)
            check_blocks(label, blocks, n_blocks, left, want, good.level)
    assert call_step(L, ctx, good, 3) == M.EINVAL


# ---------------------------------------------------------------- the packed run call
def _packed_call(al, reads, names, quals, aux, where, want_span):
    """mm355_map_batch_bam_run_packed -> (members, keys, offsets, spans or None, member offsets, packed, on_device)"""
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
    _ffi.check(L.mm355_map_batch_bam_run_packed(al._context(), C.byref(al._mo), len(reads), packed.arr, packed.lens, narr, qarr, ptrs, lens, mods, _ffi.OUT_CS, 0, where,
                                                want_span, C.byref(rp)))
    try:
        r = rp.contents
        n = int(r.n_rec)
        return (C.string_at(r.rec, r.n_bytes), [int(r.key[i]) for i in range(n)], [int(r.rec_off[i]) for i in range(n + 1)],
                [int(r.span[i]) for i in range(n)] if r.span else None, [int(r.blk_off[i]) for i in range(int(r.n_blk) + 1)], int(r.packed), int(r.on_device))
    finally:
        L.mm355_free_run(rp)


def test_packed_run_is_the_run_call_plus_deflate(al, world):
    import mappy_rs
    from mappy_rs import _ffi
    L = al._L
    rng = np.random.default_rng(17)
    reads, names, quals = _sam_reads(world, n_plain=40)
    auxes = [None if i % 4 == 3 or not r else A.mod_pair(len(r), rng) + A.tag("RG", "Z", b"g") for i, r in enumerate(reads)]
    for aux in (None, auxes):
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            for want_span in (0, 1):
                plain = _run_call(al, L.mm355_map_batch_bam_run_span if want_span else L.mm355_map_batch_bam_run, reads, names, quals, aux, where)
                rec, keys, off, spans, blk, packed, on = _packed_call(al, reads, names, quals, aux, where, want_span)
                label = (aux is not None, where, want_span)
                assert (keys, off, spans) == plain[1:], label
                assert rec == mappy_rs.bgzf_wrap(plain[0], compress=True), label                     # mm355_bgzf_deflate(level 1) of the unpacked run's rec
                assert packed == 1 and on == (where == _ffi.PAF_DEVICE), label
                raw = len(plain[0])
                assert off[-1] == raw > 2 * P and len(blk) == -(-raw // P) + 1 and blk[0] == 0 and blk[-1] == len(rec) < raw, label
                assert [len(p) for p in M.members(rec)] == [min(P, raw - at) for at in range(0, raw, P)], label
                assert all(rec[b:b + 4] == b"\x1f\x8b\x08\x04" for b in blk[:-1]), label
    # the calls without _packed return what they always did
    for fn in (L.mm355_map_batch_bam_run, L.mm355_map_batch_bam_run_span):
        packed_, narr = _ffi.pack_reads(reads[:3]), _ffi.pack_names(names[:3])
        qarr = (C.c_char_p * 3)(*[None if q is None else q.encode() for q in quals[:3]])
        rp = C.POINTER(_ffi.Run)()
        _ffi.check(fn(al._context(), C.byref(al._mo), 3, packed_.arr, packed_.lens, narr, qarr, None, None, None, _ffi.OUT_CS, 0, _ffi.PAF_DEVICE, C.byref(rp)))
        assert rp.contents.n_rec >= 3 and rp.contents.packed == 0 and rp.contents.n_blk == 0 and not rp.contents.blk_off
        L.mm355_free_run(rp)
    for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
        assert _packed_call(al, [], [], [], None, where, 1)[:6] == (b"", [], [0], [], [0], 1)


# ---------------------------------------------------------------- the file
@pytest.fixture(scope="module")
def plain_files(world, file_world):
    """compress -> (the .bam and .bai bytes, the result dict) of map_bam_file(sort=True, index=True) WITHOUT the keyword; made once"""
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(3)
    out = {}
    for compress in (False, True):
        path = str(file_world["td"] / ("plain%d.bam" % compress))
        res = al.map_bam_file(file_world["fq"], path, cs=True, sub_batch_reads=64, sort=True, compress=compress, index=True)
        out[compress] = (open(path, "rb").read(), open(path + ".bai", "rb").read(), res)
    return out


@pytest.mark.parametrize("sub,chunk,compress", [(7, 100_000, False), (64, 64 << 20, False), (7, 100_000, True), (64, 64 << 20, True)])
def test_map_bam_file_tmp_compress_writes_the_same_bytes(world, file_world, plain_files, tmp_path, monkeypatch, sub, chunk, compress):
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(3)
    monkeypatch.setattr(mappy_rs, "SORT_CHUNK_BYTES", chunk)
    out, spool = str(tmp_path / "out.bam"), tmp_path / "spool"
    spool.mkdir()
    res = al.map_bam_file(file_world["fq"], out, cs=True, sub_batch_reads=sub, sort=True, compress=compress, index=True, tmp_compress=True, tmp_dir=str(spool))
    blob, bai, res0 = plain_files[compress]
    assert open(out, "rb").read() == blob and open(out + ".bai", "rb").read() == bai
    assert os.listdir(str(spool)) == [] and sorted(os.listdir(str(tmp_path))) == ["out.bam", "out.bam.bai", "spool"]
    assert res.keys() - res0.keys() == {"n_tmp_raw_bytes"} and res0.keys() <= res.keys()
    assert res["n_tmp_raw_bytes"] == res0["n_tmp_bytes"] and res["n_lines"] == res0["n_lines"] and res["n_runs"] == -(-len(file_world["reads"]) // sub)
    # the spool: no member is longer than its stored form (at most a member per 0xff00 bytes and one more per run), and these reads compress
    members = res["n_tmp_raw_bytes"] // P + res["n_runs"]
    assert res["n_tmp_bytes"] <= res["n_tmp_raw_bytes"] + 31 * members
    assert res["n_tmp_bytes"] < res["n_tmp_raw_bytes"]
    # without `index`: the same BAM, no index
    out2 = str(tmp_path / "noix.bam")
    if sub == 64:
        al.map_bam_file(file_world["fq"], out2, cs=True, sub_batch_reads=sub, sort=True, compress=compress, tmp_compress=True)
        assert open(out2, "rb").read() == blob and not os.path.exists(out2 + ".bai")


def test_map_bam_file_tmp_compress_with_copied_tags(world, tmp_path):
    import mappy_rs
    rng = np.random.default_rng(19)
    all_reads, _, _ = _sam_reads(world, n_plain=90)
    reads = [r.replace("N", "A") for r in all_reads[-7:-1] + all_reads[70:100]]
    names = ["r%03d" % i for i in range(len(reads))]
    quals = ["".join(chr(35 + (i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
    blob, _ = _tagged_bam(reads, names, quals, rng)
    src, out, ref = str(tmp_path / "calls.bam"), str(tmp_path / "out.bam"), str(tmp_path / "ref.bam")
    open(src, "wb").write(I.bgzf_file(blob, 0xff00))
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(2)
    for kw in (dict(sub_batch_reads=9), dict(read_on_gpu=True, compress=True, sub_batch_reads=5)):      # both readers
        res0 = al.map_bam_file(src, ref, cs=True, copy_tags=True, sort=True, index=True, **kw)
        res = al.map_bam_file(src, out, cs=True, copy_tags=True, sort=True, index=True, tmp_compress=True, **kw)
        assert open(out, "rb").read() == open(ref, "rb").read() and open(out + ".bai", "rb").read() == open(ref + ".bai", "rb").read(), kw
        assert res["n_aux_bytes"] == res0["n_aux_bytes"] > 0 and res.get("reader_on_device", False) == bool(kw.get("read_on_gpu"))
        assert b"MMZ" in gzip.decompress(open(out, "rb").read())


def test_map_bam_file_tmp_compress_refusal_and_failure(world, file_world, tmp_path):
    import mappy_rs
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", devices=[0])
    al.enable_threading(2)
    fq = file_world["fq"]
    out = str(tmp_path / "out.bam")
    with pytest.raises(ValueError, match="sort"):
        al.map_bam_file(fq, out, tmp_compress=True)
    with pytest.raises(ValueError, match="sort"):
        al.map_bam_file(str(tmp_path / "no such reads"), out, tmp_compress=True)          # before anything is opened
    assert os.listdir(str(tmp_path)) == []
    blob = open(fq, "rb").read()
    cut = str(tmp_path / "cut.fq.gz")
    open(cut, "wb").write(blob[:len(blob) // 2])
    open(out, "wb").write(b"what was here before\n")
    out2 = str(tmp_path / "out2.bam")
    for target in (out2, out):
        with pytest.raises(RuntimeError):
            al.map_bam_file(cut, target, cs=True, sub_batch_reads=16, sort=True, index=True, tmp_compress=True)
    assert sorted(os.listdir(str(tmp_path))) == ["cut.fq.gz", "out.bam"] and open(out, "rb").read() == b"what was here before\n"
    with pytest.raises(TypeError):
        al.map_file(fq, out2, tmp_compress=True)                                          # SAM and PAF have no `tmp_compress`
