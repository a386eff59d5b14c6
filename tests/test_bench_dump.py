"""bench.py --dump-outputs without a GPU: dump_outputs() fed hand-made mm355_hits_t records (two sub-batches, cs present and absent,
CIGARs stored out of hit order) writes every file as float32 / float64 within the 64 MB budget, and what it writes is what the records hold."""
import ctypes as C
import os

import numpy as np

import bench
from mappy_rs import _ffi


def _batch(rng, n_reads, cs=True):
    """one mm355_hits_t of random records; returns (n_reads, pointer, what it holds, the arrays that keep its memory alive)"""
    per_read = rng.integers(0, 3, n_reads)
    nh = int(per_read.sum())
    off = np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64)
    hits = (_ffi.Hit * max(1, nh))()
    n_cig = rng.integers(1, 6, nh)
    cig_off = np.concatenate([[0], np.cumsum(n_cig[::-1])])[:-1][::-1]     # CIGARs stored last hit first
    cig = (rng.integers(1, 500, int(n_cig.sum())).astype(np.uint32) << 4) | rng.integers(0, 9, int(n_cig.sum())).astype(np.uint32)
    strs, cs_of = b"", []
    for i in range(nh):
        h = hits[i]
        h.rid, h.target_start, h.target_end, h.query_start, h.query_end = int(rng.integers(0, 24)), int(rng.integers(0, 2**31 - 1)), 7, 3, 9
        h.strand, h.mapq, h.NM, h.n_cigar, h.cigar_off = int(rng.choice([-1, 1])), int(rng.integers(0, 61)), i, int(n_cig[i]), int(cig_off[i])
        s = (":%d*ag+c" % i).encode() if cs and i % 3 else b""
        h.cs_off, h.cs_len = len(strs), (len(s) if cs and i % 3 else -1)
        cs_of.append(s)
        strs += s
    keep = [off, cig, hits, C.create_string_buffer(strs, max(1, len(strs)))]
    hs = _ffi.Hits(n_reads=n_reads, hit_off=off.ctypes.data_as(C.POINTER(C.c_int64)), hits=hits, cigar=cig.ctypes.data_as(C.POINTER(C.c_uint32)),
                   str=C.cast(keep[3], C.POINTER(C.c_char)), n_hits=nh, n_cigar=len(cig), n_str=len(strs))
    keep.append(hs)
    words = [cig[cig_off[i]:cig_off[i] + n_cig[i]] for i in range(nh)]
    return (n_reads, C.pointer(hs)), dict(per_read=per_read, hits=[hits[i] for i in range(nh)], words=words, cs=cs_of), keep


def _load(d):
    out = {}
    for fn in os.listdir(d):
        a = np.load(os.path.join(d, fn))
        assert a.dtype in (np.float32, np.float64), fn
        out[fn[:-4]] = a
    assert sum(os.path.getsize(os.path.join(d, fn)) for fn in os.listdir(d)) <= 64 << 20
    return out


def test_dump_outputs_holds_the_records(tmp_path):
    rng = np.random.default_rng(5)
    parts, truth, keep = zip(*[_batch(rng, 40), _batch(rng, 0), _batch(rng, 25, cs=False)])
    bench.dump_outputs(str(tmp_path), list(parts))
    f = _load(str(tmp_path))
    hits = [h for t in truth for h in t["hits"]]
    words = [w for t in truth for w in t["words"]]
    cs = [s for t in truth for s in t["cs"]]
    assert f["hits_per_read"].tolist() == np.concatenate([t["per_read"] for t in truth]).tolist()
    assert "hit_row" not in f
    for k in bench.DUMP_HIT_FIELDS:
        assert f["hit_" + k].tolist() == [float(getattr(h, k)) for h in hits], k
    ob = np.zeros((len(hits), 9))
    for i, w in enumerate(words):
        np.add.at(ob[i], w & 15, w >> 4)
    assert np.array_equal(f["hit_cigar_op_bases"], ob)
    picked = f["sample_hit"].astype(int).tolist()
    assert picked == sorted(set(picked)) and len(picked) == min(len(hits), bench.DUMP_SAMPLE_HITS)
    co, so = f["sample_cigar_off"].astype(int), f["sample_cs_off"].astype(int)
    for j, i in enumerate(picked):
        assert f["sample_cigar"][co[j]:co[j + 1]].tolist() == words[i].astype(np.float64).tolist()
        assert bytes(f["sample_cs"][so[j]:so[j + 1]].astype(np.uint8)) == cs[i]


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    """a budget smaller than the records: a seeded sample of the hit rows (hit_row), the same files for the same records"""
    monkeypatch.setattr(bench, "DUMP_BYTES", 40 * 8 * (len(bench.DUMP_HIT_FIELDS) + 9))
    rng = np.random.default_rng(6)
    parts, truth, keep = zip(*[_batch(rng, 60), _batch(rng, 50)])
    shapes = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), list(parts))
        shapes.append(_load(str(tmp_path / d)))
    a, b = shapes
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BYTES
    hits = [h for t in truth for h in t["hits"]]
    rows = a["hit_row"].astype(int)
    assert len(rows) < len(hits) and rows.tolist() == sorted(set(rows.tolist()))
    assert a["hit_NM"].tolist() == [float(hits[i].NM) for i in rows]
