"""Compressed BAM: the deflate stage of the BAM writer (mm355_deflate.h, mm355_bam.hip: k_bgzf_deflate, k_bgzf_compact) measured four ways.

    python tools/bgzf_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/bgzf_deflate.json]

The protocol is tools/bam_bench.py's: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode
with cs, a plain FASTQ with synthetic qualities (written once, untimed), one GPU, median of --passes passes after a warm-up with every pass
listed.
  routes   Aligner.map_bam_file with the device formatter, without and with compress=True, and with compress=True on the host formatter:
           Mbases/s, MB of output per second, host CPU seconds per million reads, the file's size.
  ratio    the unframed record stream of the first 9216 reads cut at 0xff00: the bytes of this coder's deflate streams (a stored block counts
           len + 5) against zlib level 1 and zlib Z_HUFFMAN_ONLY on the same payloads (raw deflate, on the host), and the share of blocks
           that fell back to the stored form.
  kernel   three device calls at 9216 reads with MM355_BAM_TIMES=1: the library's bgzf_deflate_times line -- k_bgzf_deflate, the scan and
           k_bgzf_compact between two events, bytes in and out -- as GB/s read plus written.
  sweep    the formatting step (mm355_text_t::ms_format) of mm355_bam_format_deflate at level 1 on the host and on the device and at level 0
           on the device, on the hits of 16 .. 9216 reads, next to zlib level 1 on one host thread over the same stream."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mappy-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthdata as S  # noqa: E402
from paf_bench import median, timed  # noqa: E402
from sam_bench import summarise  # noqa: E402

P = 0xff00


def routes(al, reads, fq, td, passes):
    from mappy_rs import _ffi
    n_reads, bases = len(reads), sum(map(len, reads))
    res = {}
    for route, where, compress in (("bam_device", _ffi.PAF_DEVICE, False), ("bam_deflate_device", _ffi.PAF_DEVICE, True), ("bam_deflate_host", _ffi.PAF_HOST, True)):
        out = os.path.join(td, "out.bam")

        def run(where=where, compress=compress, out=out):
            r = al.map_bam_file(fq, out, cs=True, where=where, compress=compress)
            size = os.path.getsize(out)
            assert not compress or r["n_bytes_out"] == size
            return r["n_lines"], {"ms_format_per_sub_batch": round(r["ms_format"] / r["n_sub_batches"], 2), "n_sub_batches": r["n_sub_batches"],
                                  "sub_batches_on_device": r["n_on_device"], "text_bytes": size}
        res[route] = summarise(timed(run, passes), n_reads, bases)
        res[route]["output_mb_per_s"] = res[route].pop("text_mb_per_s")
        res[route]["output_bytes"] = res[route].pop("text_bytes")
        res[route]["n_records"] = res[route].pop("n_lines")
        res[route].pop("lines_per_s")
        print("[bgzf] %s: %s" % (route, json.dumps(res[route])), flush=True)
    assert res["bam_device"]["n_records"] == res["bam_deflate_device"]["n_records"] == res["bam_deflate_host"]["n_records"]
    return res


def blocks_of(bgzf):
    at = 0
    while at < len(bgzf):
        n = struct.unpack_from("<H", bgzf, at + 16)[0] + 1
        yield bgzf[at:at + n]
        at += n


def raw_deflate(payload, level, strategy):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return z.compress(payload) + z.flush()


def ratio(stream, ours):
    """the deflate streams' bytes of the three coders over the payloads of `stream`; ours: the level-1 blocks"""
    payloads = [stream[a:a + P] for a in range(0, len(stream), P)]
    mine = [len(b) - 26 for b in blocks_of(ours)]
    assert len(mine) == len(payloads)
    stored = sum(m == len(p) + 5 for m, p in zip(mine, payloads))
    t0 = time.perf_counter()
    z1 = sum(len(raw_deflate(p, 1, zlib.Z_DEFAULT_STRATEGY)) for p in payloads)
    t1 = time.perf_counter()
    zh = sum(len(raw_deflate(p, 6, zlib.Z_HUFFMAN_ONLY)) for p in payloads)
    z6 = sum(len(raw_deflate(p, 6, zlib.Z_DEFAULT_STRATEGY)) for p in payloads)
    n = len(stream)
    return {"stream_bytes": n, "blocks": len(payloads), "stored_blocks": int(stored), "stored_share": round(stored / len(payloads), 4),
            "deflate_bytes": sum(mine), "ratio": round(n / sum(mine), 3), "zlib_level_1_bytes": z1, "zlib_level_1_ratio": round(n / z1, 3),
            "zlib_huffman_only_bytes": zh, "zlib_huffman_only_ratio": round(n / zh, 3), "zlib_level_6_bytes": z6, "zlib_level_6_ratio": round(n / z6, 3),
            "zlib_level_1_one_thread_ms": round((t1 - t0) * 1e3, 1), "zlib_version": zlib.ZLIB_RUNTIME_VERSION}


def timed_device_calls(call, n=3):
    """`call()` n times with MM355_BAM_TIMES=1, stderr into a file: the medians of the library's bgzf_deflate_times lines"""
    rows = []
    with tempfile.TemporaryFile() as tf:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["MM355_BAM_TIMES"] = "1"
        try:
            os.dup2(tf.fileno(), 2)
            for _ in range(n):
                call()
        finally:
            os.dup2(saved, 2); os.close(saved)
            del os.environ["MM355_BAM_TIMES"]
        tf.seek(0)
        for ln in tf.read().decode().splitlines():
            f = ln.split()
            if f[:2] == ["[mm355]", "bgzf_deflate_times"]:
                rows.append({f[i]: float(f[i + 1]) for i in range(4, len(f), 2)})
    assert len(rows) == n, rows
    m = {k: median([r[k] for r in rows]) for k in rows[0]}
    us = m["k_bgzf_deflate_compact_us"]
    return {"k_bgzf_deflate_compact_us": us, "k_bgzf_deflate_compact_us_calls": [r["k_bgzf_deflate_compact_us"] for r in rows], "bytes_in": int(m["bytes_in"]),
            "bytes_out": int(m["bytes_out"]), "blocks": int(m["blocks"]), "stored_blocks": int(m["stored_blocks"]),
            "gb_per_s_in_plus_out": round((m["bytes_in"] + m["bytes_out"]) / (us * 1e-6) / 1e9, 2), "gb_per_s_in": round(m["bytes_in"] / (us * 1e-6) / 1e9, 2)}


def sweep(al, reads, names, quals, flags, sizes):
    from mappy_rs import _ffi
    L, rows, detail, rat = al._L, [], None, None
    for n in sizes:
        if n > len(reads):
            break
        packed, narr = _ffi.pack_reads(reads[:n]), _ffi.pack_names(names[:n])
        qb = [q.encode() for q in quals[:n]]
        qarr = (C.c_char_p * n)(*qb)
        rc, hp = _ffi.call_map(L, al._context(), al._mo, packed, flags | _ffi.OUT_TAGS, narr, entry="named")
        _ffi.check(rc)
        rl = (C.c_int32 * n)()

        def call(where, level, keep=False):
            tp = C.POINTER(_ffi.Text)()
            _ffi.check(L.mm355_bam_format_deflate(al._context(), C.byref(al._mo), hp, narr, packed.arr, packed.lens, qarr, rl, 0, where, level, C.byref(tp)))
            got = tp.contents.ms_format, int(tp.contents.n_text), bytes(_ffi.text_view(tp)) if keep else None
            L.mm355_free_text(tp)
            return got
        ms = {}
        for key, where, level, reps in (("ms_host_deflate", _ffi.PAF_HOST, 1, 3 if n >= 1024 else 6), ("ms_device_deflate", _ffi.PAF_DEVICE, 1, 6), ("ms_device_stored", _ffi.PAF_DEVICE, 0, 6)):
            one = [call(where, level) for _ in range(reps)]
            ms[key] = round(median([t for t, _, _ in one[1:]]), 3)
            ms[key.replace("ms_", "bytes_")] = one[-1][1]
        framed = call(_ffi.PAF_DEVICE, 0, keep=True)[2]
        stream = b"".join(framed[a + 23:a + P + 23] for a in range(0, len(framed), P + 31))
        stream = stream[:len(framed) - 31 * ((len(framed) + P + 30) // (P + 31))]
        t0 = time.perf_counter()
        for a in range(0, len(stream), P):
            raw_deflate(stream[a:a + P], 1, zlib.Z_DEFAULT_STRATEGY)
        ms["ms_zlib_level_1_one_thread"] = round((time.perf_counter() - t0) * 1e3, 3)
        rows.append(dict(n_reads=n, n_hits=int(hp.contents.n_hits), stream_bytes=len(stream), **ms))
        if n == max(s for s in sizes if s <= len(reads)):
            ours = call(_ffi.PAF_DEVICE, 1, keep=True)[2]
            assert ours == call(_ffi.PAF_HOST, 1, keep=True)[2]
            rat = dict(n_reads=n, **ratio(stream, ours))
            detail = dict(n_reads=n, **timed_device_calls(lambda: call(_ffi.PAF_DEVICE, 1)))
        L.mm355_free_hits(hp)
        print("[bgzf] sweep: %s" % json.dumps(rows[-1]), flush=True)
    cross = None
    for r in reversed(rows):
        if r["ms_device_deflate"] >= r["ms_host_deflate"]:
            break
        cross = r["n_hits"]
    print("[bgzf] ratio: %s" % json.dumps(rat), flush=True)
    print("[bgzf] device call at the largest point: %s" % json.dumps(detail), flush=True)
    return rows, cross, rat, detail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=73728)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mappy_rs
    from mappy_rs import _ffi
    t0 = time.time()
    g = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01)))
    reads, _ = S.make_reads(2, g, args.reads, n50=8000, sigma=0.75, lo=500, hi=100000)
    names = ["read%06d" % i for i in range(len(reads))]
    pat = "".join(chr(35 + (7 * j) % 40) for j in range(101000))
    quals = [pat[i % 1000:i % 1000 + len(r)] for i, r in enumerate(reads)]
    sizes = [16, 24, 32, 48, 64, 256, 1024, 2048, 4096, 9216]
    res = {"threads": args.threads, "passes": args.passes, "sub_batch_reads": mappy_rs.SUB_BATCH_READS, "n_reads": len(reads), "bases": sum(map(len, reads))}
    with tempfile.TemporaryDirectory() as td:
        ref, fq = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fq")
        S.write_fasta(ref, g, ["chrE"])
        with open(fq, "w") as f:
            f.write("".join("@%s\n%s\n+\n%s\n" % t for t in zip(names, reads, quals)))
        print("[bgzf] genome, %d reads and their file in %.1fs" % (len(reads), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al.enable_threading(args.threads)
        res["format_sweep"], res["device_ahead_from_hits"], res["ratio"], res["device_call_at_largest"] = sweep(al, reads, names, quals, _ffi.OUT_CS, sizes)
        res.update(routes(al, reads, fq, td, args.passes))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
