"""Reads file in, BAM file out: Aligner.map_bam_file with the host and with the device formatter against Aligner.map_file(format="sam") with
either formatter -- the route a user had before, whose text a consumer then parses back into BAM -- on the same reads, and the formatting
step alone (mm355_text_t::ms_format) over the batch sizes of tools/sam_bench.py's sweep, which is where MM355_PAF_AUTO's BAM threshold
comes from.

    python tools/bam_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/bam_file.json]

The protocol is tools/sam_bench.py's: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode
with cs, a plain FASTQ with synthetic qualities (written once, untimed), one GPU.  Per route: Mbases/s and MB of output per second of the
whole run (median of --passes passes after a warm-up, every pass listed), host CPU seconds per million reads, ms_format per sub-batch.  The
sweep formats the hits of the first n reads with both formatters (median of five calls) and reports the smallest hit count from which the
device stays ahead.  At the largest point three more device calls run with MM355_BAM_TIMES=1 and the library's line on stderr is read
back: k_bgzf_frame alone between two events -- the bytes it reads plus writes over its time, and that as a fraction of the 6.3 TB/s a
streaming copy reaches on an MI355X."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mappy-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthdata as S  # noqa: E402
from paf_bench import median, timed  # noqa: E402
from sam_bench import HBM_STREAM_TB_S, summarise  # noqa: E402


def routes(al, reads, fq, td, passes):
    from mappy_rs import _ffi
    n_reads, bases = len(reads), sum(map(len, reads))
    res = {}
    for route, where, fmt in (("bam_host", _ffi.PAF_HOST, "bam"), ("sam_host", _ffi.PAF_HOST, "sam"), ("bam_device", _ffi.PAF_DEVICE, "bam"),
                              ("sam_device", _ffi.PAF_DEVICE, "sam")):
        out = os.path.join(td, "out." + fmt)

        def run(where=where, fmt=fmt, out=out):
            r = al.map_bam_file(fq, out, cs=True, where=where) if fmt == "bam" else al.map_file(fq, out, cs=True, where=where, format="sam")
            return r["n_lines"], {"ms_format_per_sub_batch": round(r["ms_format"] / r["n_sub_batches"], 2), "n_sub_batches": r["n_sub_batches"],
                                  "sub_batches_on_device": r["n_on_device"], "text_bytes": os.path.getsize(out)}
        res[route] = summarise(timed(run, passes), n_reads, bases)
        res[route]["output_mb_per_s"] = res[route].pop("text_mb_per_s")
        res[route]["output_bytes"] = res[route].pop("text_bytes")
        res[route]["n_records"] = res[route].pop("n_lines")
        res[route].pop("lines_per_s")
        print("[bam] %s: %s" % (route, json.dumps(res[route])), flush=True)
    assert res["bam_host"]["n_records"] == res["bam_device"]["n_records"] == res["sam_host"]["n_records"]
    return res


def timed_device_calls(call, n=3):
    """`call()` n times with MM355_BAM_TIMES=1, stderr into a file: the medians of the library's bam_times lines"""
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
            if f[:2] == ["[mm355]", "bam_times"]:
                rows.append({f[i]: float(f[i + 1]) for i in range(2, len(f), 2)})
    assert len(rows) == n, rows
    m = {k: median([r[k] for r in rows]) for k in rows[0]}
    moved = 2 * m["stream_bytes"] + 31 * m["blocks"]                 # the stream read once, the blocks written once
    gb_s = moved / (m["k_bgzf_frame_us"] * 1e-6) / 1e9
    return {"k_bgzf_frame_us": m["k_bgzf_frame_us"], "stream_bytes": int(m["stream_bytes"]), "blocks": int(m["blocks"]), "k_bgzf_frame_bytes_moved": int(moved),
            "k_bgzf_frame_gb_per_s": round(gb_s, 1), "k_bgzf_frame_fraction_of_streaming_rate": round(gb_s / (HBM_STREAM_TB_S * 1e3), 3),
            "pack_ms": m["pack_ms"], "total_ms": m["total_ms"], "frame_share": round(m["k_bgzf_frame_us"] / 1e3 / m["total_ms"], 3)}


def sweep(al, reads, names, quals, flags, sizes):
    """ms_format of the two formatters on the hits of the first n reads -> rows, the hit count from which the device stays ahead, and the
    timed device calls of the largest point"""
    from mappy_rs import _ffi
    L, rows, detail = al._L, [], None
    for n in sizes:
        if n > len(reads):
            break
        packed, narr = _ffi.pack_reads(reads[:n]), _ffi.pack_names(names[:n])
        qb = [q.encode() for q in quals[:n]]
        qarr = (C.c_char_p * n)(*qb)
        rc, hp = _ffi.call_map(L, al._context(), al._mo, packed, flags | _ffi.OUT_TAGS, narr, entry="named")
        _ffi.check(rc)
        rl = (C.c_int32 * n)()

        def call(where):
            tp = C.POINTER(_ffi.Text)()
            _ffi.check(L.mm355_bam_format(al._context(), C.byref(al._mo), hp, narr, packed.arr, packed.lens, qarr, rl, 0, where, C.byref(tp)))
            got = tp.contents.ms_format, int(tp.contents.n_text)
            L.mm355_free_text(tp)
            return got
        ms = {}
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            one = [call(where) for _ in range(6)]
            ms[where] = round(median([t for t, _ in one[1:]]), 3)
        rows.append({"n_reads": n, "n_hits": int(hp.contents.n_hits), "output_bytes": one[-1][1], "ms_host": ms[_ffi.PAF_HOST], "ms_device": ms[_ffi.PAF_DEVICE]})
        if n == max(s for s in sizes if s <= len(reads)):
            detail = dict(n_reads=n, **timed_device_calls(lambda: call(_ffi.PAF_DEVICE)))
        L.mm355_free_hits(hp)
        print("[bam] sweep: %s" % json.dumps(rows[-1]), flush=True)
    cross = None
    for r in reversed(rows):
        if r["ms_device"] >= r["ms_host"]:
            break
        cross = r["n_hits"]
    print("[bam] device call at the largest point: %s" % json.dumps(detail), flush=True)
    return rows, cross, detail


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
        print("[bam] genome, %d reads and their file in %.1fs" % (len(reads), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al.enable_threading(args.threads)
        res.update(routes(al, reads, fq, td, args.passes))
        res["format_sweep"], res["device_ahead_from_hits"], res["device_call_at_largest"] = sweep(al, reads, names, quals, _ffi.OUT_CS, sizes)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
