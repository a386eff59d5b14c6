"""Reads file in, SAM file out: Aligner.map_file(format="sam") with the host and with the device formatter against the route a user had
before it -- map_batch + sam_lines + file.write -- on the same reads, map_file's PAF on those reads for scale, and the formatting step
alone (mm355_text_t::ms_format) over a sweep of batch sizes, which is where MM355_PAF_AUTO's SAM threshold comes from.

    python tools/sam_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/sam_file.json]

The setting is bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode with cs; the reads file
is plain FASTQ with synthetic qualities (written once, untimed).  Per route: Mbases/s, MB of text per second and lines/s of the whole run
(reader, mapping, formatting, writing; median of --passes passes after a warm-up, every pass listed), host CPU seconds per million reads
(process time, all threads), ms_format per sub-batch.  The sweep formats the hits of the first n reads with both formatters (median of five
calls) and reports the smallest hit count from which the device stays ahead; per row also copy_bytes, the bytes k_sam_copy reads plus writes
(twice the SEQ and QUAL text).  At the largest point three more device calls run with MM355_SAM_TIMES=1 and the library's line on stderr is
read back (`device_call_at_largest`, medians): k_sam_copy alone between two events -- its bytes over its time, and that as a fraction of
the 6.3 TB/s a streaming copy reaches on an MI355X --, the host's packing of reads and qualities, and the copy of the text into the
pageable result with its share of the call (the call waits for the kernels before that copy, so its total is not the sweep's ms_format)."""
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


def summarise(runs, n_reads, bases):
    rates = [round(bases / r[0] / 1e6, 1) for r in runs]
    res = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "text_mb_per_s": round(median([r[3]["text_bytes"] / r[0] for r in runs]) / 1e6, 1),
           "lines_per_s": int(median([r[2] / r[0] for r in runs])), "cpu_s_per_million_reads": round(median([r[1] for r in runs]) / n_reads * 1e6, 1),
           "n_lines": runs[-1][2]}
    res.update(runs[-1][3])
    return res


def routes(al, al_base, reads, names, quals, fq, td, passes):
    from mappy_rs import _ffi, sam_lines
    n_reads, bases = len(reads), sum(map(len, reads))
    res = {}
    for route, where, fmt in (("sam_host", _ffi.PAF_HOST, "sam"), ("sam_device", _ffi.PAF_DEVICE, "sam"), ("paf_device", _ffi.PAF_DEVICE, "paf")):
        out = os.path.join(td, "out." + fmt)

        def run(where=where, fmt=fmt, out=out):
            r = al.map_file(fq, out, cs=True, where=where, format=fmt)
            return r["n_lines"], {"ms_format_per_sub_batch": round(r["ms_format"] / r["n_sub_batches"], 2), "n_sub_batches": r["n_sub_batches"],
                                  "sub_batches_on_device": r["n_on_device"], "text_bytes": os.path.getsize(out)}
        res[route] = summarise(timed(run, passes), n_reads, bases)
        print("[sam] %s: %s" % (route, json.dumps(res[route])), flush=True)
    items = [{"seq": r, "name": n, "qual": q} for r, n, q in zip(reads, names, quals)]      # (in memory already: the baseline pays for no reader)
    # rl of a read without hits is not reachable from map_batch: the baseline prints 0 there (it could not do better)
    def base():
        n, out = 0, os.path.join(td, "base.sam")
        with open(out, "w") as f:
            f.write(al_base.sam_header().decode())
            for ms, it in al_base.map_batch(items):
                for ln in sam_lines(ms, it["name"], it["seq"], it["qual"], rl=0):
                    f.write(ln + "\n")
                    n += 1
        return n, {"text_bytes": os.path.getsize(out)}
    res["map_batch_sam_lines"] = summarise(timed(base, passes), n_reads, bases)
    print("[sam] map_batch + sam_lines: %s" % json.dumps(res["map_batch_sam_lines"]), flush=True)
    assert res["map_batch_sam_lines"]["n_lines"] == res["sam_host"]["n_lines"] == res["sam_device"]["n_lines"]
    return res


HBM_STREAM_TB_S = 6.3


def timed_device_calls(call, copy_bytes, n=3):
    """`call()` n times with MM355_SAM_TIMES=1, stderr into a file: the medians of the library's sam_times lines"""
    rows = []
    with tempfile.TemporaryFile() as tf:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["MM355_SAM_TIMES"] = "1"
        try:
            os.dup2(tf.fileno(), 2)
            for _ in range(n):
                call()
        finally:
            os.dup2(saved, 2); os.close(saved)
            del os.environ["MM355_SAM_TIMES"]
        tf.seek(0)
        for ln in tf.read().decode().splitlines():
            f = ln.split()
            if f[:2] == ["[mm355]", "sam_times"]:
                rows.append({f[i]: float(f[i + 1]) for i in range(2, len(f), 2)})
    assert len(rows) == n, rows
    m = {k: median([r[k] for r in rows]) for k in rows[0]}
    tb_s = copy_bytes / (m["k_sam_copy_us"] * 1e-6) / 1e12
    return {"k_sam_copy_us": m["k_sam_copy_us"], "k_sam_copy_bytes": copy_bytes, "k_sam_copy_tb_per_s": round(tb_s, 2),
            "k_sam_copy_fraction_of_streaming_rate": round(tb_s / HBM_STREAM_TB_S, 2), "pack_ms": m["pack_ms"], "text_copy_ms": m["text_copy_ms"],
            "total_ms": m["total_ms"], "text_copy_share": round(m["text_copy_ms"] / m["total_ms"], 2), "pack_share": round(m["pack_ms"] / m["total_ms"], 2)}


def sweep(al, reads, names, quals, flags, sizes):
    """ms_format of the two formatters on the hits of the first n reads -> rows, the hit count from which the device stays ahead, and the
    timed device calls of the largest point"""
    from mappy_rs import _ffi
    L, rows = al._L, []
    for n in sizes:
        if n > len(reads):
            break
        packed, narr = _ffi.pack_reads(reads[:n]), _ffi.pack_names(names[:n])
        qb = [q.encode() for q in quals[:n]]
        qarr = (C.c_char_p * n)(*qb)
        rc, hp = _ffi.call_map(L, al._context(), al._mo, packed, flags | _ffi.OUT_TAGS, narr, entry="named")
        _ffi.check(rc)
        rl = (C.c_int32 * n)()
        ms = {}
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            one = []
            for _ in range(6):
                tp = C.POINTER(_ffi.Text)()
                _ffi.check(L.mm355_sam_format(al._context(), C.byref(al._mo), hp, narr, packed.arr, packed.lens, qarr, rl, 0, where, C.byref(tp)))
                one.append(tp.contents.ms_format); n_text = int(tp.contents.n_text)
                if where == _ffi.PAF_DEVICE and len(one) == 6:
                    copy_bytes = 2 * sum(len(f[9]) + len(f[10]) - (f[9] == b"*") - (f[10] == b"*")
                                         for f in (ln.split(b"\t") for ln in bytes(_ffi.text_view(tp)).split(b"\n") if ln))
                L.mm355_free_text(tp)
            ms[where] = round(median(one[1:]), 3)
        rows.append({"n_reads": n, "n_hits": int(hp.contents.n_hits), "text_bytes": n_text, "copy_bytes": copy_bytes, "ms_host": ms[_ffi.PAF_HOST],
                     "ms_device": ms[_ffi.PAF_DEVICE]})
        if n == max(s for s in sizes if s <= len(reads)):
            def call():
                tp = C.POINTER(_ffi.Text)()
                _ffi.check(L.mm355_sam_format(al._context(), C.byref(al._mo), hp, narr, packed.arr, packed.lens, qarr, rl, 0, _ffi.PAF_DEVICE, C.byref(tp)))
                L.mm355_free_text(tp)
            detail = dict(n_reads=n, **timed_device_calls(call, copy_bytes))
        L.mm355_free_hits(hp)
        print("[sam] sweep: %s" % json.dumps(rows[-1]), flush=True)
    cross = None
    for r in reversed(rows):
        if r["ms_device"] >= r["ms_host"]:
            break
        cross = r["n_hits"]
    print("[sam] device call at the largest point: %s" % json.dumps(detail), flush=True)
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
        print("[sam] genome, %d reads and their file in %.1fs" % (len(reads), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al_base = mappy_rs.Aligner(ref, preset="map-ont", tags=True, name_key="name", build_on_gpu=True)
        al.enable_threading(args.threads); al_base.enable_threading(args.threads)
        res.update(routes(al, al_base, reads, names, quals, fq, td, args.passes))
        res["format_sweep"], res["device_ahead_from_hits"], res["device_call_at_largest"] = sweep(al, reads, names, quals, _ffi.OUT_CS, sizes)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
