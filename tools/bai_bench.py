"""Reads file in, coordinate-sorted compressed BAM and its .bai out: Aligner.map_bam_file(compress=True, sort=True, index=True) against the
same call without `index` on the same reads -- what the index costs -- and k_rec_span on one sub-batch alone.

    python tools/bai_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/bam_index.json]

The protocol is tools/sort_bench.py's: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode
with cs, a plain FASTQ with synthetic qualities (written once, untimed), one GPU, --threads host threads.  Per route: Mbases/s of the whole
run (median of --passes passes after a warm-up, every pass listed).  The indexed route also lists, per pass, seconds_index (the builder's
calls and the write of the .bai), the index's bytes and the bins' chunks before and after the finishing merges (mm355_bai_finish reports
them in the text's n_reads / n_lines; the tool wraps the call to read them).
k_rec_span: mm355_map_batch_bam_run_span on the first sub-batch with the device formatter and MM355_BAM_TIMES=1, three calls; the library's
bam_sort_times line ends with the kernel's time between two events of its own.  The bytes it read are counted from the run that came
back: per record the two offsets, the fixed fields' cache line and 4 bytes per CIGAR word."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mappy-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthdata as S  # noqa: E402
from paf_bench import median, timed  # noqa: E402
from sam_bench import HBM_STREAM_TB_S  # noqa: E402


def routes(al, n_reads, bases, fq, td, passes):
    L, res = al._L, {}
    out = os.path.join(td, "out.bam")
    for route, index in (("sorted", False), ("sorted_indexed", True), ("sorted_again", False)):
        rows = []

        def run(index=index):
            finish, seen = L.mm355_bai_finish, {}

            def finish_and_look(h, tpref):
                rc = finish(h, tpref)
                if rc == 0:
                    seen["raw"], seen["fin"] = int(tpref._obj.contents.n_reads), int(tpref._obj.contents.n_lines)
                return rc
            if index:
                L.mm355_bai_finish = finish_and_look
            try:
                r = al.map_bam_file(fq, out, cs=True, compress=True, sort=True, index=True) if index else al.map_bam_file(fq, out, cs=True, compress=True, sort=True)
            finally:
                L.mm355_bai_finish = finish
            extra = {"n_sub_batches": r["n_sub_batches"], "output_bytes": r["n_bytes_out"], "seconds_merge": round(r["seconds_merge"], 3)}
            if index:
                assert os.path.getsize(out + ".bai") == r["n_index_bytes"]
                rows.append({"seconds": round(r["seconds"], 3), "seconds_merge": round(r["seconds_merge"], 3), "seconds_index": round(r["seconds_index"], 4),
                             "n_index_bytes": r["n_index_bytes"], "chunks_before_finishing": seen["raw"], "chunks_after_finishing": seen["fin"]})
                os.remove(out + ".bai")
            return r["n_lines"], extra
        runs = timed(run, passes)
        rates = [round(bases / t[0] / 1e6, 1) for t in runs]
        res[route] = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "seconds_passes": [round(t[0], 3) for t in runs],
                      "cpu_s_per_million_reads": round(median([t[1] for t in runs]) / n_reads * 1e6, 1), "n_records": runs[-1][2]}
        res[route].update(runs[-1][3])
        if index:
            res[route]["passes"] = rows[1:]                         # (the warm-up's row dropped)
            for k in ("seconds_merge", "seconds_index"):
                res[route][k] = median([r[k] for r in rows[1:]])
            for k in ("n_index_bytes", "chunks_before_finishing", "chunks_after_finishing"):
                res[route][k] = rows[-1][k]
        print("[bai] %s: %s" % (route, json.dumps(res[route])), flush=True)
    assert res["sorted"]["n_records"] == res["sorted_indexed"]["n_records"] and res["sorted"]["output_bytes"] == res["sorted_indexed"]["output_bytes"]
    res["indexed_over_sorted_seconds"] = round(median(res["sorted_indexed"]["seconds_passes"]) / median(res["sorted"]["seconds_passes"]), 3)
    return res


def span_step(al, reads, names, quals, n, calls=3):
    """k_rec_span on the first n reads' records: medians of the library's bam_sort_times lines"""
    from mappy_rs import _ffi
    L = al._L
    packed, narr = _ffi.pack_reads(reads[:n]), _ffi.pack_names(names[:n])
    qb = [q.encode() for q in quals[:n]]
    qarr = (C.c_char_p * n)(*qb)
    seen = {}

    def call():
        rp = C.POINTER(_ffi.Run)()
        _ffi.check(L.mm355_map_batch_bam_run_span(al._context(), C.byref(al._mo), n, packed.arr, packed.lens, narr, qarr, None, None, None, _ffi.OUT_CS, 0, _ffi.PAF_DEVICE,
                                                  C.byref(rp)))
        r = rp.contents
        k = int(r.n_rec)
        rec = np.ctypeslib.as_array(C.cast(r.rec, C.POINTER(C.c_uint8)), shape=(int(r.n_bytes),))
        off = np.ctypeslib.as_array(r.rec_off, shape=(k + 1,))[:-1]
        words = rec[off + 16].astype(np.int64) | rec[off + 17].astype(np.int64) << 8
        seen["words"], seen["records"] = int(words.sum()), k
        L.mm355_free_run(rp)
    call()
    rows = []
    with tempfile.TemporaryFile() as tf:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["MM355_BAM_TIMES"] = "1"
        try:
            os.dup2(tf.fileno(), 2)
            for _ in range(calls):
                call()
        finally:
            os.dup2(saved, 2); os.close(saved)
            del os.environ["MM355_BAM_TIMES"]
        tf.seek(0)
        for ln in tf.read().decode().splitlines():
            f = ln.split()
            if f[:2] == ["[mm355]", "bam_sort_times"]:
                rows.append({f[i]: float(f[i + 1]) for i in range(2, len(f), 2)})
    assert len(rows) == calls and all("k_rec_span_us" in r for r in rows), rows
    m = {k: median([r[k] for r in rows]) for k in rows[0]}
    n_bytes = 4 * seen["words"] + (16 + 64 + 8) * seen["records"]
    gb_s = n_bytes / (m["k_rec_span_us"] * 1e-6) / 1e9
    return {"n_reads": n, "records": seen["records"], "stream_bytes": int(m["stream_bytes"]), "cigar_words": seen["words"], "bytes_read_and_written": n_bytes,
            "cigar_share_of_stream": round(4 * seen["words"] / m["stream_bytes"], 4),
            "k_rec_span_us": m["k_rec_span_us"], "k_rec_span_us_calls": [r["k_rec_span_us"] for r in rows], "k_rec_span_gb_per_s": round(gb_s, 1),
            "fraction_of_streaming_rate": round(gb_s / (HBM_STREAM_TB_S * 1e3), 4),
            "k_rec_key_sort_permute_us": m["k_rec_key_sort_permute_us"], "k_rec_key_sort_permute_us_calls": [r["k_rec_key_sort_permute_us"] for r in rows],
            "total_ms": m["total_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=73728)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mappy_rs
    t0 = time.time()
    g = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01)))
    reads, _ = S.make_reads(2, g, args.reads, n50=8000, sigma=0.75, lo=500, hi=100000)
    names = ["read%06d" % i for i in range(len(reads))]
    pat = "".join(chr(35 + (7 * j) % 40) for j in range(101000))
    quals = [pat[i % 1000:i % 1000 + len(r)] for i, r in enumerate(reads)]
    res = {"threads": args.threads, "passes": args.passes, "sub_batch_reads": mappy_rs.SUB_BATCH_READS, "sort_chunk_bytes": mappy_rs.SORT_CHUNK_BYTES,
           "n_reads": len(reads), "bases": sum(map(len, reads))}
    with tempfile.TemporaryDirectory() as td:
        ref, fq = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fq")
        S.write_fasta(ref, g, ["chrE"])
        with open(fq, "w") as f:
            f.write("".join("@%s\n%s\n+\n%s\n" % t for t in zip(names, reads, quals)))
        print("[bai] genome, %d reads and their file in %.1fs" % (len(reads), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al.enable_threading(args.threads)
        res.update(routes(al, len(reads), res["bases"], fq, td, args.passes))
        res["span_step_at_largest"] = span_step(al, reads, names, quals, min(mappy_rs.SUB_BATCH_READS, len(reads)))
        print("[bai] span step: %s" % json.dumps(res["span_step_at_largest"]), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
