"""Reads file in, coordinate-sorted compressed BAM out: Aligner.map_bam_file(compress=True, sort=True) against the same call without `sort`
on the same reads -- what the sorted route costs over the unsorted one and where the time goes -- and the sort step of one sub-batch alone.

    python tools/sort_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/bam_sort.json]

The protocol is tools/bam_bench.py's: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode
with cs, a plain FASTQ with synthetic qualities (written once, untimed), one GPU, --threads host threads.  Per route: Mbases/s of the whole
run (median of --passes passes after a warm-up, every pass listed).  The sorted route also lists, per pass, seconds_merge and inside it the
seconds spent in mm355_bam_gather and in mm355_bgzf_deflate (the library calls are wrapped by a clock for the sorted passes only); what is
left of the merge is the argsort of the keys and the writes.  The run phase is the rest of the pass.
The sort step: mm355_map_batch_bam_run on the first sub-batch with the device formatter and MM355_BAM_TIMES=1, three calls; the library's
bam_sort_times line has k_rec_key + the radix sort + the gather and scans + k_rec_permute between two events, and k_bam_bulk's time on the
same records.  The sort reads the stream once and writes it once; k_bam_bulk (the tiled writer whose mode 5 is the same copy loop) reads a
base and a quality byte and writes 1.5 bytes per base of a record with SEQ, which the tool bounds from above by the reads' bases."""
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
from sam_bench import HBM_STREAM_TB_S  # noqa: E402


class Clocked:
    """a library function with a clock around it"""

    def __init__(self, f):
        self.f, self.s = f, 0.0

    def __call__(self, *a):
        t0 = time.perf_counter()
        try:
            return self.f(*a)
        finally:
            self.s += time.perf_counter() - t0


def routes(al, n_reads, bases, fq, td, passes):
    L, res = al._L, {}
    out = os.path.join(td, "out.bam")
    for route, sort in (("unsorted", False), ("sorted", True), ("unsorted_again", False)):
        rows = []

        def run(sort=sort):
            gather, deflate = L.mm355_bam_gather, L.mm355_bgzf_deflate
            if sort:
                L.mm355_bam_gather, L.mm355_bgzf_deflate = Clocked(gather), Clocked(deflate)
            try:
                r = al.map_bam_file(fq, out, cs=True, compress=True, sort=True) if sort else al.map_bam_file(fq, out, cs=True, compress=True)
                if sort:
                    rows.append({"seconds": round(r["seconds"], 3), "seconds_merge": round(r["seconds_merge"], 3), "seconds_runs": round(r["seconds"] - r["seconds_merge"], 3),
                                 "gather_s": round(L.mm355_bam_gather.s, 3), "deflate_s": round(L.mm355_bgzf_deflate.s, 3),
                                 "argsort_and_write_s": round(r["seconds_merge"] - L.mm355_bam_gather.s - L.mm355_bgzf_deflate.s, 3)})
            finally:
                L.mm355_bam_gather, L.mm355_bgzf_deflate = gather, deflate
            extra = {"n_sub_batches": r["n_sub_batches"], "sub_batches_on_device": r["n_on_device"], "output_bytes": r["n_bytes_out"]}
            if sort:
                extra.update(n_runs=r["n_runs"], n_tmp_bytes=r["n_tmp_bytes"])
            return r["n_lines"], extra
        runs = timed(run, passes)
        rates = [round(bases / t[0] / 1e6, 1) for t in runs]
        res[route] = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "seconds_passes": [round(t[0], 3) for t in runs],
                      "cpu_s_per_million_reads": round(median([t[1] for t in runs]) / n_reads * 1e6, 1), "n_records": runs[-1][2]}
        res[route].update(runs[-1][3])
        if sort:
            res[route]["passes"] = rows[1:]                         # (the warm-up's row dropped)
            for k in ("seconds_merge", "seconds_runs", "gather_s", "deflate_s", "argsort_and_write_s"):
                res[route][k] = median([r[k] for r in rows[1:]])
        print("[sort] %s: %s" % (route, json.dumps(res[route])), flush=True)
    assert res["unsorted"]["n_records"] == res["sorted"]["n_records"]
    res["sorted_over_unsorted_seconds"] = round(median(res["sorted"]["seconds_passes"]) / median(res["unsorted"]["seconds_passes"]), 3)
    return res


def sort_step(al, reads, names, quals, n, calls=3):
    """the sort step of the first n reads' records: medians of the library's bam_sort_times lines"""
    from mappy_rs import _ffi
    L = al._L
    packed, narr = _ffi.pack_reads(reads[:n]), _ffi.pack_names(names[:n])
    qb = [q.encode() for q in quals[:n]]
    qarr = (C.c_char_p * n)(*qb)

    def call():
        rp = C.POINTER(_ffi.Run)()
        _ffi.check(L.mm355_map_batch_bam_run(al._context(), C.byref(al._mo), n, packed.arr, packed.lens, narr, qarr, None, None, None, _ffi.OUT_CS, 0, _ffi.PAF_DEVICE,
                                             C.byref(rp)))
        got = rp.contents.ms_sort
        L.mm355_free_run(rp)
        return got
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
    assert len(rows) == calls, rows
    m = {k: median([r[k] for r in rows]) for k in rows[0]}
    bases = sum(map(len, reads[:n]))
    sort_gb_s = 2 * m["stream_bytes"] / (m["k_rec_key_sort_permute_us"] * 1e-6) / 1e9
    bulk_gb_s = 3.5 * bases / (m["k_bam_bulk_us"] * 1e-6) / 1e9
    return {"n_reads": n, "records": int(m["records"]), "stream_bytes": int(m["stream_bytes"]), "k_rec_key_sort_permute_us": m["k_rec_key_sort_permute_us"],
            "k_rec_key_sort_permute_us_calls": [r["k_rec_key_sort_permute_us"] for r in rows], "sort_bytes_moved": int(2 * m["stream_bytes"]),
            "sort_gb_per_s": round(sort_gb_s, 1), "sort_fraction_of_streaming_rate": round(sort_gb_s / (HBM_STREAM_TB_S * 1e3), 3),
            "k_bam_bulk_us": m["k_bam_bulk_us"], "k_bam_bulk_bytes_moved_upper_bound": int(3.5 * bases), "k_bam_bulk_gb_per_s_upper_bound": round(bulk_gb_s, 1),
            "total_ms": m["total_ms"], "sort_share_of_the_format_call": round(m["k_rec_key_sort_permute_us"] / 1e3 / m["total_ms"], 3)}


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
        print("[sort] genome, %d reads and their file in %.1fs" % (len(reads), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al.enable_threading(args.threads)
        res.update(routes(al, len(reads), res["bases"], fq, td, args.passes))
        res["sort_step_at_largest"] = sort_step(al, reads, names, quals, min(mappy_rs.SUB_BATCH_READS, len(reads)))
        print("[sort] sort step: %s" % json.dumps(res["sort_step_at_largest"]), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
