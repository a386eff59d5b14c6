"""Reads file in, coordinate-sorted compressed BAM out, with the runs spooled uncompressed or compressed: Aligner.map_bam_file(compress=True,
sort=True) against the same call with tmp_compress=True and against the unsorted call, on the same reads -- what compressed runs cost or
give back, and where the time goes -- and the three kernel times of the merge steps.

    python tools/spool_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/bam_sort_spool.json]

The protocol is tools/sort_bench.py's: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode
with cs, a plain FASTQ with synthetic qualities (written once, untimed), one GPU, --threads host threads.  Per route: Mbases/s of the whole
run (median of --passes passes after a warm-up, every pass listed), and for the sorted routes per pass seconds_merge and the run phase (the
rest of the pass), n_tmp_bytes and, with compressed runs, n_tmp_raw_bytes.  The routes run one after the other and then the first again,
so that a drift of the machine shows.
The merge steps: one more tmp_compress pass, untimed, with MM355_BAM_TIMES=1; the library's bam_merge_times lines (one per device step) have
the members and bytes in, the records, the bytes out, and k_bgzf_inflate, k_rec_gather and the deflate kernels each between two events.
The tool sums them over the pass's steps and lists every step."""
import argparse
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

ROUTES = (("unsorted", {}), ("sorted", {"sort": True}), ("sorted_tmp_compress", {"sort": True, "tmp_compress": True}), ("unsorted_again", {}))


def routes(al, n_reads, bases, fq, td, passes):
    res = {}
    out = os.path.join(td, "out.bam")
    for route, kw in ROUTES:
        rows = []

        def run(kw=kw):
            r = al.map_bam_file(fq, out, cs=True, compress=True, **kw)
            extra = {"n_sub_batches": r["n_sub_batches"], "sub_batches_on_device": r["n_on_device"], "output_bytes": r["n_bytes_out"]}
            if kw:
                rows.append({"seconds": round(r["seconds"], 3), "seconds_merge": round(r["seconds_merge"], 3), "seconds_runs": round(r["seconds"] - r["seconds_merge"], 3)})
                extra.update(n_runs=r["n_runs"], n_tmp_bytes=r["n_tmp_bytes"])
                if "n_tmp_raw_bytes" in r:
                    extra.update(n_tmp_raw_bytes=r["n_tmp_raw_bytes"], tmp_bytes_over_raw=round(r["n_tmp_bytes"] / r["n_tmp_raw_bytes"], 4))
            return r["n_lines"], extra
        runs = timed(run, passes)
        rates = [round(bases / t[0] / 1e6, 1) for t in runs]
        res[route] = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "seconds_passes": [round(t[0], 3) for t in runs],
                      "cpu_s_per_million_reads": round(median([t[1] for t in runs]) / n_reads * 1e6, 1), "n_records": runs[-1][2]}
        res[route].update(runs[-1][3])
        if kw:
            res[route]["passes"] = rows[1:]                         # (the warm-up's row dropped)
            for k in ("seconds_merge", "seconds_runs"):
                res[route][k] = median([r[k] for r in rows[1:]])
        print("[spool] %s: %s" % (route, json.dumps(res[route])), flush=True)
    assert res["unsorted"]["n_records"] == res["sorted"]["n_records"] == res["sorted_tmp_compress"]["n_records"]
    assert res["sorted"]["output_bytes"] == res["sorted_tmp_compress"]["output_bytes"]
    u = median(res["unsorted"]["seconds_passes"])
    res["sorted_over_unsorted_seconds"] = round(median(res["sorted"]["seconds_passes"]) / u, 3)
    res["sorted_tmp_compress_over_unsorted_seconds"] = round(median(res["sorted_tmp_compress"]["seconds_passes"]) / u, 3)
    res["sorted_tmp_compress_over_sorted_seconds"] = round(median(res["sorted_tmp_compress"]["seconds_passes"]) / median(res["sorted"]["seconds_passes"]), 3)
    return res


def merge_steps(al, fq, td):
    """one tmp_compress pass with MM355_BAM_TIMES=1: the library's bam_merge_times lines"""
    out = os.path.join(td, "out.bam")
    rows = []
    with tempfile.TemporaryFile() as tf:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["MM355_BAM_TIMES"] = "1"
        try:
            os.dup2(tf.fileno(), 2)
            r = al.map_bam_file(fq, out, cs=True, compress=True, sort=True, tmp_compress=True)
        finally:
            os.dup2(saved, 2); os.close(saved)
            del os.environ["MM355_BAM_TIMES"]
        tf.seek(0)
        for ln in tf.read().decode().splitlines():
            f = ln.split()
            if f[:2] == ["[mm355]", "bam_merge_times"]:
                rows.append({f[i]: float(f[i + 1]) for i in range(2, len(f), 2)})
    assert rows, "no bam_merge_times line"
    tot = {k: round(sum(r[k] for r in rows), 1) for k in rows[0]}
    us = tot["k_bgzf_inflate_us"] + tot["k_rec_gather_us"] + tot["k_bgzf_deflate_compact_us"]
    return {"n_steps": len(rows), "steps": rows, "sum": tot, "kernels_ms": round(us / 1e3, 3), "seconds_merge_of_this_pass": round(r["seconds_merge"], 3),
            "kernels_share_of_the_merge": round(us / 1e6 / r["seconds_merge"], 3),
            "k_bgzf_inflate_gb_per_s_out": round(r["n_tmp_raw_bytes"] / (tot["k_bgzf_inflate_us"] * 1e-6) / 1e9, 1),
            "k_rec_gather_gb_per_s_moved": round(2 * r["n_tmp_raw_bytes"] / (tot["k_rec_gather_us"] * 1e-6) / 1e9, 1)}


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
        print("[spool] genome, %d reads and their file in %.1fs" % (len(reads), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al.enable_threading(args.threads)
        res.update(routes(al, len(reads), res["bases"], fq, td, args.passes))
        res["merge_steps"] = merge_steps(al, fq, td)
        print("[spool] merge steps: %s" % json.dumps({k: v for k, v in res["merge_steps"].items() if k != "steps"}), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
