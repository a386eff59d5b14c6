"""What the long form of cs (minimap2 --cs=long, MM355_OUT_CS_LONG) costs beside the short form and no cs at all.

    python tools/cslong_bench.py [--reads 36864] [--passes 3] [--threads 8] [--out profiles/cs_long.json]

Workload: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2), one GPU, mm355_map_batch on sub-batches of
9216 reads, one context.  Modes: flags 0 (no cs), MM355_OUT_CS (short), MM355_OUT_CS_LONG (long).  Every mode runs in a child process of its
own (the MM355_TRACE timeline is written when a process ends): a warm-up pass, then --passes timed passes over all sub-batches, each pass a
host clock around calls that end in a device synchronise.  Reported per mode: Mbases/s of every pass and their median; KT_EXTRA (the stage
timer of k_extra / k_extra_long + k_extra_compose + k_extra_scan, mm355_stats_t::ms_kernel[17]) per pass; the x:walk and x:strings phases of the
timeline (upload + walk + compose + the regions' lengths back; compaction + the strings back) as a mean per pass over all passes, the warm-up
included; the bytes of the hits' string arena per base (what is copied back and handed on).  Then map_file(cs="long") against map_file(cs=True)
on the same reads as a FASTQ, --threads workers: Mbases/s per pass and bytes out.  Nothing here is gated."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mappy-rs_amd"))
SUB = 9216
KT_EXTRA = 17


def median(xs):
    return sorted(xs)[len(xs) // 2]


def world(n_reads, td):
    import synthdata as S
    g = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01)))
    reads, _ = S.make_reads(2, g, n_reads, n50=8000, sigma=0.75, lo=500, hi=100000)
    ref, fq = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fq")
    S.write_fasta(ref, g, ["chrE"])
    with open(fq, "w") as f:
        for i, r in enumerate(reads):
            f.write("@read%06d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    return ref, fq


def read_fastq(fq):
    with open(fq) as f:
        return [ln.rstrip("\n") for k, ln in enumerate(f) if k % 4 == 1]


def child(args):
    """one mode, in this process: prints one JSON line"""
    import mappy_rs
    from mappy_rs import _ffi
    reads = read_fastq(args.fq)
    bases = sum(map(len, reads))
    al = mappy_rs.Aligner(args.ref, preset="map-ont", build_on_gpu=True)
    L = al._L
    if args.child in ("none", "short", "long"):
        flags = {"none": 0, "short": _ffi.OUT_CS, "long": _ffi.OUT_CS_LONG}[args.child]
        subs = [_ffi.pack_reads(reads[k:k + SUB]) for k in range(0, len(reads), SUB)]
        rates, kt, str_bytes, n_hits = [], [], 0, 0
        for p in range(args.passes + 1):                     # (the first pass is the warm-up)
            t0, kt_pass, str_bytes, n_hits = time.perf_counter(), 0.0, 0, 0
            for packed in subs:
                rc, hp = _ffi.call_map(L, al._context(), al._mo, packed, flags)
                _ffi.check(rc)
                kt_pass += float(_ffi.get_stats(L, al._context()).ms_kernel[KT_EXTRA])
                str_bytes += int(hp.contents.n_str); n_hits += int(hp.contents.n_hits)
                L.mm355_free_hits(hp)
            dt = time.perf_counter() - t0
            if p:
                rates.append(round(bases / dt / 1e6, 1)); kt.append(round(kt_pass, 3))
        res = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "spread_percent": round(100.0 * (max(rates) - min(rates)) / median(rates), 2),
               "kt_extra_ms_per_pass": median(kt), "kt_extra_ms_passes": kt, "n_hits": n_hits, "string_bytes": str_bytes, "string_bytes_per_base": round(str_bytes / bases, 4)}
    else:
        al.enable_threading(args.threads)
        out = args.fq + "." + args.child + ".paf"
        rates = []
        for p in range(args.passes + 1):
            t0 = time.perf_counter()
            r = al.map_file(args.fq, out, cs="long" if args.child == "file_long" else True)
            dt = time.perf_counter() - t0
            if p:
                rates.append(round(bases / dt / 1e6, 1))
        res = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "spread_percent": round(100.0 * (max(rates) - min(rates)) / median(rates), 2),
               "bytes_out": os.path.getsize(out), "n_lines": r["n_lines"], "n_sub_batches": r["n_sub_batches"], "sub_batches_on_device": r["n_on_device"]}
        os.unlink(out)
    res.update(n_reads=len(reads), bases=bases)
    print("RESULT " + json.dumps(res), flush=True)


def phases(path, n_passes):
    """mean per pass of the x:walk / x:strings phases of an MM355_TRACE timeline (lines: context, phase, start ms, end ms)"""
    tot = {"x:walk": 0.0, "x:strings": 0.0}
    with open(path) as f:
        for line in f:
            w = line.replace(",", " ").split()
            for k in tot:
                if k in w:
                    i = w.index(k)
                    tot[k] += float(w[i + 2]) - float(w[i + 1])
    return {k.replace(":", "_") + "_ms_mean_per_pass": round(v / n_passes, 3) for k, v in tot.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4 * SUB)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--ref", default=None)
    ap.add_argument("--fq", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"workload": "bench.py configs[1]: ecoli genome seed 1, map-ont, read set seed 2 (N50 ~8 kb)", "sub_batch_reads": SUB, "passes": args.passes, "threads_map_file": args.threads}
    with tempfile.TemporaryDirectory() as td:
        t0 = time.time()
        ref, fq = world(args.reads, td)
        print("[cslong] genome and %d reads in %.1fs" % (args.reads, time.time() - t0), flush=True)
        for mode in ("none", "short", "long", "file_short", "file_long"):
            trace = os.path.join(td, mode + ".trace")
            env = dict(os.environ, MM355_TRACE=trace)
            env.pop("MM355_EXTRA_HOST", None); env.pop("MM355_EXTRA_MIN_READS", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--ref", ref, "--fq", fq, "--passes", str(args.passes), "--threads", str(args.threads)],
                               env=env, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                raise SystemExit("[cslong] mode %s failed with status %d" % (mode, p.returncode))
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for k in ("n_reads", "bases"):
                res[k] = r.pop(k)
            if not mode.startswith("file") and os.path.exists(trace):
                r.update(phases(trace, args.passes + 1))
            res[mode] = r
            print("[cslong] %s: %s" % (mode, json.dumps(r)), flush=True)
    res["long_over_short"] = {"mbases_per_s": round(res["long"]["mbases_per_s"] / res["short"]["mbases_per_s"], 4),
                              "kt_extra_ms": round(res["long"]["kt_extra_ms_per_pass"] / max(1e-9, res["short"]["kt_extra_ms_per_pass"]), 3),
                              "string_bytes": round(res["long"]["string_bytes"] / max(1, res["short"]["string_bytes"]), 2),
                              "map_file_mbases_per_s": round(res["file_long"]["mbases_per_s"] / res["file_short"]["mbases_per_s"], 4)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
