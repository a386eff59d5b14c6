"""Reads file in, PAF file out: Aligner.map_file with the host and with the device formatter against the route a user had before it --
map_batch + paf_line + file.write -- on the same reads, and the formatting step alone (mm355_text_t::ms_format) over a sweep of batch
sizes, which is where MM355_PAF_AUTO's thresholds come from.

    python tools/paf_bench.py [--reads 73728] [--ava 8192] [--threads 8] [--passes 3] [--out profiles/paf_file.json]

Two settings: `cigar` = bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode with cs;
`ava` = the first --ava of those reads indexed as their own targets, ava-ont chain-only with query names.  Per setting and route: Mbases/s
and lines/s of the whole run (reader, mapping, formatting, writing; median of --passes passes after a warm-up, every pass listed), host CPU
seconds per million reads (process time, all threads), ms_format per sub-batch.  The reads file is plain FASTA (written once, untimed).
The sweep formats the hits of the first n reads with both formatters (median of five calls) and reports the smallest hit count from which
the device stays ahead.  `reader_alone` is the streaming reader over the same file with nothing mapped: the ceiling of map_file's one reader thread."""
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

import synthdata as S  # noqa: E402


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(f, passes):
    """f() -> (n_lines, extra dict); a warm-up, then `passes` passes: wall seconds and process CPU seconds of each"""
    f()
    out = []
    for _ in range(passes):
        c0, t0 = time.process_time(), time.perf_counter()
        n_lines, extra = f()
        out.append((time.perf_counter() - t0, time.process_time() - c0, n_lines, extra))
    return out


def summarise(runs, n_reads, bases):
    rates = [round(bases / r[0] / 1e6, 1) for r in runs]
    res = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "lines_per_s": int(median([r[2] / r[0] for r in runs])),
           "cpu_s_per_million_reads": round(median([r[1] for r in runs]) / n_reads * 1e6, 1), "n_lines": runs[-1][2]}
    res.update(runs[-1][3])
    return res


def routes(al, al_base, reads, names, fa, td, where_of, cs, passes):
    from mappy_rs import paf_line
    n_reads, bases = len(reads), sum(map(len, reads))
    res = {}
    for route, where in where_of.items():
        def run(where=where):
            r = al.map_file(fa, os.path.join(td, "out.paf"), cs=cs, where=where)
            return r["n_lines"], {"ms_format_per_sub_batch": round(r["ms_format"] / r["n_sub_batches"], 2), "n_sub_batches": r["n_sub_batches"],
                                  "sub_batches_on_device": r["n_on_device"]}
        res[route] = summarise(timed(run, passes), n_reads, bases)
        print("[paf] %s: %s" % (route, json.dumps(res[route])), flush=True)
    items = [{"seq": r, "name": n, "len": len(r)} for r, n in zip(reads, names)]      # (in memory already: the baseline pays for no reader)

    def base():
        n = 0
        with open(os.path.join(td, "base.paf"), "w") as f:
            for ms, it in al_base.map_batch(items):
                for m in ms:
                    f.write(paf_line(m, it["name"], it["len"]) + "\n")
                    n += 1
        return n, {}
    res["map_batch_paf_line"] = summarise(timed(base, passes), n_reads, bases)
    print("[paf] map_batch + paf_line: %s" % json.dumps(res["map_batch_paf_line"]), flush=True)
    assert res["map_batch_paf_line"]["n_lines"] == res["host"]["n_lines"] == res["device"]["n_lines"]
    return res


def reader_alone(path, bases, passes):
    """the streaming reader by itself (mm355_fastx_next in map_file's sub-batches, nothing mapped): Mbases/s, every pass"""
    import mappy_rs
    from mappy_rs import _ffi
    L, rates = _ffi.lib(), []
    for _ in range(passes + 1):
        fx = C.c_void_p()
        _ffi.check(L.mm355_fastx_open(path.encode(), C.byref(fx)))
        t0 = time.perf_counter()
        while True:
            rp = C.POINTER(_ffi.Reads)()
            _ffi.check(L.mm355_fastx_next(fx, mappy_rs.SUB_BATCH_READS, mappy_rs.SUB_BATCH_BASES, C.byref(rp)))
            if not rp:
                break
            L.mm355_reads_free(rp)
        rates.append(round(bases / (time.perf_counter() - t0) / 1e6, 1))
        L.mm355_fastx_close(fx)
    return {"mbases_per_s": median(rates[1:]), "mbases_per_s_passes": rates[1:]}


def sweep(al, reads, names, flags, sizes):
    """ms_format of the two formatters on the hits of the first n reads -> rows, and the hit count from which the device stays ahead"""
    from mappy_rs import _ffi
    L, rows = al._L, []
    for n in sizes:
        if n > len(reads):
            break
        packed, narr = _ffi.pack_reads(reads[:n]), _ffi.pack_names(names[:n])
        rc, hp = _ffi.call_map(L, al._context(), al._mo, packed, flags | _ffi.OUT_TAGS, narr, entry="named")
        _ffi.check(rc)
        ms = {}
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            one = []
            for _ in range(6):
                tp = C.POINTER(_ffi.Text)()
                _ffi.check(L.mm355_paf_format(al._context(), C.byref(al._mo), hp, narr, packed.lens, where, C.byref(tp)))
                one.append(tp.contents.ms_format); n_text = int(tp.contents.n_text)
                L.mm355_free_text(tp)
            ms[where] = round(median(one[1:]), 3)
        rows.append({"n_reads": n, "n_hits": int(hp.contents.n_hits), "text_bytes": n_text, "ms_host": ms[_ffi.PAF_HOST], "ms_device": ms[_ffi.PAF_DEVICE]})
        L.mm355_free_hits(hp)
        print("[paf] sweep: %s" % json.dumps(rows[-1]), flush=True)
    cross = None
    for r in reversed(rows):
        if r["ms_device"] >= r["ms_host"]:
            break
        cross = r["n_hits"]
    return rows, cross


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=73728)
    ap.add_argument("--ava", type=int, default=8192)
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
    where_of = {"host": _ffi.PAF_HOST, "device": _ffi.PAF_DEVICE}
    sizes = [16, 64, 256, 1024, 2048, 4096, 9216]
    res = {"threads": args.threads, "passes": args.passes, "sub_batch_reads": mappy_rs.SUB_BATCH_READS}
    with tempfile.TemporaryDirectory() as td:
        ref, fa, ava = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fa"), os.path.join(td, "ava.fa")
        S.write_fasta(ref, g, ["chrE"])
        for path, k in ((fa, len(reads)), (ava, min(args.ava, len(reads)))):
            with open(path, "w") as f:
                f.write("".join(">%s\n%s\n" % (n, r) for n, r in zip(names[:k], reads[:k])))
        print("[paf] genome, %d reads and their files in %.1fs" % (len(reads), time.time() - t0), flush=True)
        # CIGAR mode with cs, bench.py's configs[1]
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al_base = mappy_rs.Aligner(ref, preset="map-ont", tags=True, name_key="name", build_on_gpu=True)
        al.enable_threading(args.threads); al_base.enable_threading(args.threads)
        res["cigar"] = dict(n_reads=len(reads), bases=sum(map(len, reads)), **routes(al, al_base, reads, names, fa, td, where_of, True, args.passes))
        res["cigar"]["format_sweep"], res["cigar"]["device_ahead_from_hits"] = sweep(al, reads, names, _ffi.OUT_CS, sizes)
        res["cigar"]["reader_alone"] = reader_alone(fa, res["cigar"]["bases"], args.passes)
        print("[paf] reader alone: %s" % json.dumps(res["cigar"]["reader_alone"]), flush=True)
        del al, al_base
        # all-vs-all overlaps, chain-only, the read set is its own index
        k = min(args.ava, len(reads))
        al = mappy_rs.Aligner(ava, preset="ava-ont", cigar=False, build_on_gpu=True)
        al_base = mappy_rs.Aligner(ava, preset="ava-ont", cigar=False, tags=True, name_key="name", build_on_gpu=True)
        al.enable_threading(args.threads); al_base.enable_threading(args.threads)
        res["ava"] = dict(n_reads=k, bases=sum(map(len, reads[:k])), **routes(al, al_base, reads[:k], names[:k], ava, td, where_of, False, args.passes))
        res["ava"]["format_sweep"], res["ava"]["device_ahead_from_hits"] = sweep(al, reads[:k], names[:k], 0, [s for s in sizes if s <= k])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
