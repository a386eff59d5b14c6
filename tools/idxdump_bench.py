"""Index build, .mmi save and .mmi load, host against GPU, wall times of the Python calls a user makes:

    Aligner(fa)                          the host build (mm355_index_load: parse, sketch on host threads, one std::sort, table fill)
    Aligner(fa, build_on_gpu=True)       the same FASTA built on the device (mm355_index_load_device)
    save_index() of the device index     mm355_idxdump.hip: conversion in HBM, pieces to the host, file
    save_index() of the host index       the host producer of mm355_index.cpp

and three legs timed until the index is usable in HBM, that is until mm355_upload([0]) -- the load or build plus the replica on device 0 --
has returned (written to profiles/index_load.json):

    Aligner(mmi)                         the host loader (one fread per pair, a host table, then the H2D copy of table, pos[] and sequence)
    Aligner(mmi, load_on_gpu=True)       mm355_idxload.hip: the file in pieces to the device, the table filled there
    Aligner(fa, build_on_gpu=True)       for comparison: the device build of the same reference, timed the same way

The .mmi is read right after it was written: the page cache is warm, no leg waits for a disk.

The device save is timed twice, into a file and into /dev/null; the difference is the file's share of the time.  The two files must be
equal byte for byte (checked).  A tiny device build runs first so that loading the HIP runtime and the code object is not charged to the
first timed call (reported as runtime_warmup_s).  Every leg is run --reps times; all passes are kept, the median is the figure.

    python tools/idxdump_bench.py [--workload ecoli|mid|both] [--reps 3] [--threads 3] [--out profiles/index_dump.json]
                                  [--load-out profiles/index_load.json]

ecoli: bench.py's configs[1] genome (4.64 Mbp, seed 1).  mid: the 155-Mbp human-like genome of the mid-scale tools (make_human_like(3, 0.05))."""
import argparse
import filecmp
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mappy-rs_amd"))

import synthdata as S  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def in_hbm(make):
    """make() -> Aligner; the time until its index is usable on device 0"""
    import ctypes as C

    def go():
        al = make()
        rc = al._L.mm355_upload(al._idx, (C.c_int32 * 1)(0), 1)
        assert rc == 0, rc
        return al
    return timed(go)


def load_legs(fa, mmi, reps):
    """the three legs that end with the index in HBM; `mmi` was written a moment ago (page cache warm)"""
    import mappy_rs
    out = {k: [] for k in ("host_load_in_hbm_s", "device_load_in_hbm_s", "gpu_build_in_hbm_s")}
    for _ in range(reps):
        dt, host = in_hbm(lambda: mappy_rs.Aligner(mmi, preset="map-ont"))
        out["host_load_in_hbm_s"].append(dt)
        dt, dev = in_hbm(lambda: mappy_rs.Aligner(mmi, preset="map-ont", load_on_gpu=True))
        out["device_load_in_hbm_s"].append(dt)
        dt, built = in_hbm(lambda: mappy_rs.Aligner(fa, preset="map-ont", build_on_gpu=True))
        out["gpu_build_in_hbm_s"].append(dt)
        assert dev._L.mm355_index_get(dev._idx, 0, None, 0) == -7 and host._L.mm355_index_get(host._idx, 0, None, 0) >= 0   # MM355_EUNSUP: device-resident
        del host, dev, built
    res = {"passes": out, "mmi_bytes": os.path.getsize(mmi)}
    for k, v in out.items():
        res[k] = statistics.median(v)
    return res


def legs(fa, td, reps, threads):
    import mappy_rs
    out = {k: [] for k in ("host_build_s", "gpu_build_s", "device_save_s", "device_save_devnull_s", "host_save_s")}
    f_dev, f_host = os.path.join(td, "dev.mmi"), os.path.join(td, "host.mmi")
    for _ in range(reps):
        dt, host = timed(lambda: mappy_rs.Aligner(fa, preset="map-ont", n_threads=threads))
        out["host_build_s"].append(dt)
        dt, dev = timed(lambda: mappy_rs.Aligner(fa, preset="map-ont", build_on_gpu=True))
        out["gpu_build_s"].append(dt)
        out["device_save_s"].append(timed(lambda: dev.save_index(f_dev))[0])
        out["device_save_devnull_s"].append(timed(lambda: dev.save_index("/dev/null"))[0])
        out["host_save_s"].append(timed(lambda: host.save_index(f_host))[0])
        assert filecmp.cmp(f_dev, f_host, shallow=False), "device and host producers wrote different files"
        size = os.path.getsize(f_dev)
        del host, dev
    res = {"passes": out, "mmi_bytes": size}
    for k, v in out.items():
        res[k] = statistics.median(v)
    res["device_save_file_write_share"] = max(0.0, 1.0 - res["device_save_devnull_s"] / res["device_save_s"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=("ecoli", "mid", "both"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=3, help="n_threads of the host build (the Aligner default is 3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_dump.json"))
    ap.add_argument("--load-out", default=os.path.join(ROOT, "profiles", "index_load.json"))
    args = ap.parse_args()
    import mappy_rs
    from mappy_rs import _ffi
    if _ffi.lib().mm355_device_count() < 1:
        sys.exit("idxdump_bench: no GPU (nothing is measured without one)")
    loads = {"tool": "tools/idxdump_bench.py", "reps": args.reps, "preset": "map-ont (k15 w10)", "page_cache": "warm: every .mmi is read right after it was written",
             "until": "mm355_upload([0]) has returned: load or build plus the replica on device 0", "workloads": {}}
    result = {"tool": "tools/idxdump_bench.py", "reps": args.reps, "host_build_threads": args.threads, "preset": "map-ont (k15 w10)", "workloads": {}}
    with tempfile.TemporaryDirectory() as td:
        tiny = os.path.join(td, "tiny.fa")
        S.write_fasta(tiny, S.make_genome(9, [20000], repeats=()), ["t"])
        result["runtime_warmup_s"] = timed(lambda: mappy_rs.Aligner(tiny, build_on_gpu=True).save_index(os.path.join(td, "tiny.mmi")))[0]
        for wl in (("ecoli", "mid") if args.workload == "both" else (args.workload,)):
            if wl == "ecoli":
                g, names, what = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01))), ["chrE"], "bench.py configs[1]: synthetic 4.64 Mbp genome (seed 1)"
            else:
                g, names = S.make_human_like(3, 0.05)
                what = "synthetic human-like genome, make_human_like(3, 0.05)"
            fa = os.path.join(td, wl + ".fa")
            S.write_fasta(fa, g, names)
            r = legs(fa, td, args.reps, args.threads)
            r["reference"] = what
            r["bases"] = int(sum(len(c) for c in g))
            result["workloads"][wl] = r
            print("[idxdump_bench] %s: host build %.3f s, GPU build %.3f s, device save %.3f s (file share %.0f %%), host save %.3f s, %d bytes" % (
                wl, r["host_build_s"], r["gpu_build_s"], r["device_save_s"], 100 * r["device_save_file_write_share"], r["host_save_s"], r["mmi_bytes"]), flush=True)
            ld = load_legs(fa, os.path.join(td, "dev.mmi"), args.reps)
            ld["reference"], ld["bases"] = what, r["bases"]
            loads["workloads"][wl] = ld
            print("[idxdump_bench] %s, until in HBM: host load %.3f s, device load %.3f s, GPU build %.3f s" % (
                wl, ld["host_load_in_hbm_s"], ld["device_load_in_hbm_s"], ld["gpu_build_in_hbm_s"]), flush=True)
            os.remove(fa)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    with open(args.load_out, "w") as f:
        json.dump(loads, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "workloads"}))


if __name__ == "__main__":
    main()
