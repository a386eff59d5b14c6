"""Compressed reads in: the device inflater (read_on_gpu=True: mm355_fastx_open_device, k_bgzf_inflate) against the host reader ON THE SAME
FILE -- the parent's code path, unchanged -- for a FASTQ as a plain file, a plain .gz, BGZF (what bgzip writes) and unaligned BAM.

    python tools/inflate_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/bgzf_inflate.json]

The protocol is tools/bam_bench.py's: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode
with cs, one GPU, median of --passes passes after a warm-up, every pass listed.  The files are made here with Python's zlib at level 6 (no
bgzip or samtools is assumed), untimed: BGZF members of 0xff00 payload bytes as htslib cuts them, the .gz one deflate stream.  Two quality
sets: the periodic pattern of tools/sam_bench.py, which flatters any LZ77, and qualities drawn at random from 40 values.  Reported:
  k_bgzf_inflate   the kernel alone between two events (MM355_INFLATE_TIMES=1) on the first 32 MB of whole members of each BGZF file through
                   mm355_bgzf_inflate: microseconds, GB/s of output
  reader_alone     mm355_fastx_open* + mm355_fastx_next until the end, nothing mapped: Mbases/s and MB of file per second, per file, through
                   the host and (BGZF files) through the device
  map_file, map_bam_file_compress   end to end per file and reader
Not measured: real basecaller output (its qualities and names compress differently), files on a cold page cache (the files were written a
moment ago), more than one GPU."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mappy-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthdata as S  # noqa: E402
from paf_bench import median, timed  # noqa: E402

P = 0xff00
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_NIB = np.full(256, 15, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    _NIB[_c] = _i


def _member(p):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = c.compress(p) + c.flush()
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(p), len(p))


def write_bgzf(path, data, pool):
    with open(path, "wb") as f:
        for m in pool.map(_member, (data[i:i + P] for i in range(0, len(data), P))):
            f.write(m)
        f.write(EOF)


def write_gz(path, data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(path, "wb") as f:
        for i in range(0, len(data), 1 << 24):
            f.write(c.compress(data[i:i + (1 << 24)]))
        f.write(c.flush())


def ubam(names, reads, quals):
    out = [b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 0)]
    for n, r, q in zip(names, reads, quals):
        codes = _NIB[np.frombuffer(r.encode(), np.uint8)]
        if len(codes) & 1:
            codes = np.append(codes, np.uint8(0))
        nm = n.encode() + b"\0"
        body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm), 0, 4680, 0, 4, len(r), -1, -1, 0) + nm + (codes[0::2] << 4 | codes[1::2]).tobytes() + \
            (np.frombuffer(q.encode(), np.uint8) - 33).astype(np.uint8).tobytes()
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out)


def reader_alone(path, device, sub_batch_reads, sub_batch_bases):
    """the file through the streaming reader, nothing else: (reads, bases), or None when the device open says the file is not BGZF"""
    from mappy_rs import _ffi
    L = _ffi.lib()
    fx = C.c_void_p()
    rc = L.mm355_fastx_open_device(os.fsencode(path), 1, 0, C.byref(fx)) if device else L.mm355_fastx_open_qual(os.fsencode(path), C.byref(fx))
    if device and rc == _ffi.MM355_EINVAL:
        return None
    _ffi.check(rc)
    n = b = 0
    try:
        while True:
            rp = C.POINTER(_ffi.Reads)()
            _ffi.check(L.mm355_fastx_next(fx, sub_batch_reads, sub_batch_bases, C.byref(rp)))
            if not rp:
                return n, b
            k = int(rp.contents.n)
            n += k
            b += int(np.ctypeslib.as_array(rp.contents.lens, shape=(k,)).sum(dtype=np.int64))
            L.mm355_reads_free(rp)
    finally:
        L.mm355_fastx_close(fx)


def kernel_alone(al, path, n=3):
    """mm355_bgzf_inflate on the device over the first 32 MB of whole members, MM355_INFLATE_TIMES=1: the medians of the library's lines"""
    from mappy_rs import _ffi
    data = open(path, "rb").read(32 << 20)
    at = 0
    while at + 18 <= len(data) and at + struct.unpack_from("<H", data, at + 16)[0] + 1 <= len(data):
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    data = data[:at]
    rows = []
    with tempfile.TemporaryFile() as tf:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["MM355_INFLATE_TIMES"] = "1"
        try:
            os.dup2(tf.fileno(), 2)
            for _ in range(n + 1):
                tp = C.POINTER(_ffi.Text)()
                _ffi.check(al._L.mm355_bgzf_inflate(al._context(), data, len(data), _ffi.PAF_DEVICE, C.byref(tp)))
                al._L.mm355_free_text(tp)
        finally:
            os.dup2(saved, 2); os.close(saved)
            del os.environ["MM355_INFLATE_TIMES"]
        tf.seek(0)
        for ln in tf.read().decode().splitlines():
            f = ln.split()
            if f[:2] == ["[mm355]", "bgzf_inflate_times"]:
                rows.append({f[i]: float(f[i + 1]) for i in range(3, len(f), 2)})
    assert len(rows) == n + 1, rows
    rows = rows[1:]                                        # (the first call allocates)
    us = median([r["k_bgzf_inflate_us"] for r in rows])
    return {"k_bgzf_inflate_us": us, "k_bgzf_inflate_us_calls": [r["k_bgzf_inflate_us"] for r in rows], "blocks": int(rows[0]["blocks"]),
            "bytes_in": int(rows[0]["bytes_in"]), "bytes_out": int(rows[0]["bytes_out"]), "output_gb_per_s": round(rows[0]["bytes_out"] / us / 1e3, 2)}


def rate(runs, bases, file_bytes):
    r = [round(bases / t[0] / 1e6, 1) for t in runs]
    return {"mbases_per_s": median(r), "mbases_per_s_passes": r, "file_mb_per_s": round(file_bytes / median([t[0] for t in runs]) / 1e6, 1),
            "cpu_s": round(median([t[1] for t in runs]), 2)}


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
    bases = sum(map(len, reads))
    pat = "".join(chr(35 + (7 * j) % 40) for j in range(101000))
    rng = np.random.default_rng(3)
    quals = {"periodic": [pat[i % 1000:i % 1000 + len(r)] for i, r in enumerate(reads)],
             "random40": [(rng.integers(0, 40, len(r), dtype=np.uint8) + 35).tobytes().decode() for r in reads]}
    res = {"threads": args.threads, "passes": args.passes, "sub_batch_reads": mappy_rs.SUB_BATCH_READS, "n_reads": len(reads), "bases": bases,
           "zlib_level": 6, "comparator": "the host reader on the same file", "files": {}, "k_bgzf_inflate": {}}
    with tempfile.TemporaryDirectory() as td:
        ref = os.path.join(td, "ref.fa")
        S.write_fasta(ref, g, ["chrE"])
        files = {}
        with ThreadPoolExecutor(16) as pool:
            jobs = []
            for qn, qs in quals.items():
                text = "".join("@%s\n%s\n+\n%s\n" % t for t in zip(names, reads, qs)).encode()
                paths = {k: os.path.join(td, "%s.%s" % (qn, ext)) for k, ext in (("plain", "fq"), ("gz", "fq.gz"), ("bgzf", "bgzf.fq.gz"), ("ubam", "bam"))}
                open(paths["plain"], "wb").write(text)
                jobs.append(pool.submit(write_gz, paths["gz"], text))
                write_bgzf(paths["bgzf"], text, pool)
                write_bgzf(paths["ubam"], ubam(names, reads, qs), pool)
                files.update({"%s_%s" % (qn, k): p for k, p in paths.items()})
            for j in jobs:
                j.result()
        print("[inflate] genome, %d reads and %d files in %.1fs" % (len(reads), len(files), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al.enable_threading(args.threads)
        for name, path in files.items():
            if name.endswith("bgzf") or name.endswith("ubam"):
                res["k_bgzf_inflate"][name] = kernel_alone(al, path)
                print("[inflate] k_bgzf_inflate %s: %s" % (name, json.dumps(res["k_bgzf_inflate"][name])), flush=True)
        for name, path in files.items():
            size = os.path.getsize(path)
            row = {"file_bytes": size, "bytes_per_base": round(size / bases, 3), "reader_alone": {}, "map_file": {}, "map_bam_file_compress": {}}
            for who, dev in (("host", False), ("device", True)):
                if dev and reader_alone(path, True, 1, 1 << 20) is None:
                    for k in ("reader_alone", "map_file", "map_bam_file_compress"):
                        row[k]["device"] = "not BGZF: the host reader"
                    continue

                def rd(dev=dev):
                    n, b = reader_alone(path, dev, mappy_rs.SUB_BATCH_READS, mappy_rs.SUB_BATCH_BASES)
                    assert (n, b) == (len(reads), bases), (n, b)
                    return n, {}
                row["reader_alone"][who] = rate(timed(rd, args.passes), bases, size)
                for key, call in (("map_file", lambda o, dev=dev: al.map_file(path, o, cs=True, read_on_gpu=dev)),
                                  ("map_bam_file_compress", lambda o, dev=dev: al.map_bam_file(path, o, cs=True, compress=True, read_on_gpu=dev))):
                    out = os.path.join(td, "out.bin")

                    def run(call=call, out=out, dev=dev):
                        r = call(out)
                        assert r["n_reads"] == len(reads) and r.get("reader_on_device", False) == dev
                        return r["n_lines"], {}
                    row[key][who] = rate(timed(run, args.passes), bases, size)
            res["files"][name] = row
            print("[inflate] %s: %s" % (name, json.dumps(row)), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
