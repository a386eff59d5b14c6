"""What carrying aux tags costs: Aligner.map_bam_file(compress=True) from an unaligned BAM whose reads carry MM / ML, with and without
copy_tags=True, through the host reader and through the device reader, and k_bam_bulk alone on the largest sub-batch with and without
the tags' third run.

    python tools/aux_bench.py [--reads 73728] [--threads 8] [--passes 3] [--out profiles/bam_aux.json] [--root <tree>] [--off-only]

The protocol is tools/bam_bench.py's: bench.py's configs[1] (ecoli genome seed 1, map-ont, reads N50 ~8 kb of read set seed 2) in CIGAR mode
with cs, one GPU, --threads host threads, the median of --passes passes after a warm-up, every pass listed.  The input is an unaligned BAM
the tool makes itself with Python's zlib (written once, untimed): every read carries a synthetic MM:Z / ML:B:C pair of about half a byte
per base each (random values: what matters here is their size) and RG, MN, qs, ns, ts beside them.  Per route: Mbases/s of the whole run,
bytes out, n_aux_bytes.  The kernel: three device calls of mm355_bam_format_aux on the hits of the largest sub-batch (most bases) with MM355_BAM_TIMES=1,
the library's bam_times line read back from stderr -- k_bam_bulk between two events -- with aux == NULL and with the tags.
--root <tree> imports mappy_rs from another checkout of this repository and --off-only leaves out everything that needs copy_tags: the
parent commit on the same file (the default path must lie inside the parent's pass-to-pass spread: it shares no new work)."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bgzf(data, level=1):
    """`data` as BGZF members of 0xff00 payload bytes and the EOF member"""
    out = []
    for at in range(0, len(data), 0xff00):
        p = data[at:at + 0xff00]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        c = z.compress(p) + z.flush()
        out.append(bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(c) + 25) + c + struct.pack("<II", zlib.crc32(p), len(p)))
    return b"".join(out) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def read_aux(i, n, rng):
    """the tags of read i of n bases: MM and ML of about n / 2 bytes each, and a few scalars"""
    mm = b"C+m?," + rng.integers(0, 10, n // 4).astype("S1").view("S1").tobytes().replace(b"", b",")[1:-1] + b";" if n >= 4 else b"C+m?;"
    ml = rng.integers(0, 256, n // 2, dtype=np.uint8).tobytes()
    return (b"RGZrun1\0" + b"qsf" + struct.pack("<f", 12.5 + i % 7) + b"nsi" + struct.pack("<i", 4000 * n) + b"tsi" + struct.pack("<i", i % 50) +
            b"MMZ" + mm + b"\0" + b"MLBC" + struct.pack("<I", len(ml)) + ml + b"MNi" + struct.pack("<i", n))


def ubam(reads, names, quals, rng):
    """(the uninflated bytes of an unaligned BAM of the reads, every read's aux block)"""
    code = np.full(256, 15, np.uint8)
    for k, c in enumerate(b"=ACMGRSVTWYHKDBN"):
        code[c] = k
    text = b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:run1\tPL:ONT\tSM:synthetic\n"
    out, auxes = [b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", 0)], []
    for i, (r, nm, q) in enumerate(zip(reads, names, quals)):
        n = len(r)
        c = code[np.frombuffer(r.encode(), np.uint8)]
        if n & 1:
            c = np.append(c, np.uint8(0))
        aux = read_aux(i, n, rng)
        auxes.append(aux)
        body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm) + 1, 0, 4680, 0, 4, n, -1, -1, 0) + nm.encode() + b"\0" + (c[0::2] << 4 | c[1::2]).tobytes() + \
            (np.frombuffer(q.encode(), np.uint8) - 33).astype(np.uint8).tobytes() + aux
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out), auxes


def median(xs):
    return sorted(xs)[len(xs) // 2]


def route(al, bam, out, bases, passes, **kw):
    runs = []
    for k in range(passes + 1):                            # (the first pass is the warm-up)
        t0 = time.perf_counter()
        r = al.map_bam_file(bam, out, cs=True, compress=True, **kw)
        runs.append((time.perf_counter() - t0, r))
    rates = [round(bases / t / 1e6, 1) for t, _ in runs[1:]]
    r = runs[-1][1]
    res = {"mbases_per_s": median(rates), "mbases_per_s_passes": rates, "spread_percent": round(100.0 * (max(rates) - min(rates)) / median(rates), 2),
           "bytes_out": os.path.getsize(out), "n_records": r["n_lines"], "n_sub_batches": r["n_sub_batches"], "sub_batches_on_device": r["n_on_device"]}
    if "n_aux_bytes" in r:
        res["n_aux_bytes"] = r["n_aux_bytes"]
    if "reader_on_device" in r:
        res["reader_on_device"] = r["reader_on_device"]
    return res


def bulk_alone(al, reads, names, quals, auxes, n_calls=3):
    """k_bam_bulk's time on the hits of `reads`, aux == NULL and with the tags: the bam_times lines of MM355_BAM_TIMES=1"""
    import mappy_rs
    from mappy_rs import _ffi
    L, n = al._L, len(reads)
    packed, narr = _ffi.pack_reads(reads), _ffi.pack_names(names)
    qb = [q.encode() for q in quals]
    qarr = (C.c_char_p * n)(*qb)
    rc, hp = _ffi.call_map(L, al._context(), al._mo, packed, _ffi.OUT_CS | _ffi.OUT_TAGS, narr, entry="named")
    _ffi.check(rc)
    rl = (C.c_int32 * n)()
    split = [mappy_rs.bam_aux_split(a) for a in auxes]
    bufs = [C.create_string_buffer(k, max(1, len(k))) for k, _ in split]
    ptr = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    ln, md = (C.c_int32 * n)(*[len(k) for k, _ in split]), (C.c_int32 * n)(*[m for _, m in split])
    res = {"n_reads": n, "n_hits": int(hp.contents.n_hits), "aux_bytes": int(sum(len(k) for k, _ in split))}
    for label, args in (("no_aux", (None, None, None)), ("aux", (ptr, ln, md))):
        def call():
            tp = C.POINTER(_ffi.Text)()
            _ffi.check(L.mm355_bam_format_aux(al._context(), C.byref(al._mo), hp, narr, packed.arr, packed.lens, qarr, rl, *args, 0, _ffi.PAF_DEVICE, 0, C.byref(tp)))
            n_text = int(tp.contents.n_text)
            L.mm355_free_text(tp)
            return n_text
        call()
        rows = []
        with tempfile.TemporaryFile() as tf:
            sys.stderr.flush()
            saved = os.dup(2)
            os.environ["MM355_BAM_TIMES"] = "1"
            try:
                os.dup2(tf.fileno(), 2)
                for _ in range(n_calls):
                    n_text = call()
            finally:
                os.dup2(saved, 2); os.close(saved)
                del os.environ["MM355_BAM_TIMES"]
            tf.seek(0)
            for line in tf.read().decode().splitlines():
                f = line.split()
                if f[:2] == ["[mm355]", "bam_times"]:
                    rows.append({f[i]: float(f[i + 1]) for i in range(2, len(f), 2)})
        assert len(rows) == n_calls, rows
        us = [r["k_bam_bulk_us"] for r in rows]
        res[label] = {"k_bam_bulk_us": median(us), "k_bam_bulk_us_calls": us, "tiles": int(rows[0]["tiles"]), "records": int(rows[0]["records"]), "output_bytes": n_text}
    L.mm355_free_hits(hp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=73728)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, "mappy-rs_amd"))
    import synthdata as S
    import mappy_rs
    t0 = time.time()
    g = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01)))
    reads, _ = S.make_reads(2, g, args.reads, n50=8000, sigma=0.75, lo=500, hi=100000)
    names = ["read%06d" % i for i in range(len(reads))]
    pat = "".join(chr(35 + (7 * j) % 40) for j in range(101000))
    quals = [pat[i % 1000:i % 1000 + len(r)] for i, r in enumerate(reads)]
    bases = sum(map(len, reads))
    res = {"tree": os.path.relpath(args.root, ROOT), "threads": args.threads, "passes": args.passes, "sub_batch_reads": mappy_rs.SUB_BATCH_READS, "n_reads": len(reads), "bases": bases}
    with tempfile.TemporaryDirectory() as td:
        ref, bam, out = os.path.join(td, "ref.fa"), os.path.join(td, "calls.bam"), os.path.join(td, "out.bam")
        S.write_fasta(ref, g, ["chrE"])
        blob, auxes = ubam(reads, names, quals, np.random.default_rng(5))
        with open(bam, "wb") as f:
            f.write(bgzf(blob))
        res.update(input_bam_bytes=os.path.getsize(bam), input_aux_bytes=sum(map(len, auxes)), input_aux_bytes_per_base=round(sum(map(len, auxes)) / bases, 3))
        del blob
        print("[aux] genome, %d reads and their BAM in %.1fs" % (len(reads), time.time() - t0), flush=True)
        al = mappy_rs.Aligner(ref, preset="map-ont", build_on_gpu=True)
        al.enable_threading(args.threads)
        variants = [("host_reader_no_tags", {}), ("device_reader_no_tags", dict(read_on_gpu=True))]
        if not args.off_only:
            variants += [("host_reader_copy_tags", dict(copy_tags=True)), ("device_reader_copy_tags", dict(read_on_gpu=True, copy_tags=True))]
        for name, kw in variants:
            res[name] = route(al, bam, out, bases, args.passes, **kw)
            print("[aux] %s: %s" % (name, json.dumps(res[name])), flush=True)
        if not args.off_only:
            n = mappy_rs.SUB_BATCH_READS                   # the sub-batch of n consecutive reads with the most bases
            a = max(range(0, len(reads), n), key=lambda k: sum(map(len, reads[k:k + n])))
            res["k_bam_bulk_alone"] = bulk_alone(al, reads[a:a + n], names[a:a + n], quals[a:a + n], auxes[a:a + n])
            res["k_bam_bulk_alone"]["first_read"] = a
            print("[aux] k_bam_bulk alone: %s" % json.dumps(res["k_bam_bulk_alone"]), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
