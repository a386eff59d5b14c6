"""Chain-only mapping (no MM_F_CIGAR) against the CIGAR path on the same resident sub-batches: Mbases/s of mm355_map_resident, ms per
sub-batch, reads whose region logic ran on the device / on the host, the region kernel's time (mm355_stats_t::ms_kernel[23]) next to the
other kernels of the chain-only call (ms_kernel, the rest), and a sample of reads checked against the oracle (flag &= ~4).  One context,
sub-batches of SUB reads, timed after a warm-up; the index is built on the device (as bench.py does).

    python tools/chainonly_bench.py --workload ecoli [--preset map-ont] [--reads 18432] [--sub 9216] [--n50 N --lo L --hi H] [--out F]
                                    [--tags] [--reps R]

--tags adds a third leg: chain-only with MM355_OUT_TAGS (the tags rows of every hit come back as well).  --reps R times every leg R times
and reports each pass (the spread between passes is what a difference between two builds has to exceed); the rate is the median pass.

ecoli: bench.py's configs[1] genome and read model; human: its configs[2] genome (make_human_like, seed 3, --scale 1) and read model.
--n50 / --lo / --hi override the read lengths (e.g. 150 kb - 1 Mb reads).

    python tools/chainonly_bench.py --ava 8192 [--workload ecoli] [--preset ava-ont] [--reps R] [--out F]

--ava N is the read-vs-read mode: the first N reads of the read set are indexed as their own targets (contig names r0, r1 ...) and mapped
chain-only against that index as ONE resident batch, once without names (mm355_batch_upload: every read hits itself and every pair is
reported from both sides) and once with them (mm355_batch_upload_named: skip_seed's NO_DIAG / NO_DUAL filter on the device).  Reported for
both: Mbases/s of mm355_map_resident (median pass), hits, anchors generated (n_a), and ms_kernel[3] / [4] (k_seed_select, k_seed_expand)
next to the sum of the other kernels."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mappy-rs_amd"))

import numpy as np  # noqa: E402

import synthdata as S  # noqa: E402

READS = {"ecoli": (2, dict(n50=8000, sigma=0.75, lo=500, hi=100000)), "human": (4, dict(n50=10000, sigma=0.75, lo=500, hi=100000))}


def timed_resident(L, ctx, mo, packed, flags):
    """mm355_map_resident on the context's current batch: (seconds of the call alone, the HitsView of its record)"""
    from mappy_rs import _ffi
    t = time.perf_counter()
    rc, hp = _ffi.call_map(L, ctx, mo, packed, flags, entry="current")
    dt = time.perf_counter() - t
    _ffi.check(rc)
    return dt, _ffi.take_hits(L, hp, len(packed.keep))


def ava_main(args):
    from mappy_rs import _ffi
    L = _ffi.lib()
    t0 = time.time()
    g = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01))) if args.workload == "ecoli" else S.make_human_like(3, args.scale)[0]
    seed, kw = READS[args.workload]
    reads, _ = S.make_reads(seed, g, args.ava, **kw)
    names = ["r%d" % i for i in range(len(reads))]
    preset = args.preset if args.preset.startswith("ava") else "ava-ont"
    io, mo = _ffi.IdxOpt(), _ffi.MapOpt()
    L.mm355_set_opt(None, C.byref(io), C.byref(mo))
    _ffi.check(L.mm355_set_opt(preset.encode(), C.byref(io), C.byref(mo)))
    packed = arr, rl, keep = _ffi.pack_reads(reads)
    narr = _ffi.pack_names(names)
    lens64 = (C.c_int64 * len(reads))(*[len(r) for r in reads])
    idx = C.c_void_p()
    _ffi.check(L.mm355_index_build(C.byref(io), len(reads), arr, lens64, narr, 16, C.byref(idx)))
    L.mm355_mapopt_update(C.byref(mo), idx)
    mo.flag &= ~4
    ctx = C.c_void_p()
    _ffi.check(L.mm355_ctx_create(idx, 0, C.byref(ctx)))
    bases = int(sum(map(len, reads)))
    print("[ava] %d reads, %.1f Mbases, index built in %.1fs" % (len(reads), bases / 1e6, time.time() - t0), flush=True)
    res = {"mode": "read-vs-read", "workload": args.workload, "preset": preset, "n_reads": len(reads), "bases": bases, "mid_occ": int(mo.mid_occ)}
    for leg in ("unnamed", "named"):
        if leg == "named":
            _ffi.check(L.mm355_batch_upload_named(ctx, len(reads), arr, rl, narr))
        else:
            _ffi.check(L.mm355_batch_upload(ctx, len(reads), arr, rl))
        rates = []
        for rep in range(max(1, args.reps) + 1):                  # the first pass is the warm-up
            dt, v = timed_resident(L, ctx, mo, packed, 0)
            n_hits = len(v.hits)
            if rep:
                rates.append(round(bases / dt / 1e6, 1))
        st = _ffi.get_stats(L, ctx)
        res[leg] = {"mbases_per_s": sorted(rates)[len(rates) // 2], "mbases_per_s_passes": rates, "n_hits": n_hits, "n_a": int(st.n_a),
                    "n_a_kept": int(st.n_a_kept), "ms_k_seed_select": round(st.ms_kernel[3], 3), "ms_k_seed_expand": round(st.ms_kernel[4], 3),
                    "ms_other_kernels": round(sum(st.ms_kernel[:3]) + sum(st.ms_kernel[5:]), 3), "ms_total": round(st.ms_total, 1),
                    "n_regs_dev": int(st.n_regs_dev), "n_regs_host": int(st.n_regs_host)}
        print("[ava] %s: %s" % (leg, json.dumps(res[leg])), flush=True)
    res["ratio_named_to_unnamed"] = round(res["named"]["mbases_per_s"] / res["unnamed"]["mbases_per_s"], 2)
    L.mm355_ctx_destroy(ctx); L.mm355_index_free(idx)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ecoli", choices=sorted(READS))
    ap.add_argument("--preset", default="map-ont")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reads", type=int, default=18432)
    ap.add_argument("--sub", type=int, default=9216)
    ap.add_argument("--n50", type=int, default=None)
    ap.add_argument("--lo", type=int, default=None)
    ap.add_argument("--hi", type=int, default=None)
    ap.add_argument("--check", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tags", action="store_true")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--ava", type=int, default=0, help="read-vs-read mode over the first N reads, with and without query names")
    args = ap.parse_args()
    if args.ava > 0:
        return ava_main(args)
    import mappy_rs
    from mappy_rs import _ffi
    from oracle import oracle as O
    L = _ffi.lib()
    t0 = time.time()
    if args.workload == "ecoli":
        g, names = S.make_genome(1, [4641652], gc=0.508, repeats=((5000, 7, 0.01), (1300, 20, 0.01))), ["chrE"]
    else:
        g, names = S.make_human_like(3, args.scale)
    seed, kw = READS[args.workload]
    kw = dict(kw)
    for k in ("n50", "lo", "hi"):
        if getattr(args, k) is not None:
            kw[k] = getattr(args, k)
    reads, _ = S.make_reads(seed, g, args.reads, **kw)
    print("[chainonly] genome + %d reads in %.1fs" % (len(reads), time.time() - t0), flush=True)
    io, mo0 = _ffi.IdxOpt(), _ffi.MapOpt()
    L.mm355_set_opt(None, C.byref(io), C.byref(mo0))
    _ffi.check(L.mm355_set_opt(args.preset.encode(), C.byref(io), C.byref(mo0)))
    ptrs = (C.c_char_p * len(g))(*[C.cast(c.ctypes.data, C.c_char_p) for c in g])
    lens = (C.c_int64 * len(g))(*[len(c) for c in g]); nm = (C.c_char_p * len(g))(*[n.encode() for n in names])
    idx = C.c_void_p()
    _ffi.check(L.mm355_index_build_device(C.byref(io), len(g), ptrs, lens, nm, 0, C.byref(idx)))
    L.mm355_mapopt_update(C.byref(mo0), idx)
    ctx = C.c_void_p()
    _ffi.check(L.mm355_ctx_create(idx, 0, C.byref(ctx)))
    res = {"workload": args.workload, "preset": args.preset, "scale": args.scale, "read_model": kw, "n_reads": len(reads),
           "sub_batch": args.sub, "bases": int(sum(map(len, reads)))}
    subs = [reads[i:i + args.sub] for i in range(0, len(reads), args.sub)]
    packed = [_ffi.pack_reads(sb) for sb in subs]
    for j, pk in enumerate(packed):
        _ffi.check(L.mm355_batch_select(ctx, j)); _ffi.check(L.mm355_batch_upload(ctx, len(pk.keep), pk.arr, pk.lens))
    names_l = list(names)
    for mode in ("cigar", "chain_only") + (("chain_only_tags",) if args.tags else ()):
        mo = _ffi.MapOpt.from_buffer_copy(mo0)
        if mode == "cigar":
            mo.flag |= 4
        flags = _ffi.OUT_CS if mode == "cigar" else _ffi.OUT_TAGS if mode == "chain_only_tags" else 0
        _ffi.check(L.mm355_batch_select(ctx, 0)); timed_resident(L, ctx, mo, packed[0], flags)   # warm-up
        rates = []
        for _rep in range(max(1, args.reps) - 1):      # the earlier passes: rate only, wall clock over the whole pass (select and release included)
            t = time.perf_counter()
            for j in range(len(subs)):
                _ffi.check(L.mm355_batch_select(ctx, j)); timed_resident(L, ctx, mo, packed[j], flags)
            rates.append(round(res["bases"] / (time.perf_counter() - t) / 1e6, 1))
        ms, n_dev, n_host, k_regs, k_other, n_hits = [], 0, 0, 0.0, 0.0, 0
        for j, sb in enumerate(subs):
            _ffi.check(L.mm355_batch_select(ctx, j))
            dt, v = timed_resident(L, ctx, mo, packed[j], flags)
            ms.append(dt * 1e3)
            n_hits += len(v.hits)
            if mode == "chain_only" and j == 0 and args.check:
                first = mappy_rs._batch_to_mappings(v, len(sb), names_l, chain_only=True)
            st = _ffi.get_stats(L, ctx)
            n_dev += st.n_regs_dev; n_host += st.n_regs_host; k_regs += st.ms_kernel[23]; k_other += sum(st.ms_kernel[:23])
        tot_s = sum(ms) / 1e3
        rates.append(round(res["bases"] / tot_s / 1e6, 1))
        res[mode] = {"mbases_per_s": sorted(rates)[len(rates) // 2], "ms_per_sub_batch": [round(x, 1) for x in ms], "n_hits": n_hits}
        if len(rates) > 1:
            res[mode]["mbases_per_s_passes"] = rates
        if mode != "cigar":
            res[mode].update(n_regs_dev=n_dev, n_regs_host=n_host, ms_k_regs_per_sub_batch=round(k_regs / len(subs), 3),
                             ms_other_kernels_per_sub_batch=round(k_other / len(subs), 3))
            if args.check and mode == "chain_only":
                orc = O.OracleAligner(preset=args.preset, codes=g, names=names, n_threads=16)
                orc.mo.flag &= ~4
                bad = 0
                for rd, gm in zip(subs[0][:args.check], first):
                    exp = orc.map(rd)
                    if [(m.ctg, m.r_st, m.r_en, m.q_st, m.q_en, m.strand, m.mlen, m.blen, m.mapq, m.is_primary) for m in gm] != \
                            [(e["target_name"], e["target_start"], e["target_end"], e["query_start"], e["query_end"], e["strand"],
                              e["match_len"], e["block_len"], e["mapq"], e["is_primary"]) for e in exp]:
                        bad += 1
                res[mode].update(checked=min(args.check, len(subs[0])), mismatching=bad)
        print("[chainonly] %s: %s" % (mode, json.dumps(res[mode])), flush=True)
    res["ratio_chain_only_to_cigar"] = round(res["chain_only"]["mbases_per_s"] / res["cigar"]["mbases_per_s"], 2)
    L.mm355_ctx_destroy(ctx); L.mm355_index_free(idx)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
