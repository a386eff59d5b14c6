"""The merge step of compressed runs on the host: the plan and the host step of mappy-rs_amd/csrc/mm355_bammerge.h, built with g++ under
AddressSanitizer and UBSan into a stand-alone program (tests/host_harness/bammerge_host.cpp), against the model of tests/_bammerge.py (zlib,
slices, a cut at 0xff00) -- every step and every refusal -- and, in process through the library, mm355_bam_merge_step with the host `where`:
the blocks inflate to `carry + gathered records` and are mm355_bgzf_deflate / mm355_bgzf_wrap of that stream byte for byte.
GPU side: tests/test_gpu_bammerge.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _bammerge as M
import _capi

P = M.P


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bammerge_host") / "bammerge_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "bammerge_host.cpp"), "-o", exe, "-lpthread", "-lz"])
    return exe


@pytest.fixture(scope="module")
def all_steps():
    """label -> (Step, the model's (raw bytes of the blocks, leftover)); computed once"""
    return {k: (s, M.model(s)) for k, s in M.steps().items()}


def _case(s):
    sa, sb, sr, rs, ra, rl = s.arrays()
    return (struct.pack("<7q", len(s.spool), len(sa), len(rs), len(s.carry), len(s.carry), int(s.final), s.level) + sa.tobytes() + sb.tobytes() + sr.tobytes()
            + rs.tobytes() + ra.tobytes() + rl.tobytes() + s.carry + s.spool)


def _run(exe, mode, blob, tmp_path, tag):
    src, dst = tmp_path / (tag + ".bin"), tmp_path / (tag + ".out")
    src.write_bytes(blob)
    r = subprocess.run([exe, mode, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split(), dst.read_bytes()


def _results(got, n):
    out, at = [], 0
    for _ in range(n):
        rc, n_text, n_blocks, n_left = struct.unpack_from("<iqqq", got, at)
        at += 28
        out.append((rc, got[at:at + n_text], n_blocks, got[at + n_text:at + n_text + n_left]))
        at += n_text + n_left
    assert at == len(got)
    return out


def check_blocks(label, blocks, n_blocks, left, want, level):
    """the blocks of a step against the model: they inflate to the raw bytes, member b holds payload b, stored at level 0"""
    raw, want_left = want
    ps = M.members(blocks)
    assert b"".join(ps) == raw and left == want_left, label
    assert [len(p) for p in ps] == [min(P, len(raw) - at) for at in range(0, len(raw), P)] and n_blocks == len(ps), label
    if level == 0:
        assert len(blocks) == len(raw) + 31 * len(ps), label
    else:
        assert len(blocks) <= len(raw) + 31 * len(ps), label


def test_model_against_the_runs_own_bytes():
    """the model's slicing, checked without an inflate: the records a step names are the runs' records"""
    rng = np.random.default_rng(5)
    runs = [M.Run(rng, (100, 37, 70000, 41, 4096), levels=(6, 0)), M.Run(rng, (64, 64, 64))]
    spool = M.spool_of(runs, pad=b"..")
    takes, order = [(0, 1, 5), (1, 0, 2)], [(0, 0), (1, 0), (0, 1), (0, 2), (1, 1), (0, 3)]
    raw, left = M.model(M.step_of(runs, spool, takes, order, carry=b"xy", final=False))
    assert raw + left == b"xy" + M.want_of(runs, takes, order) and len(raw) == P and 0 < len(left) < P
    raw, left = M.model(M.step_of(runs, spool, takes, order, carry=b"xy", final=True))
    assert raw == b"xy" + M.want_of(runs, takes, order) and left == b""


def test_host_step_against_the_model_under_sanitizers(harness, all_steps, tmp_path):
    out, got = _run(harness, "step", b"".join(_case(s) for s, _ in all_steps.values()), tmp_path, "steps")
    assert out == ["step", str(len(all_steps))]
    n_out = {0: 0, 1: 0}
    for (label, (s, want)), (rc, blocks, n_blocks, left) in zip(all_steps.items(), _results(got, len(all_steps))):
        assert rc == 0, label
        check_blocks(label, blocks, n_blocks, left, want, s.level)
        n_out[s.level] += n_blocks
    assert min(n_out.values()) > 30
    # what the steps reach
    assert all_steps["small-final-0"][1][0] == b"" and len(all_steps["small-final-0"][1][1]) == 1000 + 37 + 500 + 41
    assert len(all_steps["small-final-1"][1][0]) == 1578 and all_steps["nothing-final"][1] == (b"", b"")
    assert {len(s.slices) for s, _ in all_steps.values()} >= {0, 1, 2, 3, 257}
    assert {n for s, _ in all_steps.values() for _, _, n in s.recs} >= set(M.BIG)
    assert all_steps["middle-members"][0].slices[0][2] == P


def test_every_refusal_under_sanitizers(harness, tmp_path):
    cases = M.refusals()
    out, got = _run(harness, "step", b"".join(_case(s) for s, _ in cases.values()), tmp_path, "refuse")
    res = _results(got, len(cases))
    assert [r[0] for r in res] == [c for _, c in cases.values()], [n for n, r in zip(cases, res) if r[0] != cases[n][1]]
    assert all(r[1] == b"" and r[3] == b"" for r, (_, c) in zip(res, cases.values()) if c)
    good = cases["good"][0]
    check_blocks("good", res[0][1], res[0][2], res[0][3], M.model(good), good.level)


def test_pack_host_is_the_serial_coder(harness, built, tmp_path):
    import mappy_rs
    rng = np.random.default_rng(7)
    for n in (0, 1, P - 1, P, P + 1, 3 * P + 77):
        raw = M._bytes(rng, n // 2, 0) + M._bytes(rng, n - n // 2, 1)
        out, got = _run(harness, "pack", raw, tmp_path, "pack%d" % n)
        n_bytes, n_blk = struct.unpack_from("<qq", got, 0)
        off = np.frombuffer(got, np.int64, n_blk + 1, 16)
        blob = got[16 + 8 * (n_blk + 1):]
        assert out == ["pack", str(-(-n // P))] and n_blk == -(-n // P) and len(blob) == n_bytes
        assert blob == mappy_rs.bgzf_wrap(raw, compress=True)
        assert [len(p) for p in M.members(blob)] == [min(P, n - at) for at in range(0, n, P)]
        assert list(off) == list(np.cumsum([0] + [struct.unpack_from("<H", blob, int(a) + 16)[0] + 1 for a in off[:-1]]))


# ---------------------------------------------------------------- in process, without a sanitizer
def call_step(L, ctx, s, where):
    """mm355_bam_merge_step -> (blocks, n_blocks, leftover, on_device), or the return code alone"""
    from mappy_rs import _ffi
    sa, sb, sr, rs, ra, rl = s.arrays()
    spool = np.frombuffer(s.spool, np.uint8) if s.spool else np.zeros(1, np.uint8)
    carry = np.full(P, 0x5a, np.uint8)
    carry[:min(len(s.carry), P)] = np.frombuffer(s.carry[:P], np.uint8)
    n_left = C.c_int64(-1)
    tp = C.POINTER(_ffi.Text)()
    rc = L.mm355_bam_merge_step(ctx, spool.ctypes.data, len(s.spool), sa.ctypes.data, sb.ctypes.data, sr.ctypes.data, len(sa), rs.ctypes.data, ra.ctypes.data, rl.ctypes.data,
                                len(rs), carry.ctypes.data, len(s.carry), int(s.final), where, s.level, C.byref(tp), carry.ctypes.data, C.byref(n_left))
    if rc:
        assert not tp and n_left.value == -1
        assert carry[:min(len(s.carry), P)].tobytes() == s.carry[:P] and (carry[len(s.carry):] == 0x5a).all()      # nothing written
        return rc
    try:
        t = tp.contents
        return bytes(_ffi.text_view(tp)), int(t.n_lines), carry[:n_left.value].tobytes(), int(t.on_device)
    finally:
        L.mm355_free_text(tp)


def test_step_on_the_host_through_the_library(built, all_steps):
    import mappy_rs
    from mappy_rs import _ffi
    L = _ffi.lib()
    for label, (s, want) in all_steps.items():
        for where in (_ffi.PAF_HOST, _ffi.PAF_AUTO) if label.startswith("two") else (_ffi.PAF_HOST,):
            blocks, n_blocks, left, on = call_step(L, None, s, where)
            assert on == 0
            check_blocks(label, blocks, n_blocks, left, want, s.level)
            assert blocks == mappy_rs.bgzf_wrap(want[0], compress=bool(s.level)), label      # mm355_bgzf_deflate / mm355_bgzf_wrap of the stream


def test_steps_in_a_row_are_the_deflate_of_the_merged_stream(built):
    """a merge in steps of a few records: the leftover of a step is the next one's carry, and the blocks, one behind the other, are
    mm355_bgzf_deflate of the whole merged stream whatever the steps' sizes"""
    import mappy_rs
    from mappy_rs import _ffi
    L = _ffi.lib()
    rng = np.random.default_rng(11)
    runs = [M.Run(rng, [int(x) for x in rng.integers(37, 9000, 60)], levels=(6, 0, 1), kinds=(0, 0, 1)) for _ in range(3)]
    spool = M.spool_of(runs)
    merged = [(r, k) for k in range(60) for r in range(3)]                        # the merged order: run after run, record by record
    stream = b"".join(runs[r].recs[k] for r, k in merged)
    for level in (0, 1):
        want = mappy_rs.bgzf_wrap(stream, compress=bool(level))
        for per_step in (1, 7, 64, 180):
            got, carry = b"", b""
            for i in range(0, len(merged), per_step):
                part = merged[i:i + per_step]
                takes = [(r, min(k for q, k in part if q == r), max(k for q, k in part if q == r) + 1) for r in range(3) if any(q == r for q, _ in part)]
                slot = {t[0]: n for n, t in enumerate(takes)}
                order = [(slot[r], k - takes[slot[r]][1]) for r, k in part]
                s = M.step_of(runs, spool, takes, order, carry=carry, final=i + per_step >= len(merged), level=level)
                blocks, _, carry, _ = call_step(L, None, s, _ffi.PAF_HOST)
                got += blocks
            assert got == want and carry == b"", (level, per_step)


def test_refusals_through_the_library(built):
    from mappy_rs import _ffi
    L = _ffi.lib()
    cases = M.refusals()
    for label, (s, code) in cases.items():
        got = call_step(L, None, s, _ffi.PAF_HOST)
        assert (got if code else 0) == code, label
    good = cases["good"][0]
    assert call_step(L, None, good, 3) == M.EINVAL and call_step(L, None, good, -1) == M.EINVAL      # an unknown `where`
    assert call_step(L, None, good, _ffi.PAF_DEVICE) == M.EINVAL                                     # the device needs a context
    blocks, n_blocks, left, _ = call_step(L, None, good, _ffi.PAF_HOST)
    check_blocks("good", blocks, n_blocks, left, M.model(good), good.level)


def test_header_declares_what_the_library_exports(built):
    from mappy_rs import _ffi
    root = os.path.dirname(_capi.HERE)
    hdr = open(os.path.join(root, "include", "mm355.h")).read()
    declared = set(re.findall(r"\b(mm355_[a-z0-9_]+)\s*\(", hdr))
    L = _ffi.lib()
    for name in ("mm355_map_batch_bam_run_packed", "mm355_bam_merge_step"):
        assert name in declared and name in _ffi.EXPORTS and hasattr(L, name), name
    # the run record grew at its tail: the fields in front keep their place
    names = [f[0] for f in _ffi.Run._fields_]
    assert names[:9] == ["n_rec", "n_bytes", "key", "rec_off", "rec", "ms_sort", "on_device", "packed", "span"] and names[9:] == ["n_blk", "blk_off"]
    assert _ffi.Run.span.offset == 56 and _ffi.Run.n_blk.offset == 64 and C.sizeof(_ffi.Run) == 80
