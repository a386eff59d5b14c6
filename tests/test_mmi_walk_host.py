"""The host side of the device .mmi loader (mappy-rs_amd/csrc/mm355_mmiwalk.h): the walk over the bucket headers and the plan that cuts the
bucket sections into pieces, built with g++ under AddressSanitizer and UBSan into a stand-alone program (tests/host_harness/
mmi_walk_host.cpp) and compared with offsets computed here from _mmi.parse_mmi.  Files: minimap2's own tests/golden/test.mmi (khash order,
every p[] empty), the oracle's dumps of the repeat-rich reference at the four settings, an MM_I_NO_SEQ file."""
import bisect
import os
import subprocess

import pytest

import _capi
import _mmi
import _mmiload

PIECES = [64, 256, 4096, 32 << 20]
EINVAL, EIO = -2, -4


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mmi_walk") / "mmi_walk_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "mmi_walk_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def files(built, golden_dir, tmp_path_factory):
    """name -> path of every input file"""
    d = tmp_path_factory.mktemp("mmi_walk_files")
    fa = str(d / "rep.fa")
    _mmi.write_fasta(fa, _mmi.repeat_rich_records())
    out = {"golden": os.path.join(golden_dir, "test.mmi")}
    for k, w, flag in _mmi.SETTINGS:
        out["oracle_%d_%d_%d" % (k, w, flag)] = str(d / ("oracle_%d_%d_%d.mmi" % (k, w, flag)))
        _mmiload.oracle_dump(fa, k, w, flag, out["oracle_%d_%d_%d" % (k, w, flag)])
    out["noseq"] = str(d / "noseq.mmi")
    with open(out["noseq"], "wb") as f:
        f.write(_mmiload.no_seq(open(out["oracle_15_10_0"], "rb").read()))
    return out


NAMES = ["golden", "noseq"] + ["oracle_%d_%d_%d" % s for s in _mmi.SETTINGS]


def _run(exe, path, pieces=(), **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MM355_")}
    e.update(env)
    r = subprocess.run([exe, str(path)] + [str(p) for p in pieces], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln.split(" ") for ln in r.stdout.splitlines()]
    assert lines[0][0] == "rc"
    return int(lines[0][1]), lines[1:]


def _parse(lines):
    """harness output -> (walk dict, contigs, buckets, {P: [(file_off, bytes, n_items, [seg dict])]}, env P)"""
    walk, contigs, buckets, plans, env, cur = None, [], [], {}, None, None
    for ln in lines:
        if ln[0] == "walk":
            walk = dict(zip("w k b n_seq flag sum_len off_buckets off_S S_bytes file_size n_pos n_distinct".split(), map(int, ln[1:])))
        elif ln[0] == "contig":
            contigs.append((" ".join(ln[2:]).encode(), int(ln[1])))
        elif ln[0] == "bucket":
            buckets.append(tuple(int(x) for x in ln[1:]))
        elif ln[0] == "plan":
            cur = plans.setdefault(int(ln[1]), [])
        elif ln[0] == "piece":
            assert int(ln[1]) == len(cur)
            cur.append((int(ln[2]), int(ln[3]), int(ln[4]), [], int(ln[5])))
        elif ln[0] == "seg":
            cur[-1][3].append(dict(zip("kind bucket off count item0 gidx p_base n".split(), map(int, ln[1:]))))
        elif ln[0] == "env":
            env = int(ln[1])
    for pieces in plans.values():
        assert all(len(segs) == n_seg for _, _, _, segs, n_seg in pieces)
    return walk, contigs, buckets, plans, env


@pytest.fixture(scope="module")
def walked(harness, files):
    """every file walked and planned once, at every piece size: name -> (layout from Python, parsed harness output)"""
    out = {}
    for name in NAMES:
        rc, lines = _run(harness, files[name], PIECES)
        assert rc == 0
        out[name] = (_mmiload.layout(open(files[name], "rb").read()), _parse(lines))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_walk(walked, name):
    lay, (walk, contigs, buckets, _, env) = walked[name]
    m = lay["m"]
    assert (walk["w"], walk["k"], walk["b"], walk["n_seq"], walk["flag"]) == (m["w"], m["k"], m["b"], m["n_seq"], m["flag"])
    assert contigs == m["contigs"] and walk["sum_len"] == sum(ln for _, ln in m["contigs"])
    assert (walk["off_buckets"], walk["off_S"], walk["S_bytes"]) == (lay["off_buckets"], lay["off_S"], len(m["S"]))
    assert walk["file_size"] == lay["off_S"] + len(m["S"])
    assert (walk["n_pos"], walk["n_distinct"]) == (lay["n_pos"], lay["n_distinct"]) and walk["n_distinct"] > 0
    assert len(buckets) == 1 << m["b"]
    assert buckets == [(i, off, n, size, lay["p_base"][i], lay["pair_base"][i]) for i, (off, n, size) in enumerate(lay["buckets"])]
    assert env == 32 << 20
    if name == "golden":
        assert walk["n_pos"] == 0                       # minimap2's fixture: every minimizer a singleton
    elif name == "noseq":
        assert walk["flag"] & 2 and walk["S_bytes"] == 0 and walk["n_pos"] > 0
    else:
        assert walk["n_pos"] >= 100 and walk["S_bytes"] > 0
        if name == "oracle_6_3_0":
            assert walk["b"] == 12


@pytest.mark.parametrize("P", PIECES)
@pytest.mark.parametrize("name", NAMES)
def test_plan(walked, name, P):
    lay, (_, _, _, plans, _) = walked[name]
    pieces = plans[P]
    # where every item begins, from the Python-side layout: headers, position words, pairs
    headers, items = [], {}
    for i, (off, n, size) in enumerate(lay["buckets"]):
        headers += [off, off + 4 + 8 * n]
        for j in range(n):
            items[off + 4 + 8 * j] = (0, i, lay["p_base"][i] + j)
        for j in range(size):
            items[off + 8 + 8 * n + 16 * j] = (1, i, lay["pair_base"][i] + j)
    starts = set(headers) | set(items) | {lay["off_S"]}
    # the pieces tile the bucket section, none above P, every cut at the beginning of an item
    at = lay["off_buckets"]
    seen = [0, 0]
    for file_off, nbytes, n_items, segs, _ in pieces:
        assert file_off == at and 0 < nbytes <= P and file_off in starts
        at += nbytes
        item0, payload, prev_end = 0, 0, 0
        for s in segs:
            kind, width = s["kind"], (8, 16)[s["kind"]]
            first = file_off + s["off"]
            assert s["count"] > 0 and s["item0"] == item0 and s["off"] >= prev_end and s["off"] % 4 == 0
            assert s["off"] + width * s["count"] <= nbytes                         # no item hangs out of its piece
            assert items[first] == (kind, s["bucket"], s["gidx"])                  # the segment begins at the item it names
            off, n, size = lay["buckets"][s["bucket"]]
            end_of_kind = off + 4 + 8 * n if kind == 0 else off + 8 + 8 * n + 16 * size
            assert first + width * s["count"] <= end_of_kind                       # ... and stays inside that bucket's p[] or pairs
            assert (s["p_base"], s["n"]) == (lay["p_base"][s["bucket"]], n)
            item0 += s["count"]; payload += width * s["count"]; prev_end = s["off"] + width * s["count"]; seen[kind] += s["count"]
        assert n_items == item0
        # what the segments do not cover is headers, whole
        n_headers = bisect.bisect_left(headers, file_off + nbytes) - bisect.bisect_left(headers, file_off)
        assert nbytes == payload + 4 * n_headers
    assert at == lay["off_S"]
    assert seen == [lay["n_pos"], lay["n_distinct"]]                               # with the tiling above: every payload item exactly once
    if P == 32 << 20:
        assert len(pieces) == 1


def test_small_pieces_split_buckets(walked):
    """P = 256 on the (15, 10, 0) file: the tandem repeat's run of >= 100 positions is >= 800 bytes"""
    lay, (_, _, _, plans, _) = walked["oracle_15_10_0"]
    cuts = [file_off for file_off, _, _, _, _ in plans[256]]

    def n_pieces(lo, hi):      # pieces that hold a byte of [lo, hi)
        return bisect.bisect_left(cuts, hi) - bisect.bisect_right(cuts, lo) + 1 if hi > lo else 0

    p_span = [n_pieces(off + 4, off + 4 + 8 * n) for off, n, _ in lay["buckets"]]
    pair_span = [n_pieces(off + 8 + 8 * n, off + 8 + 8 * n + 16 * size) for off, n, size in lay["buckets"]]
    assert max(p_span) >= 3 and max(pair_span) >= 2
    assert max(n for _, n, _ in lay["buckets"]) >= 100


def test_bad_files_are_refused(harness, files, tmp_path):
    data = open(files["oracle_15_10_0"], "rb").read()
    for what, raw in _mmiload.bad_files(data):
        f = tmp_path / "bad.mmi"
        f.write_bytes(raw)
        assert _run(harness, f)[0] == EIO, what
    assert _run(harness, tmp_path / "missing.mmi")[0] == EIO
    fa = tmp_path / "x.fa"
    fa.write_text(">a\nACGT\n")
    assert _run(harness, fa)[0] == EINVAL                                          # not an index: nothing for this loader
    assert _run(harness, files["golden"])[0] == 0


def test_piece_size_from_the_environment(harness, files):
    for env, want in (("256", 256), ("1", 64), ("4096", 4096), ("", 32 << 20)):
        _, lines = _run(harness, files["golden"], MM355_IDXLOAD_PIECE=env)
        assert _parse(lines)[4] == want
