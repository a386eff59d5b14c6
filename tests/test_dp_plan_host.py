"""The plan of one extension problem (mappy-rs_amd/csrc/mm355_dpplan.h: launch group, direction-matrix layout and bytes, band) on the CPU.  The
header is compiled with g++ under AddressSanitizer and UBSan into a stand-alone program (tests/host_harness/dpplan_host.cpp) and run over a grid
of problems: six scorings (the presets' three, an irregular cost, a re-ordered one, a single piece) x target lengths at every size-class border
x query lengths x flags x bands.  The expected values (tests/golden/dp_plan_parent.json) were dumped from the driver as it stood BEFORE the plan
became a header of its own -- mm355_dp_run's layout loop and mm355_dp_matrix_bytes, then two separate texts -- with the switches set through
that version's environment variables: every third problem of the grid, outputs only (the inputs are regenerated here); the band-switch columns
only for the problems the row sweep takes (the others do not read the switches, which the dump checked)."""
import json
import os
import subprocess

import pytest

import _capi

SCORINGS = [(2, 4, 1, 4, 2, 24, 1), (1, 4, 1, 6, 2, 26, 1), (1, 19, 1, 39, 3, 81, 1), (4, 10, 1, 3, 3, 12, 3), (4, 6, 1, 10, 1, 3, 4), (2, 5, 1, 5, 2, 5, 2)]
TLENS = [1, 128, 129, 200, 256, 257, 384, 512, 513, 700, 900, 1024, 1025, 4096, 4097, 8192, 8193, 12288, 12289, 20000]
FLAGS = [0, 8, 8 | 2, 0x40, 8 | 0x10]
MAX_SW_MAT = 10 ** 8
COLUMNS = ["group", "pad", "dlo", "lmin", "bw", "matrix_bytes", "budget_minus_matrix_bytes"]
# fixture column -> (use_band, band_force) of DpKnobs
KNOBS = {"default": (1, 0), "band_off": (0, 0), "force_64": (1, 64), "force_1": (1, 1), "force_2": (1, 2), "force_4": (1, 4)}


def grid(keep):
    """(a, b, sc_ambi, q, e, q2, e2, max_sw_mat, qlen, tlen, w, flag) of every keep-th problem; the short queries reach the HBM-state groups
    (12289 x 12289 is beyond max_sw_mat)"""
    rows, i = [], 0
    for sc in SCORINGS:
        for tl in TLENS:
            for ql in sorted({tl - 600, tl - 1, tl, tl + 40, min(tl, 3000), 1 + tl // 3}):
                if ql <= 0:
                    continue
                for fl in FLAGS:
                    for w in (16, 832, 833, ql + tl):
                        if i % keep == 0:
                            rows.append(sc + (MAX_SW_MAT, ql, tl, w, fl))
                        i += 1
    return rows


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "dp_plan_parent.json")) as f:
        fx = json.load(f)
    assert fx["columns"] == COLUMNS
    return fx


@pytest.fixture(scope="module")
def plans(golden, tmp_path_factory):
    """column -> the harness's lines for the whole grid, as tuples of int"""
    exe = str(tmp_path_factory.mktemp("dpplan") / "dpplan_host")
    # the sanitizer runtimes are linked statically: the program must not depend on what else the process that runs it has loaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "dpplan_host.cpp"), "-o", exe])
    rows = grid(golden["keep"])
    inp = "".join(" ".join(map(str, r)) + "\n" for r in rows)
    out = {}
    for col, (use_band, force) in KNOBS.items():
        r = subprocess.run([exe, str(use_band), str(force)], input=inp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, (col, r.returncode, r.stderr[-4000:])
        out[col] = [tuple(map(int, l.split())) for l in r.stdout.splitlines()]
        assert len(out[col]) == len(rows)
    return rows, out


def as_fixture(line):
    _skip, g, pad, dlo, lmin, bw, pb, _line, _cig, _st, _regw, budget = line
    return [g, pad, dlo, lmin, bw, pb, budget - pb]


def test_the_fixture_reaches_every_group(golden):
    """the thinned grid still has at least 20 problems in each of the 23 groups a problem can plan into, under default switches"""
    count = [0] * 23
    for r in golden["default"]:
        count[r[0]] += 1
    assert min(count) >= 20, count
    assert all(golden["default"][i][1] != 0 for i in golden["row_class_rows"]) and len(golden["row_class_rows"]) == sum(r[1] != 0 for r in golden["default"])


def test_plan_equals_the_parent_under_default_switches(golden, plans):
    rows, out = plans
    assert len(rows) == len(golden["default"])
    for i, (line, exp) in enumerate(zip(out["default"], golden["default"])):
        assert as_fixture(line) == exp, (i, rows[i], line, exp)


@pytest.mark.parametrize("col", ["band_off", "force_64", "force_1", "force_2", "force_4"])
def test_plan_equals_the_parent_under_band_switches(golden, plans, col):
    rows, out = plans
    rc = golden["row_class_rows"]
    assert len(golden[col]) == len(rc)
    for i, exp in zip(rc, golden[col]):
        assert as_fixture(out[col][i]) == exp, (col, i, rows[i], out[col][i], exp)
    taken = set(rc)
    for i in range(len(rows)):                          # the band switches are read for no other problem
        if i not in taken:
            assert out[col][i] == out["default"][i], (col, i, rows[i])


def test_budget_covers_the_layout_and_the_other_fields_follow(plans):
    """what the budget of a round counts for a problem is at least what the layout adds for it, the worst-case alignment of its first tile
    included (up to 63 bytes in front of a matrix that starts on a 64-byte line); CIGAR words, HBM state words, LDS bytes and the skip mark
    follow from the group and the lengths"""
    rows, out = plans
    for col, lines in out.items():
        for r, (skip, g, pad, _dlo, _lmin, _bw, pb, line, cig, st, regw, budget) in zip(rows, lines):
            ql, tl = r[8], r[9]
            T = (tl + 15) // 16 * 16
            assert budget >= pb + (63 if line else 0), (col, r)
            assert line == (pad != 0) and skip == (ql * tl > MAX_SW_MAT), (col, r)
            assert cig == (0 if skip else ql + tl + 2) and (pb > 0) == (not skip), (col, r)
            assert st == (T if g in (12, 13) else 0) and regw == (((ql + 15) & ~15) + T if g == 18 else 0), (col, r)
            assert not skip or (g, pad, pb, budget) == (0, 0, 0, 0), (col, r)
