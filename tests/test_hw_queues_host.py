"""The library owns its hardware queue count (mm355_runtime_init, mappy-rs_amd/csrc/mm355_ctx.cpp): before its first HIP call it sets
GPU_MAX_HW_QUEUES to MM355_HW_QUEUES (clamped to 1..32) or to the tuned default 8, over whatever the process inherited.  A child process
with the variable preset to 4 loads the library, calls mm355_device_count() and reads the C environment back.  Needs no GPU: without one
mm355_device_count() returns 0."""
import os
import subprocess
import sys

import pytest

CODE = ("import ctypes as C, sys\n"
        "L = C.CDLL(sys.argv[1])\n"
        "libc = C.CDLL(None); libc.getenv.restype = C.c_char_p; libc.getenv.argtypes = [C.c_char_p]\n"
        "before = libc.getenv(b'GPU_MAX_HW_QUEUES')\n"
        "L.mm355_device_count.restype = C.c_int\n"
        "n = L.mm355_device_count()\n"
        "assert n >= 0\n"
        "print('queues', before.decode(), libc.getenv(b'GPU_MAX_HW_QUEUES').decode())\n")


@pytest.mark.parametrize("want,expect", [(None, "8"), ("6", "6"), ("99", "32"), ("0", "1"), ("", "8"), ("many", "8"), ("8x", "8")])
def test_library_sets_its_queue_count(built, want, expect):
    from mappy_rs import _ffi
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    env.pop("MM355_HW_QUEUES", None)
    if want is not None:
        env["MM355_HW_QUEUES"] = want
    r = subprocess.run([sys.executable, "-c", CODE, _ffi.LIB_PATH], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert r.stdout.split() == ["queues", "4", expect], r.stdout
