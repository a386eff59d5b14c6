"""Life cycle of a context on the CPU (mappy-rs_amd/csrc/mm355_ctx.cpp, mm355_pipeline.h, mm355_timers.h): built with g++ against the HIP
stubs of tests/host_harness/ctx_life_host.cpp under AddressSanitizer and UBSan -- a stand-alone program, run as a child process, one
scenario per run.  What each scenario shows is written beside it in the harness:
  cycle    create + use + destroy leaves no device buffer, pinned buffer or event, and only the pool's streams
  inject   every HIP call of a create fails once (fresh device, ninth context of a device, with MM355_KPROF): non-zero, *out == 0,
           nothing left but a completed pool, and the next create gets pool slot 0
  devices  20 devices, contexts on 3, 16 and 19: every stream made on its own device; nine contexts on one device; slot 2 handed out again
  order    the order of stream creations (the hardware queue of a stream follows from it), with and without MM355_DP_QALIGN=1
  shared   MM355_DP_SHARED_STREAMS=1: the device's eight extension streams, made once and whole
  buffers  DBuf / HBuf: growth frees the old block, a moved-from buffer frees nothing, std::vector<ResidentBatch> 1 -> 40
  timers   an open pair keeps its slot through 300 inner pairs; the 121st begin with none open resolves and takes slot 0; timers_on off"""
import os
import subprocess

import pytest

import _capi

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ctx_life") / "ctx_life_host")
    # the sanitizer runtimes are linked statically: the program must not depend on what else the process that runs it has loaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           os.path.join(_capi.HERE, "host_harness", "ctx_life_host.cpp"), os.path.join(_capi.CSRC, "mm355_ctx.cpp"),
                           "-o", exe, "-lpthread"])
    return exe


def _run(exe, scenario, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MM355_")}
    e.update(env)
    r = subprocess.run([exe, scenario], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines()[-1] == "ok " + scenario
    return r


@pytest.mark.parametrize("scenario", ["cycle", "devices", "buffers", "timers"])
def test_scenario(harness, scenario):
    _run(harness, scenario)


def test_every_call_of_a_create_fails_once(harness):
    r = _run(harness, "inject")
    # K is whatever the code makes it; the harness prints it.  A create on a fresh device makes at least the sixteen pool streams, six extension
    # streams, four events and two buffers
    k = int(r.stdout.split("fresh device:")[1].split(",")[0])
    assert k >= 28


def test_shared_extension_streams(harness):
    _run(harness, "shared", MM355_DP_SHARED_STREAMS="1")


@pytest.mark.parametrize("qalign", [False, True], ids=["plain", "qalign"])
def test_stream_creation_order(harness, qalign):
    _run(harness, "order", **({"MM355_DP_QALIGN": "1"} if qalign else {}))
