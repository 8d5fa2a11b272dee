"""The host-pointer pipeline of msj_stage1 (mojo_simdjson_amd/csrc/host_pipe.cpp: uploader, downloader, copy pool, pinned
rings, events, slot-reuse waits, every failure branch) on a fake asynchronous device, CPU only.

tests/cpp/host_pipe_sanitize.cpp is a program with its own main that links the real host_pipe.cpp -- compiled with 4 KiB
chunks and 2 KiB pieces, so that kilobyte inputs reach every chunk and piece border -- against tests/cpp/fake_hip_device.h.
Two builds: AddressSanitizer + UndefinedBehaviorSanitizer with the lazy and the threaded scheduler of the fake device, and
ThreadSanitizer with the threaded one.  Nothing is preloaded and nothing is loaded into Python: the test builds the two
programs and runs them.  Any sanitizer report, any wrong word, any call that does not return (the program's watchdog) is a
non-zero exit."""
import os
import subprocess

import pytest

from tests import helpers

SIZES = ["-DMSJ_PIPE_CHUNK_BYTES=4096", "-DMSJ_PIPE_PIECE_BYTES=2048"]
COMMON = ["-std=c++17", "-Wall", "-Wno-attributes", "-fno-omit-frame-pointer", "-O1", "-g",
          "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]  # types only: the runtime's entry points are the fake device's
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TSAN = ["-fsanitize=thread"]
SEEDS = (1, 2, 3)


def _out():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    return out


def _build(tag, san):
    out = _out()
    objs = []
    for src in ("mojo_simdjson_amd/csrc/host_pipe.cpp", "tests/cpp/host_pipe_sanitize.cpp"):
        obj = os.path.join(out, f"hp_{tag}_" + os.path.basename(src).rsplit(".", 1)[0] + ".o")
        subprocess.check_call(["g++"] + COMMON + SIZES + san + ["-c", os.path.join(helpers.ROOT, src), "-o", obj])
        objs.append(obj)
    exe = os.path.join(out, "host_pipe_" + tag)
    subprocess.check_call(["g++"] + san + objs + ["-o", exe, "-lpthread"])
    return exe


def _run(exe, schedulers, env):
    for seed in SEEDS:
        r = subprocess.run([exe, str(seed), schedulers, "400"], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
        assert r.stdout.strip().splitlines()[-1].startswith("host_pipe_sanitize ok"), r.stdout[-2000:]


def _tsan_cannot_start():
    """None where a one-line ThreadSanitizer program runs on this host, else what it printed (e.g. a kernel whose
    address-space layout the runtime does not support)."""
    out = _out()
    src, exe = os.path.join(out, "tsan_probe.cpp"), os.path.join(out, "tsan_probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    subprocess.check_call(["g++"] + TSAN + [src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return None if r.returncode == 0 else f"exit {r.returncode}: " + (r.stdout + r.stderr)[-500:]


def test_host_pipeline_asan_ubsan():
    """Every output word and the guards round the caller's array at every chunk and piece border, capacity and final code,
    with and without registered caller memory, on one context across growing and shrinking calls; then every entry point
    of a call failing in turn (at once, asynchronously, by exception): the call returns, reports the failure, leaves
    nothing queued that touches the caller's freed arrays, and the context works afterwards."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    _run(_build("asan", ASAN), "lazy,threaded", env)


def test_host_pipeline_tsan():
    """The same cases with one thread per stream of the fake device: the device's reads and writes of the pinned slots,
    the carries and registered caller memory are another thread's, ordered only by what the pipeline waits for."""
    why = _tsan_cannot_start()
    if why is not None:
        pytest.skip("a one-line ThreadSanitizer program cannot start on this host: " + why)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    _run(_build("tsan", TSAN), "threaded", env)
