"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of the arithmetic of msj_join_rows_device
(mojo_simdjson_amd/csrc/join_rows_math.h through tests/join_rows_math_host.cpp): one stand-alone program with its own main,
tests/cpp/join_rows_sanitize.cpp, built here with -fsanitize=address,undefined -fno-sanitize-recover=all and run on a pinned
corpus and on 4 000 rounds of hostile key columns -- wild keys, counts on the "device" above the rooms, a G above
keys_capacity, pair rooms around M, every output optional.  Every array at its exact size.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_join_rows_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "join_rows_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "join_rows_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "join_rows_sanitize ok" in r.stdout
