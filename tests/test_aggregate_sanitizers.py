"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of the arithmetic of msj_aggregate_device
(mojo_simdjson_amd/csrc/aggregate_math.h through tests/aggregate_math_host.cpp): one stand-alone program with its own main,
tests/cpp/aggregate_sanitize.cpp, built here with -fsanitize=address,undefined -fno-sanitize-recover=all and run on a pinned
corpus and on 3 000 rounds of hostile records -- wild tags, flags and codes, NaN and infinity patterns, every exponent in one
group, codes of -1, G, INT32_MIN and INT32_MAX, a row count below and above the stride, a group count below and above the
capacity.  Every array at its exact size.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_aggregate_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "aggregate_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "aggregate_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "aggregate_sanitize ok" in r.stdout
