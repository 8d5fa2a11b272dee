"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of the arithmetic of msj_sort_rows_device
(mojo_simdjson_amd/csrc/sort_rows_math.h through tests/sort_rows_math_host.cpp): one stand-alone program with its own main,
tests/cpp/sort_rows_sanitize.cpp, built here with -fsanitize=address,undefined -fno-sanitize-recover=all and run on a pinned
corpus and on 4 000 rounds of hostile records and row lists -- wild tags, flags and codes, NaN and infinity patterns, ints of
every size beside the doubles next to them, row numbers at and past R, repeats, a row count above the stride, a list longer
than the capacity, limits around K.  Every array at its exact size.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_sort_rows_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sort_rows_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "sort_rows_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "sort_rows_sanitize ok" in r.stdout
