"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of msj_raw_column_device's arithmetic
(mojo_simdjson_amd/csrc/raw_column_math.h through tests/raw_column_math_host.cpp): one stand-alone program with its own
main, tests/cpp/raw_column_sanitize.cpp, built here with -fsanitize=address,undefined -fno-sanitize-recover=all and run on a
pinned window (nesting, escapes, a LONG number in front of blanks and one that ends the window) and on 600 damaged copies of
its arrays -- a d_idx that does not ascend, d_end beyond len, flags, types and d_match from a generator, a window shorter
than its index says -- each with hostile records: tokens at and past n, containers whose partner lies at or in front of the
token or at or past n, records with codes.  Every array at its exact size, verbatim and compact, with room, clipped and
layout-only.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_raw_column_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "raw_column_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "raw_column_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "raw_column_sanitize ok" in r.stdout
