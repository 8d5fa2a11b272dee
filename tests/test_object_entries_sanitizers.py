"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of msj_object_entries_device's arithmetic
(mojo_simdjson_amd/csrc/object_entries_math.h through tests/object_entries_math_host.cpp): one stand-alone program with its
own main, tests/cpp/object_entries_sanitize.cpp, built here with -fsanitize=address,undefined -fno-sanitize-recover=all and
run on a window of pinned documents (maps, a map of maps, lists of structs with maps, malformed members), on 400 byte-edited
copies of it and on hostile records for each -- ascending tokens from anywhere with coded records between them, a swapped and
an equal pair, every token a row, partners moved about -- every array at its exact size.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_object_entries_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "object_entries_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "object_entries_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "object_entries_sanitize ok" in r.stdout
