"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of the arithmetic of msj_patterns_create and
msj_match_strings_device (mojo_simdjson_amd/csrc/match_strings_math.h through tests/match_strings_math_host.cpp): one
stand-alone program with its own main, tests/cpp/match_strings_sanitize.cpp, built here with
-fsanitize=address,undefined -fno-sanitize-recover=all and run on the masked word fetch at every residue and end and on
3 000 rounds of hostile arrays -- offsets, valid bytes and R from anywhere, patterns of every shape, few blocks, short
stages -- against a matcher of its own.  Every array at its exact size.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_match_strings_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "match_strings_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "match_strings_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "match_strings_sanitize ok" in r.stdout
