"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of msj_dictionary_device's arithmetic
(mojo_simdjson_amd/csrc/dictionary_math.h through tests/dictionary_math_host.cpp): one stand-alone program with its own main,
tests/cpp/dictionary_sanitize.cpp, built here with -fsanitize=address,undefined -fno-sanitize-recover=all and run on a pinned
column (repeated values, "", null rows, prefixes, values of 3 000 bytes that differ in their last byte) and on 300 damaged
copies of its offsets and valid arrays -- offsets that descend, lie past bytes_len or are huge, valid bytes from a generator,
a byte buffer shorter than the offsets say, a row count below and above `rows`.  Every array at its exact size, under both
hashes and both orders of insertion, with room, with each capacity one short, without any room and layout-only.  Nothing is
loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_dictionary_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dictionary_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "dictionary_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "dictionary_sanitize ok" in r.stdout
