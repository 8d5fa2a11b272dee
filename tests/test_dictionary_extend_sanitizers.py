"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of msj_dictionary_extend_device's arithmetic
(mojo_simdjson_amd/csrc/dictionary_extend_math.h through tests/dictionary_extend_math_host.cpp): one stand-alone program with
its own main, tests/cpp/dictionary_extend_sanitize.cpp, built here with -fsanitize=address,undefined
-fno-sanitize-recover=all and run on a pinned chain of three windows into one dictionary and on 300 damaged copies -- row
offsets and valid bytes from a generator, prior offsets that descend, lie past dict_bytes_capacity or are huge, a byte buffer
shorter than the offsets say, P and the row count below, at and above their capacities.  Every array at its exact size,
under both hashes and both orders of insertion, unfrozen and frozen, with room, with one entry or one byte of room and with
none.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_dictionary_extend_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dictionary_extend_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "dictionary_extend_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "dictionary_extend_sanitize ok" in r.stdout
